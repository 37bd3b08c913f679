// Stand-alone host program for tests/test_host_polyiou.py: runs convex_quad_iou of csrc/polyiou.cuh -- the function the
// kernels run -- on the CPU, pair by pair.  Built with the address and undefined-behaviour sanitizers.
//   polyiou_host <in: float32 a [N, 4, 2]> <in: float32 b [N, 4, 2]> <N> <out: float64 [N, 4] (iou, area a, area b,
//                 quad_area(a))>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "polyiou.cuh"

using namespace cnuda::polyiou;

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: polyiou_host a.bin b.bin N out.bin\n");
        return 2;
    }
    const long n = atol(argv[3]);
    if (n < 0) return 2;
    std::vector<float> a((size_t)n * 8), b((size_t)n * 8);
    FILE* fa = fopen(argv[1], "rb");
    FILE* fb = fopen(argv[2], "rb");
    if (!fa || !fb || fread(a.data(), sizeof(float), a.size(), fa) != a.size() ||
        fread(b.data(), sizeof(float), b.size(), fb) != b.size()) {
        fprintf(stderr, "polyiou_host: cannot read %ld quads from both inputs\n", n);
        return 2;
    }
    fclose(fa), fclose(fb);
    std::vector<double> out((size_t)n * 4);
    for (long i = 0; i < n; ++i) {
        const Quad qa = load_quad(&a[(size_t)i * 8]), qb = load_quad(&b[(size_t)i * 8]);
        const QuadIou r = convex_quad_iou(qa, qb);
        out[(size_t)i * 4] = r.iou, out[(size_t)i * 4 + 1] = r.area_a, out[(size_t)i * 4 + 2] = r.area_b;
        out[(size_t)i * 4 + 3] = quad_area(qa);
    }
    FILE* fo = fopen(argv[4], "wb");
    if (!fo || fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 2;
    fclose(fo);
    return 0;
}
