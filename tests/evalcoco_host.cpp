// Stand-alone host program for tests/test_host_cocoeval.py: runs the closed-form mask rule of csrc/evalcoco.cuh on the
// CPU (every "lane" of the kernel one after the other) and exercises the host-only argument checks and workspace sizes
// of the cnuda_eval_* entry points.  Built with the address and undefined-behaviour sanitizers.
//   evalcoco_host <in: int32 verts [N, 4, 2]> <N> <H> <W> <out: int32 [N, H, 2] (left, right), (0, -1) = empty row>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "evalcoco.cuh"

using namespace cnuda::evalcoco;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 2;                                                       \
        }                                                                   \
    } while (0)

static int host_helpers() {
    EXPECT(spans_workspace_bytes(10, 64) >= (size_t)10 * 64 * 8);
    EXPECT(spans_workspace_bytes(0, 64) > 0);
    EXPECT(spans_workspace_bytes(-1, 64) == 0 && spans_workspace_bytes(10, 0) == 0 && spans_workspace_bytes(10, 8193) == 0);
    EXPECT(spans_workspace_bytes(INT_MAX, 8192) == (size_t)INT_MAX * 8192 * 8 + 256);
    EXPECT(!image_error(512, 640) && image_error(0, 4) && image_error(4, -1) && image_error(8193, 4) && image_error(4, 8193));
    EXPECT(!groups_error(0, 0, 0, 0) && !groups_error(96, 2400, 800, 30000));
    EXPECT(groups_error(-1, 0, 0, 0) && groups_error(1, -1, 0, 0) && groups_error(1, 1, -1, 0) && groups_error(1, 1, 1, -1));
    EXPECT(groups_error(1, 1, 1, 1ll << 31) && groups_error(1, INT_MAX, 1, 1) && groups_error(1 << 24, 1, 1, 1));
    const double thr[3] = {0.5, 0.75, 0.95}, bad_thr[2] = {0.5, 1.5};
    const double rng[8] = {0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10}, bad_rng[8] = {0, 1e10, 5, 1, 0, 1, 0, 1};
    EXPECT(!match_error(thr, 3, rng));
    EXPECT(match_error(nullptr, 3, rng) && match_error(thr, 3, nullptr) && match_error(thr, 0, rng) && match_error(thr, 17, rng));
    EXPECT(match_error(bad_thr, 2, rng) && match_error(thr, 3, bad_rng));
    return 0;
}

int main(int argc, char** argv) {
    if (host_helpers()) return 2;
    if (argc != 6) return 64;
    const int N = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]);
    std::vector<int> verts((size_t)N * 8), out((size_t)N * H * 2);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(verts.data(), sizeof(int), verts.size(), f) != verts.size()) return 65;
    fclose(f);
    std::vector<int> left(H), right(H);
    for (int b = 0; b < N; ++b) {
        int vx[4], vy[4];
        for (int i = 0; i < 4; ++i) vx[i] = verts[8 * b + 2 * i], vy[i] = verts[8 * b + 2 * i + 1];
        for (int r = 0; r < H; ++r) left[r] = INT_MAX, right[r] = INT_MIN;
        for (int e = 0; e < 4; ++e) {
            const int p = (e + 3) & 3;
            const Line l = line_setup(vx[p], vy[p], vx[e], vy[e], W, H);
            for (int k = 0; k <= l.count + 1 && l.count >= 0; ++k) {
                int x, y;
                if (k <= l.count) line_pixel(l, k, x, y);
                else x = l.end_x, y = l.end_y;
                if (x >= 0 && x < W && y >= 0 && y < H) {
                    if (x < left[y]) left[y] = x;
                    if (x > right[y]) right[y] = x;
                }
            }
        }
        ScanInterval scan[kMaxScanIntervals];
        const int n = scan_setup(vx, vy, W, H, scan);
        for (int s = 0; s < n; ++s) {
            const int lo = scan[s].row_begin < 0 ? 0 : scan[s].row_begin, hi = scan[s].row_end < H ? scan[s].row_end : H;
            for (int r = lo; r < hi; ++r) {
                int a, c;
                if (scan_row(scan[s], r, W, a, c)) {
                    if (a < left[r]) left[r] = a;
                    if (c > right[r]) right[r] = c;
                }
            }
        }
        for (int r = 0; r < H; ++r) {
            const bool any = left[r] <= right[r];
            out[((size_t)b * H + r) * 2] = any ? left[r] : 0;
            out[((size_t)b * H + r) * 2 + 1] = any ? right[r] : -1;
        }
    }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), sizeof(int), out.size(), f) != out.size()) return 66;
    fclose(f);
    return 0;
}
