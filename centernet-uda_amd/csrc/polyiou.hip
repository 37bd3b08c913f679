// hip_runtime.ops.rotated_iou: the exact IoU of every (a, b) pair of two sets of quadrilaterals per image, and the
// sets' areas (polyiou.cuh).  One thread per pair, then one per quad for the areas, in one grid-stride launch; every
// value is a pure function of its own operands, so the results are the same bits on every run.
#include "common.h"
#include "polyiou.cuh"

namespace cnuda {
namespace {

using namespace polyiou;

__global__ __launch_bounds__(256) void quad_iou_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             double* __restrict__ iou, double* __restrict__ area_a,
                                                             double* __restrict__ area_b, int B, int N, int M) {
    const long long pairs = (long long)B * N * M;
    const long long na = area_a ? (long long)B * N : 0, nb = area_b ? (long long)B * M : 0;
    const long long total = pairs + na + nb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        if (i < pairs) {
            const long long row = i / M;                   // image * N + n
            const long long col = (row / N) * M + i % M;   // image * M + m
            iou[i] = convex_quad_iou(load_quad(a + 8 * row), load_quad(b + 8 * col)).iou;
        } else if (i < pairs + na) {
            area_a[i - pairs] = quad_area(load_quad(a + 8 * (i - pairs)));
        } else {
            area_b[i - pairs - na] = quad_area(load_quad(b + 8 * (i - pairs - na)));
        }
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_quad_iou_pairs(const float* a, const float* b, double* iou, double* area_a, double* area_b,
                                    int B, int N, int M, cnuda_stream_t stream) {
    const char* who = "cnuda_quad_iou_pairs";
    CNUDA_REQUIRE(B > 0 && N >= 0 && M >= 0, "%s: bad sizes (B %d, N %d, M %d)", who, B, N, M);
    CNUDA_REQUIRE((long long)B * N < (1ll << 31) && (long long)B * M < (1ll << 31), "%s: too many quads", who);
    CNUDA_REQUIRE((a || N == 0) && (b || M == 0), "%s: null pointer", who);
    const long long pairs = (long long)B * N * M;
    CNUDA_REQUIRE(iou || pairs == 0, "%s: null pointer", who);
    const long long total = pairs + (area_a ? (long long)B * N : 0) + (area_b ? (long long)B * M : 0);
    if (total == 0) return 0;
    CNUDA_LAUNCH(quad_iou_pairs_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, a, b, iou,
                 area_a, area_b, B, N, M);
    return check_launch(who);
}
