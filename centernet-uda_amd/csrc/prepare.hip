// Input normalisation on the GPU: datasets/coco.py:160-162 (and 105-109 for the target-domain image),
//   inp = ((img.astype(float32) / 255) - mean) / std, transposed HWC -> CHW,
// from the uint8 image, so that the batch's `input` keys cross the bus as bytes and not as fp32.
//
// Every step is one float32 operation in numpy's order (the build has -ffp-contract=off and hipcc's correctly rounded
// fp32 divide), so the result is bit-identical to numpy.  Memory-bound: a thread takes four consecutive pixels of the
// flattened [B*H*W] pixel axis = twelve packed bytes = three aligned dwords, and writes four values to each plane; as
// one float4 where H*W is a multiple of four (then a group never straddles two images and every plane address is
// 16-byte aligned), as four scalars otherwise.  The up to three pixels after the last whole group go one per thread.
#include "common.h"

namespace cnuda {
namespace {

struct Norm3 { float mean[3], std[3]; };

__device__ __forceinline__ float norm1(unsigned v, float mean, float std) {
    return ((float)v / 255.0f - mean) / std;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void prepare_input_kernel(const unsigned char* __restrict__ img,
                                                            float* __restrict__ out, long long HW, long long N,
                                                            Norm3 nm) {
    const long long groups = N / 4, step = (long long)gridDim.x * blockDim.x;
    const uint32_t* img4 = reinterpret_cast<const uint32_t*>(img);
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += step) {
        const uint32_t d0 = img4[3 * g], d1 = img4[3 * g + 1], d2 = img4[3 * g + 2];
        // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
        const unsigned c0[4] = {d0 & 255u, d0 >> 24, (d1 >> 16) & 255u, (d2 >> 8) & 255u};
        const unsigned c1[4] = {(d0 >> 8) & 255u, d1 & 255u, d1 >> 24, (d2 >> 16) & 255u};
        const unsigned c2[4] = {(d0 >> 16) & 255u, (d1 >> 8) & 255u, d2 & 255u, d2 >> 24};
        float v[3][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v[0][p] = norm1(c0[p], nm.mean[0], nm.std[0]);
            v[1][p] = norm1(c1[p], nm.mean[1], nm.std[1]);
            v[2][p] = norm1(c2[p], nm.mean[2], nm.std[2]);
        }
        const long long n0 = 4 * g;
        if (WIDE) {
            const long long b = n0 / HW, pix = n0 - b * HW;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(out + (b * 3 + c) * HW + pix) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const long long b = (n0 + p) / HW, pix = (n0 + p) - b * HW;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(b * 3 + c) * HW + pix] = v[c][p];
            }
        }
    }
    // scalar tail: pixels 4 * groups .. N - 1 (WIDE has none: N = B * HW is a multiple of four there)
    if (!WIDE && blockIdx.x == 0 && threadIdx.x < (unsigned)(N - 4 * groups)) {
        const long long n = 4 * groups + threadIdx.x, b = n / HW, pix = n - b * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(b * 3 + c) * HW + pix] = norm1(img[3 * n + c], nm.mean[c], nm.std[c]);
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_prepare_input(const unsigned char* images, float* out, int B, int H, int W, float mean0,
                                   float mean1, float mean2, float std0, float std1, float std2,
                                   cnuda_stream_t stream) {
    CNUDA_REQUIRE(images && out, "cnuda_prepare_input: null pointer");
    CNUDA_REQUIRE(B > 0 && H > 0 && W > 0, "cnuda_prepare_input: bad sizes");
    CNUDA_REQUIRE(((uintptr_t)images & 3) == 0 && ((uintptr_t)out & 15) == 0,
                  "cnuda_prepare_input: images must be 4-byte and out 16-byte aligned");
    const long long HW = (long long)H * W, N = HW * B;
    const Norm3 nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
    hipStream_t st = (hipStream_t)stream;
    const int grid = stream_grid(N / 4, 256);
    if (HW % 4 == 0)
        CNUDA_LAUNCH(prepare_input_kernel<true>, dim3(grid), dim3(256), 0, st, images, out, HW, N, nm);
    else
        CNUDA_LAUNCH(prepare_input_kernel<false>, dim3(grid), dim3(256), 0, st, images, out, HW, N, nm);
    return check_launch("cnuda_prepare_input");
}
