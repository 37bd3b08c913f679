// The student's strong view for weak/strong self-training (uda/mean_teacher.py, WeakStrongTeacher; DESIGN.md, "Strong
// view"): colour jitter, grayscale, gaussian blur and random erasing applied to a normalised float32 batch as it sits on
// the device.  All of it is photometric or occluding, so the teacher's boxes stay valid.
//
//   strong_view_pivot_kernel   the contrast pivot of every image: the mean luma of the un-augmented image, from a 64-bit
//                              INTEGER sum of 16-bit quantised lumas -- exact, so the atomics on the counter give the same
//                              bits whatever the order;
//   strong_view_kernel         one 64 x 32 tile of one image per workgroup: the tile and its blur halo are read once into
//                              LDS, the pointwise steps run there in place, the separable blur goes channel by channel
//                              through a second LDS plane (horizontal, then vertical), and the tile is written once --
//                              re-normalised, or the uniform fill inside a rectangle.
//
// The draws happen on the host (datasets/strong_view.py); the kernels receive per-image tables.  Every float32 step is
// one IEEE operation in the documented order (-ffp-contract=off, correctly rounded divide), only + - * / min max: bit-identical
// to the numpy restatement in tests/strong_view_oracle.py.  Rows are contiguous float32: global loads and stores take 16
// bytes where the four elements are 16-byte aligned IN MEMORY and inside the span, single elements at the heads and tails
// (W is arbitrary and a tensor may start 4 bytes off a 16-byte boundary, so the grouping is decided per row).
#include "common.h"
#include "philox.h"

namespace cnuda {
namespace {

constexpr int kSvThreads = 256;
constexpr int kSvMaxRadius = 6;
constexpr int kSvTaps = 2 * kSvMaxRadius + 1;
constexpr int kSvTW = 64, kSvTH = 32;                                   // the output tile
constexpr int kSvAW = kSvTW + 2 * kSvMaxRadius, kSvAH = kSvTH + 2 * kSvMaxRadius;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float luma(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }
__device__ __forceinline__ float denormalise(float x, float mean, float std) { return clamp01(x * std + mean); }

// ---------------------------------------------------------------------------------------------------------------------
// pivot
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long quantised_luma(float r, float g, float b, const float mean[3],
                                                              const float std[3]) {
    const float l = luma(denormalise(r, mean[0], std[0]), denormalise(g, mean[1], std[1]),
                         denormalise(b, mean[2], std[2]));
    return (unsigned long long)(unsigned)rintf(l * 65536.0f);
}

// x [B, 3, HW]; work [B, 2] u64, zero on entry: (sum of the quantised lumas, workgroups done); pivot [B].  `bpi`
// workgroups per image; the one that takes the last ticket of its image turns the sum into the pivot.
__global__ __launch_bounds__(kSvThreads) void strong_view_pivot_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ mean3,
                                                                       const float* __restrict__ std3,
                                                                       unsigned long long* __restrict__ work,
                                                                       float* __restrict__ pivot, long long HW, int bpi) {
    __shared__ unsigned long long red[kSvThreads / kWave];
    const int b = blockIdx.x / bpi, blk = blockIdx.x % bpi;
    const float mean[3] = {mean3[0], mean3[1], mean3[2]}, std[3] = {std3[0], std3[1], std3[2]};
    const float* r = x + (long long)b * 3 * HW;
    const float* g = r + HW;
    const float* bl = g + HW;
    const long long step = (long long)bpi * kSvThreads, first = (long long)blk * kSvThreads + threadIdx.x;
    unsigned long long sum = 0;
    if ((((uintptr_t)r) & 15) == 0 && (HW & 3) == 0) {                    // the three planes start on 16 bytes
        for (long long q = first; q < HW / 4; q += step) {
            const float4 a = *reinterpret_cast<const float4*>(r + 4 * q);
            const float4 c = *reinterpret_cast<const float4*>(g + 4 * q);
            const float4 d = *reinterpret_cast<const float4*>(bl + 4 * q);
            sum += quantised_luma(a.x, c.x, d.x, mean, std) + quantised_luma(a.y, c.y, d.y, mean, std)
                   + quantised_luma(a.z, c.z, d.z, mean, std) + quantised_luma(a.w, c.w, d.w, mean, std);
        }
    } else {
        for (long long p = first; p < HW; p += step) sum += quantised_luma(r[p], g[p], bl[p], mean, std);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < kSvThreads / kWave; ++w) total += red[w];
        atomicAdd(&work[2 * b], total);
        __threadfence();
        if (atomicAdd(&work[2 * b + 1], 1ull) == (unsigned long long)(bpi - 1)) {
            __threadfence();
            const unsigned long long all = atomicAdd(&work[2 * b], 0ull);
            pivot[b] = (float)((double)all / (65536.0 * (double)HW));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the view
// ---------------------------------------------------------------------------------------------------------------------
// The elements [lo, hi) of a row whose element 0 is `row`, cut into groups of four that are 16-byte aligned in memory:
// group g starts at element lo - mis + 4 g, mis = the row's element `lo` counted from the 16-byte boundary below it.
__device__ __forceinline__ int row_misalignment(const float* at) { return (int)(((uintptr_t)at >> 2) & 3); }
__host__ __device__ __forceinline__ int row_groups(int span) { return (span + 3) / 4 + 1; }

// x, y [B, 3, H, W]; mean3, std3 [3]; photo [B, 4] (brightness, contrast, saturation, gray flag); taps [B, 13] with
// radius [B] (clamped to 0..max_radius here: it bounds every LDS address); rects [B, 3, 4] (x0, y0, x1, y1) half-open;
// ids [B]; pivot [B], read only for images with contrast != 1.  blockIdx.x = (image, tile row, tile column).
__global__ __launch_bounds__(kSvThreads) void strong_view_kernel(
    const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mean3, const float* __restrict__ std3,
    const float* __restrict__ photo, const float* __restrict__ taps, const int* __restrict__ radius,
    const int* __restrict__ rects, const long long* __restrict__ ids, unsigned long long seed,
    const float* __restrict__ pivot, int H, int W, int tiles_x, int tiles_y, int max_radius) {
    __shared__ float A[3][kSvAH][kSvAW];          // the tile and its halo: raw, then after the pointwise steps, then blurred
    __shared__ float Hs[kSvAH][kSvTW];            // one channel after the horizontal pass
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int R = min(max(radius[b], 0), max_radius);
    const float fb = photo[4 * b], fc = photo[4 * b + 1], fs = photo[4 * b + 2];
    const bool gray = photo[4 * b + 3] != 0.0f;
    const bool neutral = fb == 1.0f && fc == 1.0f && fs == 1.0f && !gray && R == 0;
    const float mean[3] = {mean3[0], mean3[1], mean3[2]}, std[3] = {std3[0], std3[1], std3[2]};
    // the tile [y0, y1) x [x0, x1), the part of the image it needs [ys, ye) x [xs, xe), and the image coordinates
    // (oy, ox) of A[.][0][0]
    const int x0 = tx * kSvTW, x1 = min(x0 + kSvTW, W), y0 = ty * kSvTH, y1 = min(y0 + kSvTH, H);
    const int xs = max(x0 - R, 0), xe = min(x1 + R, W), ys = max(y0 - R, 0), ye = min(y1 + R, H);
    const int ox = x0 - R, oy = y0 - R;
    const int span = xe - xs, rows = ye - ys, tw = x1 - x0, th = y1 - y0;
    const long long HW = (long long)H * W;
    const float* xb = x + (long long)b * 3 * HW;
    float* yb = y + (long long)b * 3 * HW;

    // 1. the needed part of the image, as it is, into A
    {
        const int ng = row_groups(span), per = ng * rows;
        for (int it = tid; it < 3 * per; it += kSvThreads) {
            const int c = it / per, rr = (it - c * per) / ng, g = it - c * per - rr * ng;
            const float* row = xb + c * HW + (long long)(ys + rr) * W;
            float* dst = &A[c][ys + rr - oy][0];
            const int cs = xs - row_misalignment(row + xs) + 4 * g;
            if (cs >= xs && cs + 4 <= xe) {
                const float4 v = *reinterpret_cast<const float4*>(row + cs);
                dst[cs - ox] = v.x, dst[cs + 1 - ox] = v.y, dst[cs + 2 - ox] = v.z, dst[cs + 3 - ox] = v.w;
            } else {
                for (int j = 0; j < 4; ++j)
                    if (cs + j >= xs && cs + j < xe) dst[cs + j - ox] = row[cs + j];
            }
        }
    }
    __syncthreads();

    if (!neutral) {
        // 2. the pointwise steps, in place; a factor of exactly 1 skips its step (contrast = 1: the pivot is never read)
        const float m = fc != 1.0f ? pivot[b] : 0.0f;
        for (int it = tid; it < rows * span; it += kSvThreads) {
            const int rr = it / span, at = it - rr * span + xs - ox, ar = ys + rr - oy;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = denormalise(A[c][ar][at], mean[c], std[c]);
            if (fb != 1.0f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = fminf(v[c] * fb, 1.0f);
            }
            if (fc != 1.0f) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = clamp01((v[c] - m) * fc + m);
            }
            if (fs != 1.0f) {
                const float g = luma(v[0], v[1], v[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = clamp01((v[c] - g) * fs + g);
            }
            if (gray) v[0] = v[1] = v[2] = luma(v[0], v[1], v[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) A[c][ar][at] = v[c];
        }
        __syncthreads();

        // 3. the blur, channel by channel: rows of A -> Hs (neighbour columns clamped to the image), Hs -> the tile's
        // part of A (neighbour rows clamped to the image: the pass over a replicated row is that row's own pass)
        if (R > 0) {
            const float* w = taps + kSvTaps * b;
            for (int c = 0; c < 3; ++c) {
                for (int it = tid; it < rows * tw; it += kSvThreads) {
                    const int rr = it / tw, col = x0 + it - rr * tw;
                    const float* src = &A[c][ys + rr - oy][0];
                    float acc = 0.0f;
                    for (int k = 0; k <= 2 * R; ++k) acc = acc + w[k] * src[min(max(col + k - R, 0), W - 1) - ox];
                    Hs[ys + rr - oy][col - x0] = acc;
                }
                __syncthreads();
                for (int it = tid; it < th * tw; it += kSvThreads) {
                    const int rr = it / tw, cc = it - rr * tw, row = y0 + rr;
                    float acc = 0.0f;
                    for (int k = 0; k <= 2 * R; ++k) acc = acc + w[k] * Hs[min(max(row + k - R, 0), H - 1) - oy][cc];
                    A[c][row - oy][x0 + cc - ox] = acc;
                }
                __syncthreads();
            }
        }
    }

    // 4. the tile out: re-normalised (a neutral image: its own bits), or the fill inside a non-empty rectangle
    int rc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) rc[i] = rects[12 * b + i];
    const long long id = ids[b];
    const int ng = row_groups(tw), per = ng * th;
    for (int it = tid; it < 3 * per; it += kSvThreads) {
        const int c = it / per, rr = (it - c * per) / ng, g = it - c * per - rr * ng;
        const int row = y0 + rr;
        float* out = yb + c * HW + (long long)row * W;
        const float* src = &A[c][row - oy][0];
        const int cs = x0 - row_misalignment(out + x0) + 4 * g;
        const float mc = c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]);
        const float sc = c == 0 ? std[0] : (c == 1 ? std[1] : std[2]);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = cs + j;
            v[j] = 0.0f;
            if (col < x0 || col >= x1) continue;
            bool inside = false;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                inside = inside || (col >= rc[4 * q] && col < rc[4 * q + 2] && row >= rc[4 * q + 1] && row < rc[4 * q + 3]);
            if (inside) {
                uint32_t word[4];
                philox_pixel_block(seed, id, (long long)row * W + col, word);
                v[j] = (philox_uniform(c == 0 ? word[0] : (c == 1 ? word[1] : word[2])) * 2.0f - 1.0f) * 1.7320508f;
            } else {
                const float a = src[col - ox];
                v[j] = neutral ? a : (a - mc) / sc;
            }
        }
        if (cs >= x0 && cs + 4 <= x1) {
            *reinterpret_cast<float4*>(out + cs) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cs + j >= x0 && cs + j < x1) out[cs + j] = v[j];
        }
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_strong_view_pivot(const float* x, const float* mean, const float* std, float* pivot, void* workspace,
                                       int B, int H, int W, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && mean && std && pivot && workspace, "cnuda_strong_view_pivot: null pointer");
    CNUDA_REQUIRE(B > 0 && H > 0 && W > 0, "cnuda_strong_view_pivot: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    CNUDA_REQUIRE((((uintptr_t)x | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)pivot) & 3) == 0
                      && ((uintptr_t)workspace & 7) == 0,
                  "cnuda_strong_view_pivot: arrays must be aligned to their element size (the workspace to 8 bytes)");
    const long long HW = (long long)H * W;
    // 16 pixels per thread and pass; at most 256 workgroups per image
    long long bpi = (HW + 16 * kSvThreads - 1) / (16 * kSvThreads);
    bpi = bpi > 256 ? 256 : bpi;
    CNUDA_REQUIRE(bpi * B < (1ll << 31), "cnuda_strong_view_pivot: batch too large (B=%d)", B);
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(workspace, 0, 16 * (size_t)B, st);
    if (e != hipSuccess) {
        set_error("cnuda_strong_view_pivot: %s", hipGetErrorString(e));
        return (int)e;
    }
    CNUDA_LAUNCH(strong_view_pivot_kernel, dim3((unsigned)(bpi * B)), dim3(kSvThreads), 0, st, x, mean, std,
                 static_cast<unsigned long long*>(workspace), pivot, HW, (int)bpi);
    return check_launch("cnuda_strong_view_pivot");
}

extern "C" int cnuda_strong_view(const float* x, float* y, const float* mean, const float* std, const float* photo,
                                 const float* taps, const int* radius, int max_radius, const int* rects,
                                 const long long* ids, unsigned long long seed, const float* pivot, int B, int H, int W,
                                 cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && mean && std && photo && taps && radius && rects && ids && pivot,
                  "cnuda_strong_view: null pointer");
    CNUDA_REQUIRE(B > 0 && H > 0 && W > 0, "cnuda_strong_view: bad sizes (B=%d, H=%d, W=%d)", B, H, W);
    CNUDA_REQUIRE(max_radius >= 0 && max_radius <= kSvMaxRadius, "cnuda_strong_view: radius %d outside 0..%d", max_radius,
                  kSvMaxRadius);
    const long long total = (long long)B * 3 * H * W;
    CNUDA_REQUIRE(!(x < y + total && y < x + total), "cnuda_strong_view: x and y overlap");
    CNUDA_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)photo | (uintptr_t)taps
                    | (uintptr_t)radius | (uintptr_t)rects | (uintptr_t)pivot) & 3) == 0 && ((uintptr_t)ids & 7) == 0,
                  "cnuda_strong_view: arrays must be aligned to their element size");
    const int tiles_x = ceil_div(W, kSvTW), tiles_y = ceil_div(H, kSvTH);
    const long long tiles = (long long)tiles_x * tiles_y * B;
    CNUDA_REQUIRE(tiles < (1ll << 31), "cnuda_strong_view: batch too large (%lld tiles)", tiles);
    CNUDA_LAUNCH(strong_view_kernel, dim3((unsigned)tiles), dim3(kSvThreads), 0, (hipStream_t)stream, x, y, mean, std,
                 photo, taps, radius, rects, ids, seed, pivot, H, W, tiles_x, tiles_y, max_radius);
    return check_launch("cnuda_strong_view");
}
