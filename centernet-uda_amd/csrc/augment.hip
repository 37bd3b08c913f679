// Image augmentation and resizing on the GPU ("Augmentation on the device"): what the reference's imgaug
// chain does per image on the host (datasets/coco.py:140-158 with configs/defaults.yaml:38-60), restated as
//   augment_color_kernel   grayscale blend, hue rotation and brightness shift, pointwise on the source image;
//   augment_warp_kernel    ONE resampling per image: motion-blur taps around the inverse-mapped sample point, bilinear
//                          with replicated edges, plus white gaussian noise at output resolution;
//   augment_points_kernel  the forward matrix applied to keypoints and box corners in float64.
// The random draws and the matrix composition happen on the host (datasets/augment.py); the kernels receive per-image
// parameter tables.  Every float32 step is one IEEE operation in the documented order (the build has
// -ffp-contract=off and hipcc's correctly rounded fp32 divide), so colour and warp are bit-identical to the numpy
// restatement in tests/augment_oracle.py.  The gather is byte-granular and lives on L2; no rate is claimed for it.
#include "common.h"
#include "philox.h"

namespace cnuda {
namespace {

constexpr int kMaxTaps = 10;

// ---------------------------------------------------------------------------------------------------------------------
// colour
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wrap6(float k) { return k - 6.0f * floorf(k / 6.0f); }

__device__ __forceinline__ float hsv_channel(float n, float h, float v, float vs) {
    const float k = wrap6(n + h);
    const float t = fminf(fmaxf(fminf(k, 4.0f - k), 0.0f), 1.0f);
    return v - vs * t;
}

__device__ __forceinline__ unsigned to_byte(float x) { return (unsigned)fminf(fmaxf(rintf(x), 0.0f), 255.0f); }

// (alpha, hue in degrees, brightness add) on one pixel: grayscale blend, RGB -> HSV in sextants, hue rotation, V shift,
// HSV -> RGB.  Only + - * / floor min max: neutral parameters return the input bytes.
__device__ __forceinline__ void color_pixel(unsigned r8, unsigned g8, unsigned b8, float alpha, float hue, float add,
                                            unsigned out[3]) {
    float r = (float)r8, g = (float)g8, b = (float)b8;
    const float gray = (0.299f * r + 0.587f * g) + 0.114f * b;
    const float keep = 1.0f - alpha;
    r = keep * r + alpha * gray;
    g = keep * g + alpha * gray;
    b = keep * b + alpha * gray;
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    const float c = mx - mn;
    const float safe = c > 0.0f ? c : 1.0f;
    float h = mx == r ? (g - b) / safe : (mx == g ? (b - r) / safe + 2.0f : (r - g) / safe + 4.0f);
    h = c > 0.0f ? h : 0.0f;
    h = wrap6(h + hue / 60.0f);
    const float s = mx > 0.0f ? c / mx : 0.0f;
    const float v = fminf(fmaxf(mx + add, 0.0f), 255.0f);
    const float vs = v * s;
    out[0] = to_byte(hsv_channel(5.0f, h, v, vs));
    out[1] = to_byte(hsv_channel(3.0f, h, v, vs));
    out[2] = to_byte(hsv_channel(1.0f, h, v, vs));
}

// src, dst: [B, H, W, 3] uint8; color: [B, 3] (alpha, hue degrees, add).  Four pixels = three dwords per thread over
// the flattened pixel axis, like prepare_input_kernel; a group may straddle two images, so the parameters are looked up
// per pixel.  The up to three pixels after the last whole group go one per thread.
__global__ __launch_bounds__(256) void augment_color_kernel(const unsigned char* __restrict__ src,
                                                            unsigned char* __restrict__ dst,
                                                            const float* __restrict__ color, long long HW,
                                                            long long N) {
    const long long groups = N / 4, step = (long long)gridDim.x * blockDim.x;
    const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst);
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += step) {
        const uint32_t d0 = src4[3 * g], d1 = src4[3 * g + 1], d2 = src4[3 * g + 2];
        // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
        const unsigned c0[4] = {d0 & 255u, d0 >> 24, (d1 >> 16) & 255u, (d2 >> 8) & 255u};
        const unsigned c1[4] = {(d0 >> 8) & 255u, d1 & 255u, d1 >> 24, (d2 >> 16) & 255u};
        const unsigned c2[4] = {(d0 >> 16) & 255u, (d1 >> 8) & 255u, d2 & 255u, d2 >> 24};
        unsigned o[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long long b = (4 * g + p) / HW;
            const float alpha = color[3 * b], hue = color[3 * b + 1], add = color[3 * b + 2];
            if (alpha == 0.0f && hue == 0.0f && add == 0.0f) {
                o[p][0] = c0[p], o[p][1] = c1[p], o[p][2] = c2[p];
            } else {
                color_pixel(c0[p], c1[p], c2[p], alpha, hue, add, o[p]);
            }
        }
        dst4[3 * g] = o[0][0] | (o[0][1] << 8) | (o[0][2] << 16) | (o[1][0] << 24);
        dst4[3 * g + 1] = o[1][1] | (o[1][2] << 8) | (o[2][0] << 16) | (o[2][1] << 24);
        dst4[3 * g + 2] = o[2][2] | (o[3][0] << 8) | (o[3][1] << 16) | (o[3][2] << 24);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(N - 4 * groups)) {
        const long long n = 4 * groups + threadIdx.x, b = n / HW;
        unsigned o[3];
        color_pixel(src[3 * n], src[3 * n + 1], src[3 * n + 2], color[3 * b], color[3 * b + 1], color[3 * b + 2], o);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[3 * n + c] = (unsigned char)o[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// noise: Philox4x32-10 (philox.h), key = the 64-bit seed, counter = (pixel index, image id)
// ---------------------------------------------------------------------------------------------------------------------
// one standard normal deviate per (seed, image id, pixel): Box-Muller on two 23-bit uniforms in (0, 1)
__device__ __forceinline__ float normal_deviate(unsigned long long seed, long long id, long long pixel) {
    uint32_t c[4];
    philox_pixel_block(seed, id, pixel, c);
    const float u1 = philox_uniform(c[0]), u2 = philox_uniform(c[1]);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// ---------------------------------------------------------------------------------------------------------------------
// warp
// ---------------------------------------------------------------------------------------------------------------------
// bilinear sample at pixel-index position (pu, pv) of one image (valid size hs x ws, row pitch in bytes), neighbour
// indices clamped to the image
__device__ __forceinline__ void bilinear(const unsigned char* __restrict__ img, long long pitch, int hs, int ws, float pu,
                                         float pv, float s[3]) {
    const float x0 = floorf(pu), y0 = floorf(pv);
    const float fx = pu - x0, fy = pv - y0;
    const float xm = (float)(ws - 1), ym = (float)(hs - 1);
    const int xa = (int)fminf(fmaxf(x0, 0.0f), xm), xb = (int)fminf(fmaxf(x0 + 1.0f, 0.0f), xm);
    const int ya = (int)fminf(fmaxf(y0, 0.0f), ym), yb = (int)fminf(fmaxf(y0 + 1.0f, 0.0f), ym);
    const unsigned char* ra = img + ya * pitch;
    const unsigned char* rb = img + yb * pitch;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = gx * (float)ra[3 * xa + c] + fx * (float)ra[3 * xb + c];
        const float bot = gx * (float)rb[3 * xa + c] + fx * (float)rb[3 * xb + c];
        s[c] = gy * top + fy * bot;
    }
}

// src [B, Hmax, Wmax, 3] uint8 with valid sizes [B, 2] (h, w); inverse [B, 6]; taps [B, 10, 3] (ox, oy, weight) with
// ntaps [B]; noise [B] standard deviations; ids [B] the images' noise counters; dst [B, Hin, Win, 3] uint8.  A thread
// produces four consecutive pixels of one output row (fewer at the row's end) and stores them as three dwords when
// the run is whole and starts on a dword, byte by byte otherwise.
__global__ __launch_bounds__(256) void augment_warp_kernel(const unsigned char* __restrict__ src,
                                                           unsigned char* __restrict__ dst,
                                                           const int* __restrict__ sizes,
                                                           const float* __restrict__ inverse,
                                                           const float* __restrict__ taps,
                                                           const int* __restrict__ ntaps,
                                                           const float* __restrict__ noise,
                                                           const long long* __restrict__ ids,
                                                           unsigned long long seed, int B, int Hmax, int Wmax, int Hin,
                                                           int Win) {
    const int runs = (Win + 3) / 4;
    const long long total = (long long)B * Hin * runs, step = (long long)gridDim.x * blockDim.x;
    const long long pitch = (long long)Wmax * 3;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const int r = (int)(t % runs);
        const long long row = t / runs;
        const int i = (int)(row % Hin), b = (int)(row / Hin);
        const int j0 = 4 * r, n = min(4, Win - j0);
        // the valid size and the tap count bound every address below: clamp what the tables say
        const int hs = min(max(sizes[2 * b], 1), Hmax), ws = min(max(sizes[2 * b + 1], 1), Wmax);
        const int k = min(max(ntaps[b], 0), kMaxTaps);
        const float* a = inverse + 6 * b;
        const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
        const float* tp = taps + 3 * kMaxTaps * b;
        const float sigma = noise[b];
        const long long id = ids ? ids[b] : (long long)b;
        const unsigned char* img = src + (long long)b * Hmax * pitch;
        const float y = (float)i + 0.5f;
        unsigned o[4][3];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            o[p][0] = o[p][1] = o[p][2] = 0u;
            if (p >= n) continue;
            const int j = j0 + p;
            const float x = (float)j + 0.5f;
            const float u = (a0 * x + a1 * y) + a2, v = (a3 * x + a4 * y) + a5;
            if (!(u >= 0.0f && u <= (float)ws && v >= 0.0f && v <= (float)hs)) continue;      // outside (or NaN): 0
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (int m = 0; m < k; ++m) {
                const float ox = tp[3 * m], oy = tp[3 * m + 1], w = tp[3 * m + 2];
                float s[3];
                bilinear(img, pitch, hs, ws, (u + ox) - 0.5f, (v + oy) - 0.5f, s);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * s[c];
            }
            float e = 0.0f;
            if (sigma > 0.0f) e = sigma * normal_deviate(seed, id, (long long)i * Win + j);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[p][c] = to_byte(acc[c] + e);
        }
        const long long base = (row * Win + j0) * 3;
        if (n == 4 && (base & 3) == 0) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + base);
            d4[0] = o[0][0] | (o[0][1] << 8) | (o[0][2] << 16) | (o[1][0] << 24);
            d4[1] = o[1][1] | (o[1][2] << 8) | (o[2][0] << 16) | (o[2][1] << 24);
            d4[2] = o[2][2] | (o[3][0] << 8) | (o[3][1] << 16) | (o[3][2] << 24);
        } else {
            for (int p = 0; p < n; ++p)
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[base + 3 * p + c] = (unsigned char)o[p][c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// points and boxes
// ---------------------------------------------------------------------------------------------------------------------
// forward [B, 6] double; points [B, N, 2] -> (m0 u + m1 v) + m2, (m3 u + m4 v) + m5; boxes [B, M, 4] (x1, y1, x2, y2) ->
// the bounding box of the four mapped corners.  One thread per point or box.
__global__ __launch_bounds__(256) void augment_points_kernel(const double* __restrict__ forward,
                                                             const double* __restrict__ points,
                                                             double* __restrict__ points_out, int N,
                                                             const double* __restrict__ boxes,
                                                             double* __restrict__ boxes_out, int M, int B) {
    const long long per = (long long)N + M, total = per * B, step = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const long long b = t / per, e = t - b * per;
        const double* m = forward + 6 * b;
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        if (e < N) {
            const long long at = (b * N + e) * 2;
            const double u = points[at], v = points[at + 1];
            points_out[at] = (m0 * u + m1 * v) + m2;
            points_out[at + 1] = (m3 * u + m4 * v) + m5;
        } else {
            const long long at = (b * M + (e - N)) * 4;
            const double x1 = boxes[at], y1 = boxes[at + 1], x2 = boxes[at + 2], y2 = boxes[at + 3];
            const double cx[4] = {x1, x2, x2, x1}, cy[4] = {y1, y1, y2, y2};
            double lox = 0, loy = 0, hix = 0, hiy = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double px = (m0 * cx[c] + m1 * cy[c]) + m2, py = (m3 * cx[c] + m4 * cy[c]) + m5;
                lox = c ? fmin(lox, px) : px, hix = c ? fmax(hix, px) : px;
                loy = c ? fmin(loy, py) : py, hiy = c ? fmax(hiy, py) : py;
            }
            boxes_out[at] = lox, boxes_out[at + 1] = loy, boxes_out[at + 2] = hix, boxes_out[at + 3] = hiy;
        }
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_augment_color(const unsigned char* src, unsigned char* dst, const float* color, int B, int H,
                                   int W, cnuda_stream_t stream) {
    CNUDA_REQUIRE(src && dst && color, "cnuda_augment_color: null pointer");
    CNUDA_REQUIRE(src != dst, "cnuda_augment_color: src and dst must be different buffers");
    CNUDA_REQUIRE(B > 0 && H > 0 && W > 0, "cnuda_augment_color: bad sizes");
    CNUDA_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)color & 3) == 0,
                  "cnuda_augment_color: src, dst and color must be 4-byte aligned");
    const long long HW = (long long)H * W, N = HW * B;
    hipStream_t st = (hipStream_t)stream;
    CNUDA_LAUNCH(augment_color_kernel, dim3(stream_grid(N / 4, 256)), dim3(256), 0, st, src, dst, color, HW, N);
    return check_launch("cnuda_augment_color");
}

extern "C" int cnuda_augment_warp(const unsigned char* src, unsigned char* dst, const int* sizes,
                                  const float* inverse, const float* taps, const int* ntaps, const float* noise,
                                  const long long* ids, unsigned long long seed, int B, int Hmax, int Wmax, int Hin,
                                  int Win, cnuda_stream_t stream) {
    CNUDA_REQUIRE(src && dst && sizes && inverse && taps && ntaps && noise, "cnuda_augment_warp: null pointer");
    CNUDA_REQUIRE(B > 0 && Hmax > 0 && Wmax > 0 && Hin > 0 && Win > 0, "cnuda_augment_warp: bad sizes");
    CNUDA_REQUIRE((long long)Hmax * Wmax < (1ll << 40) && (long long)Hin * Win < (1ll << 40),
                  "cnuda_augment_warp: image too large");
    CNUDA_REQUIRE(((uintptr_t)dst & 3) == 0, "cnuda_augment_warp: dst must be 4-byte aligned");
    CNUDA_REQUIRE((((uintptr_t)sizes | (uintptr_t)inverse | (uintptr_t)taps | (uintptr_t)ntaps | (uintptr_t)noise) & 3) == 0
                      && ((uintptr_t)ids & 7) == 0,
                  "cnuda_augment_warp: parameter tables must be aligned to their element size");
    const long long work = (long long)B * Hin * ((Win + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
    CNUDA_LAUNCH(augment_warp_kernel, dim3(stream_grid(work, 256)), dim3(256), 0, st, src, dst, sizes, inverse, taps,
                 ntaps, noise, ids, seed, B, Hmax, Wmax, Hin, Win);
    return check_launch("cnuda_augment_warp");
}

extern "C" int cnuda_augment_points(const double* forward, const double* points, double* points_out, int N,
                                    const double* boxes, double* boxes_out, int M, int B, cnuda_stream_t stream) {
    CNUDA_REQUIRE(forward, "cnuda_augment_points: null pointer");
    CNUDA_REQUIRE(B > 0 && N >= 0 && M >= 0 && N + (long long)M > 0, "cnuda_augment_points: bad sizes");
    CNUDA_REQUIRE(N == 0 || (points && points_out), "cnuda_augment_points: N > 0 needs points and points_out");
    CNUDA_REQUIRE(M == 0 || (boxes && boxes_out), "cnuda_augment_points: M > 0 needs boxes and boxes_out");
    CNUDA_REQUIRE((((uintptr_t)forward | (uintptr_t)points | (uintptr_t)points_out | (uintptr_t)boxes
                    | (uintptr_t)boxes_out) & 7) == 0, "cnuda_augment_points: arrays must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    CNUDA_LAUNCH(augment_points_kernel, dim3(stream_grid(((long long)N + M) * B, 256)), dim3(256), 0, st, forward,
                 points, points_out, N, boxes, boxes_out, M, B);
    return check_launch("cnuda_augment_points");
}
