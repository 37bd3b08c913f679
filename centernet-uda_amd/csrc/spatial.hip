// HBM-bound spatial / elementwise kernels (NCHW fp32).  Of the DLA-34 graph:
//   max-pool k=s (Tree.downsample, backends/dla.py:202-203), depthwise
//   ConvTranspose2d k=2f s=f p=f/2 (IDAUp.up, dla.py:385-388), channel
//   concat / slice (Root, dla.py:162), elementwise add (IDAUp, dla.py:399),
//   ReLU / LeakyReLU gradients, and the offset|mask split + sigmoid of
//   DCN.forward (libs/DCNv2/dcn_v2.py:119-122).
// Of the other trunks: the windowed max-pool (ResNet stem) and the depthwise convolution, 3x3 / 5x5, with symmetric
//   padding (MobileNetV2) or TensorFlow "SAME" padding (EfficientNet's MBConv): one kernel family for both.
#include "common.h"

namespace cnuda {
namespace {

constexpr int kT = 256;

// ---- the pieces the kernels below share --------------------------------------------
// grid-stride walk of [first, total) along x, 64-bit
#define FOR_EACH_INDEX_FROM(i, first, total)                                                        \
    for (long long i = (first) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (total); \
         i += (long long)gridDim.x * blockDim.x)
#define FOR_EACH_INDEX(i, total) FOR_EACH_INDEX_FROM(i, 0, total)
// i = (plane * H + y) * W + x
struct PlaneYX {
    long long plane;
    int y, x;
};
__device__ __forceinline__ PlaneYX plane_yx(long long i, int H, int W) {
    return {i / ((long long)W * H), (int)((i / W) % H), (int)(i % W)};
}
// the max-pool rule of every scan below: first maximum wins, NaN propagates (ATen's rule)
__device__ __forceinline__ bool pool_take(float v, float m) { return v > m || v != v; }
// a channel's n weights into LDS
__device__ __forceinline__ void stage_weights(float* ws, const float* __restrict__ w, int c, int n) {
    for (int i = threadIdx.x; i < n; i += kT) ws[i] = w[(size_t)c * n + i];
    __syncthreads();
}

// ---- max pool, window k x k, stride k, no padding ---------------------------------
// the window at src (rows W apart), scanned (dy, dx) ascending -> the arg-max as dy * W + dx, its value in m
__device__ __forceinline__ int pool_scan(const float* __restrict__ src, int W, int k, float& m) {
    int arg = 0;
    m = src[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const float v = src[dy * W + dx];
            if (pool_take(v, m)) { m = v; arg = dy * W + dx; }
        }
    return arg;
}
__global__ void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long planes, int H, int W,
                                   int Ho, int Wo, int k) {
    FOR_EACH_INDEX(i, planes * Ho * Wo) {
        const PlaneYX o = plane_yx(i, Ho, Wo);
        float m;
        pool_scan(x + (size_t)o.plane * H * W + (size_t)(o.y * k) * W + o.x * k, W, k, m);
        y[i] = m;
    }
}
// gx is written completely (zeros where not the arg-max); one thread per output cell
// accumulate: gx already holds another consumer's share of x's gradient -- only the arg-max cell is touched (+= g)
__global__ void maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx,
                                   long long planes, int H, int W, int Ho, int Wo, int k, int accumulate) {
    FOR_EACH_INDEX(i, planes * Ho * Wo) {
        const PlaneYX o = plane_yx(i, Ho, Wo);
        const size_t base = (size_t)o.plane * H * W + (size_t)(o.y * k) * W + o.x * k;
        float m;
        const int arg = pool_scan(x + base, W, k, m);
        const float g = gy[i];
        if (accumulate) {
            gx[base + arg] += g;
            continue;
        }
        for (int dy = 0; dy < k; ++dy)
            for (int dx = 0; dx < k; ++dx) gx[base + dy * W + dx] = (dy * W + dx == arg) ? g : 0.0f;
    }
}
// The 2 x 2 pools of DLA-34 (Tree.downsample: every level's input, 134 MB at 128 x 128 x 64 x 32) with 16-byte accesses: a
// thread owns TWO neighbouring windows -- one float4 of each of the two input rows -- instead of four 4-byte loads per window
// at an 8-byte lane stride (round 6: 1.6 -> 4+ TB/s).  W % 4 == 0, H even, 16-byte aligned tensors.  Same scan order and
// NaN rule as the scalar kernels: (0,0), (0,1), (1,0), (1,1), first maximum wins, NaN propagates.
__device__ __forceinline__ void pool2_pick(float a, float b, float c, float d, float& m, int& arg) {
    m = a; arg = 0;
    if (pool_take(b, m)) { m = b; arg = 1; }
    if (pool_take(c, m)) { m = c; arg = 2; }
    if (pool_take(d, m)) { m = d; arg = 3; }
}
// window pair i of `total` -> its (plane, output row) flattened, the pair's place q in the row of Wq: input rows 2 row and
// 2 row + 1.  32-bit division where the index allows (always, in DLA-34)
__device__ __forceinline__ long long pool2_row(long long i, long long total, int Wq, int& q) {
    const long long row = total < (1ll << 32) ? (long long)((unsigned)i / (unsigned)Wq) : i / Wq;
    q = (int)(i - row * Wq);
    return row;
}
__global__ void maxpool2_fwd_vec_kernel(const float4* __restrict__ x, float2* __restrict__ y, long long total /* planes * Ho * Wo / 2 */,
                                        int Wq /* W / 4 */) {
    FOR_EACH_INDEX(i, total) {
        int q;
        const long long row = pool2_row(i, total, Wq, q);
        const float4 r0 = x[(2 * row) * Wq + q], r1 = x[(2 * row + 1) * Wq + q];
        float m0, m1;
        int a0, a1;
        pool2_pick(r0.x, r0.y, r1.x, r1.y, m0, a0);
        pool2_pick(r0.z, r0.w, r1.z, r1.w, m1, a1);
        y[i] = make_float2(m0, m1);
    }
}
__global__ void maxpool2_bwd_vec_kernel(const float4* __restrict__ x, const float2* __restrict__ gy, float4* __restrict__ gx,
                                        long long total, int Wq, int accumulate) {
    FOR_EACH_INDEX(i, total) {
        int q;
        const long long row = pool2_row(i, total, Wq, q);
        const long long i0 = (2 * row) * Wq + q, i1 = (2 * row + 1) * Wq + q;
        const float4 r0 = x[i0], r1 = x[i1];
        const float2 g = gy[i];
        float m;
        int a0, a1;
        pool2_pick(r0.x, r0.y, r1.x, r1.y, m, a0);
        pool2_pick(r0.z, r0.w, r1.z, r1.w, m, a1);
        float4 o0 = make_float4(a0 == 0 ? g.x : 0.0f, a0 == 1 ? g.x : 0.0f, a1 == 0 ? g.y : 0.0f, a1 == 1 ? g.y : 0.0f);
        float4 o1 = make_float4(a0 == 2 ? g.x : 0.0f, a0 == 3 ? g.x : 0.0f, a1 == 2 ? g.y : 0.0f, a1 == 3 ? g.y : 0.0f);
        if (accumulate) {          // (gx holds another consumer's share: only the arg-max cells change)
            const float4 c0 = gx[i0], c1 = gx[i1];
            o0 = make_float4(a0 == 0 ? c0.x + g.x : c0.x, a0 == 1 ? c0.y + g.x : c0.y, a1 == 0 ? c0.z + g.y : c0.z, a1 == 1 ? c0.w + g.y : c0.w);
            o1 = make_float4(a0 == 2 ? c1.x + g.x : c1.x, a0 == 3 ? c1.y + g.x : c1.y, a1 == 2 ? c1.z + g.y : c1.z, a1 == 3 ? c1.w + g.y : c1.w);
        }
        gx[i0] = o0;
        gx[i1] = o1;
    }
}
inline bool pool2_vec_ok(const void* a, const void* b, const void* c, int H, int W, int k) {
    return k == 2 && (W & 3) == 0 && (H & 1) == 0 && aligned16(a, b, c);
}

// rows/cols of x not covered by any window (H % k != 0) get zero gradient
__global__ void maxpool_bwd_tail_kernel(float* __restrict__ gx, long long planes, int H, int W, int Hc, int Wc) {
    FOR_EACH_INDEX(i, planes * H * W) {
        const PlaneYX at = plane_yx(i, H, W);
        if (at.y >= Hc || at.x >= Wc) gx[i] = 0.0f;
    }
}

// ---- max pool, window k x k, stride s, padding p (-inf): torchvision resnet stem pool k3 s2 p1
//      (backends/resnet.py:27-30 keeps it in `base`) --------------------------------------------
__device__ __forceinline__ int window_argmax(const float* __restrict__ src, int H, int W, int oy, int ox, int k, int s,
                                             int p, float& m) {
    // scan order (dy, dx) ascending, first maximum wins, NaN propagates: ATen's max_pool2d rule
    int arg = -1;
    m = -INFINITY;
    for (int dy = 0; dy < k; ++dy) {
        const int iy = oy * s - p + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < k; ++dx) {
            const int ix = ox * s - p + dx;
            if (ix < 0 || ix >= W) continue;
            const float v = src[iy * W + ix];
            if (arg < 0 || pool_take(v, m)) { m = v; arg = iy * W + ix; }
        }
    }
    return arg;
}
__global__ void maxpool_win_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long planes, int H,
                                       int W, int Ho, int Wo, int k, int s, int p) {
    FOR_EACH_INDEX(i, planes * Ho * Wo) {
        const PlaneYX o = plane_yx(i, Ho, Wo);
        float m;
        window_argmax(x + (size_t)o.plane * H * W, H, W, o.y, o.x, k, s, p, m);
        y[i] = m;
    }
}
// gather form (windows overlap when s < k): each input cell sums grad_y of the windows whose arg-max it is,
// in ascending window order -- deterministic, no atomics
__global__ void maxpool_win_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                       float* __restrict__ gx, long long planes, int H, int W, int Ho, int Wo, int k,
                                       int s, int p) {
    FOR_EACH_INDEX(i, planes * H * W) {
        const PlaneYX at = plane_yx(i, H, W);
        const int iy = at.y, ix = at.x;
        const float* src = x + (size_t)at.plane * H * W;
        const float* g = gy + (size_t)at.plane * Ho * Wo;
        // windows with oy*s - p <= iy <= oy*s - p + k - 1
        int oy0 = (iy + p - k + s) / s, ox0 = (ix + p - k + s) / s;   // ceil((iy+p-k+1)/s) for non-negative numerators
        if (iy + p - k + 1 <= 0) oy0 = 0;
        if (ix + p - k + 1 <= 0) ox0 = 0;
        const int oy1 = min((iy + p) / s, Ho - 1), ox1 = min((ix + p) / s, Wo - 1);
        float acc = 0.0f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) {
                float m;
                if (window_argmax(src, H, W, oy, ox, k, s, p, m) == iy * W + ix) acc += g[oy * Wo + ox];
            }
        gx[i] = acc;
    }
}

// ---- depthwise transposed conv: k = 2f, stride f, padding f/2 (any k,s,p accepted) ----
// y[b,c,oy,ox] = sum_{ky,kx} x[b,c,(oy+p-ky)/s,(ox+p-kx)/s] * w[c,ky,kx]   (exact divisions only)
// grid = (output tiles of 256, planes): 32-bit index math, the channel's kernel in LDS; store-bound
__global__ __launch_bounds__(kT) void dwconvt_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ skip, float* __restrict__ y, int C,
                                                         int H, int W, int Ho, int Wo, int k, int s, int p) {
    __shared__ float ws[1024];
    const int pl = blockIdx.y;
    stage_weights(ws, w, pl % C, k * k);
    const int o = blockIdx.x * kT + threadIdx.x;
    if (o >= Ho * Wo) return;
    const int oy = o / Wo, ox = o - oy * Wo;
    const float* xp = x + (size_t)pl * H * W;
    float acc = 0.0f;
    // valid ky: (oy + p - ky) % s == 0  ->  ky = (oy + p) % s + t*s
    for (int ky = (oy + p) % s; ky < k; ky += s) {
        const int iy = (oy + p - ky) / s;
        if (iy < 0 || iy >= H) continue;
        for (int kx = (ox + p) % s; kx < k; kx += s) {
            const int ix = (ox + p - kx) / s;
            if (ix < 0 || ix >= W) continue;
            acc += xp[iy * W + ix] * ws[ky * k + kx];
        }
    }
    y[(size_t)pl * Ho * Wo + o] = skip ? acc + skip[(size_t)pl * Ho * Wo + o] : acc;
}
// k = 2f, s = f, p = f/2 (IDAUp.up, dla.py:385-388) with compile-time f: every output pixel has exactly 2 x 2 taps and
// all index arithmetic is shifts; one thread produces four consecutive outputs of a row (Wo % 4 == 0).  `skip` (may be
// null) is IDAUp's other summand (dla.py:400-401 node(up(project(x)) + layers[i-1])): added after the taps, in the
// rounding order of the separate add, so the upsampled tensor is written once and never re-read
// ROWS consecutive output rows per thread (Ho % ROWS == 0): 8 KB of traffic per workgroup and row is little enough for
// the workgroup launch rate to bound the kernel (32,768 workgroups for a 134 MB map: 2.7 TB/s)
template <int F, int ROWS>
__global__ __launch_bounds__(kT) void dwconvt_fwd_f_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ skip, float* __restrict__ y, int C,
                                                           int H, int W) {
    constexpr int K = 2 * F, P = F / 2;
    __shared__ float ws[K * K];
    const int pl = blockIdx.y;
    stage_weights(ws, w, pl % C, K * K);
    const int Ho = H * F, Wo = W * F;                       // (H-1)*F - 2*(F/2) + 2F
    const int q = blockIdx.x * kT + threadIdx.x;           // quad of outputs in a band of ROWS rows
    const int qw = Wo >> 2;
    if (q >= qw * (Ho / ROWS)) return;
    const int band = q / qw, ox0 = (q - band * qw) * 4;
    const float* xp = x + (size_t)pl * H * W;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int oy = band * ROWS + r;
        // rows: ky = (oy + P) % F + {0, F}  ->  iy = (oy + P) / F - {0, 1}
        const int ky0 = (oy + P) % F, iy0 = (oy + P) / F;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ox = ox0 + j;
            const int kx0 = (ox + P) % F, ix0 = (ox + P) / F;
            float acc = 0.0f;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int iy = iy0 - a;
                if (iy < 0 || iy >= H) continue;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int ix = ix0 - b;
                    if (ix < 0 || ix >= W) continue;
                    acc += xp[iy * W + ix] * ws[(ky0 + a * F) * K + kx0 + b * F];
                }
            }
            o[j] = acc;
        }
        const size_t at = (size_t)pl * Ho * Wo + (size_t)oy * Wo + ox0;
        if (skip) {
            const float4 k4 = *reinterpret_cast<const float4*>(skip + at);
            o[0] += k4.x; o[1] += k4.y; o[2] += k4.z; o[3] += k4.w;
        }
        *reinterpret_cast<float4*>(y + at) = make_float4(o[0], o[1], o[2], o[3]);
    }
}
// k = 4, stride 2, padding 1 (every IDAUp layer of DLA-34 but one), H and W even: a thread produces a 4 x 4 block of
// outputs from the 4 x 4 block of inputs around it -- twelve loads (per input row one aligned 8-byte load and two edge
// scalars) instead of sixty-four bounds-checked ones; the taps of an output are added in the generic kernels' order
// (a = 0, 1 over rows, b = 0, 1 over columns), so the result is theirs bit for bit.
__global__ __launch_bounds__(kT) void dwconvt_fwd_k4s2_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ skip, float* __restrict__ y, int C,
                                                              int H, int W) {
    __shared__ float ws[16];
    const int pl = blockIdx.y;
    stage_weights(ws, w, pl % C, 16);
    const int Wo = 2 * W, qw = W >> 1;                     // blocks of 4 x 4 outputs: (H / 2) x (W / 2)
    const int q = blockIdx.x * kT + threadIdx.x;
    if (q >= qw * (H >> 1)) return;
    const int br = q / qw, bc = q - br * qw;
    const float* xp = x + (size_t)pl * H * W;
    float xin[4][4];                                        // input rows 2 br - 1 .. + 2, columns 2 bc - 1 .. + 2
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int iy = 2 * br - 1 + a;
        xin[a][0] = xin[a][1] = xin[a][2] = xin[a][3] = 0.0f;
        if (iy >= 0 && iy < H) {
            const float* row = xp + (size_t)iy * W + 2 * bc;
            const float2 m = *reinterpret_cast<const float2*>(row);
            xin[a][1] = m.x; xin[a][2] = m.y;
            if (bc > 0) xin[a][0] = row[-1];
            if (2 * bc + 2 < W) xin[a][3] = row[2];
        }
    }
    // output j of the block (row or column alike): first tap input index r0[j] with kernel index k0[j], second tap
    // input index r0[j] - 1 with kernel index k0[j] + 2
    constexpr int r0[4] = {1, 2, 2, 3}, k0[4] = {1, 0, 1, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float acc = 0.0f;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc += xin[r0[j] - a][r0[i] - b] * ws[(k0[j] + 2 * a) * 4 + k0[i] + 2 * b];
            o[i] = acc;
        }
        const size_t at = (size_t)pl * (2 * H) * Wo + (size_t)(4 * br + j) * Wo + 4 * bc;
        if (skip) {
            const float4 k4 = *reinterpret_cast<const float4*>(skip + at);
            o[0] += k4.x; o[1] += k4.y; o[2] += k4.z; o[3] += k4.w;
        }
        *reinterpret_cast<float4*>(y + at) = make_float4(o[0], o[1], o[2], o[3]);
    }
}
// Both gradients read the same K x K window of gy around an input pixel:
//   gx[b,c,iy,ix]  = sum_{ky,kx} gy[b,c,iy*s-p+ky, ix*s-p+kx] * w[c,ky,kx]
//   gw[c,ky,kx]    = sum_{b,iy,ix} x[b,c,iy,ix] * gy[b,c,iy*s-p+ky, ix*s-p+kx]
// one workgroup per plane (c, b): gx written directly, K*K partial sums reduced in the block (fixed order)
// into part[c][b][K*K]; dwconvt_wsum_kernel adds the B partials in order (reproducible, no atomics).
// the block's K*K tap sums in a fixed order -- lanes, then (wave 0 + wave 1) + (wave 2 + wave 3) -- into part[K*K]
template <int K>
__device__ __forceinline__ void store_tap_partials(const float (&acc)[K * K], float (&red)[4][K * K], float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        const float v = wave_sum(acc[t]);
        if (lane == 0) red[wid][t] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K * K; t += kT) part[t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
template <int K>
__global__ __launch_bounds__(kT) void dwconvt_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ gy, float* __restrict__ gx,
                                                         float* __restrict__ part, int B, int C, int H, int W, int Ho,
                                                         int Wo, int s, int p) {
    __shared__ float ws[K * K];
    __shared__ float red[4][K * K];
    const int c = blockIdx.x, b = blockIdx.y;
    const size_t pl = (size_t)b * C + c;
    stage_weights(ws, w, c, K * K);
    const float* xp = x + pl * H * W;
    const float* gp = gy + pl * Ho * Wo;
    float acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = 0.0f;
    for (int i = threadIdx.x; i < H * W; i += kT) {
        const int iy = i / W, ix = i - iy * W;
        const float xv = part ? xp[i] : 0.0f;
        const int oy0 = iy * s - p, ox0 = ix * s - p;
        float g = 0.0f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int oy = oy0 + ky;
            const bool rok = oy >= 0 && oy < Ho;
            const float* row = gp + (rok ? oy : 0) * Wo;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int ox = ox0 + kx;
                const bool ok = rok && ox >= 0 && ox < Wo;
                const float v = ok ? row[ox] : 0.0f;
                g += v * ws[ky * K + kx];
                acc[ky * K + kx] += xv * v;
            }
        }
        if (gx) gx[pl * H * W + i] = g;
    }
    if (part) store_tap_partials<K>(acc, red, part + ((size_t)c * B + b) * K * K);
}
// The same for IDAUp's commonest layer (k = 4, stride 2, padding 1; W even): a thread takes TWO neighbouring input pixels
// (ix even).  Their windows are the six output columns 2 ix - 1 .. 2 ix + 4 of four output rows: per row one aligned
// 16-byte load and two edge scalars instead of eight bounds-checked scalar loads -- the generic kernel above spends its
// time on index math (about 160 vector instructions per input pixel, 2 TB/s).
__global__ __launch_bounds__(kT) void dwconvt_bwd_k4s2_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ gy, float* __restrict__ gx,
                                                              float* __restrict__ part, int B, int C, int H, int W) {
    constexpr int K = 4;
    __shared__ float ws[K * K];
    __shared__ float red[4][K * K];
    const int c = blockIdx.x, b = blockIdx.y;
    const size_t pl = (size_t)b * C + c;
    stage_weights(ws, w, c, K * K);
    const int Ho = 2 * H, Wo = 2 * W, W2 = W >> 1;
    const float* xp = x + pl * H * W;
    const float* gp = gy + pl * Ho * Wo;
    float acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = 0.0f;
    for (int i = threadIdx.x; i < H * W2; i += kT) {
        const int iy = i / W2, ix = (i - iy * W2) * 2;
        float x0 = 0.0f, x1 = 0.0f;
        if (part) { const float2 xv = *reinterpret_cast<const float2*>(xp + iy * W + ix); x0 = xv.x; x1 = xv.y; }
        float g0 = 0.0f, g1 = 0.0f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int oy = 2 * iy - 1 + ky;
            float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};          // output columns 2 ix - 1 .. 2 ix + 4
            if (oy >= 0 && oy < Ho) {
                const float* row = gp + (size_t)oy * Wo + 2 * ix;
                const float4 m = *reinterpret_cast<const float4*>(row);
                v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w;
                if (ix > 0) v[0] = row[-1];
                if (2 * ix + 4 < Wo) v[5] = row[4];
            }
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {                       // pixel ix sees v[kx], pixel ix + 1 sees v[kx + 2]
                const float wk = ws[ky * K + kx];
                g0 += v[kx] * wk;
                g1 += v[kx + 2] * wk;
                acc[ky * K + kx] += x0 * v[kx];
                acc[ky * K + kx] += x1 * v[kx + 2];
            }
        }
        if (gx) *reinterpret_cast<float2*>(gx + pl * H * W + iy * W + ix) = make_float2(g0, g1);
    }
    if (part) store_tap_partials<K>(acc, red, part + ((size_t)c * B + b) * K * K);
}
// gw[c,tap] = sum_b part[(c*B + b)*T + tap], the images in increasing order: the second step of every depthwise weight
// gradient (transposed and plain)
__global__ void dwconvt_wsum_kernel(const float* __restrict__ part, float* __restrict__ gw, int B, int C, int T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * T) return;
    const int c = i / T, t = i - c * T;
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) acc += part[((size_t)c * B + b) * T + t];
    gw[i] = acc;
}
// generic kernel sizes: one thread per input pixel / one workgroup per (c, tap)
__global__ void dwconvt_bwd_data_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                        float* __restrict__ gx, int B, int C, int H, int W, int Ho, int Wo, int k,
                                        int s, int p) {
    FOR_EACH_INDEX(i, (long long)B * C * H * W) {
        const PlaneYX at = plane_yx(i, H, W);
        const int iy = at.y, ix = at.x, c = (int)(at.plane % C);
        const float* gp = gy + (size_t)at.plane * Ho * Wo;
        const float* wp = w + (size_t)c * k * k;
        float acc = 0.0f;
        for (int ky = 0; ky < k; ++ky) {
            const int oy = iy * s - p + ky;
            if (oy < 0 || oy >= Ho) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int ox = ix * s - p + kx;
                if (ox < 0 || ox >= Wo) continue;
                acc += gp[oy * Wo + ox] * wp[ky * k + kx];
            }
        }
        gx[i] = acc;
    }
}
__global__ __launch_bounds__(kT) void dwconvt_bwd_weight_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gy, float* __restrict__ gw,
                                                                int B, int C, int H, int W, int Ho, int Wo, int k, int s,
                                                                int p) {
    __shared__ float red[16];
    const int c = blockIdx.x, tap = blockIdx.y;
    const int ky = tap / k, kx = tap - ky * k;
    float acc = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float* xp = x + ((size_t)b * C + c) * H * W;
        const float* gp = gy + ((size_t)b * C + c) * Ho * Wo;
        for (int i = threadIdx.x; i < H * W; i += kT) {
            const int iy = i / W, ix = i - iy * W;
            const int oy = iy * s - p + ky, ox = ix * s - p + kx;
            if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) acc += xp[i] * gp[oy * Wo + ox];
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) gw[(size_t)c * k * k + tap] = acc;
}

// ---- elementwise ------------------------------------------------------------
// gradient through ReLU (slope 0) / LeakyReLU: g * (y > 0 ? 1 : slope)
__device__ __forceinline__ float act_gate(float g, float y, float slope) { return y > 0.0f ? g : g * slope; }
struct Identity {
    __device__ float operator()(float v) const { return v; }
};
// n4 quads of 16 bytes, then the scalar rest (the host passes n4 == 0 for operands off 16-byte alignment)
// (no __restrict__: out may be a or b -- hip_runtime.fork sums gradients in place)
__global__ void add_kernel(const float* a, const float* b, float* out, long long n4, long long n) {
    FOR_EACH_INDEX(i, n4) {
        const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
    FOR_EACH_INDEX_FROM(i, n4 * 4, n) out[i] = a[i] + b[i];
}
// gx = gy * (y > 0 ? 1 : slope)      (ReLU: slope 0; LeakyReLU(0.2): slope 0.2)
__global__ void act_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y, float* __restrict__ gx,
                               long long n4, long long n, float slope) {
    FOR_EACH_INDEX(i, n4) {
        const float4 g = reinterpret_cast<const float4*>(gy)[i], v = reinterpret_cast<const float4*>(y)[i];
        reinterpret_cast<float4*>(gx)[i] = make_float4(act_gate(g.x, v.x, slope), act_gate(g.y, v.y, slope),
                                                       act_gate(g.z, v.z, slope), act_gate(g.w, v.w, slope));
    }
    FOR_EACH_INDEX_FROM(i, n4 * 4, n) gx[i] = act_gate(gy[i], y[i], slope);
}
// The input gradient of a 1x1 convolution with a handful of output channels (a detection head's last layer,
// dla.py:474-483: 256 -> classes / 2 / 2) fused with the backward of the activation in front of it:
//   gh[b][m][p] = (hid[b][m][p] > 0 ? 1 : slope) * sum_c w[c][m] * go[b][c][p]            (c in increasing order)
// K = CO <= 8 is no GEMM: the kernel is one read of the hidden map (for the gate) and one write of its gradient, the
// CO gradient planes of a pixel quad stay in registers across the channel loop and the weights are scalar loads.
// grid (quads of pixels / kT, channel chunks, B)
template <int CO>
__global__ __launch_bounds__(kT) void conv1x1_dgrad_act_kernel(const float* __restrict__ go, const float* __restrict__ w,
                                                               const float* __restrict__ hid, float* __restrict__ gh,
                                                               int Ch, int ch_chunk, long long HW, float slope) {
    const long long q = (long long)blockIdx.x * kT + threadIdx.x;
    if (q * 4 >= HW) return;
    const int b = blockIdx.z, m0 = blockIdx.y * ch_chunk, m1 = min(m0 + ch_chunk, Ch);
    float4 g[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) g[c] = *reinterpret_cast<const float4*>(go + ((size_t)b * CO + c) * HW + q * 4);
    for (int m = m0; m < m1; ++m) {
        const size_t at = ((size_t)b * Ch + m) * HW + q * 4;
        const float4 h = *reinterpret_cast<const float4*>(hid + at);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            const float wc = w[(size_t)c * Ch + m];
            o.x += wc * g[c].x; o.y += wc * g[c].y; o.z += wc * g[c].z; o.w += wc * g[c].w;
        }
        *reinterpret_cast<float4*>(gh + at) = make_float4(act_gate(o.x, h.x, slope), act_gate(o.y, h.y, slope),
                                                          act_gate(o.z, h.z, slope), act_gate(o.w, h.w, slope));
    }
}
// Row-wise kernels: grid (chunks of a row, rows); a row is one (image, channel) plane of HW floats, so the
// channel bookkeeping is per workgroup and the inner loop is 16-byte copies when `vec`: HW % 4 == 0 and every tensor
// 16-byte aligned (rows_vec_ok, decided by the host); else 4-byte copies of the same values.
// d[i] = f(in[i]...) over the row, grid-stride: float4 with f on each of .x .y .z .w when `vec`, else float
template <typename F, typename... In>
__device__ __forceinline__ void map_row(int vec, long long HW, float* d, F f, In... in) {
    if (vec) {
        FOR_EACH_INDEX(i, HW >> 2) {
            const auto at = [i](const float* p) { return reinterpret_cast<const float4*>(p)[i]; };
            reinterpret_cast<float4*>(d)[i] = make_float4(f(at(in).x...), f(at(in).y...), f(at(in).z...), f(at(in).w...));
        }
    } else {
        FOR_EACH_INDEX(i, HW) d[i] = f(in[i]...);
    }
}
// copy a [B, Cn, HW] block between tensors with Csrc / Cdst channels at channel offsets
__global__ void copy_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int Cn,
                                     long long HW, int Csrc, int src_off, int Cdst, int dst_off, int vec) {
    for (int row = blockIdx.y; row < rows; row += gridDim.y) {
        const int b = row / Cn, c = row - b * Cn;
        map_row(vec, HW, dst + ((size_t)b * Cdst + dst_off + c) * HW, Identity(), src + ((size_t)b * Csrc + src_off + c) * HW);
    }
}
// om [B, 3T, HW] -> offset [B, 2T, HW] (channels 0..2T-1 unchanged) and mask = sigmoid(channels 2T..3T-1)
__global__ void split_offset_mask_kernel(const float* __restrict__ om, float* __restrict__ offset,
                                         float* __restrict__ mask, int rows, int T, long long HW, int vec) {
    for (int row = blockIdx.y; row < rows; row += gridDim.y) {
        const int b = row / (3 * T), c = row - b * 3 * T;
        const float* s = om + (size_t)row * HW;
        if (c >= 2 * T) map_row(vec, HW, mask + ((size_t)b * T + (c - 2 * T)) * HW, [](float v) { return sigmoid_f32(v); }, s);
        else map_row(vec, HW, offset + ((size_t)b * 2 * T + c) * HW, Identity(), s);
    }
}
__global__ void split_offset_mask_bwd_kernel(const float* __restrict__ goff, const float* __restrict__ gmask,
                                             const float* __restrict__ mask, float* __restrict__ gom, int rows,
                                             int T, long long HW, int vec) {
    for (int row = blockIdx.y; row < rows; row += gridDim.y) {
        const int b = row / (3 * T), c = row - b * 3 * T;
        float* d = gom + (size_t)row * HW;
        if (c >= 2 * T) {
            const size_t at = ((size_t)b * T + (c - 2 * T)) * HW;          // the row's place in mask and gmask
            map_row(vec, HW, d, [](float g, float m) { return g * m * (1.0f - m); }, gmask + at, mask + at);
        } else {
            map_row(vec, HW, d, Identity(), goff + ((size_t)b * 2 * T + c) * HW);
        }
    }
}

// ---------------- depthwise convolution (groups == channels), top / left padding given ----------------
// torchvision MobileNetV2's `ConvBNReLU(hidden, hidden, stride, groups=hidden)` (pt = pl = p) and EfficientNet's MBConv
// with TensorFlow "SAME" padding (pt, pl the smaller halves).  y[b,c,oy,ox] = sum_{r,t} w[c,r,t] * x[b,c, oy*s - pt + r,
// ox*s - pl + t]; taps outside the map read zero, whichever side they fall off: the bottom / right padding is implied
// by the output size and may be negative (trailing rows / columns never read).  s, pt, pl are run-time values, any
// s >= 1 and pt, pl >= 0.  One thread per output, k*k weights in registers.  No float atomics.
template <int K>
__global__ __launch_bounds__(kT) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ y, int C, int H, int W, int Ho, int Wo,
                                                        int s, int pt, int pl) {
    const int c = blockIdx.x % C;
    const size_t plane = blockIdx.x;
    float wk[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) wk[i] = w[(size_t)c * K * K + i];
    const float* xp = x + plane * H * W;
    float* yp = y + plane * Ho * Wo;
    for (int o = blockIdx.y * kT + threadIdx.x; o < Ho * Wo; o += gridDim.y * kT) {
        const int oy = o / Wo, ox = o - oy * Wo;
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int iy = oy * s - pt + r;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int ix = ox * s - pl + t;
                if (ix >= 0 && ix < W) acc += wk[r * K + t] * xp[iy * W + ix];
            }
        }
        yp[o] = acc;
    }
}
// W % 4 == 0 and Wo % 4 == 0, stride S 1 or 2, left padding PL in 0..2 (what p = (k-1)/2 and SAME padding give k = 3
// and 5; a compile-time constant, so the row window stays in registers): one thread per four outputs of a row.
// The input window of the quad lies inside the NV aligned float4 segments that start at column S*ox - 4 (a segment is
// wholly inside or wholly outside the row, because W is a multiple of 4): 16-byte loads, one 16-byte store; taps are
// accumulated in the scalar kernel's order (r, then t), so both paths round alike.
template <int K, int S, int PL>
__global__ __launch_bounds__(kT) void dwconv_fwd_vec_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            float* __restrict__ y, int C, int H, int W, int Ho, int Wo,
                                                            int pt) {
    constexpr int NV = S == 1 ? 3 : 4;
    const int c = blockIdx.x % C;
    const size_t plane = blockIdx.x;
    float wk[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) wk[i] = w[(size_t)c * K * K + i];
    const float* xp = x + plane * H * W;
    float* yp = y + plane * Ho * Wo;
    const int Wq = Wo >> 2;
    for (int q = blockIdx.y * kT + threadIdx.x; q < Ho * Wq; q += gridDim.y * kT) {
        const int oy = q / Wq, ox = (q - oy * Wq) * 4;
        const int x0 = S * ox - 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int iy = oy * S - pt + r;
            if (iy < 0 || iy >= H) continue;
            float v[NV * 4];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int xs = x0 + 4 * j;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (xs >= 0 && xs + 3 < W) f = *reinterpret_cast<const float4*>(xp + (size_t)iy * W + xs);
                v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
            }
#pragma unroll
            for (int t = 0; t < K; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    constexpr int kLast = S * 3 - PL + K - 1 + 4;
                    static_assert(PL <= 4 && kLast < NV * 4, "the quad's window must lie inside the loaded segments");
                    acc[i] += wk[r * K + t] * v[S * i - PL + t + 4];      // column S*(ox+i) - PL + t
                }
            }
        }
        *reinterpret_cast<float4*>(yp + (size_t)oy * Wo + ox) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}
// gx[b,c,iy,ix] = sum_{r,t} w[c,r,t] * gy[b,c,(iy+pt-r)/s,(ix+pl-t)/s] over the taps that divide.  VEC: W % 4 == 0, one
// thread per four inputs of a row and one 16-byte store (the gradient loads stay scalar: they are strided by 1/s).
template <int K, int VEC>
__global__ __launch_bounds__(kT) void dwconv_bwd_data_kernel(const float* __restrict__ gy, const float* __restrict__ w,
                                                             float* __restrict__ gx, int C, int H, int W, int Ho, int Wo,
                                                             int s, int pt, int pl) {
    const int c = blockIdx.x % C;
    const size_t plane = blockIdx.x;
    float wk[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) wk[i] = w[(size_t)c * K * K + i];
    const float* gp = gy + plane * Ho * Wo;
    float* xp = gx + plane * H * W;
    const int Wv = W / VEC;
    for (int q = blockIdx.y * kT + threadIdx.x; q < H * Wv; q += gridDim.y * kT) {
        const int iy = q / Wv, ix0 = (q - iy * Wv) * VEC;
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int ty = iy + pt - r;
            if (ty < 0 || ty % s) continue;
            const int oy = ty / s;
            if (oy >= Ho) continue;
#pragma unroll
            for (int t = 0; t < K; ++t) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int tx = ix0 + i + pl - t;
                    if (tx < 0 || tx % s) continue;
                    const int ox = tx / s;
                    if (ox < Wo) acc[i] += wk[r * K + t] * gp[oy * Wo + ox];
                }
            }
        }
        if constexpr (VEC == 4)
            *reinterpret_cast<float4*>(xp + (size_t)iy * W + ix0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            xp[(size_t)iy * W + ix0] = acc[0];
    }
}
// Weight gradient, step 1: one workgroup per (channel, image) reduces its plane to k*k sums (each thread its strided
// share in order, then a fixed-shape fp64 block reduction) -> part[(c*B + b)*K*K + tap].  Step 2 is dwconvt_wsum_kernel.
template <int K>
__global__ __launch_bounds__(kT) void dwconv_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                               float* __restrict__ part, int B, int C, int H, int W,
                                                               int Ho, int Wo, int s, int pt, int pl) {
    __shared__ double red[16];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* xp = x + ((size_t)b * C + c) * H * W;
    const float* gp = gy + ((size_t)b * C + c) * Ho * Wo;
    float acc[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) acc[i] = 0.0f;
    for (int o = threadIdx.x; o < Ho * Wo; o += kT) {
        const int oy = o / Wo, ox = o - oy * Wo;
        const float g = gp[o];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int iy = oy * s - pt + r;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int ix = ox * s - pl + t;
                if (ix >= 0 && ix < W) acc[r * K + t] += g * xp[iy * W + ix];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < K * K; ++i) {
        const double v = block_sum((double)acc[i], red);
        if (threadIdx.x == 0) part[((size_t)c * B + b) * K * K + i] = (float)v;
    }
}
}  // namespace
}  // namespace cnuda

using namespace cnuda;

// output sizes: a (max-pool or convolution) window by torch's floor rule, and the transposed convolution
static int pool_out(int H, int k, int s, int p) { return (H + 2 * p - k) / s + 1; }
static int convt_out(int H, int k, int s, int p) { return (H - 1) * s - 2 * p + k; }
// a grid-stride kernel (FOR_EACH_INDEX) over `items`
#define CNUDA_LAUNCH_1D(kernel, items, stream, ...) \
    CNUDA_LAUNCH(kernel, dim3(stream_grid(items, kT)), dim3(kT), 0, (hipStream_t)(stream), __VA_ARGS__)

extern "C" int cnuda_maxpool2d_forward(const float* x, float* y, int B, int C, int H, int W, int k,
                                       cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && B > 0 && C > 0 && k > 0 && H >= k && W >= k, "cnuda_maxpool2d_forward: bad arguments");
    const int Ho = H / k, Wo = W / k;
    const long long planes = (long long)B * C;
    if (pool2_vec_ok(x, y, nullptr, H, W, k)) {
        const long long total = planes * Ho * (Wo / 2);
        CNUDA_LAUNCH_1D(maxpool2_fwd_vec_kernel, total, stream, reinterpret_cast<const float4*>(x), reinterpret_cast<float2*>(y),
                        total, W / 4);
        return check_launch("cnuda_maxpool2d_forward");
    }
    CNUDA_LAUNCH_1D(maxpool_fwd_kernel, planes * Ho * Wo, stream, x, y, planes, H, W, Ho, Wo, k);
    return check_launch("cnuda_maxpool2d_forward");
}
extern "C" int cnuda_maxpool2d_backward(const float* x, const float* grad_y, float* grad_x, int B, int C, int H, int W,
                                        int k, cnuda_stream_t stream) {
    return cnuda_maxpool2d_backward_acc(x, grad_y, grad_x, 0, B, C, H, W, k, stream);
}
extern "C" int cnuda_maxpool2d_backward_acc(const float* x, const float* grad_y, float* grad_x, int accumulate, int B, int C,
                                            int H, int W, int k, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && grad_y && grad_x && B > 0 && C > 0 && k > 0 && H >= k && W >= k,
                  "cnuda_maxpool2d_backward: bad arguments");
    const int Ho = H / k, Wo = W / k;
    const long long planes = (long long)B * C;
    if (pool2_vec_ok(x, grad_y, grad_x, H, W, k)) {
        const long long total = planes * Ho * (Wo / 2);
        CNUDA_LAUNCH_1D(maxpool2_bwd_vec_kernel, total, stream, reinterpret_cast<const float4*>(x),
                        reinterpret_cast<const float2*>(grad_y), reinterpret_cast<float4*>(grad_x), total, W / 4, accumulate);
        return check_launch("cnuda_maxpool2d_backward");
    }
    if (!accumulate && (Ho * k != H || Wo * k != W))
        CNUDA_LAUNCH_1D(maxpool_bwd_tail_kernel, planes * H * W, stream, grad_x, planes, H, W, Ho * k, Wo * k);
    CNUDA_LAUNCH_1D(maxpool_bwd_kernel, planes * Ho * Wo, stream, x, grad_y, grad_x, planes, H, W, Ho, Wo, k, accumulate);
    return check_launch("cnuda_maxpool2d_backward");
}

extern "C" int cnuda_maxpool2d_window_forward(const float* x, float* y, int B, int C, int H, int W, int k, int s, int p,
                                              cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && B > 0 && C > 0 && k > 0 && s > 0 && p >= 0 && 2 * p <= k && H + 2 * p >= k && W + 2 * p >= k,
                  "cnuda_maxpool2d_window_forward: bad arguments (need 2*padding <= kernel <= padded size)");
    const int Ho = pool_out(H, k, s, p), Wo = pool_out(W, k, s, p);
    const long long planes = (long long)B * C;
    CNUDA_LAUNCH_1D(maxpool_win_fwd_kernel, planes * Ho * Wo, stream, x, y, planes, H, W, Ho, Wo, k, s, p);
    return check_launch("cnuda_maxpool2d_window_forward");
}
extern "C" int cnuda_maxpool2d_window_backward(const float* x, const float* grad_y, float* grad_x, int B, int C, int H,
                                               int W, int k, int s, int p, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && grad_y && grad_x && B > 0 && C > 0 && k > 0 && s > 0 && p >= 0 && 2 * p <= k && H + 2 * p >= k &&
                      W + 2 * p >= k,
                  "cnuda_maxpool2d_window_backward: bad arguments");
    const int Ho = pool_out(H, k, s, p), Wo = pool_out(W, k, s, p);
    const long long planes = (long long)B * C;
    CNUDA_LAUNCH_1D(maxpool_win_bwd_kernel, planes * H * W, stream, x, grad_y, grad_x, planes, H, W, Ho, Wo, k, s, p);
    return check_launch("cnuda_maxpool2d_window_backward");
}

extern "C" int cnuda_dwconvt2d_add_forward(const float* x, const float* w, const float* skip, float* y, int B, int C,
                                           int H, int W, int k, int s, int p, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && w && y && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && k <= 32 && s > 0 && p >= 0,
                  "cnuda_dwconvt2d_forward: bad arguments (kernel size 1..32)");
    const int Ho = convt_out(H, k, s, p), Wo = convt_out(W, k, s, p);
    CNUDA_REQUIRE(Ho > 0 && Wo > 0, "cnuda_dwconvt2d_forward: empty output");
    CNUDA_REQUIRE((long long)B * C <= 65535, "cnuda_dwconvt2d_forward: more than 65535 planes");
    // the vector kernels read `skip` and write `y` 16 bytes at a time (and read x 8 bytes at a time): a view at an
    // odd offset takes the scalar kernel
    const bool upsample = k == 2 * s && p == s / 2 && (s == 2 || s == 4) && Wo % 4 == 0 && aligned16(x, y, skip);   // IDAUp's bilinear-style layers
    const int rows = (upsample && Ho % 4 == 0 && (long long)Ho * Wo >= 4096) ? 4 : 1;
    const dim3 fgrid(ceil_div((long long)Ho * Wo / 4 / rows, kT), B * C);
    hipStream_t st = (hipStream_t)stream;
    if (upsample && s == 2 && rows == 4 && (H & 1) == 0 && (W & 1) == 0)
        CNUDA_LAUNCH(dwconvt_fwd_k4s2_kernel, dim3(ceil_div((long long)(H / 2) * (W / 2), kT), B * C), dim3(kT), 0, st, x, w, skip, y, C, H, W);
    else if (upsample && s == 2)         // (rows == 4 means H and W even here: the branch above has taken it)
        CNUDA_LAUNCH((dwconvt_fwd_f_kernel<2, 1>), fgrid, dim3(kT), 0, st, x, w, skip, y, C, H, W);
    else if (upsample && rows == 4)
        CNUDA_LAUNCH((dwconvt_fwd_f_kernel<4, 4>), fgrid, dim3(kT), 0, st, x, w, skip, y, C, H, W);
    else if (upsample)
        CNUDA_LAUNCH((dwconvt_fwd_f_kernel<4, 1>), fgrid, dim3(kT), 0, st, x, w, skip, y, C, H, W);
    else
        CNUDA_LAUNCH(dwconvt_fwd_kernel, dim3(ceil_div((long long)Ho * Wo, kT), B * C), dim3(kT), 0, st, x, w, skip, y, C, H, W, Ho, Wo, k, s, p);
    return check_launch("cnuda_dwconvt2d_forward");
}
extern "C" int cnuda_dwconvt2d_forward(const float* x, const float* w, float* y, int B, int C, int H, int W, int k,
                                       int s, int p, cnuda_stream_t stream) {
    return cnuda_dwconvt2d_add_forward(x, w, nullptr, y, B, C, H, W, k, s, p, stream);
}
// ---- depthwise convolution: cnuda_dwconv2d_* (symmetric padding p, torch's floor rule for the output size) and
// cnuda_dwconv2d_same_* (top / left padding and the output size given) share the kernels and the two launch bodies ----
// per-image partial weight gradients [C][B][k*k] of every depthwise backward, the transposed one included
static size_t dw_workspace_bytes(int B, int C, int k) {
    return (size_t)(B > 0 ? B : 0) * (C > 0 ? C : 0) * k * k * sizeof(float) + 256;
}
extern "C" size_t cnuda_dwconv2d_workspace_bytes(int B, int C, int k) { return dw_workspace_bytes(B, C, k); }
extern "C" size_t cnuda_dwconv2d_same_workspace_bytes(int B, int C, int k) { return dw_workspace_bytes(B, C, k); }
extern "C" size_t cnuda_dwconvt2d_workspace_bytes(int B, int C, int k) { return dw_workspace_bytes(B, C, k); }

// one plane per blockIdx.x, up to 64 workgroups stride over its `items`
static dim3 dwconv_grid(int planes, long long items) {
    const int g = ceil_div(items, kT);
    return dim3(planes, g < 64 ? g : 64);
}
// the kernels' index math is 32-bit
static int dwconv_sizes_ok(const char* who, int B, int C, int H, int W, int Ho, int Wo) {
    CNUDA_REQUIRE((long long)B * C <= 2147483647LL && (long long)H * W <= 2147483647LL && (long long)Ho * Wo <= 2147483647LL,
                  "%s: tensor too large", who);
    return 0;
}
// f(K) with the kernel size, 3 or 5 (the entries have checked it), as a compile-time constant: K.value
template <typename F>
static void dispatch_k35(int k, F f) {
    if (k == 3) f(std::integral_constant<int, 3>());
    else f(std::integral_constant<int, 5>());
}
// step 2 of every depthwise weight gradient: gw = the B partials of `part` added in order
static void launch_wsum(const float* part, float* gw, int B, int C, int k, hipStream_t st) {
    CNUDA_LAUNCH(dwconvt_wsum_kernel, dim3(ceil_div((long long)C * k * k, 256)), dim3(256), 0, st, part, gw, B, C, k * k);
}
// The launch bodies.  The entry (`who` in messages) has checked its own contract, which is at least: B, C, H, W, Ho,
// Wo > 0, k 3 or 5, s >= 1, pt, pl >= 0.  Whatever the 16-byte forms do not take goes to the scalar kernels, which are
// right for every such geometry and accumulate in the same order.
static int dwconv_forward(const char* who, const float* x, const float* w, float* y, int B, int C, int H, int W, int k,
                          int s, int pt, int pl, int Ho, int Wo, hipStream_t st) {
    CNUDA_REQUIRE(x && w && y, "%s: null pointer", who);
    if (int rc = dwconv_sizes_ok(who, B, C, H, W, Ho, Wo)) return rc;
    // the quad's window, columns S*ox - PL .. S*(ox+3) - PL + k - 1, lies inside [S*ox - 4, S*ox + 4*NV) for S <= 2, PL <= 2, k <= 5
    const bool vec = (W % 4 == 0) && (Wo % 4 == 0) && pl <= 2 && s <= 2 && aligned16(x, y);
    if (vec) {
        const dim3 grid = dwconv_grid(B * C, (long long)Ho * (Wo / 4));
#define CNUDA_DWV(K, S, PL) CNUDA_LAUNCH((dwconv_fwd_vec_kernel<K, S, PL>), grid, dim3(kT), 0, st, x, w, y, C, H, W, Ho, Wo, pt)
#define CNUDA_DWP(K, S) do { if (pl == 0) CNUDA_DWV(K, S, 0); else if (pl == 1) CNUDA_DWV(K, S, 1); else CNUDA_DWV(K, S, 2); } while (0)
        dispatch_k35(k, [&](auto K) {           // (no geometry reaches <3, 2, 2>: W % 4 == 0 and left padding 2 make Wo odd)
            if (s == 1) CNUDA_DWP(K.value, 1);
            else CNUDA_DWP(K.value, 2);
        });
#undef CNUDA_DWP
#undef CNUDA_DWV
    } else {
        const dim3 grid = dwconv_grid(B * C, (long long)Ho * Wo);
        dispatch_k35(k, [&](auto K) { CNUDA_LAUNCH(dwconv_fwd_kernel<K.value>, grid, dim3(kT), 0, st, x, w, y, C, H, W, Ho, Wo, s, pt, pl); });
    }
    return check_launch(who);
}
static int dwconv_backward(const char* who, const float* x, const float* w, const float* grad_y, float* grad_x,
                           float* grad_w, int B, int C, int H, int W, int k, int s, int pt, int pl, int Ho, int Wo,
                           void* workspace, size_t workspace_bytes, hipStream_t st) {
    CNUDA_REQUIRE(x && w && grad_y, "%s: null pointer", who);
    if (int rc = dwconv_sizes_ok(who, B, C, H, W, Ho, Wo)) return rc;
    if (grad_x) {
        const bool vec = W % 4 == 0 && aligned16(grad_x);
        const dim3 grid = dwconv_grid(B * C, (long long)H * (vec ? W / 4 : W));
        dispatch_k35(k, [&](auto K) {
            if (vec) CNUDA_LAUNCH((dwconv_bwd_data_kernel<K.value, 4>), grid, dim3(kT), 0, st, grad_y, w, grad_x, C, H, W, Ho, Wo, s, pt, pl);
            else CNUDA_LAUNCH((dwconv_bwd_data_kernel<K.value, 1>), grid, dim3(kT), 0, st, grad_y, w, grad_x, C, H, W, Ho, Wo, s, pt, pl);
        });
    }
    if (grad_w) {
        CNUDA_REQUIRE(workspace && workspace_bytes >= dw_workspace_bytes(B, C, k), "%s: workspace too small", who);
        CNUDA_REQUIRE(B <= 65535, "%s: batch > 65535", who);
        float* part = reinterpret_cast<float*>(workspace);
        dispatch_k35(k, [&](auto K) {
            CNUDA_LAUNCH(dwconv_bwd_weight_kernel<K.value>, dim3(C, B), dim3(kT), 0, st, x, grad_y, part, B, C, H, W, Ho, Wo, s, pt, pl);
        });
        launch_wsum(part, grad_w, B, C, k, st);
    }
    return check_launch(who);
}

// any stride s >= 1 and padding p >= 0; the output size by torch's floor rule
static int dwconv_geom(int B, int C, int H, int W, int k, int s, int p, int& Ho, int& Wo, const char* who) {
    CNUDA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && s > 0 && p >= 0, "%s: bad arguments", who);
    CNUDA_REQUIRE(k == 3 || k == 5, "%s: kernel size %d (3 and 5 are built)", who, k);
    CNUDA_REQUIRE(H + 2 * p >= k && W + 2 * p >= k, "%s: empty output", who);
    Ho = pool_out(H, k, s, p);
    Wo = pool_out(W, k, s, p);
    return 0;
}
extern "C" int cnuda_dwconv2d_forward(const float* x, const float* w, float* y, int B, int C, int H, int W, int k,
                                      int s, int p, cnuda_stream_t stream) {
    int Ho, Wo;
    if (int rc = dwconv_geom(B, C, H, W, k, s, p, Ho, Wo, "cnuda_dwconv2d_forward")) return rc;
    return dwconv_forward("cnuda_dwconv2d_forward", x, w, y, B, C, H, W, k, s, p, p, Ho, Wo, (hipStream_t)stream);
}
extern "C" int cnuda_dwconv2d_backward(const float* x, const float* w, const float* grad_y, float* grad_x, float* grad_w,
                                       int B, int C, int H, int W, int k, int s, int p, void* workspace,
                                       size_t workspace_bytes, cnuda_stream_t stream) {
    int Ho, Wo;
    if (int rc = dwconv_geom(B, C, H, W, k, s, p, Ho, Wo, "cnuda_dwconv2d_backward")) return rc;
    return dwconv_backward("cnuda_dwconv2d_backward", x, w, grad_y, grad_x, grad_w, B, C, H, W, k, s, p, p, Ho, Wo, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

// stride 1 or 2; top / left padding and the bottom / right padding that the output size implies all in [0, k)
static int dwconv_same_geom(int B, int C, int H, int W, int k, int s, int pt, int pl, int Ho, int Wo, const char* who) {
    CNUDA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (k == 3 || k == 5) && (s == 1 || s == 2), "%s: k must be 3 or 5, stride 1 or 2", who);
    CNUDA_REQUIRE(pt >= 0 && pl >= 0 && pt < k && pl < k, "%s: top / left padding must lie in [0, k)", who);
    CNUDA_REQUIRE(Ho > 0 && Wo > 0, "%s: empty output", who);
    // the implied bottom / right padding (Ho-1)*s + k - pt - H must lie in [0, k) as well: every output sees the map
    const int pb = (Ho - 1) * s + k - pt - H, pr = (Wo - 1) * s + k - pl - W;
    CNUDA_REQUIRE(pb >= 0 && pb < k && pr >= 0 && pr < k,
                  "%s: output %dx%d does not fit input %dx%d (k %d, stride %d, top %d, left %d)", who, Ho, Wo, H, W, k, s, pt, pl);
    return 0;
}
extern "C" int cnuda_dwconv2d_same_forward(const float* x, const float* w, float* y, int B, int C, int H, int W, int k, int s,
                                           int pad_top, int pad_left, int Ho, int Wo, cnuda_stream_t stream) {
    if (int rc = dwconv_same_geom(B, C, H, W, k, s, pad_top, pad_left, Ho, Wo, "cnuda_dwconv2d_same_forward")) return rc;
    return dwconv_forward("cnuda_dwconv2d_same_forward", x, w, y, B, C, H, W, k, s, pad_top, pad_left, Ho, Wo, (hipStream_t)stream);
}
extern "C" int cnuda_dwconv2d_same_backward(const float* x, const float* w, const float* grad_y, float* grad_x, float* grad_w,
                                            int B, int C, int H, int W, int k, int s, int pad_top, int pad_left, int Ho, int Wo,
                                            void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    if (int rc = dwconv_same_geom(B, C, H, W, k, s, pad_top, pad_left, Ho, Wo, "cnuda_dwconv2d_same_backward")) return rc;
    return dwconv_backward("cnuda_dwconv2d_same_backward", x, w, grad_y, grad_x, grad_w, B, C, H, W, k, s, pad_top, pad_left, Ho,
                           Wo, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int cnuda_dwconvt2d_backward(const float* x, const float* w, const float* grad_y, float* grad_x,
                                        float* grad_w, int B, int C, int H, int W, int k, int s, int p,
                                        void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && w && grad_y && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && s > 0 && p >= 0,
                  "cnuda_dwconvt2d_backward: bad arguments");
    const int Ho = convt_out(H, k, s, p), Wo = convt_out(W, k, s, p);
    hipStream_t st = (hipStream_t)stream;
    if ((k == 4 || k == 8) && C <= 65535 && B <= 65535) {
        float* part = nullptr;
        if (grad_w) {
            CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_dwconvt2d_workspace_bytes(B, C, k),
                          "cnuda_dwconvt2d_backward: workspace too small");
            part = (float*)workspace;
        }
        if (k == 4 && s == 2 && p == 1 && (W & 1) == 0 && aligned16(x, grad_y, grad_x))
            CNUDA_LAUNCH(dwconvt_bwd_k4s2_kernel, dim3(C, B), dim3(kT), 0, st, x, w, grad_y, grad_x, part, B, C, H, W);
        else if (k == 4)
            CNUDA_LAUNCH(dwconvt_bwd_kernel<4>, dim3(C, B), dim3(kT), 0, st, x, w, grad_y, grad_x, part, B, C, H, W, Ho, Wo, s, p);
        else
            CNUDA_LAUNCH(dwconvt_bwd_kernel<8>, dim3(C, B), dim3(kT), 0, st, x, w, grad_y, grad_x, part, B, C, H, W, Ho, Wo, s, p);
        if (grad_w) launch_wsum(part, grad_w, B, C, k, st);
        return check_launch("cnuda_dwconvt2d_backward");
    }
    if (grad_x)
        CNUDA_LAUNCH_1D(dwconvt_bwd_data_kernel, (long long)B * C * H * W, st, grad_y, w, grad_x, B, C, H, W, Ho, Wo, k, s, p);
    if (grad_w)
        CNUDA_LAUNCH(dwconvt_bwd_weight_kernel, dim3(C, k * k), dim3(kT), 0, st, x, grad_y, grad_w, B, C, H, W, Ho,
                           Wo, k, s, p);
    return check_launch("cnuda_dwconvt2d_backward");
}

extern "C" int cnuda_add(const float* a, const float* b, float* out, long long n, cnuda_stream_t stream) {
    CNUDA_REQUIRE(a && b && out && n > 0, "cnuda_add: bad arguments");
    const long long n4 = aligned16(a, b, out) ? n / 4 : 0;
    CNUDA_LAUNCH_1D(add_kernel, n4 > 0 ? n4 : n, stream, a, b, out, n4, n);
    return check_launch("cnuda_add");
}
extern "C" int cnuda_act_backward(const float* grad_y, const float* y, float* grad_x, long long n, float slope,
                                  cnuda_stream_t stream) {
    CNUDA_REQUIRE(grad_y && y && grad_x && n > 0, "cnuda_act_backward: bad arguments");
    // 16-byte accesses for the aligned quads; a view at an odd offset takes the scalar loop, as in cnuda_add
    CNUDA_LAUNCH_1D(act_bwd_kernel, n, stream, grad_y, y, grad_x, aligned16(grad_y, y, grad_x) ? n / 4 : 0, n, slope);
    return check_launch("cnuda_act_backward");
}
extern "C" int cnuda_conv1x1_backward_data_act(const float* grad_y, const float* weight, const float* hidden,
                                               float* grad_hidden, int B, int Co, int Ch, long long HW, float slope,
                                               cnuda_stream_t stream) {
    CNUDA_REQUIRE(grad_y && weight && hidden && grad_hidden && B > 0 && Ch > 0 && HW > 0,
                  "cnuda_conv1x1_backward_data_act: bad arguments");
    CNUDA_REQUIRE(Co >= 1 && Co <= 8, "cnuda_conv1x1_backward_data_act: %d output channels (1..8 are built)", Co);
    CNUDA_REQUIRE((HW & 3) == 0 && B <= 65535, "cnuda_conv1x1_backward_data_act: plane size %lld not a multiple of 4",
                  HW);
    CNUDA_REQUIRE(aligned16(grad_y, hidden, grad_hidden),
                  "cnuda_conv1x1_backward_data_act: tensors must be 16-byte aligned");
    // enough workgroups for the chip: channel chunks of >= 32 until there are ~2048
    const long long quads = ceil_div(HW / 4, kT);
    int chunks = 1;
    while (chunks * 2 * 32 <= Ch && quads * B * chunks < 2048) chunks *= 2;
    const int ch_chunk = (int)ceil_div(Ch, chunks);
    const dim3 grid((unsigned)quads, (unsigned)ceil_div(Ch, ch_chunk), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
#define CNUDA_C1(CO) case CO: CNUDA_LAUNCH(conv1x1_dgrad_act_kernel<CO>, grid, dim3(kT), 0, st, grad_y, weight, \
                                                  hidden, grad_hidden, Ch, ch_chunk, HW, slope); break
    switch (Co) {
        CNUDA_C1(1); CNUDA_C1(2); CNUDA_C1(3); CNUDA_C1(4); CNUDA_C1(5); CNUDA_C1(6); CNUDA_C1(7); CNUDA_C1(8);
    }
#undef CNUDA_C1
    return check_launch("cnuda_conv1x1_backward_data_act");
}
// the row-wise launches: 16-byte copies where the rows allow them, and the grid -- a workgroup per 4,096 floats of a row,
// up to 65,535 rows along y (the kernels stride over the rest)
static int rows_vec_ok(long long HW, const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    return (HW & 3) == 0 && aligned16(a, b, c, d);
}
static dim3 rows_grid(long long HW, long long rows) {
    const int chunks = (int)((HW / 4 + kT * 4 - 1) / (kT * 4));
    return dim3(chunks > 0 ? chunks : 1, (unsigned)(rows < 65535 ? rows : 65535));
}
extern "C" int cnuda_copy_channels(const float* src, float* dst, int B, int Cn, long long HW, int Csrc, int src_off,
                                   int Cdst, int dst_off, cnuda_stream_t stream) {
    CNUDA_REQUIRE(src && dst && B > 0 && Cn > 0 && HW > 0, "cnuda_copy_channels: bad arguments");
    CNUDA_REQUIRE(src_off >= 0 && dst_off >= 0 && src_off + Cn <= Csrc && dst_off + Cn <= Cdst,
                  "cnuda_copy_channels: channel range out of bounds");
    const long long rows = (long long)B * Cn;
    CNUDA_REQUIRE(rows < (1ll << 31), "cnuda_copy_channels: too many planes");
    CNUDA_LAUNCH(copy_channels_kernel, rows_grid(HW, rows), dim3(kT), 0,
                       (hipStream_t)stream, src, dst, (int)rows, Cn, HW, Csrc, src_off, Cdst, dst_off, rows_vec_ok(HW, src, dst));
    return check_launch("cnuda_copy_channels");
}
extern "C" int cnuda_split_offset_mask(const float* om, float* offset, float* mask, int B, int taps, long long HW,
                                       cnuda_stream_t stream) {
    CNUDA_REQUIRE(om && offset && mask && B > 0 && taps > 0 && HW > 0, "cnuda_split_offset_mask: bad arguments");
    const long long rows = (long long)B * 3 * taps;
    CNUDA_REQUIRE(rows < (1ll << 31), "cnuda_split_offset_mask: too many planes");
    CNUDA_LAUNCH(split_offset_mask_kernel, rows_grid(HW, rows), dim3(kT), 0,
                       (hipStream_t)stream, om, offset, mask, (int)rows, taps, HW, rows_vec_ok(HW, om, offset, mask));
    return check_launch("cnuda_split_offset_mask");
}
extern "C" int cnuda_split_offset_mask_backward(const float* grad_offset, const float* grad_mask, const float* mask,
                                                float* grad_om, int B, int taps, long long HW, cnuda_stream_t stream) {
    CNUDA_REQUIRE(grad_offset && grad_mask && mask && grad_om && B > 0 && taps > 0 && HW > 0,
                  "cnuda_split_offset_mask_backward: bad arguments");
    const long long rows = (long long)B * 3 * taps;
    CNUDA_REQUIRE(rows < (1ll << 31), "cnuda_split_offset_mask_backward: too many planes");
    CNUDA_LAUNCH(split_offset_mask_bwd_kernel, rows_grid(HW, rows), dim3(kT), 0,
                       (hipStream_t)stream, grad_offset, grad_mask, mask, grad_om, (int)rows, taps, HW,
                       rows_vec_ok(HW, grad_offset, grad_mask, mask, grad_om));
    return check_launch("cnuda_split_offset_mask_backward");
}
