// HBM-bound kernels specific to the EfficientNet MBConv block (backends/efficientnet.py; NCHW fp32, all on the caller's
//   stream): swish, squeeze-and-excite (pool, gate, scale), drop-connect + residual, and the right / bottom zero-pad
//   copy in front of the dense stem.  (The block's depthwise convolution with TensorFlow "SAME" padding is
//   cnuda_dwconv2d_same_* in spatial.hip.)  No float atomics anywhere: every reduction has a fixed order, so two runs
//   give the same bits.
#include "common.h"

namespace cnuda {
namespace {

constexpr int kT = 256;

__device__ __forceinline__ float swishf(float v) { return v * sigmoid_f32(v); }
__device__ __forceinline__ float swish_gradf(float v) {
    const float s = sigmoid_f32(v);
    return s + v * s * (1.0f - s);
}

// ---------------- swish ----------------
__global__ void swish_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long n4 = n >> 2, step = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = i0; i < n4; i += step) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<float4*>(y)[i] = make_float4(swishf(v.x), swishf(v.y), swishf(v.z), swishf(v.w));
    }
    for (long long i = n4 * 4 + i0; i < n; i += step) y[i] = swishf(x[i]);
}
// gx = gy * (s + x*s*(1-s)), s = sigmoid(x): recomputed from the input, the output is not kept
__global__ void swish_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ gx,
                                 long long n) {
    const long long n4 = n >> 2, step = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = i0; i < n4; i += step) {
        const float4 g = reinterpret_cast<const float4*>(gy)[i], v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<float4*>(gx)[i] = make_float4(g.x * swish_gradf(v.x), g.y * swish_gradf(v.y),
                                                       g.z * swish_gradf(v.z), g.w * swish_gradf(v.w));
    }
    for (long long i = n4 * 4 + i0; i < n; i += step) gx[i] = gy[i] * swish_gradf(x[i]);
}

// ---------------- squeeze-and-excite ----------------
// One wave per (image, channel) plane: out[plane] = scale * sum_hw a[plane,hw] (* b[plane,hw]).  Each lane adds its
// strided share in order, then the wave's xor tree: a fixed order.  16-byte loads when HW % 4 == 0.
template <bool DOT>
__global__ __launch_bounds__(kT) void se_plane_sum_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ out, long long planes, int HW, float scale) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (kT / 64) + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * (kT / 64);
    for (long long p = wave; p < planes; p += nwaves) {
        const float* ap = a + p * HW;
        const float* bp = DOT ? b + p * HW : nullptr;
        float acc = 0.0f;
        if ((HW & 3) == 0) {
            for (int i = lane; i < (HW >> 2); i += 64) {
                const float4 u = reinterpret_cast<const float4*>(ap)[i];
                if (DOT) {
                    const float4 v = reinterpret_cast<const float4*>(bp)[i];
                    acc += (u.x * v.x + u.y * v.y) + (u.z * v.z + u.w * v.w);
                } else {
                    acc += (u.x + u.y) + (u.z + u.w);
                }
            }
        } else {
            for (int i = lane; i < HW; i += 64) acc += DOT ? ap[i] * bp[i] : ap[i];
        }
        acc = wave_sum(acc);
        if (lane == 0) out[p] = acc * scale;
    }
}
// One workgroup per image; dynamic LDS: pool[C] | hidden[Cse].
//   hpre[b,j] = b1[j] + sum_c W1[j,c] * pool[b,c]   (one wave per j: lanes stride c, xor tree)
//   gate[b,c] = sigmoid(b2[c] + sum_j W2[c,j] * swish(hpre[b,j]))   (one thread per c, j in order)
__global__ __launch_bounds__(kT) void se_gate_fwd_kernel(const float* __restrict__ pool, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ hpre,
                                                         float* __restrict__ gate, int C, int Cse) {
    extern __shared__ float lds[];
    float* sp = lds;
    float* sh = lds + C;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += kT) sp[c] = pool[(size_t)b * C + c];
    __syncthreads();
    for (int j = wid; j < Cse; j += kT / 64) {
        float acc = 0.0f;
        for (int c = lane; c < C; c += 64) acc += w1[(size_t)j * C + c] * sp[c];
        acc = wave_sum(acc) + b1[j];
        if (lane == 0) {
            hpre[(size_t)b * Cse + j] = acc;
            sh[j] = swishf(acc);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kT) {
        float acc = b2[c];
        for (int j = 0; j < Cse; ++j) acc += w2[(size_t)c * Cse + j] * sh[j];
        gate[(size_t)b * C + c] = sigmoid_f32(acc);
    }
}
// y[i] = x[i] * g[i / HW] (+ add[i / HW] with ADD: the backward's dx = dy*g + dpool/HW).  I: 32-bit indices while the
// tensor has fewer than 2^31 elements.  VEC 4 needs HW % 4 == 0 (a quad never straddles two planes).
template <typename I, int VEC, bool ADD>
__global__ void se_scale_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ add,
                                float* __restrict__ y, I nv, I HWv) {
    const I step = (I)gridDim.x * blockDim.x;
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += step) {
        const I p = i / HWv;
        const float s = g[p], a = ADD ? add[p] : 0.0f;
        if constexpr (VEC == 4) {
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(y)[i] = make_float4(v.x * s + a, v.y * s + a, v.z * s + a, v.w * s + a);
        } else {
            y[i] = x[i] * s + a;
        }
    }
}
// Backward of the gate, one workgroup per image; dynamic LDS: dz2[C] | dhpre[Cse].
//   dz2[c]   = dg[c] * g[c] * (1 - g[c])
//   dhpre[j] = swish'(hpre[j]) * sum_c W2[c,j] * dz2[c]      (one wave per j)
//   dpool[c] = (sum_j W1[j,c] * dhpre[j]) / HW               (one thread per c, j in order; the 1/HW of the mean folded in)
__global__ __launch_bounds__(kT) void se_gate_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ gate,
                                                         const float* __restrict__ hpre, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, float* __restrict__ dz2,
                                                         float* __restrict__ dhpre, float* __restrict__ dpool, int C,
                                                         int Cse, float inv_hw) {
    extern __shared__ float lds[];
    float* sz = lds;
    float* sh = lds + C;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += kT) {
        const float g = gate[(size_t)b * C + c];
        const float v = dg[(size_t)b * C + c] * g * (1.0f - g);
        sz[c] = v;
        dz2[(size_t)b * C + c] = v;
    }
    __syncthreads();
    for (int j = wid; j < Cse; j += kT / 64) {
        float acc = 0.0f;
        for (int c = lane; c < C; c += 64) acc += w2[(size_t)c * Cse + j] * sz[c];
        acc = wave_sum(acc) * swish_gradf(hpre[(size_t)b * Cse + j]);
        if (lane == 0) {
            sh[j] = acc;
            dhpre[(size_t)b * Cse + j] = acc;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kT) {
        float acc = 0.0f;
        for (int j = 0; j < Cse; ++j) acc += w1[(size_t)j * C + c] * sh[j];
        dpool[(size_t)b * C + c] = acc * inv_hw;
    }
}
// Parameter gradients, one thread per element of [W1 | W2 | b1 | b2], the images in increasing order:
//   dW1[j,c] = sum_b dhpre[b,j] * pool[b,c]    dW2[c,j] = sum_b dz2[b,c] * swish(hpre[b,j])
//   db1[j]   = sum_b dhpre[b,j]                db2[c]   = sum_b dz2[b,c]
// A null output is skipped.
__global__ void se_param_grad_kernel(const float* __restrict__ pool, const float* __restrict__ hpre,
                                     const float* __restrict__ dz2, const float* __restrict__ dhpre, float* __restrict__ gw1,
                                     float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2, int B, int C,
                                     int Cse) {
    const int nw = C * Cse;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float acc = 0.0f;
    if (i < nw) {
        if (!gw1) return;
        const int j = i / C, c = i - j * C;
        for (int b = 0; b < B; ++b) acc += dhpre[(size_t)b * Cse + j] * pool[(size_t)b * C + c];
        gw1[i] = acc;
    } else if (i < 2 * nw) {
        if (!gw2) return;
        const int k = i - nw, c = k / Cse, j = k - c * Cse;
        for (int b = 0; b < B; ++b) acc += dz2[(size_t)b * C + c] * swishf(hpre[(size_t)b * Cse + j]);
        gw2[k] = acc;
    } else if (i < 2 * nw + Cse) {
        if (!gb1) return;
        const int j = i - 2 * nw;
        for (int b = 0; b < B; ++b) acc += dhpre[(size_t)b * Cse + j];
        gb1[j] = acc;
    } else if (i < 2 * nw + Cse + C) {
        if (!gb2) return;
        const int c = i - 2 * nw - Cse;
        for (int b = 0; b < B; ++b) acc += dz2[(size_t)b * C + c];
        gb2[c] = acc;
    }
}

// ---------------- drop-connect + residual ----------------
// y[b,i] = x[b,i] * m[b] (+ r[b,i]; r nullable: the backward's dx = dy * m[b]).  VEC 4 needs per_image % 4 == 0.
template <typename I, int VEC>
__global__ void drop_connect_kernel(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ r,
                                    float* __restrict__ y, I nv, I per_image_v) {
    const I step = (I)gridDim.x * blockDim.x;
    for (I i = (I)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += step) {
        const float s = m[i / per_image_v];
        if constexpr (VEC == 4) {
            float4 v = reinterpret_cast<const float4*>(x)[i];
            v = make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
            if (r) {
                const float4 u = reinterpret_cast<const float4*>(r)[i];
                v = make_float4(v.x + u.x, v.y + u.y, v.z + u.z, v.w + u.w);
            }
            reinterpret_cast<float4*>(y)[i] = v;
        } else {
            y[i] = r ? x[i] * s + r[i] : x[i] * s;
        }
    }
}

// ---------------- zero-pad copy (right / bottom) ----------------
// y [planes, H+pb, W+pr]: x in the top-left corner, zeros elsewhere
__global__ void pad_rb_kernel(const float* __restrict__ x, float* __restrict__ y, long long planes, int H, int W, int Hp,
                              int Wp) {
    const long long total = planes * Hp * Wp, step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int ix = (int)(i % Wp);
        const long long row = i / Wp;
        const int iy = (int)(row % Hp);
        const long long p = row / Hp;
        y[i] = (ix < W && iy < H) ? x[(p * H + iy) * W + ix] : 0.0f;
    }
}

template <bool ADD>
int launch_scale(const float* x, const float* g, const float* add, float* y, long long planes, int HW, hipStream_t st) {
    const long long n = planes * HW;
    if ((HW & 3) == 0) {
        const long long nv = n >> 2;
        if (n < 2147483647LL)
            CNUDA_LAUNCH((se_scale_kernel<unsigned, 4, ADD>), dim3(stream_grid(nv, kT)), dim3(kT), 0, st, x, g, add, y,
                         (unsigned)nv, (unsigned)(HW >> 2));
        else
            CNUDA_LAUNCH((se_scale_kernel<long long, 4, ADD>), dim3(stream_grid(nv, kT)), dim3(kT), 0, st, x, g, add, y, nv,
                         (long long)(HW >> 2));
    } else {
        if (n < 2147483647LL)
            CNUDA_LAUNCH((se_scale_kernel<unsigned, 1, ADD>), dim3(stream_grid(n, kT)), dim3(kT), 0, st, x, g, add, y,
                         (unsigned)n, (unsigned)HW);
        else
            CNUDA_LAUNCH((se_scale_kernel<long long, 1, ADD>), dim3(stream_grid(n, kT)), dim3(kT), 0, st, x, g, add, y, n,
                         (long long)HW);
    }
    return 0;
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_swish_forward(const float* x, float* y, long long n, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && n > 0, "cnuda_swish_forward: bad arguments");
    CNUDA_LAUNCH(swish_fwd_kernel, dim3(stream_grid((n + 3) / 4, kT)), dim3(kT), 0, (hipStream_t)stream, x, y, n);
    return check_launch("cnuda_swish_forward");
}

extern "C" int cnuda_swish_backward(const float* grad_y, const float* x, float* grad_x, long long n, cnuda_stream_t stream) {
    CNUDA_REQUIRE(grad_y && x && grad_x && n > 0, "cnuda_swish_backward: bad arguments");
    CNUDA_LAUNCH(swish_bwd_kernel, dim3(stream_grid((n + 3) / 4, kT)), dim3(kT), 0, (hipStream_t)stream, grad_y, x, grad_x, n);
    return check_launch("cnuda_swish_backward");
}

static int se_geom(int B, int C, int Cse, long long HW, const char* who) {
    CNUDA_REQUIRE(B > 0 && C > 0 && Cse > 0 && HW > 0, "%s: bad geometry", who);
    // pool / dz2 [C] and the hidden vector [Cse] of one image live in LDS
    CNUDA_REQUIRE((size_t)(C + Cse) * sizeof(float) <= 60 * 1024, "%s: C + Cse = %d does not fit 60 KiB of LDS", who, C + Cse);
    CNUDA_REQUIRE(HW <= 2147483647LL && (long long)C * Cse <= 500000000LL, "%s: tensor too large", who);
    return 0;
}

extern "C" size_t cnuda_se_workspace_bytes(int B, int C, int Cse) {
    if (B <= 0 || C <= 0 || Cse <= 0) return 0;
    return ((size_t)3 * B * C + (size_t)B * Cse) * sizeof(float);      // dg, dz2, dpool [B,C]; dhpre [B,Cse]
}

extern "C" int cnuda_se_forward(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y,
                                float* pool, float* hpre, float* gate, int B, int C, int Cse, long long HW,
                                cnuda_stream_t stream) {
    if (int rc = se_geom(B, C, Cse, HW, "cnuda_se_forward")) return rc;
    CNUDA_REQUIRE(x && w1 && b1 && w2 && b2 && y && pool && hpre && gate, "cnuda_se_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long planes = (long long)B * C;
    CNUDA_LAUNCH(se_plane_sum_kernel<false>, dim3(stream_grid(planes, kT / 64)), dim3(kT), 0, st, x, (const float*)nullptr,
                 pool, planes, (int)HW, 1.0f / (float)HW);
    CNUDA_LAUNCH(se_gate_fwd_kernel, dim3(B), dim3(kT), (size_t)(C + Cse) * sizeof(float), st, pool, w1, b1, w2, b2, hpre,
                 gate, C, Cse);
    launch_scale<false>(x, gate, nullptr, y, planes, (int)HW, st);
    return check_launch("cnuda_se_forward");
}

extern "C" int cnuda_se_backward(const float* x, const float* grad_y, const float* w1, const float* w2, const float* pool,
                                 const float* hpre, const float* gate, float* grad_x, float* grad_w1, float* grad_b1,
                                 float* grad_w2, float* grad_b2, int B, int C, int Cse, long long HW, void* workspace,
                                 size_t workspace_bytes, cnuda_stream_t stream) {
    if (int rc = se_geom(B, C, Cse, HW, "cnuda_se_backward")) return rc;
    CNUDA_REQUIRE(x && grad_y && w1 && w2 && pool && hpre && gate && grad_x, "cnuda_se_backward: null pointer");
    CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_se_workspace_bytes(B, C, Cse), "cnuda_se_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const long long planes = (long long)B * C;
    float* dg = reinterpret_cast<float*>(workspace);
    float* dz2 = dg + planes;
    float* dpool = dz2 + planes;
    float* dhpre = dpool + planes;
    CNUDA_LAUNCH(se_plane_sum_kernel<true>, dim3(stream_grid(planes, kT / 64)), dim3(kT), 0, st, grad_y, x, dg, planes,
                 (int)HW, 1.0f);
    CNUDA_LAUNCH(se_gate_bwd_kernel, dim3(B), dim3(kT), (size_t)(C + Cse) * sizeof(float), st, dg, gate, hpre, w1, w2, dz2,
                 dhpre, dpool, C, Cse, 1.0f / (float)HW);
    if (grad_w1 || grad_b1 || grad_w2 || grad_b2)
        CNUDA_LAUNCH(se_param_grad_kernel, dim3(ceil_div(2LL * C * Cse + C + Cse, 256)), dim3(256), 0, st, pool, hpre, dz2,
                     dhpre, grad_w1, grad_b1, grad_w2, grad_b2, B, C, Cse);
    launch_scale<true>(grad_y, gate, dpool, grad_x, planes, (int)HW, st);
    return check_launch("cnuda_se_backward");
}

extern "C" int cnuda_drop_connect_add(const float* x, const float* mask, const float* residual, float* y, int B,
                                      long long per_image, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && mask && y && B > 0 && per_image > 0, "cnuda_drop_connect_add: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * per_image;
    if ((per_image & 3) == 0) {
        if (n < 2147483647LL)
            CNUDA_LAUNCH((drop_connect_kernel<unsigned, 4>), dim3(stream_grid(n >> 2, kT)), dim3(kT), 0, st, x, mask, residual, y,
                         (unsigned)(n >> 2), (unsigned)(per_image >> 2));
        else
            CNUDA_LAUNCH((drop_connect_kernel<long long, 4>), dim3(stream_grid(n >> 2, kT)), dim3(kT), 0, st, x, mask, residual, y,
                         n >> 2, per_image >> 2);
    } else {
        if (n < 2147483647LL)
            CNUDA_LAUNCH((drop_connect_kernel<unsigned, 1>), dim3(stream_grid(n, kT)), dim3(kT), 0, st, x, mask, residual, y,
                         (unsigned)n, (unsigned)per_image);
        else
            CNUDA_LAUNCH((drop_connect_kernel<long long, 1>), dim3(stream_grid(n, kT)), dim3(kT), 0, st, x, mask, residual, y, n,
                         per_image);
    }
    return check_launch("cnuda_drop_connect_add");
}

extern "C" int cnuda_pad_right_bottom(const float* x, float* y, long long planes, int H, int W, int pad_bottom, int pad_right,
                                      cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && planes > 0 && H > 0 && W > 0 && pad_bottom >= 0 && pad_right >= 0,
                  "cnuda_pad_right_bottom: bad arguments");
    const int Hp = H + pad_bottom, Wp = W + pad_right;
    CNUDA_LAUNCH(pad_rb_kernel, dim3(stream_grid(planes * Hp * Wp, kT)), dim3(kT), 0, (hipStream_t)stream, x, y, planes, H, W,
                 Hp, Wp);
    return check_launch("cnuda_pad_right_bottom");
}
