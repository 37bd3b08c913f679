// Dense teacher (uda.DenseTeacher; DESIGN.md, "Dense teacher") for gfx950: the student regresses the teacher's heat map
// inside the top `ratio` of every image's positions.  No reference counterpart (Dense Teacher, Zhou et al., ECCV 2022).
//   cnuda_dense_select            score keys (grid-wide) + an exact radix select per image -> tau [B], count [B]
//   cnuda_dense_teacher_forward   quality focal loss + score-weighted L1 of the sizes, fp64 sums in a fixed order
//   cnuda_dense_teacher_backward  both gradients, written whole by one launch
// The definitions are in include/centernet_uda_hip.h; tests/dense_teacher_oracle.py restates them in float64.
#include <math.h>

#include <initializer_list>

#include "common.h"

namespace cnuda {
namespace {

constexpr int kT = 256;
constexpr int kLossBlocks = 1024;        // rows of partial sums: cnuda_loss_workspace_bytes() holds 1024 x 3 doubles
constexpr int kDenseMaxClasses = 1024;   // the class limit of the library's per-image tables (loss.hip kIwMaxClasses)
constexpr int kSelectThreads = 1024;
constexpr long long kSelectOnChip = 32768;   // keys (128 KiB) an image may have to be selected from LDS

__device__ __forceinline__ float sgnf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// ---------------- the score and its key ----------------
// One position's score over the channels: the maximum, NaN as soon as one channel is.
struct Score {
    float mx = -INFINITY;
    bool nan = false;
    __device__ __forceinline__ void add(float v) {
        nan |= (v != v);
        mx = v > mx ? v : mx;
    }
    __device__ __forceinline__ float value() const { return nan ? NAN : mx; }
};
// float -> a 32-bit key in the order of the values: NaN -> 0, -inf -> 0x007fffff, ..., -0 and +0 -> 0x80000000, ...
__device__ __forceinline__ unsigned score_key(float s) {
    if (s != s) return 0u;
    const unsigned u = __float_as_uint(s + 0.0f);   // -0 + 0 = +0: the two zeros share a key
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(unsigned key) {   // of a number's key
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(kT) void dense_score_kernel(const float* __restrict__ t_hm, unsigned* __restrict__ keys,
                                                         int B, int C, long long HW) {
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
        const long long b = i / HW, p = i - b * HW;
        const float* px = t_hm + (size_t)b * C * HW + p;
        Score s;
        for (int c = 0; c < C; ++c) s.add(px[(size_t)c * HW]);
        keys[i] = score_key(s.value());
    }
}

// One workgroup per image: the k-th largest key by four 8-bit digits from the top.  A pass counts, among the keys
// that share the digits found so far, each value of the next digit (LDS integer atomics); thread d < 256 then sums the
// counts above digit d, and the one digit with above < k <= above + hist[d] is the key's.  `greater` collects the
// keys strictly above the k-th one, so count = greater + (keys equal to it): every tie is in, whatever the order.
// OnChip: the image's keys are copied into dynamic LDS once; otherwise every pass re-reads them from memory.
template <bool OnChip>
__global__ __launch_bounds__(kSelectThreads) void dense_select_kernel(const unsigned* __restrict__ keys_all,
                                                                      float* __restrict__ tau, int* __restrict__ count,
                                                                      long long HW, long long k) {
    extern __shared__ unsigned held[];
    __shared__ int hist[256];
    __shared__ unsigned s_prefix;
    __shared__ long long s_k, s_greater;
    __shared__ int s_equal;
    const int b = blockIdx.x;
    const unsigned* keys = keys_all + (size_t)b * HW;
    if (OnChip) {
        for (long long i = threadIdx.x; i < HW; i += kSelectThreads) held[i] = keys[i];
        keys = held;
    }
    if (threadIdx.x == 0) { s_prefix = 0u; s_k = k; s_greater = 0; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix;
        const unsigned high = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        for (long long i = threadIdx.x; i < HW; i += kSelectThreads) {
            const unsigned key = keys[i];
            if ((key & high) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const long long want = s_k;
        long long above = 0;
        int mine = 0;
        if (threadIdx.x < 256) {
            mine = hist[threadIdx.x];
            for (int d = threadIdx.x + 1; d < 256; ++d) above += hist[d];
        }
        __syncthreads();   // s_k and s_prefix are read by all before the one writer below
        if (threadIdx.x < 256 && above < want && want <= above + mine) {
            s_prefix = prefix | ((unsigned)threadIdx.x << shift);
            s_k = want - above;
            s_greater += above;
            s_equal = mine;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned key = s_prefix;
        // key 0: fewer than k numbers in the image; every number is selected and no NaN
        tau[b] = key ? key_score(key) : -INFINITY;
        count[b] = (int)(s_greater + (key ? s_equal : 0));
    }
}

// ---------------- the walk shared by the loss and its gradient ----------------
// An item is V consecutive cells of one row of the STUDENT's maps (V = 4: 16-byte accesses, W % 4 == 0 and aligned
// bases; V = 1 otherwise).  With the mirror its teacher cells are the V cells that end at W - 1 - x, read as one vector
// and reversed inside it: both sides stay coalesced.
template <int V> struct Vec;
template <> struct Vec<1> {
    float v[1];
    __device__ __forceinline__ static Vec load(const float* p) { return {{p[0]}}; }
    __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <> struct Vec<4> {
    float v[4];
    __device__ __forceinline__ static Vec load(const float* p) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        return {{q.x, q.y, q.z, q.w}};
    }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
struct DenseMaps {
    const float *hm, *wh, *t_hm, *t_wh, *tau;
    int B, C, H, W, mirror;
};
template <int V>
struct DenseItem {
    int b;
    size_t s_off, t_off;   // the item's first cell inside one [H, W] plane: student's, teacher's
    size_t HW;
    bool sel[V];           // by STUDENT cell j
    float u[V];            // sigmoid(score) where selected, else 0
    bool any;
    // of a teacher vector, the element that student cell j looks at (j is an unrolled constant: two fixed registers)
    __device__ __forceinline__ static float pick(const float (&t)[V], int j, int mirror) {
        return mirror ? t[V - 1 - j] : t[j];
    }
    __device__ __forceinline__ DenseItem(const DenseMaps& m, long long item) {
        const int wq = m.W / V;
        const int xq = (int)(item % wq);
        const long long row = item / wq;
        const int y = (int)(row % m.H);
        b = (int)(row / m.H);
        HW = (size_t)m.H * m.W;
        s_off = (size_t)y * m.W + (size_t)xq * V;
        t_off = m.mirror ? (size_t)y * m.W + (size_t)(m.W - V - xq * V) : s_off;
        Score sc[V];
        const float* px = m.t_hm + (size_t)b * m.C * HW + t_off;
        for (int c = 0; c < m.C; ++c) {
            const Vec<V> t = Vec<V>::load(px + (size_t)c * HW);
#pragma unroll
            for (int j = 0; j < V; ++j) sc[j].add(t.v[j]);
        }
        const float th = m.tau[b];
        float sv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) sv[j] = sc[j].value();
        any = false;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float s = pick(sv, j, m.mirror);
            sel[j] = s >= th;
            u[j] = sel[j] ? sigmoid_f32(s) : 0.0f;
            any |= sel[j];
        }
    }
    // channel c: the student's logits and the targets y (0 off the selection; the teacher is read only when needed)
    __device__ __forceinline__ void channel(const DenseMaps& m, int c, Vec<V>& x, Vec<V>& y) const {
        const size_t plane = ((size_t)b * m.C + c) * HW;
        x = Vec<V>::load(m.hm + plane + s_off);
#pragma unroll
        for (int j = 0; j < V; ++j) y.v[j] = 0.0f;
        if (any) {
            const Vec<V> t = Vec<V>::load(m.t_hm + plane + t_off);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (sel[j]) y.v[j] = sigmoid_f32(pick(t.v, j, m.mirror));
        }
    }
    // size channel c (0, 1): student minus teacher per student cell
    __device__ __forceinline__ Vec<V> size_residual(const DenseMaps& m, int c) const {
        const size_t plane = ((size_t)b * 2 + c) * HW;
        const Vec<V> x = Vec<V>::load(m.wh + plane + s_off), t = Vec<V>::load(m.t_wh + plane + t_off);
        Vec<V> r;
#pragma unroll
        for (int j = 0; j < V; ++j) r.v[j] = x.v[j] - pick(t.v, j, m.mirror);
        return r;
    }
};
__device__ __forceinline__ float bce_logits(float x, float y) {
    return fmaxf(x, 0.0f) - x * y + log1pf(expf(-fabsf(x)));
}

// partial[blk*3 + {0,1,2}] = sum (y - q)^2 bce, sum u |residuals|, sum u
template <int V>
__global__ __launch_bounds__(kT) void dense_loss_kernel(DenseMaps m, double* __restrict__ partial, long long items) {
    __shared__ double red[16];
    double s_hm = 0.0, s_wh = 0.0, s_u = 0.0;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < items; i += (long long)gridDim.x * kT) {
        const DenseItem<V> it(m, i);
        for (int c = 0; c < m.C; ++c) {
            Vec<V> x, y;
            it.channel(m, c, x, y);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = y.v[j] - sigmoid_f32(x.v[j]);
                s_hm += (double)((d * d) * bce_logits(x.v[j], y.v[j]));
            }
        }
        if (it.any) {
            const Vec<V> r0 = it.size_residual(m, 0), r1 = it.size_residual(m, 1);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (!it.sel[j]) continue;
                s_wh += (double)(it.u[j] * (fabsf(r0.v[j]) + fabsf(r1.v[j])));
                s_u += (double)it.u[j];
            }
        }
    }
    s_hm = block_sum(s_hm, red);
    s_wh = block_sum(s_wh, red);
    s_u = block_sum(s_u, red);
    if (threadIdx.x == 0) {
        double* row = partial + (size_t)blockIdx.x * 3;
        row[0] = s_hm; row[1] = s_wh; row[2] = s_u;
    }
}
// One workgroup re-sums the partial rows in their order and writes out5.
__global__ __launch_bounds__(kT) void dense_finalize_kernel(const double* __restrict__ partial, int blocks,
                                                            const int* __restrict__ count, int B, float hm_weight,
                                                            float wh_weight, float* __restrict__ out5) {
    __shared__ double red[16];
    double acc[3] = {};
    for (int i = threadIdx.x; i < blocks; i += kT)
        for (int k = 0; k < 3; ++k) acc[k] += partial[(size_t)i * 3 + k];
    for (int k = 0; k < 3; ++k) acc[k] = block_sum(acc[k], red);
    if (threadIdx.x == 0) {
        long long n = 0;
        for (int b = 0; b < B; ++b) n += count[b];
        const double hm_loss = acc[0] / (double)(n > 1 ? n : 1), wh_loss = acc[1] / (acc[2] + 1e-4);
        out5[0] = (float)((double)hm_weight * hm_loss + (double)wh_weight * wh_loss);
        out5[1] = (float)hm_loss;
        out5[2] = (float)wh_loss;
        out5[3] = (float)n;
        out5[4] = (float)acc[2];
    }
}

template <int V>
__global__ __launch_bounds__(kT) void dense_grad_kernel(DenseMaps m, const float* __restrict__ out5,
                                                        const float* __restrict__ upstream, float hm_weight,
                                                        float wh_weight, float* __restrict__ grad_hm,
                                                        float* __restrict__ grad_wh, long long items) {
    const float up = upstream[0];
    const float k_hm = up * hm_weight / fmaxf(out5[3], 1.0f), k_wh = up * wh_weight / (out5[4] + 1e-4f);
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < items; i += (long long)gridDim.x * kT) {
        const DenseItem<V> it(m, i);
        for (int c = 0; c < m.C; ++c) {
            Vec<V> x, y, g;
            it.channel(m, c, x, y);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float q = sigmoid_f32(x.v[j]), d = q - y.v[j];
                g.v[j] = d * (d * d + 2.0f * q * (1.0f - q) * bce_logits(x.v[j], y.v[j])) * k_hm;
            }
            g.store(grad_hm + ((size_t)it.b * m.C + c) * it.HW + it.s_off);
        }
        for (int c = 0; c < 2; ++c) {
            Vec<V> g;
#pragma unroll
            for (int j = 0; j < V; ++j) g.v[j] = 0.0f;
            if (it.any) {
                const Vec<V> r = it.size_residual(m, c);
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (it.sel[j]) g.v[j] = it.u[j] * sgnf(r.v[j]) * k_wh;
            }
            g.store(grad_wh + ((size_t)it.b * 2 + c) * it.HW + it.s_off);
        }
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

static bool dense_shape_ok(int B, int C, long long HW) {
    return B > 0 && C > 0 && HW > 0 && HW <= 0x7fffffffLL;
}

extern "C" size_t cnuda_dense_select_workspace_bytes(int B, long long HW) {
    if (!dense_shape_ok(B, 1, HW)) return 0;
    return (size_t)B * (size_t)HW * sizeof(unsigned) + 256;
}

extern "C" int cnuda_dense_select(const float* teacher_hm, double ratio, float* tau, int32_t* count, int B, int C,
                                  long long HW, void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(teacher_hm && tau && count && dense_shape_ok(B, C, HW), "cnuda_dense_select: bad arguments");
    CNUDA_REQUIRE(ratio > 0.0 && ratio <= 1.0, "cnuda_dense_select: ratio %g outside (0, 1]", ratio);
    CNUDA_REQUIRE(C <= kDenseMaxClasses, "cnuda_dense_select: %d classes, the library's tables hold %d", C,
                  kDenseMaxClasses);
    CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_dense_select_workspace_bytes(B, HW),
                  "cnuda_dense_select: workspace");
    hipStream_t st = (hipStream_t)stream;
    unsigned* keys = reinterpret_cast<unsigned*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    long long k = (long long)floor(ratio * (double)HW);
    if (k < 1) k = 1;
    CNUDA_LAUNCH(dense_score_kernel, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0, st, teacher_hm, keys, B, C,
                 HW);
    if (HW <= kSelectOnChip) {
        const size_t lds = (size_t)HW * sizeof(unsigned);
        CNUDA_REQUIRE(raise_dynamic_lds(reinterpret_cast<const void*>(&dense_select_kernel<true>), lds),
                      "cnuda_dense_select: dynamic LDS");
        CNUDA_LAUNCH(dense_select_kernel<true>, dim3(B), dim3(kSelectThreads), lds, st, keys, tau, (int*)count, HW, k);
    } else {
        CNUDA_LAUNCH(dense_select_kernel<false>, dim3(B), dim3(kSelectThreads), 0, st, keys, tau, (int*)count, HW, k);
    }
    return check_launch("cnuda_dense_select");
}

// -> the item width (4 or 1) of the loss walk over these maps
static int dense_item_width(int W, std::initializer_list<const void*> maps) {
    if (W % 4) return 1;
    for (const void* p : maps)
        if (!aligned16(p)) return 1;
    return 4;
}

extern "C" int cnuda_dense_teacher_forward(const float* hm, const float* wh, const float* teacher_hm,
                                           const float* teacher_wh, const float* tau, const int32_t* count,
                                           float* out5, int B, int C, int H, int W, int mirror, float hm_weight,
                                           float wh_weight, void* workspace, size_t workspace_bytes,
                                           cnuda_stream_t stream) {
    CNUDA_REQUIRE(hm && wh && teacher_hm && teacher_wh && tau && count && out5 && H > 0 && W > 0 &&
                      dense_shape_ok(B, C, (long long)H * W), "cnuda_dense_teacher_forward: bad arguments");
    CNUDA_REQUIRE(C <= kDenseMaxClasses, "cnuda_dense_teacher_forward: %d classes, the library's tables hold %d", C,
                  kDenseMaxClasses);
    CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_loss_workspace_bytes(), "cnuda_dense_teacher_forward: workspace");
    hipStream_t st = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const DenseMaps m{hm, wh, teacher_hm, teacher_wh, tau, B, C, H, W, mirror ? 1 : 0};
    const int V = dense_item_width(W, {hm, wh, teacher_hm, teacher_wh});
    const long long items = (long long)B * H * (W / V);
    int blocks = stream_grid(items, kT);
    if (blocks > kLossBlocks) blocks = kLossBlocks;
    if (V == 4) CNUDA_LAUNCH(dense_loss_kernel<4>, dim3(blocks), dim3(kT), 0, st, m, partial, items);
    else CNUDA_LAUNCH(dense_loss_kernel<1>, dim3(blocks), dim3(kT), 0, st, m, partial, items);
    CNUDA_LAUNCH(dense_finalize_kernel, dim3(1), dim3(kT), 0, st, partial, blocks, (const int*)count, B, hm_weight,
                 wh_weight, out5);
    return check_launch("cnuda_dense_teacher_forward");
}

extern "C" int cnuda_dense_teacher_backward(const float* hm, const float* wh, const float* teacher_hm,
                                            const float* teacher_wh, const float* tau, const float* out5,
                                            const float* upstream, float* grad_hm, float* grad_wh, int B, int C, int H,
                                            int W, int mirror, float hm_weight, float wh_weight,
                                            cnuda_stream_t stream) {
    CNUDA_REQUIRE(hm && wh && teacher_hm && teacher_wh && tau && out5 && upstream && grad_hm && grad_wh && H > 0 &&
                      W > 0 && dense_shape_ok(B, C, (long long)H * W), "cnuda_dense_teacher_backward: bad arguments");
    CNUDA_REQUIRE(C <= kDenseMaxClasses, "cnuda_dense_teacher_backward: %d classes, the library's tables hold %d", C,
                  kDenseMaxClasses);
    const DenseMaps m{hm, wh, teacher_hm, teacher_wh, tau, B, C, H, W, mirror ? 1 : 0};
    const int V = dense_item_width(W, {hm, wh, teacher_hm, teacher_wh, grad_hm, grad_wh});
    const long long items = (long long)B * H * (W / V);
    const int blocks = stream_grid(items, kT);
    hipStream_t st = (hipStream_t)stream;
    if (V == 4)
        CNUDA_LAUNCH(dense_grad_kernel<4>, dim3(blocks), dim3(kT), 0, st, m, out5, upstream, hm_weight, wh_weight,
                     grad_hm, grad_wh, items);
    else
        CNUDA_LAUNCH(dense_grad_kernel<1>, dim3(blocks), dim3(kT), 0, st, m, out5, upstream, hm_weight, wh_weight,
                     grad_hm, grad_wh, items);
    return check_launch("cnuda_dense_teacher_backward");
}
