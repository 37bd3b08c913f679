// Detection and UDA losses for gfx950 (fp32 values, fp64 block reductions).
// Replaces, on device and without host synchronisation:
//   utils/tensor.py:5-7         _sigmoid (clamp(sigmoid, 1e-4, 1-1e-4))
//   losses/centernet.py:69-95   FocalLoss._neg_loss (incl. the num_pos == 0 branch, Q11)
//   losses/centernet.py:98-133  RegL1Loss (+ rotated), :192-223 PeriodicRegL1Loss, :136-189 KPSL1Loss
//   losses/entropy.py:10-28     EntropyLoss      losses/max_square.py:6-14 MaxSquareLoss
//   utils/image.py:121-124      entropy_map      losses/advent.py:10-18    BCE-with-logits vs constant
//   image-wise class-balanced max-squares (ICCV 2019, not in the reference): argmax histogram, weights, loss
//   multi-level self-produced guidance (same paper, not in the reference): labels from two heat maps, their cross-entropy
// Every loss is a pair (forward -> scalar(s) in device memory, backward ->
// gradient w.r.t. the logits given a device-resident upstream scalar).
// The shared pieces keep every order of operations and so the bits: tests/test_gpu_loss_bits.py.
#include "common.h"

namespace cnuda {
namespace {

constexpr int kT = 256;
constexpr int kLossBlocks = 1024;

__device__ __forceinline__ float sgnf(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ bool in_clamp(float s) { return s >= kProbLo && s <= kProbHi; }   // clamp passes gradient

// ---------------- the reduction tail ----------------
// Every thread's N fp64 sums -> the block's (valid in thread 0), one after the other through `red`.  N is 1, 2 or 3: the
// loops over the sums unroll, and the sums stay in registers (no loss kernel has scratch: profiles/loss_dedupe_ab.txt).
template <int N>
__device__ __forceinline__ void block_sums(double (&acc)[N], double* red) {
    for (int k = 0; k < N; ++k) acc[k] = block_sum(acc[k], red);
}
// The tail of a reducing forward: partial[blk*N + k] receives the block's k-th sum.  (The accumulation loop stays in the
// kernel, on named sums: focal's three sums behind a lambda went to scratch or cost an add each per item.)
template <int N>
__device__ __forceinline__ void store_partials(double (&acc)[N], double* __restrict__ partial, double* red) {
    block_sums(acc, red);
    if (threadIdx.x == 0)
        for (int k = 0; k < N; ++k) partial[(size_t)blockIdx.x * N + k] = acc[k];
}
// One workgroup re-sums the `blocks` partial rows; epilogue(sums, out) turns them into the loss.
template <class Epilogue>
__global__ void finalize_kernel(const double* __restrict__ partial, int blocks, Epilogue epilogue,
                                float* __restrict__ out) {
    __shared__ double red[16];
    double acc[Epilogue::N] = {};
    for (int i = threadIdx.x; i < blocks; i += blockDim.x)
        for (int k = 0; k < Epilogue::N; ++k) acc[k] += partial[(size_t)i * Epilogue::N + k];
    block_sums(acc, red);
    if (threadIdx.x == 0) epilogue(acc, out);
}
struct ScaleEpilogue {   // the scalar losses: out[0] = sum * scale
    static constexpr int N = 1;
    double scale;
    __device__ void operator()(const double (&s)[1], float* out) const { out[0] = (float)(s[0] * scale); }
};

// ---------------- focal ----------------
// partial[blk*3 + {0,1,2}] = sum pos_loss, sum neg_loss, num_pos
__global__ __launch_bounds__(kT) void focal_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                       float* __restrict__ prob, double* __restrict__ partial,
                                                       long long n) {
    __shared__ double red[16];
    double ps = 0.0, ns = 0.0, np = 0.0;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < n; i += (long long)gridDim.x * kT) {
        const float p = sigmoid_clamped(logits[i]);
        prob[i] = p;
        const float g = gt[i];
        if (g == 1.0f) {
            const float q = 1.0f - p;
            ps += (double)(logf(p) * (q * q));
            np += 1.0;
        } else if (g < 1.0f) {
            const float w = 1.0f - g, w2 = w * w;
            ns += (double)(logf(1.0f - p) * (p * p) * (w2 * w2));
        }
    }
    double acc[3] = {ps, ns, np};
    store_partials(acc, partial, red);
}
struct FocalEpilogue {   // out[0] = loss, out[1] = num_pos (kept for backward)
    static constexpr int N = 3;
    float weight;
    __device__ void operator()(const double (&s)[3], float* out) const {
        const float pos = (float)s[0], neg = (float)s[1], n = (float)s[2];
        const float loss = (n == 0.0f) ? (0.0f - neg) : (0.0f - (pos + neg) / n);
        out[0] = loss * weight;
        out[1] = n;
    }
};
// dlogits = upstream * weight * dL/dp * dp/dx
__global__ void focal_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                 const float* __restrict__ fwd_out, const float* __restrict__ upstream, float weight,
                                 float* __restrict__ grad, long long n) {
    const float np = fwd_out[1];
    const float scale = upstream[0] * weight * (np == 0.0f ? -1.0f : -1.0f / np);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float s = sigmoid_f32(logits[i]);
        float gval = 0.0f;
        if (in_clamp(s)) {
            const float p = s, q = 1.0f - s, g = gt[i];
            float dldp = 0.0f;
            if (g == 1.0f) {
                if (np != 0.0f) dldp = (q * q) / p - 2.0f * q * logf(p);
            } else if (g < 1.0f) {
                const float w = 1.0f - g, w2 = w * w;
                dldp = (2.0f * p * logf(q) - (p * p) / q) * (w2 * w2);
            }
            gval = scale * dldp * (s * q);
        }
        grad[i] = gval;
    }
}

// ---------------- gather + masked L1: what the wh / reg / angle loss and the keypoint loss share ----------------
// feat [B,ch,HW] is gathered at ind [B,M]; prediction and target are multiplied by the mask, the batch's target tensor
// is masked in place (Q2); out[0] = loss, out[1] = denominator (expanded-mask sum + 1e-4): the backward divides by it.
// The forwards run in a single workgroup (B*M*ch is tens of thousands at most, M = max_detections); the backwards
// scatter-add into a zero-initialised grad [B,ch,HW].
// `ind` comes from the data loader (datasets/coco.py:211).  The reference's torch.gather device-asserts on an index
// outside [0, HW) (e.g. targets encoded for another output size); here such a row never touches memory: the forward
// kernels read cell 0 instead and poison the loss with NaN (loud, no host sync), the backward kernels skip the row.
__device__ __forceinline__ bool ind_ok(long long id, long long HW) { return id >= 0 && id < HW; }
__device__ __forceinline__ long long fwd_cell(long long id, long long HW, double& poisoned) {
    if (!ind_ok(id, HW)) { id = 0; poisoned = (double)NAN; }
    return id;
}
struct L1Elem { int c, bm, b; };   // element i of a [B,M,ch] tensor: channel, row of [B,M], image
__device__ __forceinline__ L1Elem l1_elem(int i, int ch, int M) { return {i % ch, i / ch, i / ch / M}; }
__device__ __forceinline__ size_t feat_at(int b, int ch, int c, size_t HW, long long id) {
    return ((size_t)b * ch + c) * HW + id;
}
// -> prediction * m; the masked target is returned and written back in place
__device__ __forceinline__ float masked_pair(const float* __restrict__ feat, size_t cell, float* __restrict__ target,
                                             size_t t, float m, float& tg) {
    const float pred = feat[cell] * m;
    tg = target[t] * m;
    target[t] = tg;
    return pred;
}
// s[0]: the main L1 sum, s[1]: the second term's (angle / pair distance), s[2]: the mask sum; valid in thread 0
__device__ __forceinline__ void l1_epilogue(const double (&s)[3], float weight, bool second, float second_weight,
                                            float* __restrict__ out) {
    const float denom = (float)s[2] + 1e-4f;
    float loss = (float)s[0] / denom * weight;
    if (second) loss += (float)s[1] / denom * second_weight;
    out[0] = loss;
    out[1] = denom;
}
__device__ __forceinline__ float l1_upstream(const float* up, const float* fwd_out) { return up[0] / fwd_out[1]; }

// ---------------- wh / reg / angle ----------------
// mode 0: plain (ch 2 or 3: with 3 channels = rotated non-periodic: angle through clamped sigmoid)
// mode 1: periodic angle
constexpr float kPi = 3.14159265358979323846f;
// PeriodicRegL1Loss: the clamped sigmoid `ps` spans (-pi, pi), the target is in degrees -> remainder(d - pi/2, pi) - pi/2
__device__ __forceinline__ float periodic_residual(float ps, float tg) {
    const float pa = ps * 2.0f * kPi - kPi;
    const float ta = tg * (kPi / 180.0f);
    float r = fmodf((pa - ta) - kPi / 2.0f, kPi);
    if (r != 0.0f && r < 0.0f) r += kPi;   // torch.remainder: sign of the divisor
    return r - kPi / 2.0f;
}
__global__ __launch_bounds__(kT) void regl1_fwd_kernel(const float* __restrict__ feat, const unsigned char* __restrict__ mask,
                                                       const long long* __restrict__ ind, float* __restrict__ target,
                                                       int B, int M, int ch, int HW, int mode, float weight,
                                                       float angle_weight, float* __restrict__ out) {
    __shared__ double red[16];
    double s_wh = 0.0, s_a = 0.0, s_m = 0.0;   // named, not s[k]: the compiler then keeps one add per branch
    for (int i = threadIdx.x; i < B * M; i += kT) {
        const int b = i / M;
        const float m = mask[i] ? 1.0f : 0.0f;
        const long long id = fwd_cell(ind[i], HW, s_wh);
        for (int c = 0; c < ch; ++c) {
            const size_t t = (size_t)i * ch + c;
            float tg;
            const float pred = masked_pair(feat, feat_at(b, ch, c, HW, id), target, t, m, tg);
            s_m += (double)m;
            if (ch == 3 && c == 2) {
                const float ps = sigmoid_clamped(pred);
                if (mode == 0) {
                    const float tsig = sigmoid_f32(tg);
                    target[t] = tsig;   // target[...,2:3].sigmoid_() is in place too (Q2)
                    s_a += (double)fabsf(ps - clamp_prob(tsig));
                } else {
                    s_a += (double)fabsf(periodic_residual(ps, tg));
                }
            } else {
                s_wh += (double)fabsf(pred - tg);
            }
        }
    }
    double s[3] = {s_wh, s_a, s_m};
    block_sums(s, red);
    if (threadIdx.x == 0) l1_epilogue(s, weight, ch == 3, angle_weight, out);
}
// `target` is the (already masked / sigmoided) tensor
__global__ void regl1_bwd_kernel(const float* __restrict__ feat, const unsigned char* __restrict__ mask,
                                 const long long* __restrict__ ind, const float* __restrict__ target,
                                 const float* __restrict__ fwd_out, const float* __restrict__ upstream, int B, int M,
                                 int ch, int HW, int mode, float weight, float angle_weight, float* __restrict__ grad) {
    const float up = l1_upstream(upstream, fwd_out);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * M * ch; i += gridDim.x * blockDim.x) {
        const L1Elem e = l1_elem(i, ch, M);
        if (!mask[e.bm]) continue;
        const long long id = ind[e.bm];
        if (!ind_ok(id, HW)) continue;
        const size_t cell = feat_at(e.b, ch, e.c, HW, id);
        const float pred = feat[cell];
        const float tg = target[i];
        float g;
        if (ch == 3 && e.c == 2) {
            const float s = sigmoid_f32(pred);
            const float ds = in_clamp(s) ? s * (1.0f - s) : 0.0f;
            const float ps = clamp_prob(s);
            if (mode == 0) g = sgnf(ps - clamp_prob(tg)) * ds * angle_weight;   // target already holds sigmoid(target)
            else g = sgnf(periodic_residual(ps, tg)) * (2.0f * kPi) * ds * angle_weight;
        } else {
            g = sgnf(pred - tg) * weight;
        }
        atomicAdd(grad + cell, g * up);
    }
}

// ---------------- softmax-over-channels losses ----------------
// One pixel's softmax over the channels: i -> (b, hw), the channel maximum, the denominator.  Channels are visited in
// ascending order here and by every user; v(c) is recomputed at each use (C is 80 for COCO: no per-thread array).
struct SoftmaxPixel {
    const float* px;   // channel 0 of this pixel: x + base
    size_t base, HW;
    float mx, den;
    __device__ __forceinline__ SoftmaxPixel(const float* x, long long i, int C, long long HW_) : HW(HW_) {
        const long long b = i / HW_, hw = i - b * HW_;
        base = (size_t)b * C * HW_ + hw;
        px = x + base;
        mx = px[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, px[(size_t)c * HW]);
        den = 0.0f;
        for (int c = 0; c < C; ++c) den += expf(px[(size_t)c * HW] - mx);
    }
    __device__ __forceinline__ size_t at(int c) const { return base + (size_t)c * HW; }
    __device__ __forceinline__ float v(int c) const { return expf(px[(size_t)c * HW] - mx) / den; }
};
// f(v) = v*log2(v + 1e-30);   f'(v) = log2(v + eps) + v / ((v + eps) ln 2)
__device__ __forceinline__ float fent(float v) { return v * log2f(v + 1e-30f); }
__device__ __forceinline__ float dfent(float v) { return log2f(v + 1e-30f) + v / ((v + 1e-30f) * 0.6931471805599453f); }

// A scalar softmax loss is scale * sum over pixels of pixel(sum_c each(v_c)).  Its term gives the host's scale and
//   each(v), slope(v) = each'(v), pixel(s), and coef(up, s) = up * pixel'(s)   (up = upstream * scale)
// so that dx_j = coef * v_j * (slope_j - sum_i v_i slope_i).  A term is built on the device from (C, param).
struct EntropyTerm {     // EntropyLoss = -sum f(v) / (n*h*w*log2 c)
    static double scale(int B, int C, long long HW) { return -1.0 / ((double)B * (double)HW * (double)log2f((float)C)); }
    __device__ EntropyTerm(int, float) {}
    __device__ float each(float v) const { return fent(v); }
    __device__ float slope(float v) const { return dfent(v); }
    __device__ float pixel(float s) const { return s; }
    __device__ float coef(float up, float) const { return up; }
};
struct MaxSquareTerm {   // MaxSquareLoss = -mean(v^2)/2
    static double scale(int B, int C, long long HW) { return -1.0 / (2.0 * (double)B * (double)C * (double)HW); }
    __device__ MaxSquareTerm(int, float) {}
    __device__ float each(float v) const { return v * v; }
    __device__ float slope(float v) const { return 2.0f * v; }
    __device__ float pixel(float s) const { return s; }
    __device__ float coef(float up, float) const { return up; }
};
// eta-weighted entropy (losses/entropy.py:17-22, the FDA plugin's form): e = -sum_c f(v_c) / log2(C) per pixel,
// loss = mean (e^2 + 1e-30)^eta;  d/de = 2 eta e (e^2 + 1e-30)^(eta-1)
struct EtaEntropyTerm {
    float eta, inv;
    static double scale(int B, int, long long HW) { return 1.0 / ((double)B * (double)HW); }
    __device__ EtaEntropyTerm(int C, float eta_) : eta(eta_), inv(1.0f / log2f((float)C)) {}
    __device__ float each(float v) const { return fent(v); }
    __device__ float slope(float v) const { return dfent(v); }
    __device__ float pixel(float s) const {
        const float e = -s * inv;
        return powf(e * e + 1e-30f, eta);
    }
    __device__ float coef(float up, float s) const {
        const float e = -s * inv;
        const float ge = 2.0f * eta * e * powf(e * e + 1e-30f, eta - 1.0f);
        return -up * ge * inv;
    }
};
template <class Term>
__global__ __launch_bounds__(kT) void softmax_reduce_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                            int B, int C, long long HW, float param) {
    __shared__ double red[16];
    const Term term(C, param);
    double acc[1] = {};
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
        const SoftmaxPixel p(x, i, C, HW);
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s += term.each(p.v(c));
        acc[0] += (double)term.pixel(s);
    }
    store_partials(acc, partial, red);
}
template <class Term>
__global__ void softmax_grad_kernel(const float* __restrict__ x, const float* __restrict__ upstream, float scale,
                                    float* __restrict__ grad, int B, int C, long long HW, float param) {
    const float up = upstream[0] * scale;
    const Term term(C, param);
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const SoftmaxPixel p(x, i, C, HW);
        float s = 0.0f, dot = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            s += term.each(v);
            dot += v * term.slope(v);
        }
        const float k = term.coef(up, s);
        float* pg = grad + p.base;
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            pg[(size_t)c * p.HW] = k * v * (term.slope(v) - dot);
        }
    }
}
// ---------------- image-wise class-balanced max-squares (Chen, Xue, Cai, ICCV 2019, section 3.3) ----------------
//   a[b,p] = argmax_c x[b,c,p] on the LOGITS, lowest channel on a tie;  hist[b,c] = #{p : a[b,p] == c}
//   w[b,c] = 1 / max(hist^ratio * HW^(1-ratio), 1);  loss = -sum v^2 w[b,a] / (2 B C)   
// The three kernels below take the argmax from this one walk, so a pixel counts for the class whose weight it gets.
constexpr int kIwMaxClasses = 1024;   // the per-workgroup LDS table (4 KiB) of the histogram and of the weights
constexpr int kIwBallotClasses = 16;  // up to here a wave counts a class with one ballot + popcount, no LDS atomics
__device__ __forceinline__ int argmax_channel(const float* __restrict__ px, int C, size_t HW) {
    float best = px[0];
    int a = 0;
    for (int c = 1; c < C; ++c) {
        const float v = px[(size_t)c * HW];
        if (v > best) { best = v; a = c; }   // strict: the lowest channel keeps a tie
    }
    return a;
}
// grid (gx, gy): blockIdx.y walks the images, the gx workgroups of a row share one image's pixels.  Ballot: lane c of
// every wave keeps class c's count in a register, the table holds one row per wave.  Otherwise: one LDS integer atomic
// per pixel.  Either way one global integer atomic per (workgroup, image, class that occurred): integer adds commute, the
// counts are exact whatever the order.
template <bool Ballot>
__global__ __launch_bounds__(kT) void argmax_hist_kernel(const float* __restrict__ x, int* __restrict__ hist, int B,
                                                         int C, long long HW) {
    __shared__ int table[kIwMaxClasses];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* xb = x + (size_t)b * C * HW;
        int mine = 0;
        if (!Ballot) {
            for (int c = threadIdx.x; c < C; c += kT) table[c] = 0;
            __syncthreads();
        }
        for (long long base = (long long)blockIdx.x * kT; base < HW; base += (long long)gridDim.x * kT) {   // wave-uniform
            const long long hw = base + threadIdx.x;
            const bool live = hw < HW;
            const int a = live ? argmax_channel(xb + hw, C, (size_t)HW) : -1;
            if (Ballot) {
                for (int c = 0; c < C; ++c) {
                    const int n = __popcll(__ballot(a == c));
                    if (lane == c) mine += n;
                }
            } else if (live) {
                atomicAdd(&table[a], 1);
            }
        }
        if (Ballot) {
            if (lane < C) table[wid * kIwBallotClasses + lane] = mine;
            __syncthreads();
            if (threadIdx.x < C) {
                int n = 0;
                for (int w = 0; w < kT / kWave; ++w) n += table[w * kIwBallotClasses + threadIdx.x];
                if (n) atomicAdd(hist + (size_t)b * C + threadIdx.x, n);
            }
        } else {
            __syncthreads();
            for (int c = threadIdx.x; c < C; c += kT)
                if (table[c]) atomicAdd(hist + (size_t)b * C + c, table[c]);
        }
        __syncthreads();   // the table is the next image's
    }
}
__device__ __forceinline__ float iw_weight(int count, float ratio, float hw_pow) {
    return 1.0f / fmaxf(powf((float)count, ratio) * hw_pow, 1.0f);
}
// blockIdx.x = by * gx + bx: row `by` of gy walks the images, its gx workgroups share one image's pixels and each
// turns that image's counts into its own LDS copy of the weights; the first of them also saves them for the backward.
__global__ __launch_bounds__(kT) void iw_max_square_reduce_kernel(const float* __restrict__ x, const int* __restrict__ hist,
                                                                  float ratio, float* __restrict__ weights,
                                                                  double* __restrict__ partial, int B, int C,
                                                                  long long HW, int gx, int gy) {
    __shared__ double red[16];
    __shared__ float w[kIwMaxClasses];
    const int bx = blockIdx.x % gx, by = blockIdx.x / gx;
    const float hw_pow = powf((float)HW, 1.0f - ratio);
    double acc[1] = {};
    for (int b = by; b < B; b += gy) {
        __syncthreads();   // the previous image's weights are read no more
        for (int c = threadIdx.x; c < C; c += kT) {
            const float wc = iw_weight(hist[(size_t)b * C + c], ratio, hw_pow);
            w[c] = wc;
            if (bx == 0) weights[(size_t)b * C + c] = wc;
        }
        __syncthreads();
        for (long long hw = (long long)bx * kT + threadIdx.x; hw < HW; hw += (long long)gx * kT) {
            const SoftmaxPixel p(x, (long long)b * HW + hw, C, HW);
            float s = 0.0f;
            for (int c = 0; c < C; ++c) {
                const float v = p.v(c);
                s += v * v;
            }
            acc[0] += (double)(s * w[argmax_channel(p.px, C, p.HW)]);
        }
    }
    store_partials(acc, partial, red);
}
// dx_j = k v_j (2 v_j - sum_i 2 v_i^2), k = upstream * scale * w[b, a]: MaxSquareTerm's gradient with the pixel's weight
// in the coefficient; the weights are constants of the backward pass
__global__ void iw_max_square_grad_kernel(const float* __restrict__ x, const float* __restrict__ weights,
                                          const float* __restrict__ upstream, float scale, float* __restrict__ grad,
                                          int B, int C, long long HW) {
    const float up = upstream[0] * scale;
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const SoftmaxPixel p(x, i, C, HW);
        float dot = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            dot += v * (2.0f * v);
        }
        const float k = up * weights[(size_t)(i / HW) * C + argmax_channel(p.px, C, p.HW)];
        float* pg = grad + p.base;
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            pg[(size_t)c * p.HW] = k * v * (2.0f * v - dot);
        }
    }
}

// ---------------- multi-level self-produced guidance (the max-squares paper's third part) ----------------
//   p = softmax_c(x) of the final heat map, q = softmax_c(z) of the low-level one;  e = (p + q) / 2
//   a = argmax_c e, the lowest channel on a tie;  the pixel is guided when max_c e > threshold
//   loss = sum_{guided} (logsumexp_c z - z[a]) / max(N_guided, 1);   labels[b,p] = a, or -1 where unguided
// partial[blk*2 + {0,1}] = sum of the guided pixels' cross-entropies, their number (whole numbers in fp64: exact)
__global__ __launch_bounds__(kT) void guidance_fwd_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                          float threshold, int* __restrict__ labels,
                                                          double* __restrict__ partial, int B, int C, long long HW) {
    __shared__ double red[16];
    double ce = 0.0, ng = 0.0;
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
        const SoftmaxPixel p(x, i, C, HW), q(z, i, C, HW);
        float best = 0.5f * (p.v(0) + q.v(0));
        int a = 0;
        for (int c = 1; c < C; ++c) {
            const float e = 0.5f * (p.v(c) + q.v(c));
            if (e > best) { best = e; a = c; }   // strict: the lowest channel keeps a tie
        }
        const bool guided = best > threshold;
        labels[i] = guided ? a : -1;
        if (guided) {
            // -log q_a as logsumexp(z) - z[a]: finite whatever the logits (q_a itself underflows near |z| = 80)
            ce += (double)(logf(q.den) + (q.mx - q.px[(size_t)a * q.HW]));
            ng += 1.0;
        }
    }
    double acc[2] = {ce, ng};
    store_partials(acc, partial, red);
}
struct GuidanceEpilogue {   // out[0] = loss, out[1] = N_guided (kept for backward)
    static constexpr int N = 2;
    __device__ void operator()(const double (&s)[2], float* out) const {
        out[0] = (float)(s[0] / (s[1] > 1.0 ? s[1] : 1.0));
        out[1] = (float)s[1];
    }
};
// dz_c = upstream * (q_c - [c == a]) / max(N_guided, 1) on a guided pixel, a plain 0 elsewhere: every element is written
__global__ void guidance_grad_kernel(const float* __restrict__ z, const int* __restrict__ labels,
                                     const float* __restrict__ fwd_out, const float* __restrict__ upstream,
                                     float* __restrict__ grad, int B, int C, long long HW) {
    const float up = upstream[0] / fmaxf(fwd_out[1], 1.0f);
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int a = labels[i];
        if (a < 0 || a >= C) {                    // unguided (a label outside the channels is treated as unguided too)
            const long long b = i / HW;
            float* pg = grad + (size_t)b * C * HW + (i - b * HW);
            for (int c = 0; c < C; ++c) pg[(size_t)c * HW] = 0.0f;
            continue;
        }
        const SoftmaxPixel q(z, i, C, HW);
        float* pg = grad + q.base;
        for (int c = 0; c < C; ++c) pg[(size_t)c * q.HW] = up * (q.v(c) - (c == a ? 1.0f : 0.0f));
    }
}

// entropy_map: out_c = -f(v_c) / log2(C)
__global__ void entropy_map_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C,
                                       long long HW) {
    const float inv = 1.0f / log2f((float)C);
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const SoftmaxPixel p(x, i, C, HW);
        for (int c = 0; c < C; ++c) out[p.at(c)] = -fent(p.v(c)) * inv;
    }
}
// gx_j = -(1/log2 C) * v_j * (g_j f'_j - sum_i g_i f'_i v_i)
__global__ void entropy_map_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                       float* __restrict__ grad, int B, int C, long long HW) {
    const float inv = 1.0f / log2f((float)C);
    const long long total = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const SoftmaxPixel p(x, i, C, HW);
        float dot = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            dot += gout[p.at(c)] * dfent(v) * v;
        }
        for (int c = 0; c < C; ++c) {
            const float v = p.v(c);
            grad[p.at(c)] = -inv * v * (gout[p.at(c)] * dfent(v) - dot);
        }
    }
}

// ---------------- BCE with logits against a constant label, mean reduction ----------------
__global__ __launch_bounds__(kT) void bce_const_fwd_kernel(const float* __restrict__ x, float label, long long n,
                                                           float* __restrict__ out) {
    __shared__ double red[16];
    double acc[1] = {};
    for (long long i = threadIdx.x; i < n; i += kT) {
        const float v = x[i];
        acc[0] += (double)(fmaxf(v, 0.0f) - v * label + log1pf(expf(-fabsf(v))));
    }
    block_sums(acc, red);
    if (threadIdx.x == 0) out[0] = (float)(acc[0] / (double)n);
}
__global__ void bce_const_bwd_kernel(const float* __restrict__ x, float label, const float* __restrict__ upstream,
                                     long long n, float* __restrict__ grad) {
    const float up = upstream[0] / (float)n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        grad[i] = (sigmoid_f32(x[i]) - label) * up;
}

// y = clamp(sigmoid(x)); x <- sigmoid(x) in place (x.sigmoid_())
__global__ void sigmoid_clamp_kernel(float* __restrict__ x, float* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float s = sigmoid_f32(x[i]);
        x[i] = s;
        y[i] = clamp_prob(s);
    }
}

// ---------------- keypoint L1 (+ pair-distance term) ----------------
// losses/centernet.py:136-189 (KPSL1Loss).  feat [B,2J,HW]; mask [B,M,2J] u8; target [B,M,2J] is masked in
// place like the reference's `target *= mask`; pairs [P][2] keypoint indices (kps_weight_indices) or P = 0.
//   loss  = sum |pred*m - tg*m| / (sum m + 1e-4) * weight
//         + sum_{b,m,p} |d(pred_a, pred_b) - d(tg_a, tg_b)| / (sum m + 1e-4) * distance_weight
//   d = L1 norm (use_l1) or sqrt(|.|^2 + 1e4)  (the literal 1e4 of :178-179)
__device__ __forceinline__ float kps_dist(float ax, float ay, float bx, float by, int use_l1) {
    const float dx = ax - bx, dy = ay - by;
    return use_l1 ? fabsf(dx) + fabsf(dy) : sqrtf((dx * dx + dy * dy) + 1e4f);
}
__global__ __launch_bounds__(kT) void kpsl1_fwd_kernel(const float* __restrict__ feat, const unsigned char* __restrict__ mask,
                                                       const long long* __restrict__ ind, float* __restrict__ target,
                                                       const int* __restrict__ pairs, int B, int M, int J, int HW, int P,
                                                       int use_l1, float weight, float distance_weight,
                                                       float* __restrict__ out) {
    __shared__ double red[16];
    const int ch = 2 * J;
    double s[3] = {};   // L1, pair distance, mask
    for (int i = threadIdx.x; i < B * M * ch; i += kT) {
        const L1Elem e = l1_elem(i, ch, M);
        const float m = mask[i] ? 1.0f : 0.0f;
        const long long id = fwd_cell(ind[e.bm], HW, s[0]);
        float tg;
        const float pred = masked_pair(feat, feat_at(e.b, ch, e.c, HW, id), target, i, m, tg);
        s[2] += (double)m;
        s[0] += (double)fabsf(pred - tg);
    }
    __syncthreads();                                      // the pair term reads the masked targets
    for (int i = threadIdx.x; i < B * M * P; i += kT) {
        const int pr = i % P, bm = i / P, b = bm / M;
        const int ja = pairs[2 * pr], jb = pairs[2 * pr + 1];
        const size_t fb = (size_t)b * ch * HW + (ind_ok(ind[bm], HW) ? ind[bm] : 0), tb = (size_t)bm * ch;
        auto pm = [&](int c) { return feat[fb + (size_t)c * HW] * (mask[tb + c] ? 1.0f : 0.0f); };
        const float pd = kps_dist(pm(2 * ja), pm(2 * ja + 1), pm(2 * jb), pm(2 * jb + 1), use_l1);
        const float td = kps_dist(target[tb + 2 * ja], target[tb + 2 * ja + 1], target[tb + 2 * jb], target[tb + 2 * jb + 1], use_l1);
        s[1] += (double)fabsf(pd - td);
    }
    block_sums(s, red);
    if (threadIdx.x == 0) l1_epilogue(s, weight, P > 0, distance_weight, out);
}
// `target` already masked
__global__ void kpsl1_bwd_kernel(const float* __restrict__ feat, const unsigned char* __restrict__ mask,
                                 const long long* __restrict__ ind, const float* __restrict__ target,
                                 const int* __restrict__ pairs, const float* __restrict__ fwd_out,
                                 const float* __restrict__ upstream, int B, int M, int J, int HW, int P, int use_l1,
                                 float weight, float distance_weight, float* __restrict__ grad) {
    const int ch = 2 * J;
    const float up = l1_upstream(upstream, fwd_out);
    const int n1 = B * M * ch, n2 = B * M * P;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += gridDim.x * blockDim.x) {
        if (i < n1) {
            const L1Elem e = l1_elem(i, ch, M);
            if (!mask[i] || !ind_ok(ind[e.bm], HW)) continue;
            const size_t cell = feat_at(e.b, ch, e.c, HW, ind[e.bm]);
            atomicAdd(grad + cell, sgnf(feat[cell] - target[i]) * weight * up);
        } else {
            const int k = i - n1, pr = k % P, bm = k / P, b = bm / M;
            const int ja = pairs[2 * pr], jb = pairs[2 * pr + 1];
            if (!ind_ok(ind[bm], HW)) continue;
            const size_t fb = (size_t)b * ch * HW + ind[bm], tb = (size_t)bm * ch;
            const int cs[4] = {2 * ja, 2 * ja + 1, 2 * jb, 2 * jb + 1};
            float mk[4], pv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { mk[t] = mask[tb + cs[t]] ? 1.0f : 0.0f; pv[t] = feat[fb + (size_t)cs[t] * HW] * mk[t]; }
            const float pd = kps_dist(pv[0], pv[1], pv[2], pv[3], use_l1);
            const float td = kps_dist(target[tb + cs[0]], target[tb + cs[1]], target[tb + cs[2]], target[tb + cs[3]], use_l1);
            const float e = sgnf(pd - td) * distance_weight * up;
            const float dx = pv[0] - pv[2], dy = pv[1] - pv[3];
            const float gx = use_l1 ? sgnf(dx) : dx / pd, gy = use_l1 ? sgnf(dy) : dy / pd;   // d(pd)/d(a) = -d(pd)/d(b)
            const float g[4] = {gx, gy, -gx, -gy};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (mk[t] != 0.0f && e * g[t] != 0.0f) atomicAdd(grad + fb + (size_t)cs[t] * HW, e * g[t]);
        }
    }
}
// keypoint branch of the decode (backends/decode.py:44-51,69-74)
__global__ void decode_kps_kernel(const float* __restrict__ kps, const float* __restrict__ reg,
                                  const long long* __restrict__ inds, float* __restrict__ out, int B, int J, int K,
                                  int H, int W) {
    const int HW = H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * K * J; i += gridDim.x * blockDim.x) {
        const int j = i % J, bk = i / J, b = bk / K;
        const long long id = inds[bk];
        float xs = (float)(int)(id % W), ys = (float)(int)(id / W);
        if (reg) { xs += reg[((size_t)b * 2 + 0) * HW + id]; ys += reg[((size_t)b * 2 + 1) * HW + id]; }
        else { xs += 0.5f; ys += 0.5f; }
        out[(size_t)i * 2 + 0] = kps[((size_t)b * 2 * J + 2 * j) * HW + id] + xs;
        out[(size_t)i * 2 + 1] = kps[((size_t)b * 2 * J + 2 * j + 1) * HW + id] + ys;
    }
}
// feat [B,ch,HW], ind [B,M] -> out [B,M,ch]
__global__ void gather_feat_kernel(const float* __restrict__ feat, const long long* __restrict__ ind,
                                   float* __restrict__ out, int B, int M, int ch, long long HW) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * M * ch; i += gridDim.x * blockDim.x) {
        const int c = i % ch, bm = i / ch, b = bm / M;
        out[i] = ind_ok(ind[bm], HW) ? feat[((size_t)b * ch + c) * HW + ind[bm]] : NAN;
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" size_t cnuda_loss_workspace_bytes(void) { return (size_t)kLossBlocks * 3 * sizeof(double) + 512; }
static double* ws_ptr(void* ws) { return reinterpret_cast<double*>(((uintptr_t)ws + 255) & ~(uintptr_t)255); }

// A reducing forward on the host, `who` the entry point's name for the error texts: the grid over `items` is capped at
// kLossBlocks, launch(blocks, partial) starts the loss's own kernel, finalize_kernel<Epilogue> writes `out`.
template <class Epilogue, class Launch>
static int reduced_loss(const char* who, void* workspace, size_t workspace_bytes, long long items, hipStream_t st,
                        Epilogue epilogue, float* out, Launch launch) {
    CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_loss_workspace_bytes(), "%s: workspace", who);
    int blocks = stream_grid(items, kT);
    if (blocks > kLossBlocks) blocks = kLossBlocks;
    double* partial = ws_ptr(workspace);
    launch(blocks, partial);
    CNUDA_LAUNCH(finalize_kernel<Epilogue>, dim3(1), dim3(kT), 0, st, partial, blocks, epilogue, out);
    return check_launch(who);
}
// A masked-L1 backward on the host: zero the gradient, then launch() scatters into it.
template <class Launch>
static int scattered_grad(const char* who, const char* who_memset, float* grad, size_t cells, hipStream_t st,
                          Launch launch) {
    if (hipMemsetAsync(grad, 0, cells * sizeof(float), st) != hipSuccess) return check_launch(who_memset);
    launch();
    return check_launch(who);
}

extern "C" int cnuda_focal_loss_forward(const float* logits, const float* gt, float* prob, float* out2, long long n,
                                        float weight, void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && gt && prob && out2 && n > 0, "cnuda_focal_loss_forward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    return reduced_loss("cnuda_focal_loss_forward", workspace, workspace_bytes, n, st, FocalEpilogue{weight}, out2,
                        [&](int blocks, double* partial) {
        CNUDA_LAUNCH(focal_fwd_kernel, dim3(blocks), dim3(kT), 0, st, logits, gt, prob, partial, n);
    });
}
extern "C" int cnuda_focal_loss_backward(const float* logits, const float* gt, const float* out2,
                                         const float* upstream, float* grad_logits, long long n, float weight,
                                         cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && gt && out2 && upstream && grad_logits && n > 0, "cnuda_focal_loss_backward: bad arguments");
    CNUDA_LAUNCH(focal_bwd_kernel, dim3(stream_grid(n, kT)), dim3(kT), 0, (hipStream_t)stream, logits, gt, out2,
                       upstream, weight, grad_logits, n);
    return check_launch("cnuda_focal_loss_backward");
}

extern "C" int cnuda_reg_l1_forward(const float* feat, const uint8_t* mask, const int64_t* ind, float* target,
                                    float* out2, int B, int M, int ch, long long HW, int periodic, float weight,
                                    float angle_weight, cnuda_stream_t stream) {
    CNUDA_REQUIRE(feat && mask && ind && target && out2 && B > 0 && M > 0 && HW > 0, "cnuda_reg_l1_forward: bad arguments");
    CNUDA_REQUIRE(ch >= 1 && (!periodic || ch == 3), "cnuda_reg_l1_forward: periodic loss needs 3 channels, got %d", ch);
    CNUDA_LAUNCH(regl1_fwd_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, feat, mask,
                       (const long long*)ind, target, B, M, ch, (int)HW, periodic ? 1 : 0, weight, angle_weight, out2);
    return check_launch("cnuda_reg_l1_forward");
}
extern "C" int cnuda_reg_l1_backward(const float* feat, const uint8_t* mask, const int64_t* ind, const float* target,
                                     const float* out2, const float* upstream, float* grad_feat, int B, int M, int ch,
                                     long long HW, int periodic, float weight, float angle_weight,
                                     cnuda_stream_t stream) {
    CNUDA_REQUIRE(feat && mask && ind && target && out2 && upstream && grad_feat && B > 0 && M > 0 && HW > 0,
                  "cnuda_reg_l1_backward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    return scattered_grad("cnuda_reg_l1_backward", "cnuda_reg_l1_backward(memset)", grad_feat, (size_t)B * ch * HW, st,
                          [&] {
        CNUDA_LAUNCH(regl1_bwd_kernel, dim3(stream_grid((long long)B * M * ch, kT)), dim3(kT), 0, st, feat, mask,
                     (const long long*)ind, target, out2, upstream, B, M, ch, (int)HW, periodic ? 1 : 0, weight,
                     angle_weight, grad_feat);
    });
}

extern "C" int cnuda_kps_l1_forward(const float* feat, const uint8_t* mask, const int64_t* ind, float* target,
                                    const int32_t* pairs, float* out2, int B, int M, int J, long long HW, int n_pairs,
                                    int use_l1, float weight, float distance_weight, cnuda_stream_t stream) {
    CNUDA_REQUIRE(feat && mask && ind && target && out2 && B > 0 && M > 0 && J > 0 && HW > 0 && n_pairs >= 0 &&
                      (n_pairs == 0 || pairs), "cnuda_kps_l1_forward: bad arguments");
    CNUDA_LAUNCH(kpsl1_fwd_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, feat, mask, (const long long*)ind,
                       target, (const int*)pairs, B, M, J, (int)HW, n_pairs, use_l1 ? 1 : 0, weight, distance_weight, out2);
    return check_launch("cnuda_kps_l1_forward");
}
extern "C" int cnuda_kps_l1_backward(const float* feat, const uint8_t* mask, const int64_t* ind, const float* target,
                                     const int32_t* pairs, const float* out2, const float* upstream, float* grad_feat,
                                     int B, int M, int J, long long HW, int n_pairs, int use_l1, float weight,
                                     float distance_weight, cnuda_stream_t stream) {
    CNUDA_REQUIRE(feat && mask && ind && target && out2 && upstream && grad_feat && B > 0 && M > 0 && J > 0 && HW > 0 &&
                      n_pairs >= 0 && (n_pairs == 0 || pairs), "cnuda_kps_l1_backward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    return scattered_grad("cnuda_kps_l1_backward", "cnuda_kps_l1_backward(memset)", grad_feat, (size_t)B * 2 * J * HW,
                          st, [&] {
        CNUDA_LAUNCH(kpsl1_bwd_kernel, dim3(stream_grid((long long)B * M * (2 * J + n_pairs), kT)), dim3(kT), 0, st,
                     feat, mask, (const long long*)ind, target, (const int*)pairs, out2, upstream, B, M, J, (int)HW, n_pairs,
                     use_l1 ? 1 : 0, weight, distance_weight, grad_feat);
    });
}
extern "C" int cnuda_decode_keypoints(const float* kps, const float* reg, const int64_t* inds, float* out, int B, int J,
                                      int K, int H, int W, cnuda_stream_t stream) {
    CNUDA_REQUIRE(kps && inds && out && B > 0 && J > 0 && K > 0 && H > 0 && W > 0, "cnuda_decode_keypoints: bad arguments");
    CNUDA_LAUNCH(decode_kps_kernel, dim3(stream_grid((long long)B * K * J, kT)), dim3(kT), 0, (hipStream_t)stream,
                       kps, reg, (const long long*)inds, out, B, J, K, H, W);
    return check_launch("cnuda_decode_keypoints");
}

// The scalar softmax losses: the term's scale multiplies the pixel sum (forward) and the upstream scalar (backward).
template <class Term>
static int softmax_loss_forward(const char* who, const float* logits, float* out1, int B, int C, long long HW,
                                float param, void* workspace, size_t workspace_bytes, hipStream_t st) {
    return reduced_loss(who, workspace, workspace_bytes, (long long)B * HW, st, ScaleEpilogue{Term::scale(B, C, HW)},
                        out1, [&](int blocks, double* partial) {
        CNUDA_LAUNCH(softmax_reduce_kernel<Term>, dim3(blocks), dim3(kT), 0, st, logits, partial, B, C, HW, param);
    });
}
template <class Term>
static int softmax_loss_backward(const char* who, const float* logits, const float* upstream, float* grad_logits, int B,
                                 int C, long long HW, float param, hipStream_t st) {
    CNUDA_LAUNCH(softmax_grad_kernel<Term>, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0, st, logits, upstream,
                 (float)Term::scale(B, C, HW), grad_logits, B, C, HW, param);
    return check_launch(who);
}
// kind 0: EntropyLoss, kind 1: MaxSquareLoss
extern "C" int cnuda_softmax_loss_forward(const float* logits, float* out1, int B, int C, long long HW, int kind,
                                          void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && out1 && B > 0 && C > 0 && HW > 0 && (kind == 0 || kind == 1),
                  "cnuda_softmax_loss_forward: bad arguments");
    const auto forward = kind == 0 ? softmax_loss_forward<EntropyTerm> : softmax_loss_forward<MaxSquareTerm>;
    return forward("cnuda_softmax_loss_forward", logits, out1, B, C, HW, 0.0f, workspace, workspace_bytes,
                   (hipStream_t)stream);
}
extern "C" int cnuda_softmax_loss_backward(const float* logits, const float* upstream, float* grad_logits, int B, int C,
                                           long long HW, int kind, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && upstream && grad_logits && B > 0 && C > 0 && HW > 0 && (kind == 0 || kind == 1),
                  "cnuda_softmax_loss_backward: bad arguments");
    const auto backward = kind == 0 ? softmax_loss_backward<EntropyTerm> : softmax_loss_backward<MaxSquareTerm>;
    return backward("cnuda_softmax_loss_backward", logits, upstream, grad_logits, B, C, HW, 0.0f, (hipStream_t)stream);
}
extern "C" int cnuda_entropy_eta_loss_forward(const float* logits, float* out1, int B, int C, long long HW, float eta,
                                              void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && out1 && B > 0 && C > 0 && HW > 0, "cnuda_entropy_eta_loss_forward: bad arguments");
    return softmax_loss_forward<EtaEntropyTerm>("cnuda_entropy_eta_loss_forward", logits, out1, B, C, HW, eta, workspace,
                                                workspace_bytes, (hipStream_t)stream);
}
extern "C" int cnuda_entropy_eta_loss_backward(const float* logits, const float* upstream, float* grad_logits, int B,
                                               int C, long long HW, float eta, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && upstream && grad_logits && B > 0 && C > 0 && HW > 0,
                  "cnuda_entropy_eta_loss_backward: bad arguments");
    return softmax_loss_backward<EtaEntropyTerm>("cnuda_entropy_eta_loss_backward", logits, upstream, grad_logits, B, C,
                                                 HW, eta, (hipStream_t)stream);
}
// The grid of the two image-wise kernels: gy rows over the images, gx workgroups per row, gx * gy <= kLossBlocks.
struct IwGrid { int gx, gy; };
static IwGrid iw_grid(int B, long long HW) {
    const int gy = B < kLossBlocks ? B : kLossBlocks;
    const long long want = (HW + kT - 1) / kT, cap = kLossBlocks / gy;
    return {(int)(want < cap ? want : cap), gy};
}
extern "C" int cnuda_argmax_histogram(const float* logits, int32_t* hist, int B, int C, long long HW,
                                      cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && hist && B > 0 && C > 0 && HW > 0 && HW <= 0x7fffffffLL, "cnuda_argmax_histogram: bad arguments");
    CNUDA_REQUIRE(C <= kIwMaxClasses, "cnuda_argmax_histogram: %d classes, the workgroup's table holds %d", C, kIwMaxClasses);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)B * C * sizeof(int32_t), st) != hipSuccess)
        return check_launch("cnuda_argmax_histogram(memset)");
    const IwGrid g = iw_grid(B, HW);
    if (C <= kIwBallotClasses)
        CNUDA_LAUNCH(argmax_hist_kernel<true>, dim3(g.gx, g.gy), dim3(kT), 0, st, logits, (int*)hist, B, C, HW);
    else
        CNUDA_LAUNCH(argmax_hist_kernel<false>, dim3(g.gx, g.gy), dim3(kT), 0, st, logits, (int*)hist, B, C, HW);
    return check_launch("cnuda_argmax_histogram");
}
static double iw_max_square_scale(int B, int C) { return -1.0 / (2.0 * (double)B * (double)C); }
extern "C" int cnuda_iw_max_square_forward(const float* logits, const int32_t* hist, float ratio, float* weights_out,
                                           float* out1, int B, int C, long long HW, void* workspace,
                                           size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && hist && weights_out && out1 && B > 0 && C > 0 && HW > 0,
                  "cnuda_iw_max_square_forward: bad arguments");
    CNUDA_REQUIRE(ratio >= 0.0f && ratio <= 1.0f, "cnuda_iw_max_square_forward: ratio %g outside [0, 1]", (double)ratio);
    CNUDA_REQUIRE(C <= kIwMaxClasses, "cnuda_iw_max_square_forward: %d classes, the workgroup's table holds %d", C,
                  kIwMaxClasses);
    hipStream_t st = (hipStream_t)stream;
    const IwGrid g = iw_grid(B, HW);
    // reduced_loss sizes its grid from an item count: gx * gy workgroups' worth of threads gives exactly this grid
    return reduced_loss("cnuda_iw_max_square_forward", workspace, workspace_bytes, (long long)g.gx * g.gy * kT, st,
                        ScaleEpilogue{iw_max_square_scale(B, C)}, out1, [&](int blocks, double* partial) {
        CNUDA_LAUNCH(iw_max_square_reduce_kernel, dim3(blocks), dim3(kT), 0, st, logits, (const int*)hist, ratio,
                     weights_out, partial, B, C, HW, g.gx, g.gy);
    });
}
extern "C" int cnuda_iw_max_square_backward(const float* logits, const float* weights, const float* upstream,
                                            float* grad_logits, int B, int C, long long HW, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && weights && upstream && grad_logits && B > 0 && C > 0 && HW > 0,
                  "cnuda_iw_max_square_backward: bad arguments");
    CNUDA_LAUNCH(iw_max_square_grad_kernel, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0, (hipStream_t)stream,
                 logits, weights, upstream, (float)iw_max_square_scale(B, C), grad_logits, B, C, HW);
    return check_launch("cnuda_iw_max_square_backward");
}
extern "C" int cnuda_guidance_forward(const float* high, const float* low, float threshold, int32_t* labels,
                                      float* out2, int B, int C, long long HW, void* workspace, size_t workspace_bytes,
                                      cnuda_stream_t stream) {
    CNUDA_REQUIRE(high && low && labels && out2 && B > 0 && C > 0 && HW > 0, "cnuda_guidance_forward: bad arguments");
    CNUDA_REQUIRE(threshold >= 0.0f && threshold < 1.0f, "cnuda_guidance_forward: threshold %g outside [0, 1)",
                  (double)threshold);
    hipStream_t st = (hipStream_t)stream;
    return reduced_loss("cnuda_guidance_forward", workspace, workspace_bytes, (long long)B * HW, st, GuidanceEpilogue{},
                        out2, [&](int blocks, double* partial) {
        CNUDA_LAUNCH(guidance_fwd_kernel, dim3(blocks), dim3(kT), 0, st, high, low, threshold, (int*)labels, partial, B,
                     C, HW);
    });
}
extern "C" int cnuda_guidance_backward(const float* low, const int32_t* labels, const float* out2,
                                       const float* upstream, float* grad_low, int B, int C, long long HW,
                                       cnuda_stream_t stream) {
    CNUDA_REQUIRE(low && labels && out2 && upstream && grad_low && B > 0 && C > 0 && HW > 0,
                  "cnuda_guidance_backward: bad arguments");
    CNUDA_LAUNCH(guidance_grad_kernel, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0, (hipStream_t)stream, low,
                 (const int*)labels, out2, upstream, grad_low, B, C, HW);
    return check_launch("cnuda_guidance_backward");
}
extern "C" int cnuda_entropy_map_forward(const float* logits, float* out, int B, int C, long long HW,
                                         cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && out && B > 0 && C > 0 && HW > 0, "cnuda_entropy_map_forward: bad arguments");
    CNUDA_LAUNCH(entropy_map_fwd_kernel, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0,
                       (hipStream_t)stream, logits, out, B, C, HW);
    return check_launch("cnuda_entropy_map_forward");
}
extern "C" int cnuda_entropy_map_backward(const float* logits, const float* grad_out, float* grad_logits, int B, int C,
                                          long long HW, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && grad_out && grad_logits && B > 0 && C > 0 && HW > 0, "cnuda_entropy_map_backward: bad arguments");
    CNUDA_LAUNCH(entropy_map_bwd_kernel, dim3(stream_grid((long long)B * HW, kT)), dim3(kT), 0,
                       (hipStream_t)stream, logits, grad_out, grad_logits, B, C, HW);
    return check_launch("cnuda_entropy_map_backward");
}
extern "C" int cnuda_bce_const_forward(const float* logits, float label, float* out1, long long n,
                                       cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && out1 && n > 0, "cnuda_bce_const_forward: bad arguments");
    CNUDA_LAUNCH(bce_const_fwd_kernel, dim3(1), dim3(kT), 0, (hipStream_t)stream, logits, label, n, out1);
    return check_launch("cnuda_bce_const_forward");
}
extern "C" int cnuda_bce_const_backward(const float* logits, float label, const float* upstream, float* grad_logits,
                                        long long n, cnuda_stream_t stream) {
    CNUDA_REQUIRE(logits && upstream && grad_logits && n > 0, "cnuda_bce_const_backward: bad arguments");
    CNUDA_LAUNCH(bce_const_bwd_kernel, dim3(stream_grid(n, kT)), dim3(kT), 0, (hipStream_t)stream, logits, label,
                       upstream, n, grad_logits);
    return check_launch("cnuda_bce_const_backward");
}
extern "C" int cnuda_sigmoid_clamp_(float* x, float* y, long long n, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && n > 0, "cnuda_sigmoid_clamp_: bad arguments");
    CNUDA_LAUNCH(sigmoid_clamp_kernel, dim3(stream_grid(n, kT)), dim3(kT), 0, (hipStream_t)stream, x, y, n);
    return check_launch("cnuda_sigmoid_clamp_");
}
extern "C" int cnuda_gather_feat(const float* feat, const int64_t* ind, float* out, int B, int M, int ch, long long HW,
                                 cnuda_stream_t stream) {
    CNUDA_REQUIRE(feat && ind && out && B > 0 && M > 0 && ch > 0 && HW > 0, "cnuda_gather_feat: bad arguments");
    CNUDA_LAUNCH(gather_feat_kernel, dim3(stream_grid((long long)B * M * ch, kT)), dim3(kT), 0,
                       (hipStream_t)stream, feat, (const long long*)ind, out, B, M, ch, HW);
    return check_launch("cnuda_gather_feat");
}
