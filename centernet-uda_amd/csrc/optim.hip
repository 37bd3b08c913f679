// SGD, the Adam family beyond plain Adam (AdamW, amsgrad, maximize) and RMSprop over a flat range of the fp32 parameter
// arena: one launch per (parameter group, run of touched parameters) instead of torch.optim's per-tensor loops
// (train.py:88-90 builds torch.optim.<name>).  Plain Adam stays on adam_kernel (adam.hip).
//
// Arithmetic: torch.optim's single-tensor form, in its order of operations (what the CPU runs; ATen's element-wise
// formulas: add(alpha) = a + alpha*b, addcmul = a + (value*t1)*t2, addcdiv = a + (value*t1)/t2, lerp as below):
//   SGD      g = -g (maximize);  g += wd*p;  buf = g (first update) | buf*mu + (1-dampening)*g;
//            g = g + mu*buf (nesterov) | buf;  p += (-lr)*g
//   Adam     g = -g;  p *= 1 - lr*wd (decoupled) | g += wd*p;  m = lerp(m, g, 1-b1);  v = v*b2 + ((1-b2)*g)*g;
//            vmax = max(vmax, v) (amsgrad);  p += ((-lr/bc1)*m) / (sqrt(vmax | v)/sqrt(bc2) + eps)
//   RMSprop  g = -g;  g += wd*p;  sq = sq*alpha + ((1-alpha)*g)*g;  ga = lerp(ga, g, 1-alpha) (centered);
//            avg = sqrt(sq - ga*ga | sq) + eps;  buf = buf*mu + g/avg, p += (-lr)*buf (momentum) | p += ((-lr)*g)/avg
// Constants that torch forms in Python floats (1-dampening, 1-b1, 1 - lr*wd, lr/bc1, sqrt(bc2), ...) are formed in
// double on the host and rounded to fp32 once, like a Python scalar applied to a float tensor.
//
// Streaming: 12 (SGD) to 36 (Adam + amsgrad) bytes per element, no reuse.  A run of the arena begins and ends on a
// slot boundary (ParamArena.ALIGN = 64 elements), so every operand is 16-byte aligned and a multiple of four floats
// long: one 16-byte load / store per operand, lane and iteration, no scalar tail (the entry points check both).
// 256 threads, grid capped by stream_grid, grid-stride; up to five independent 16-byte loads per lane are in flight
// before the first use, and occupancy (no LDS, few registers) covers the rest of the HBM latency.
//
// Gap guard.  A run includes the alignment gaps between tensors, where parameter, gradient and state are zero.  The
// quotient of Adam and RMSprop is 0 / (sqrt(0) + eps) there: NaN once eps = 0, and it would stay in the arena for ever.
// Rule: A ZERO NUMERATOR GIVES A ZERO QUOTIENT, whatever the denominator.  Wherever torch's result is finite that is
// torch's result too (0 / x = 0 for x > 0), so real elements are unaffected; SGD divides by nothing.  Where torch's
// result is NaN and the numerator zero, the results differ: a real element with zero gradient, zero state and eps = 0
// (torch: 0 / 0), or a zero numerator over a NaN denominator (centered RMSprop with sq < ga*ga), stays where it is here.
#include "common.h"

namespace cnuda {
namespace {

// torch.lerp's element formula (ATen/native/Lerp.h)
__host__ __device__ __forceinline__ float lerp_like_torch(float a, float b, float w) {
    return (fabsf(w) < 0.5f) ? a + w * (b - a) : b - (b - a) * (1.0f - w);
}

__host__ __device__ __forceinline__ float guarded_div(float num, float den) { return num == 0.0f ? 0.0f : num / den; }

// A rule updates one element: operator()(p, g, s0, s1, s2); kMask says which of the three state operands exist (the
// kernel neither loads nor stores the others).
template <bool kBuf>
struct SgdRule {
    static constexpr int kMask = kBuf ? 1 : 0;          // s0 = momentum_buffer
    float neg_lr, mu, one_minus_damp, wd;
    int first, nesterov, maximize;
    __host__ __device__ __forceinline__ void operator()(float& p, float g, float& buf, float&, float&) const {
        if (maximize) g = -g;
        if (wd != 0.0f) g = g + wd * p;
        if (kBuf) {
            buf = first ? g : buf * mu + one_minus_damp * g;
            g = nesterov ? g + mu * buf : buf;
        }
        p = p + neg_lr * g;
    }
};

template <bool kAmsgrad>
struct AdamRule {
    static constexpr int kMask = kAmsgrad ? 7 : 3;      // s0 = exp_avg, s1 = exp_avg_sq, s2 = max_exp_avg_sq
    float keep, wd, w1, beta2, w2, neg_step_size, bc2_sqrt, eps;
    int decoupled, maximize;
    __host__ __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, float& vmax) const {
        if (maximize) g = -g;
        if (wd != 0.0f) {
            if (decoupled) p = p * keep;
            else g = g + wd * p;
        }
        m = lerp_like_torch(m, g, w1);
        v = v * beta2 + (w2 * g) * g;
        float d = v;
        if (kAmsgrad) {
            vmax = (v > vmax || v != v) ? v : vmax;      // torch.maximum: a NaN wins
            d = vmax;
        }
        const float denom = sqrtf(d) / bc2_sqrt + eps;
        p = p + guarded_div(neg_step_size * m, denom);
    }
};

template <bool kCentered, bool kMomentum>
struct RmspropRule {
    static constexpr int kMask = 1 | (kCentered ? 2 : 0) | (kMomentum ? 4 : 0);   // square_avg, grad_avg, momentum_buffer
    float neg_lr, alpha, w, eps, wd, mu;
    int maximize;
    __host__ __device__ __forceinline__ void operator()(float& p, float g, float& sq, float& ga, float& buf) const {
        if (maximize) g = -g;
        if (wd != 0.0f) g = g + wd * p;
        sq = sq * alpha + (w * g) * g;
        float avg;
        if (kCentered) {
            ga = lerp_like_torch(ga, g, w);
            avg = sqrtf(sq + (-ga) * ga);
        } else {
            avg = sqrtf(sq);
        }
        avg = avg + eps;
        if (kMomentum) {
            buf = buf * mu + guarded_div(g, avg);
            p = p + neg_lr * buf;
        } else {
            p = p + guarded_div(neg_lr * g, avg);
        }
    }
};

template <class Rule>
__global__ __launch_bounds__(256) void optim_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                    float4* __restrict__ s0, float4* __restrict__ s1,
                                                    float4* __restrict__ s2, long long n4, const Rule rule) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 pv = p[i];
        const float4 gv = g[i];
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
        if (Rule::kMask & 1) a = s0[i];
        if (Rule::kMask & 2) b = s1[i];
        if (Rule::kMask & 4) c = s2[i];
        rule(pv.x, gv.x, a.x, b.x, c.x);
        rule(pv.y, gv.y, a.y, b.y, c.y);
        rule(pv.z, gv.z, a.z, b.z, c.z);
        rule(pv.w, gv.w, a.w, b.w, c.w);
        p[i] = pv;
        if (Rule::kMask & 1) s0[i] = a;
        if (Rule::kMask & 2) s1[i] = b;
        if (Rule::kMask & 4) s2[i] = c;
    }
}

bool flag(int v) { return v == 0 || v == 1; }
bool vec16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <class Rule>
int launch(const char* what, hipStream_t st, float* p, const float* g, float* s0, float* s1, float* s2, long long n,
           const Rule& rule) {
    const long long n4 = n / 4;
    CNUDA_LAUNCH(optim_kernel<Rule>, dim3(stream_grid(n4, 256)), dim3(256), 0, st, reinterpret_cast<float4*>(p),
                 reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(s0), reinterpret_cast<float4*>(s1),
                 reinterpret_cast<float4*>(s2), n4, rule);
    return check_launch(what);
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_sgd_step(float* param, const float* grad, float* momentum_buffer, long long n, double lr,
                              double momentum, double dampening, double weight_decay, int nesterov, int maximize,
                              int first, cnuda_stream_t stream) {
    CNUDA_REQUIRE(param && grad && n > 0 && n % 4 == 0 && vec16(param) && vec16(grad) && vec16(momentum_buffer),
                  "cnuda_sgd_step: null operand, n <= 0, or a range that is not 16-byte aligned and a multiple of 4 floats");
    CNUDA_REQUIRE((momentum != 0.0) == (momentum_buffer != nullptr),
                  "cnuda_sgd_step: a momentum buffer is passed exactly when momentum != 0");
    CNUDA_REQUIRE(flag(nesterov) && flag(maximize) && flag(first) && (!nesterov || (momentum > 0.0 && dampening == 0.0)),
                  "cnuda_sgd_step: flags are 0 or 1, and nesterov needs momentum > 0 and dampening == 0");
    if (momentum_buffer) {
        SgdRule<true> r{(float)-lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay, first, nesterov, maximize};
        return launch("cnuda_sgd_step", (hipStream_t)stream, param, grad, momentum_buffer, nullptr, nullptr, n, r);
    }
    SgdRule<false> r{(float)-lr, 0.0f, 1.0f, (float)weight_decay, 0, 0, maximize};
    return launch("cnuda_sgd_step", (hipStream_t)stream, param, grad, nullptr, nullptr, nullptr, n, r);
}

extern "C" int cnuda_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                float* max_exp_avg_sq, long long n, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int decoupled, int maximize, int step, cnuda_stream_t stream) {
    CNUDA_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n % 4 == 0 && vec16(param) && vec16(grad) &&
                      vec16(exp_avg) && vec16(exp_avg_sq) && vec16(max_exp_avg_sq),
                  "cnuda_adamw_step: null operand, n <= 0, or a range that is not 16-byte aligned and a multiple of 4 floats");
    CNUDA_REQUIRE(flag(decoupled) && flag(maximize) && step >= 1, "cnuda_adamw_step: flags are 0 or 1, step >= 1");
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const float keep = (float)(1.0 - lr * weight_decay), wd = (float)weight_decay, w1 = (float)(1.0 - beta1),
                w2 = (float)(1.0 - beta2), neg_step = (float)-(lr / bc1), bc2s = (float)sqrt(bc2);
    if (max_exp_avg_sq) {
        AdamRule<true> r{keep, wd, w1, (float)beta2, w2, neg_step, bc2s, (float)eps, decoupled, maximize};
        return launch("cnuda_adamw_step", (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, r);
    }
    AdamRule<false> r{keep, wd, w1, (float)beta2, w2, neg_step, bc2s, (float)eps, decoupled, maximize};
    return launch("cnuda_adamw_step", (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, nullptr, n, r);
}

extern "C" int cnuda_rmsprop_step(float* param, const float* grad, float* square_avg, float* grad_avg,
                                  float* momentum_buffer, long long n, double lr, double alpha, double eps,
                                  double weight_decay, double momentum, int maximize, cnuda_stream_t stream) {
    CNUDA_REQUIRE(param && grad && square_avg && n > 0 && n % 4 == 0 && vec16(param) && vec16(grad) && vec16(square_avg) &&
                      vec16(grad_avg) && vec16(momentum_buffer),
                  "cnuda_rmsprop_step: null operand, n <= 0, or a range that is not 16-byte aligned and a multiple of 4 floats");
    CNUDA_REQUIRE((momentum > 0.0) == (momentum_buffer != nullptr) && momentum >= 0.0 && flag(maximize),
                  "cnuda_rmsprop_step: a momentum buffer is passed exactly when momentum > 0; maximize is 0 or 1");
    const float neg_lr = (float)-lr, a = (float)alpha, w = (float)(1.0 - alpha), e = (float)eps, wd = (float)weight_decay,
                mu = (float)momentum;
    hipStream_t st = (hipStream_t)stream;
    if (grad_avg && momentum_buffer)
        return launch("cnuda_rmsprop_step", st, param, grad, square_avg, grad_avg, momentum_buffer, n,
                      RmspropRule<true, true>{neg_lr, a, w, e, wd, mu, maximize});
    if (grad_avg)
        return launch("cnuda_rmsprop_step", st, param, grad, square_avg, grad_avg, nullptr, n,
                      RmspropRule<true, false>{neg_lr, a, w, e, wd, mu, maximize});
    if (momentum_buffer)
        return launch("cnuda_rmsprop_step", st, param, grad, square_avg, nullptr, momentum_buffer, n,
                      RmspropRule<false, true>{neg_lr, a, w, e, wd, mu, maximize});
    return launch("cnuda_rmsprop_step", st, param, grad, square_avg, nullptr, nullptr, n,
                  RmspropRule<false, false>{neg_lr, a, w, e, wd, mu, maximize});
}
