// Fourier domain adaptation for gfx950: the amplitude transfer of utils/image.py:137-230 (FDA_source_to_target).
//
//   S = fft2(src), T = fft2(trg) per image and channel;  Z = mask ? |T| S/|S| (|S| = 0: (|T|, 0)) : S;
//   out = irfft2(Z[..., :W/2+1], s=(H, W))   -- torch 1.x's irfft(onesided=False, signal_sizes) narrowing
//
// Only the W/2+1 columns of the half spectrum are ever formed.  Four launches over a workspace holding the two half
// spectra S | T ([2][B*C][H][W/2+1] complex fp32):
//   (a) rows, forward: two rows y, y+1 of src (or of trg) as row_y + i row_{y+1}, one complex FFT of length W,
//       split into the two half spectra
//   (b) columns, forward: complex FFT of length H over S and T, a block of adjacent columns per workgroup
//   (c) columns, inverse: builds Z from S, T and the mask while it loads, inverse FFT of length H, Z' over S
//   (d) rows, inverse: two rows y, y+1 Hermitian-extended (DC / Nyquist: real part only) as X_y + i X_{y+1}, inverse
//       FFT of length W, real and imaginary part scaled by 1/(HW) are the two output rows
// A line lives in LDS (two ping-pong buffers); lengths made of 2, 3, 4, 5 run a mixed-radix Stockham FFT, any other
// length a direct O(N^2) DFT.  Twiddles: one table per length, exp(-2 pi i t / N) in fp64 rounded to fp32, built on
// the host and cached on the device.  No atomics: the result is deterministic.
#include <map>
#include <math.h>
#include <mutex>
#include <vector>

#include "common.h"

namespace cnuda {
namespace {

constexpr int kT = 256;
constexpr int kMaxLen = 4096;         // two LDS buffers of one line: 64 KiB
constexpr int kLdsElems = 4096;       // complex elements per LDS buffer (lines x leading dimension)
constexpr int kMaxLines = 16;
constexpr int kMaxFactors = 16;

struct LinePlan {
    int n, nf, direct;
    int f[kMaxFactors];   // radices, first stage first
};

LinePlan make_plan(int n) {
    LinePlan p{};
    p.n = n;
    int m = n;
    while (m % 4 == 0 && p.nf < kMaxFactors) { p.f[p.nf++] = 4; m /= 4; }
    for (int r : {2, 3, 5})
        while (m % r == 0 && p.nf < kMaxFactors) { p.f[p.nf++] = r; m /= r; }
    p.direct = m != 1;
    return p;
}

// lines per workgroup and their LDS leading dimension (+1 element against bank conflicts when there are several)
void line_geometry(int n, int& nl, int& ld) {
    nl = kLdsElems / (n + 1);
    if (nl < 1) { nl = 1; ld = n; return; }
    if (nl > kMaxLines) nl = kMaxLines;
    ld = n + 1;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int R> struct Roots;
template <> struct Roots<3> {
    static constexpr float c[3] = {1.0f, -0.5f, -0.5f};
    static constexpr float s[3] = {0.0f, 0.866025403784438647f, -0.866025403784438647f};
};
template <> struct Roots<5> {
    static constexpr float c[5] = {1.0f, 0.309016994374947424f, -0.809016994374947424f, -0.809016994374947424f,
                                   0.309016994374947424f};
    static constexpr float s[5] = {0.0f, 0.951056516295153572f, 0.587785252292473129f, -0.587785252292473129f,
                                   -0.951056516295153572f};
};

// y_q = sum_r v_r exp(sgn 2 pi i r q / R), sgn = -1 forward, +1 inverse
template <int R, bool INV>
__device__ __forceinline__ void butterfly(float2* v) {
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]);
        const float2 s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
        const float2 rot = INV ? make_float2(-d13.y, d13.x) : make_float2(d13.y, -d13.x);   // (+-i) * d13
        v[0] = cadd(s02, s13);
        v[2] = csub(s02, s13);
        v[1] = cadd(d02, rot);
        v[3] = csub(d02, rot);
    } else {
        float2 y[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float2 acc = v[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const int t = (r * q) % R;
                const float2 w = make_float2(Roots<R>::c[t], INV ? Roots<R>::s[t] : -Roots<R>::s[t]);
                acc = cadd(acc, cmul(v[r], w));
            }
            y[q] = acc;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) v[q] = y[q];
    }
}

// One Stockham stage (Govindaraju et al., SC'08): butterfly j of every line reads x[j + r N/R], twiddles by
// w_{Ns R}^{r (j mod Ns)} and writes y[(j - k) R + k + r Ns].
template <int R, bool INV>
__device__ void stockham_stage(const float2* a, float2* b, int nl, int ld, int n, int ns,
                               const float2* __restrict__ tw) {
    const int m = n / R, tstride = n / (ns * R);
    for (int i = threadIdx.x; i < nl * m; i += blockDim.x) {
        const int c = i / m, j = i - c * m;
        const int k = j % ns;
        const float2* x = a + c * ld;
        float2* y = b + c * ld;
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            v[r] = x[j + r * m];
            if (r > 0 && k > 0) {
                float2 w = tw[r * k * tstride];
                if (INV) w.y = -w.y;
                v[r] = cmul(v[r], w);
            }
        }
        butterfly<R, INV>(v);
        const int d = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) y[d + r * ns] = v[r];
    }
    __syncthreads();
}

// Transforms nl lines (a[c*ld + t], t < n) in place of the ping-pong pair; returns the buffer holding the result.
template <bool INV>
__device__ float2* fft_lines(float2* a, float2* b, int nl, int ld, const LinePlan& p, const float2* __restrict__ tw) {
    const int n = p.n;
    if (p.direct) {
        for (int i = threadIdx.x; i < nl * n; i += blockDim.x) {
            const int c = i / n, k = i - c * n;
            const float2* x = a + c * ld;
            float2 acc = make_float2(0.0f, 0.0f);
            int t = 0;
            for (int s = 0; s < n; ++s) {
                float2 w = tw[t];
                if (INV) w.y = -w.y;
                acc = cadd(acc, cmul(x[s], w));
                t += k;
                if (t >= n) t -= n;
            }
            b[c * ld + k] = acc;
        }
        __syncthreads();
        return b;
    }
    int ns = 1;
    for (int s = 0; s < p.nf; ++s) {
        switch (p.f[s]) {
            case 4: stockham_stage<4, INV>(a, b, nl, ld, n, ns, tw); break;
            case 2: stockham_stage<2, INV>(a, b, nl, ld, n, ns, tw); break;
            case 3: stockham_stage<3, INV>(a, b, nl, ld, n, ns, tw); break;
            default: stockham_stage<5, INV>(a, b, nl, ld, n, ns, tw); break;
        }
        float2* t = a;
        a = b;
        b = t;
        ns *= p.f[s];
    }
    return a;
}

// (a) rows: line q of the grid = rows 2j, 2j+1 of src (q < P) or of trg (q - P = j), P = ceil(rows / 2), as one
// complex FFT of row 2j + i * row 2j+1, split into their half spectra.  Two rows of ONE tensor share a line: a source
// line carries no rounding noise of the target (a zero source stays exactly zero: the (|T|, 0) rule).
__global__ __launch_bounds__(kT) void fda_rows_fwd_kernel(const float* __restrict__ src, const float* __restrict__ trg,
                                                          float2* __restrict__ S, float2* __restrict__ T, long long rows,
                                                          int nl, int ld, LinePlan p, const float2* __restrict__ tw) {
    extern __shared__ float2 lds[];
    float2* a = lds;
    float2* b = lds + nl * ld;
    const int n = p.n, wh = n / 2 + 1;
    const long long P = (rows + 1) / 2, q0 = (long long)blockIdx.x * nl;
    const int nb = (int)(2 * P - q0 < nl ? 2 * P - q0 : nl);
    for (int i = threadIdx.x; i < nb * n; i += blockDim.x) {
        const int c = i / n, t = i - c * n;
        const long long q = q0 + c;
        const float* x = q < P ? src : trg;
        const long long ra = 2 * (q < P ? q : q - P);
        const float xb = ra + 1 < rows ? x[(size_t)(ra + 1) * n + t] : 0.0f;
        a[c * ld + t] = make_float2(x[(size_t)ra * n + t], xb);
    }
    __syncthreads();
    const float2* z = fft_lines<false>(a, b, nb, ld, p, tw);
    for (int i = threadIdx.x; i < nb * wh; i += blockDim.x) {
        const int c = i / wh, k = i - c * wh;
        const long long q = q0 + c;
        float2* y = q < P ? S : T;
        const long long ra = 2 * (q < P ? q : q - P);
        const float2 u = z[c * ld + k], v = z[c * ld + (k == 0 ? 0 : n - k)];
        y[(size_t)ra * wh + k] = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));   // (Z_k + conj Z_{N-k}) / 2
        if (ra + 1 < rows)
            y[(size_t)(ra + 1) * wh + k] = make_float2(0.5f * (u.y + v.y), 0.5f * (v.x - u.x));   // (Z_k - conj Z_{N-k}) / 2i
    }
}

// (b) / (c) columns of one image: block (x0 / nl, image) owns columns x0 .. x0+nl-1 of an [H][wh] spectrum.
// MIX: the image is spectrum `img` of S, T its target twin; loads Z (the amplitude transfer), writes the inverse over S.
template <bool MIX>
__global__ __launch_bounds__(kT) void fda_cols_kernel(float2* __restrict__ S, const float2* __restrict__ T,
                                                      const unsigned char* __restrict__ mask, int wh, int nl, int ld,
                                                      LinePlan p, const float2* __restrict__ tw) {
    extern __shared__ float2 lds[];
    float2* a = lds;
    float2* b = lds + nl * ld;
    const int h = p.n;
    const int x0 = blockIdx.x * nl;
    const int nb = wh - x0 < nl ? wh - x0 : nl;
    const size_t base = (size_t)blockIdx.y * h * wh;
    for (int i = threadIdx.x; i < nb * h; i += blockDim.x) {
        const int y = i / nb, c = i - y * nb;
        const size_t g = base + (size_t)y * wh + x0 + c;
        float2 s = S[g];
        if (MIX && mask[(size_t)y * wh + x0 + c]) {
            const float2 t = T[g];
            const float at = sqrtf(t.x * t.x + t.y * t.y), as = sqrtf(s.x * s.x + s.y * s.y);
            if (as > 0.0f) {
                const float q = at / as;
                s = make_float2(s.x * q, s.y * q);
            } else {
                s = make_float2(at, 0.0f);           // atan2(0, 0) = 0
            }
        }
        a[c * ld + y] = s;
    }
    __syncthreads();
    const float2* z = fft_lines<MIX>(a, b, nb, ld, p, tw);
    for (int i = threadIdx.x; i < nb * h; i += blockDim.x) {
        const int y = i / nb, c = i - y * nb;
        S[base + (size_t)y * wh + x0 + c] = z[c * ld + y];
    }
}

// (d) rows, inverse: line c of the block = rows 2(r0 + c), 2(r0 + c) + 1 of Y = S
__global__ __launch_bounds__(kT) void fda_rows_inv_kernel(const float2* __restrict__ Y, float* __restrict__ out,
                                                          long long rows, float scale, int nl, int ld, LinePlan p,
                                                          const float2* __restrict__ tw) {
    extern __shared__ float2 lds[];
    float2* a = lds;
    float2* b = lds + nl * ld;
    const int n = p.n, wh = n / 2 + 1;
    const long long pairs = (rows + 1) / 2, q0 = (long long)blockIdx.x * nl;
    const int nb = (int)(pairs - q0 < nl ? pairs - q0 : nl);
    for (int i = threadIdx.x; i < nb * n; i += blockDim.x) {
        const int c = i / n, k = i - c * n;
        const long long ra = 2 * (q0 + c), rb = ra + 1;
        float2 xa, xb = make_float2(0.0f, 0.0f);
        const bool real_bin = k == 0 || 2 * k == n;           // DC, Nyquist: the imaginary part is dropped
        const int kk = k < wh ? k : n - k;
        xa = Y[(size_t)ra * wh + kk];
        if (rb < rows) xb = Y[(size_t)rb * wh + kk];
        if (real_bin) {
            xa.y = 0.0f;
            xb.y = 0.0f;
        } else if (k >= wh) {
            xa.y = -xa.y;
            xb.y = -xb.y;
        }
        a[c * ld + k] = make_float2(xa.x - xb.y, xa.y + xb.x);   // X_a + i X_b
    }
    __syncthreads();
    const float2* z = fft_lines<true>(a, b, nb, ld, p, tw);
    for (int i = threadIdx.x; i < nb * n; i += blockDim.x) {
        const int c = i / n, t = i - c * n;
        const long long ra = 2 * (q0 + c);
        const float2 v = z[c * ld + t];
        out[(size_t)ra * n + t] = v.x * scale;
        if (ra + 1 < rows) out[(size_t)(ra + 1) * n + t] = v.y * scale;
    }
}

// per (device, length) twiddle table, exp(-2 pi i t / n) for t < n, fp64 on the host rounded to fp32
const float2* twiddles(int n) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, float2*> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, n});
    if (it != cache.end()) return it->second;
    std::vector<float2> h(n);
    for (int t = 0; t < n; ++t) {
        const double ang = -2.0 * M_PI * (double)t / (double)n;
        h[t] = make_float2((float)cos(ang), (float)sin(ang));
    }
    float2* d = nullptr;
    if (hipMalloc(&d, sizeof(float2) * n) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    cache[{dev, n}] = d;
    return d;
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" size_t cnuda_fda_workspace_bytes(int B, int C, int H, int W) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * B * C * H * (W / 2 + 1) * sizeof(float2);
}

extern "C" int cnuda_fda_source_to_target(const float* src, const float* trg, const uint8_t* use_target_amp,
                                          float* out, int B, int C, int H, int W, void* workspace,
                                          size_t workspace_bytes, cnuda_stream_t stream) {
    CNUDA_REQUIRE(src && trg && use_target_amp && out && B > 0 && C > 0 && H > 0 && W > 0,
                  "cnuda_fda_source_to_target: bad arguments");
    CNUDA_REQUIRE(H <= kMaxLen && W <= kMaxLen,
                  "cnuda_fda_source_to_target: image %d x %d exceeds the %d-point line one workgroup's LDS holds", H,
                  W, kMaxLen);
    CNUDA_REQUIRE(workspace && workspace_bytes >= cnuda_fda_workspace_bytes(B, C, H, W),
                  "cnuda_fda_source_to_target: workspace");
    const float2* twh = twiddles(H);
    const float2* tww = twiddles(W);
    CNUDA_REQUIRE(twh && tww, "cnuda_fda_source_to_target: twiddle table allocation failed");
    hipStream_t st = (hipStream_t)stream;
    const int wh = W / 2 + 1;
    const long long rows = (long long)B * C * H;
    float2* S = (float2*)workspace;
    float2* T = S + (size_t)rows * wh;
    const LinePlan pw = make_plan(W), ph = make_plan(H);
    int nlw, ldw, nlh, ldh;
    line_geometry(W, nlw, ldw);
    line_geometry(H, nlh, ldh);
    const size_t ldsw = sizeof(float2) * 2 * nlw * ldw, ldsh = sizeof(float2) * 2 * nlh * ldh;
    const dim3 gcols(ceil_div(wh, nlh), B * C);
    CNUDA_LAUNCH(fda_rows_fwd_kernel, dim3(ceil_div(2 * ((rows + 1) / 2), nlw)), dim3(kT), ldsw, st, src, trg, S, T, rows, nlw, ldw,
                 pw, tww);
    CNUDA_LAUNCH(fda_cols_kernel<false>, dim3(gcols.x, 2 * B * C), dim3(kT), ldsh, st, S, (const float2*)nullptr,
                 (const unsigned char*)nullptr, wh, nlh, ldh, ph, twh);
    CNUDA_LAUNCH(fda_cols_kernel<true>, gcols, dim3(kT), ldsh, st, S, (const float2*)T, use_target_amp, wh, nlh,
                 ldh, ph, twh);
    CNUDA_LAUNCH(fda_rows_inv_kernel, dim3(ceil_div((rows + 1) / 2, nlw)), dim3(kT), ldsw, st, (const float2*)S, out,
                 rows, (float)(1.0 / ((double)H * (double)W)), nlw, ldw, pw, tww);
    return check_launch("cnuda_fda_source_to_target");
}
