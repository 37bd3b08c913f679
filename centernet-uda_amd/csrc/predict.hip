// Prediction over images (predict.py): the three device steps between the network's heads and a list of detections in
// source-image pixels that the training path never needed.
//
//   mirror + merge   cnuda_mirror_input makes the left-right mirrors that ride in the same 2B forward; cnuda_tta_merge
//                    folds the two halves of the raw head maps into B maps (the published CenterNet flip test).
//   projection       cnuda_project_detections maps decoded boxes / vertices / keypoints through the float64 inverse of
//                    the resize matrix, clips axis-aligned boxes to the source image and counts the rows at or above
//                    the score threshold.
//   soft-NMS merge   cnuda_soft_nms_merge runs Gaussian soft-NMS per (image, class) over the candidates of several
//                    scales and orders what survives per image; cnuda_soft_nms_merge_rotated is the same two kernels
//                    on quadrilaterals, with the exact polygon IoU of polyiou.cuh.
//
// All of it is element-wise or tiny: the merge is one grid-stride pass (one float32 rounding per output, no contraction:
// the build has -ffp-contract=off), the projection one workgroup per image, the soft-NMS a latency chain of arg-max
// rounds over at most CNUDA_SOFT_NMS_MAX_CANDIDATES candidates held in LDS.  No floating-point atomics anywhere; the
// one integer LDS atomic (compaction of a class's members) cannot change a result, because every order below is
// decided by explicit (score, class, index) keys.
#include "common.h"
#include "polyiou.cuh"

#include <math.h>

namespace cnuda {
namespace {

constexpr int kT = 256;
constexpr int kMaxCand = CNUDA_SOFT_NMS_MAX_CANDIDATES;

__global__ void mirror_input_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int W) {
    const long long total = rows * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / W;
        const int j = (int)(i - r * W);
        y[i] = x[r * W + (W - 1 - j)];
    }
}

// One pass over the four merged heads, laid end to end on the work axis: hm [B,C,HW], wh [B,wh_ch,HW], reg [B,2,HW]
// (or nothing), kps [B,2J,HW] (or nothing).  `m` is the mirrored pixel of the same row.
__global__ void tta_merge_kernel(const float* __restrict__ hm, const float* __restrict__ wh, const float* __restrict__ reg,
                                 const float* __restrict__ kps, const int* __restrict__ perm,
                                 float* __restrict__ hm_out, float* __restrict__ wh_out, float* __restrict__ reg_out,
                                 float* __restrict__ kps_out, int B, int C, int wh_ch, int J, int H, int W) {
    const long long HW = (long long)H * W;
    const long long n_hm = (long long)B * C * HW, n_wh = (long long)B * wh_ch * HW;
    const long long n_reg = reg ? (long long)B * 2 * HW : 0, n_kps = (long long)B * 2 * J * HW;
    const long long total = n_hm + n_wh + n_reg + n_kps;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long e = i;
        int head = 0, ch_n = C;
        if (e >= n_hm) { e -= n_hm; head = 1; ch_n = wh_ch; }
        if (head == 1 && e >= n_wh) { e -= n_wh; head = 2; ch_n = 2; }
        if (head == 2 && e >= n_reg) { e -= n_reg; head = 3; ch_n = 2 * J; }
        const long long pix = e % HW, plane = e / HW;
        const int ch = (int)(plane % ch_n), b = (int)(plane / ch_n);
        const int xcol = (int)(pix % W);
        const long long mpix = pix - xcol + (W - 1 - xcol);
        const long long own = ((long long)b * ch_n + ch) * HW + pix;            // image b of the first half
        const long long base2 = (long long)(B + b) * ch_n;                      // image B + b: plane base
        if (head == 0) {
            const float a = sigmoid_clamped(hm[own]), m = sigmoid_clamped(hm[(base2 + ch) * HW + mpix]);
            hm_out[e] = 0.5f * (a + m);
        } else if (head == 1) {
            wh_out[e] = ch < 2 ? 0.5f * (wh[own] + wh[(base2 + ch) * HW + mpix]) : wh[own];
        } else if (head == 2) {
            reg_out[e] = reg[own];
        } else {
            const int j = ch >> 1, pj = perm ? perm[j] : j;
            const float m = kps[(base2 + 2 * pj + (ch & 1)) * HW + mpix];
            kps_out[e] = (ch & 1) ? 0.5f * (kps[own] + m) : 0.5f * (kps[own] - m);
        }
    }
}

// One workgroup per image.  Row k: geometry x scale in float32, then double: X = (m0 x + m1 y) + m2, Y = (m3 x + m4 y) + m5.
__global__ __launch_bounds__(kT) void project_detections_kernel(
    const float* __restrict__ dets, const float* __restrict__ kps, const double* __restrict__ matrix,
    const int* __restrict__ sizes, float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ classes,
    float* __restrict__ kps_out, int* __restrict__ counts, int K, int J, int rotated, float scale, float threshold,
    int out_rows, int out_first) {
    __shared__ int red[16];
    const int b = blockIdx.x;
    const double* m = matrix + (size_t)b * 6;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const double hmax = (double)sizes[2 * b], wmax = (double)sizes[2 * b + 1];
    const int ncol = rotated ? 7 : 6;
    int above = 0;
    for (int k = threadIdx.x; k < K; k += kT) {
        const float* d = dets + ((size_t)b * K + k) * ncol;
        const size_t row = (size_t)b * out_rows + out_first + k;
        const double g0 = (double)(d[0] * scale), g1 = (double)(d[1] * scale);
        const double g2 = (double)(d[2] * scale), g3 = (double)(d[3] * scale);
        double px[4], py[4];
        if (rotated) {
            const double rad = (double)d[4] * (M_PI / 180.0);
            const double c = cos(rad), s = sin(rad);
            const double hw = g2 / 2.0, hh = g3 / 2.0;
            const double ox[4] = {-hw, hw, hw, -hw}, oy[4] = {-hh, -hh, hh, hh};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                px[v] = g0 + (ox[v] * c + oy[v] * (-s));
                py[v] = g1 + (ox[v] * s + oy[v] * c);
            }
        } else {
            px[0] = g0; py[0] = g1; px[1] = g2; py[1] = g1; px[2] = g2; py[2] = g3; px[3] = g0; py[3] = g3;
        }
        double X[4], Y[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            X[v] = (m0 * px[v] + m1 * py[v]) + m2;
            Y[v] = (m3 * px[v] + m4 * py[v]) + m5;
        }
        if (rotated) {
            float* o = boxes + row * 8;
#pragma unroll
            for (int v = 0; v < 4; ++v) { o[2 * v] = (float)X[v]; o[2 * v + 1] = (float)Y[v]; }
        } else {
            const double x1 = fmin(fmin(X[0], X[1]), fmin(X[2], X[3])), x2 = fmax(fmax(X[0], X[1]), fmax(X[2], X[3]));
            const double y1 = fmin(fmin(Y[0], Y[1]), fmin(Y[2], Y[3])), y2 = fmax(fmax(Y[0], Y[1]), fmax(Y[2], Y[3]));
            float* o = boxes + row * 4;
            o[0] = (float)fmin(fmax(x1, 0.0), wmax);
            o[1] = (float)fmin(fmax(y1, 0.0), hmax);
            o[2] = (float)fmin(fmax(x2, 0.0), wmax);
            o[3] = (float)fmin(fmax(y2, 0.0), hmax);
        }
        const float score = d[ncol - 2];
        scores[row] = score;
        classes[row] = (int)d[ncol - 1];
        above += score >= threshold ? 1 : 0;
    }
    for (int i = threadIdx.x; i < K * J; i += kT) {
        const int k = i / J, j = i - k * J;
        const float* p = kps + ((size_t)b * K * J + i) * 2;
        const double x = (double)(p[0] * scale), y = (double)(p[1] * scale);
        float* o = kps_out + (((size_t)b * out_rows + out_first + k) * J + j) * 2;
        o[0] = (float)((m0 * x + m1 * y) + m2);
        o[1] = (float)((m3 * x + m4 * y) + m5);
    }
    above = block_sum(above, red);
    if (threadIdx.x == 0) counts[b] = above;
}

// ---- soft-NMS ---------------------------------------------------------------------------------------------------------
// The order key of an arg-max round: larger score first, then the lower candidate index.
struct Best { double score; int idx; int pos; };
__device__ __forceinline__ bool better(double s, int idx, const Best& o) { return s > o.score || (s == o.score && idx < o.idx); }
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best t;
        t.score = __shfl_xor(v.score, o, 64);
        t.idx = __shfl_xor(v.idx, o, 64);
        t.pos = __shfl_xor(v.pos, o, 64);
        if (better(t.score, t.idx, v)) v = t;
    }
    return v;
}

__device__ __forceinline__ int image_candidates(const int* __restrict__ ncand, int b, int N) {
    return ncand ? min(max(ncand[b], 0), N) : N;
}

// The box record: what the two stages know about a candidate's geometry.  `Rec` is a row as it is stored (global memory
// and LDS), `Winner` a round's winner widened once, `iou` the overlap of the winner with a candidate.
struct AxisBox {                                      // (x1, y1, x2, y2)
    using Rec = float4;
    struct Winner { double x1, y1, x2, y2, area; };
    static __device__ __forceinline__ Rec load(const float* rows, size_t row) {
        return *reinterpret_cast<const float4*>(rows + row * 4);
    }
    static __device__ __forceinline__ void store(float* rows, size_t row, const Rec& r) {
        *reinterpret_cast<float4*>(rows + row * 4) = r;
    }
    static __device__ __forceinline__ Rec zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ Winner winner(const Rec& b) {
        Winner w = {b.x, b.y, b.z, b.w, 0.0};
        w.area = (w.x2 - w.x1) * (w.y2 - w.y1);
        return w;
    }
    static __device__ __forceinline__ double iou(const Winner& w, const Rec& bj) {
        const double jx1 = bj.x, jy1 = bj.y, jx2 = bj.z, jy2 = bj.w;
        const double iw = fmin(w.x2, jx2) - fmax(w.x1, jx1), ih = fmin(w.y2, jy2) - fmax(w.y1, jy1);
        double o = 0.0;
        if (iw > 0.0 && ih > 0.0) {
            const double inter = iw * ih, ua = (w.area + (jx2 - jx1) * (jy2 - jy1)) - inter;
            if (ua > 0.0) o = inter / ua;
        }
        return o;
    }
};
struct QuadBox {                                      // four (x, y) vertices; the overlap is polyiou.cuh's
    struct Rec { float4 lo, hi; };
    using Winner = polyiou::Quad;
    static __device__ __forceinline__ Rec load(const float* rows, size_t row) {
        const float4* p = reinterpret_cast<const float4*>(rows + row * 8);
        return {p[0], p[1]};
    }
    static __device__ __forceinline__ void store(float* rows, size_t row, const Rec& r) {
        float4* p = reinterpret_cast<float4*>(rows + row * 8);
        p[0] = r.lo, p[1] = r.hi;
    }
    static __device__ __forceinline__ Rec zero() { return {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}; }
    static __device__ __forceinline__ Winner winner(const Rec& b) {
        return {{b.lo.x, b.lo.z, b.hi.x, b.hi.z}, {b.lo.y, b.lo.w, b.hi.y, b.hi.w}};
    }
    static __device__ __forceinline__ double iou(const Winner& w, const Rec& bj) {
        return polyiou::convex_quad_iou(w, winner(bj)).iou;           // subject = winner, clipper = candidate
    }
};

// Stage 1: one workgroup per (image, class).  final_score [B,N] double: the emitted score of a candidate, -1 for every
// candidate of this class that was not emitted (candidates of no class in [0, C) are never written: stage 2 skips them).
// Static LDS: 56 KiB with AxisBox, 88 KiB with QuadBox (2048 quads are 64 KiB; a workgroup of gfx950 may hold 160 KiB).
template <class Box>
__global__ __launch_bounds__(kT) void soft_nms_class_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const int* __restrict__ classes, const int* __restrict__ ncand,
                                                            double* __restrict__ final_score, int N, int C) {
    __shared__ typename Box::Rec box[kMaxCand];
    __shared__ double score[kMaxCand];
    __shared__ int index[kMaxCand];
    __shared__ Best wbest[kT / 64];
    __shared__ int members;
    const int b = blockIdx.x / C, c = blockIdx.x - b * C;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = image_candidates(ncand, b, N);
    const size_t base = (size_t)b * N;
    if (tid == 0) members = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kT) {
        if (classes[base + i] != c) continue;
        const int at = atomicAdd(&members, 1);        // (placement only: every decision below compares `index`)
        box[at] = Box::load(boxes, base + i);
        score[at] = (double)scores[base + i];
        index[at] = i;
        final_score[base + i] = -1.0;
    }
    __syncthreads();
    const int m = members;
    for (int round = 0; round < m; ++round) {
        Best best = {-INFINITY, 0x7fffffff, -1};
        for (int p = tid; p < m; p += kT)
            if (better(score[p], index[p], best)) best = {score[p], index[p], p};
        best = wave_best(best);
        if (lane == 0) wbest[wid] = best;
        __syncthreads();
        best = wbest[0];
#pragma unroll
        for (int w = 1; w < kT / 64; ++w)
            if (better(wbest[w].score, wbest[w].idx, best)) best = wbest[w];
        if (!(best.score >= 1e-3)) break;             // uniform: every thread reads the same four records
        const typename Box::Winner bi = Box::winner(box[best.pos]);
        for (int p = tid; p < m; p += kT) {
            if (p == best.pos) {
                final_score[base + best.idx] = best.score;
                score[p] = -INFINITY;                 // emitted: no longer live
                continue;
            }
            if (score[p] == -INFINITY) continue;
            const double iou = Box::iou(bi, box[p]);
            score[p] = score[p] * exp(-(iou * iou) / 0.5);
        }
        __syncthreads();                              // the scores of this round before the next arg-max; wbest reusable
    }
}

// Stage 2: one workgroup per image; rank of every emitted candidate by (score desc, class asc, index asc), by counting.
constexpr int kT2 = 1024;
template <class Box>
__global__ __launch_bounds__(kT2) void soft_nms_order_kernel(
    const float* __restrict__ boxes, const int* __restrict__ classes, const float* __restrict__ kps,
    const int* __restrict__ ncand, const double* __restrict__ final_score, float* __restrict__ out_boxes,
    float* __restrict__ out_scores, int* __restrict__ out_classes, float* __restrict__ out_kps, int* __restrict__ counts,
    int N, int C, int J, int max_det, float threshold) {
    __shared__ double score[kMaxCand];                // -1: not emitted
    __shared__ int cls[kMaxCand];
    __shared__ int red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = image_candidates(ncand, b, N);
    const size_t base = (size_t)b * N;
    int emitted = 0;
    for (int i = tid; i < n; i += kT2) {
        const int c = classes[base + i];
        const bool in = c >= 0 && c < C;
        const double s = in ? final_score[base + i] : -1.0;
        score[i] = s;
        cls[i] = c;
        emitted += s >= 0.0 ? 1 : 0;
    }
    emitted = block_sum(emitted, red);                // (its barriers also publish score / cls)
    int above = 0;
    for (int i = tid; i < n; i += kT2) {
        const double s = score[i];
        if (!(s >= 0.0)) continue;
        const int c = cls[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double t = score[j];
            rank += (t > s || (t == s && t >= 0.0 && (cls[j] < c || (cls[j] == c && j < i)))) ? 1 : 0;
        }
        if (rank >= max_det) continue;
        const size_t row = (size_t)b * max_det + rank;
        Box::store(out_boxes, row, Box::load(boxes, base + i));
        const float sf = (float)s;
        out_scores[row] = sf;
        out_classes[row] = c;
        for (int q = 0; q < 2 * J; ++q) out_kps[row * 2 * J + q] = kps[(base + i) * 2 * J + q];
        above += sf >= threshold ? 1 : 0;
    }
    for (int r = min(emitted, max_det) + tid; r < max_det; r += kT2) {
        const size_t row = (size_t)b * max_det + r;
        Box::store(out_boxes, row, Box::zero());
        out_scores[row] = 0.0f;
        out_classes[row] = -1;
        for (int q = 0; q < 2 * J; ++q) out_kps[row * 2 * J + q] = 0.0f;
    }
    above = block_sum(above, red);
    if (tid == 0) counts[b] = above;
}

// Both entries: the checks, the two launches.
template <class Box>
int soft_nms_merge(const char* who, const float* boxes, const float* scores, const int* classes, const float* kps,
                   const int* ncand, float* out_boxes, float* out_scores, int* out_classes, float* out_kps, int* counts,
                   int B, int N, int C, int J, int max_detections, float threshold, void* workspace, size_t workspace_bytes,
                   cnuda_stream_t stream) {
    CNUDA_REQUIRE(out_boxes && out_scores && out_classes && counts, "%s: null pointer", who);
    CNUDA_REQUIRE(B > 0 && N >= 0 && C > 0 && max_detections > 0, "%s: bad sizes", who);
    CNUDA_REQUIRE(N <= kMaxCand, "%s: N=%d candidates per image exceed the supported %d", who, N, kMaxCand);
    CNUDA_REQUIRE(N == 0 || (boxes && scores && classes), "%s: null pointer", who);
    CNUDA_REQUIRE(J >= 0 && (J > 0 ? (out_kps && (kps || N == 0)) : (!kps && !out_kps)),
                  "%s: kps and out_kps are given exactly when J > 0 (J=%d)", who, J);
    CNUDA_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)out_boxes & 15) == 0,
                  "%s: boxes and out_boxes must be 16-byte aligned", who);
    CNUDA_REQUIRE(workspace && workspace_bytes >= (size_t)B * N * sizeof(double) + 256, "%s: workspace too small", who);
    double* final_score = reinterpret_cast<double*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        CNUDA_LAUNCH(soft_nms_class_kernel<Box>, dim3(B * C), dim3(kT), 0, st, boxes, scores, classes, ncand, final_score,
                     N, C);
        const int rc = check_launch(who);
        if (rc) return rc;
    }
    CNUDA_LAUNCH(soft_nms_order_kernel<Box>, dim3(B), dim3(kT2), 0, st, boxes, classes, kps, ncand, final_score, out_boxes,
                 out_scores, out_classes, out_kps, counts, N, C, J, max_detections, threshold);
    return check_launch(who);
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_mirror_input(const float* x, float* y, long long planes, int H, int W, cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y, "cnuda_mirror_input: null pointer");
    CNUDA_REQUIRE(planes > 0 && H > 0 && W > 0, "cnuda_mirror_input: bad sizes");
    const long long rows = planes * H, total = rows * W;
    CNUDA_REQUIRE(!(x < y + total && y < x + total), "cnuda_mirror_input: x and y overlap");
    CNUDA_LAUNCH(mirror_input_kernel, dim3(stream_grid(total, kT)), dim3(kT), 0, (hipStream_t)stream, x, y, rows, W);
    return check_launch("cnuda_mirror_input");
}

extern "C" int cnuda_tta_merge(const float* hm, const float* wh, const float* reg, const float* kps, const int* perm,
                               float* hm_out, float* wh_out, float* reg_out, float* kps_out,
                               int B, int C, int wh_ch, int J, int H, int W, cnuda_stream_t stream) {
    CNUDA_REQUIRE(hm && wh && hm_out && wh_out, "cnuda_tta_merge: null pointer");
    CNUDA_REQUIRE((reg == nullptr) == (reg_out == nullptr), "cnuda_tta_merge: reg and reg_out go together");
    CNUDA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "cnuda_tta_merge: bad sizes");
    CNUDA_REQUIRE(wh_ch == 2 || wh_ch == 3, "cnuda_tta_merge: wh has %d channels (2, or 3 with the angle)", wh_ch);
    CNUDA_REQUIRE(J >= 0 && (J > 0 ? (kps && kps_out) : (!kps && !kps_out && !perm)),
                  "cnuda_tta_merge: kps, kps_out (and perm) are given exactly when J > 0 (J=%d)", J);
    const long long total = (long long)B * ((long long)C + wh_ch + (reg ? 2 : 0) + 2 * J) * H * W;
    CNUDA_LAUNCH(tta_merge_kernel, dim3(stream_grid(total, kT)), dim3(kT), 0, (hipStream_t)stream, hm, wh, reg, kps, perm,
                 hm_out, wh_out, reg_out, kps_out, B, C, wh_ch, J, H, W);
    return check_launch("cnuda_tta_merge");
}

extern "C" int cnuda_project_detections(const float* dets, const float* kps, const double* matrix, const int* sizes,
                                        float* boxes, float* scores, int* classes, float* kps_out, int* counts,
                                        int B, int K, int J, int rotated, float scale, float threshold,
                                        int out_rows, int out_first, cnuda_stream_t stream) {
    CNUDA_REQUIRE(dets && matrix && sizes && boxes && scores && classes && counts, "cnuda_project_detections: null pointer");
    CNUDA_REQUIRE(B > 0 && K > 0, "cnuda_project_detections: bad sizes");
    CNUDA_REQUIRE(J >= 0 && (J > 0 ? (kps && kps_out) : (!kps && !kps_out)),
                  "cnuda_project_detections: kps and kps_out are given exactly when J > 0 (J=%d)", J);
    CNUDA_REQUIRE(out_first >= 0 && (long long)out_first + K <= (long long)out_rows,
                  "cnuda_project_detections: rows %d..%d do not fit %d output rows", out_first, out_first + K, out_rows);
    CNUDA_LAUNCH(project_detections_kernel, dim3(B), dim3(kT), 0, (hipStream_t)stream, dets, kps, matrix, sizes, boxes,
                 scores, classes, kps_out, counts, K, J, rotated ? 1 : 0, scale, threshold, out_rows, out_first);
    return check_launch("cnuda_project_detections");
}

extern "C" size_t cnuda_predict_workspace_bytes(int B, int N) {
    if (B <= 0 || N < 0 || N > kMaxCand) {
        set_error("cnuda_predict_workspace_bytes: B=%d, N=%d (at most %d candidates per image)", B, N, kMaxCand);
        return 0;
    }
    return (size_t)B * N * sizeof(double) + 256;
}

extern "C" int cnuda_soft_nms_merge(const float* boxes, const float* scores, const int* classes, const float* kps,
                                    const int* ncand, float* out_boxes, float* out_scores, int* out_classes,
                                    float* out_kps, int* counts, int B, int N, int C, int J, int max_detections,
                                    float threshold, void* workspace, size_t workspace_bytes, cnuda_stream_t stream) {
    return soft_nms_merge<AxisBox>("cnuda_soft_nms_merge", boxes, scores, classes, kps, ncand, out_boxes, out_scores,
                                   out_classes, out_kps, counts, B, N, C, J, max_detections, threshold, workspace,
                                   workspace_bytes, stream);
}

extern "C" int cnuda_soft_nms_merge_rotated(const float* boxes, const float* scores, const int* classes, const float* kps,
                                            const int* ncand, float* out_boxes, float* out_scores, int* out_classes,
                                            float* out_kps, int* counts, int B, int N, int C, int J, int max_detections,
                                            float threshold, void* workspace, size_t workspace_bytes,
                                            cnuda_stream_t stream) {
    return soft_nms_merge<QuadBox>("cnuda_soft_nms_merge_rotated", boxes, scores, classes, kps, ncand, out_boxes,
                                   out_scores, out_classes, out_kps, counts, B, N, C, J, max_detections, threshold,
                                   workspace, workspace_bytes, stream);
}
