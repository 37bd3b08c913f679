// COCO evaluation on the GPU (evaluation/coco.py): the masks of rotated boxes as one span per image row, the IoU of
// every (detection, ground truth) pair of one image and one category in float64, and COCOeval's greedy matching for
// the ten IoU thresholds and four area ranges.  For keypoints (evaluation/coco_keypoints.py) the pair similarity is the
// object keypoint similarity instead, and a ground truth without a labelled joint is ignored by the matching.
// Everything here is integers and doubles that do not depend on scheduling: no floating-point atomics, the only atomics
// are integer min / max on LDS.
//
// A "group" is one (image, category): five ints {first detection, detections, first ground truth, ground truths,
// first pair}; pair (d, g) of a group lives at first pair + d * ground truths + g.  Groups are built on the host; every
// kernel checks a group against the array sizes before it touches memory and skips one that does not fit.
#include <limits.h>

#include "common.h"
#include "evalcoco.cuh"
#include "polyiou.cuh"

// the axis IoU's last bit decides comparisons against a threshold: no fused multiply-add (the Makefile says so too)
#pragma clang fp contract(off)

namespace cnuda {
namespace {

using namespace evalcoco;

constexpr int kSpanThreads = 256;
constexpr int kPairChunks = 8;

struct Group {
    int det0, nd, gt0, ng, pair0;
};

__device__ __forceinline__ bool load_group(const int* groups, int g, int ND, int NGT, long long num_pairs, Group& q) {
    q.det0 = groups[5 * g], q.nd = groups[5 * g + 1], q.gt0 = groups[5 * g + 2], q.ng = groups[5 * g + 3];
    q.pair0 = groups[5 * g + 4];
    return q.det0 >= 0 && q.nd >= 0 && q.gt0 >= 0 && q.ng >= 0 && q.pair0 >= 0 && (long long)q.det0 + q.nd <= ND &&
           (long long)q.gt0 + q.ng <= NGT && (long long)q.pair0 + (long long)q.nd * q.ng <= num_pairs;
}

// One workgroup per box.  lds: left[H], right[H].  spans: [box][row] (left, right), (0, -1) for an empty row.
__global__ __launch_bounds__(kSpanThreads) void eval_box_spans_kernel(const int* __restrict__ verts, int H, int W,
                                                                      int2* __restrict__ spans, int* __restrict__ rows,
                                                                      double* __restrict__ area) {
    extern __shared__ int lds[];
    int* left = lds;
    int* right = lds + H;
    __shared__ int vx[4], vy[4], n_scan, row_lo, row_hi, red[16];
    __shared__ Line lines[4];
    __shared__ ScanInterval scan[kMaxScanIntervals];
    const int box = blockIdx.x, tid = threadIdx.x;
    if (tid < 4) {
        vx[tid] = verts[8 * box + 2 * tid];
        vy[tid] = verts[8 * box + 2 * tid + 1];
    }
    for (int r = tid; r < H; r += kSpanThreads) left[r] = INT_MAX, right[r] = INT_MIN;
    if (tid == 0) row_lo = INT_MAX, row_hi = INT_MIN;
    __syncthreads();
    if (tid < 4) {
        const int p = (tid + 3) & 3;
        lines[tid] = line_setup(vx[p], vy[p], vx[tid], vy[tid], W, H);
    } else if (tid == 64) {
        n_scan = scan_setup(vx, vy, W, H, scan);
    }
    __syncthreads();
    // the outline: lanes take steps
    for (int e = 0; e < 4; ++e) {
        const Line l = lines[e];
        if (l.count < 0) continue;
        for (int k = tid; k <= l.count + 1; k += kSpanThreads) {
            int x, y;
            if (k <= l.count) line_pixel(l, k, x, y);
            else x = l.end_x, y = l.end_y;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                atomicMin(&left[y], x);
                atomicMax(&right[y], x);
            }
        }
    }
    // the scanlines: lanes take rows
    for (int s = 0; s < n_scan; ++s) {
        const int lo = scan[s].row_begin < 0 ? 0 : scan[s].row_begin, hi = scan[s].row_end < H ? scan[s].row_end : H;
        for (int r = lo + tid; r < hi; r += kSpanThreads) {
            int a, b;
            if (scan_row(scan[s], r, W, a, b)) {
                atomicMin(&left[r], a);
                atomicMax(&right[r], b);
            }
        }
    }
    __syncthreads();
    int count = 0;
    for (int r = tid; r < H; r += kSpanThreads) {
        int a = left[r], b = right[r];
        if (a <= b) {
            count += b - a + 1;
            atomicMin(&row_lo, r);
            atomicMax(&row_hi, r);
        } else {
            a = 0, b = -1;
        }
        spans[(size_t)box * H + r] = make_int2(a, b);
    }
    count = block_sum<int>(count, red);      // its barriers also order row_lo / row_hi
    if (tid == 0) {
        const bool any = row_lo <= row_hi;
        rows[2 * box] = any ? row_lo : 0;
        rows[2 * box + 1] = any ? row_hi : -1;
        area[box] = (double)count;
    }
}

// One wave per pair, lanes over the rows both masks cover.  Boxes [0, ND) are the detections, [ND, ND + NGT) the
// ground truths.
__global__ __launch_bounds__(256) void eval_iou_rotated_kernel(const int* __restrict__ groups, int ND, int NGT,
                                                               long long num_pairs, const int2* __restrict__ spans,
                                                               const int* __restrict__ rows,
                                                               const double* __restrict__ area, int H,
                                                               double* __restrict__ iou) {
    Group q;
    if (!load_group(groups, blockIdx.x, ND, NGT, num_pairs, q)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const long long pairs = (long long)q.nd * q.ng;
    for (long long p = (long long)blockIdx.y * waves + wave; p < pairs; p += (long long)gridDim.y * waves) {
        const int bd = q.det0 + (int)(p / q.ng), bg = ND + q.gt0 + (int)(p % q.ng);
        int ya = max(rows[2 * bd], rows[2 * bg]), yb = min(rows[2 * bd + 1], rows[2 * bg + 1]);
        ya = max(ya, 0), yb = min(yb, H - 1);
        int inter = 0;
        for (int r = ya + lane; r <= yb; r += 64) {
            const int2 a = spans[(size_t)bd * H + r], b = spans[(size_t)bg * H + r];
            const int o = min(a.y, b.y) - max(a.x, b.x) + 1;
            inter += o > 0 ? o : 0;
        }
        inter = wave_sum(inter);
        if (lane == 0) {
            const double i = (double)inter, u = area[bd] + area[bg] - i;
            iou[q.pair0 + p] = u > 0.0 ? i / u : 0.0;
        }
    }
}

// One thread per pair.  Boxes are float32 (x, y, w, h); the arithmetic is double, as pycocotools' bbIou.
__global__ __launch_bounds__(256) void eval_iou_axis_kernel(const int* __restrict__ groups, int ND, int NGT,
                                                            long long num_pairs, const float* __restrict__ det,
                                                            const float* __restrict__ gt, double* __restrict__ iou) {
    Group q;
    if (!load_group(groups, blockIdx.x, ND, NGT, num_pairs, q)) return;
    const long long pairs = (long long)q.nd * q.ng;
    for (long long p = (long long)blockIdx.y * blockDim.x + threadIdx.x; p < pairs; p += (long long)gridDim.y * blockDim.x) {
        const float* D = det + 4 * (size_t)(q.det0 + (int)(p / q.ng));
        const float* Gt = gt + 4 * (size_t)(q.gt0 + (int)(p % q.ng));
        const double dx = D[0], dy = D[1], dw = D[2], dh = D[3], gx = Gt[0], gy = Gt[1], gw = Gt[2], gh = Gt[3];
        const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx), h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        double o = 0.0;
        if (w > 0.0 && h > 0.0) {
            const double i = w * h;
            o = i / (dw * dh + gw * gh - i);
        }
        iou[q.pair0 + p] = o;
    }
}

// One thread per pair: the exact polygon IoU (polyiou.cuh), subject = detection, clipper = ground truth.  quads: float32
// [ND + NGT, 4, 2], detections first.  The columns of the grid past the groups write the areas of all boxes, whatever
// the groups say.
__global__ __launch_bounds__(256) void eval_iou_quads_kernel(const int* __restrict__ groups, int num_groups, int ND, int NGT,
                                                             long long num_pairs, const float* __restrict__ quads,
                                                             double* __restrict__ iou, double* __restrict__ area) {
    if ((int)blockIdx.x >= num_groups) {
        const long long box = ((long long)(blockIdx.x - num_groups) * gridDim.y + blockIdx.y) * blockDim.x + threadIdx.x;
        if (box < (long long)ND + NGT) area[box] = polyiou::quad_area(polyiou::load_quad(quads + 8 * box));
        return;
    }
    Group q;
    if (!load_group(groups, blockIdx.x, ND, NGT, num_pairs, q)) return;
    const long long pairs = (long long)q.nd * q.ng;
    for (long long p = (long long)blockIdx.y * blockDim.x + threadIdx.x; p < pairs; p += (long long)gridDim.y * blockDim.x) {
        const float* D = quads + 8 * (size_t)(q.det0 + (int)(p / q.ng));
        const float* Gt = quads + 8 * ((size_t)ND + (size_t)(q.gt0 + (int)(p % q.ng)));
        iou[q.pair0 + p] = polyiou::convex_quad_iou(polyiou::load_quad(D), polyiou::load_quad(Gt)).iou;
    }
}

constexpr int kMaxJoints = 64;

// One thread per detection, then per ground truth: the area COCO's loadRes gives a keypoint result (the bounds of its J
// predicted joints), and the flag of a ground truth without a labelled joint (COCOeval._prepare ignores it).
__global__ __launch_bounds__(256) void eval_kps_prepare_kernel(const float* __restrict__ det_kps,
                                                               const unsigned char* __restrict__ gt_vis, int ND, int NGT,
                                                               int J, double* __restrict__ det_area,
                                                               unsigned char* __restrict__ gt_flags) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ND) {
        const float* P = det_kps + 2 * (size_t)J * (size_t)i;
        double x0 = P[0], x1 = x0, y0 = P[1], y1 = y0;
        for (int j = 1; j < J; ++j) {
            const double x = P[2 * j], y = P[2 * j + 1];
            x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
        }
        det_area[i] = (x1 - x0) * (y1 - y0);
    } else if (i < (long long)ND + NGT) {
        const size_t g = (size_t)(i - ND);
        int k1 = 0;
        for (int j = 0; j < J; ++j) k1 += gt_vis[g * J + j] > 0;
        gt_flags[g] = k1 == 0;
    }
}

// One thread per pair: COCOeval.computeOks in its order of operations.  Joints are float32 (x, y), the arithmetic is
// double; the sum runs over ascending j.  lds: var_j = (2 sigma_j)^2.
__global__ __launch_bounds__(256) void eval_oks_kernel(const int* __restrict__ groups, int ND, int NGT, long long num_pairs,
                                                       const float* __restrict__ det_kps, const float* __restrict__ gt_kps,
                                                       const unsigned char* __restrict__ gt_vis,
                                                       const double* __restrict__ gt_area, const float* __restrict__ gt_box,
                                                       const double* __restrict__ sigmas, int J, double* __restrict__ oks) {
    __shared__ double var[kMaxJoints];
    Group q;
    if (!load_group(groups, blockIdx.x, ND, NGT, num_pairs, q)) return;      // the whole workgroup leaves
    if ((int)threadIdx.x < J) {
        const double s = 2.0 * sigmas[threadIdx.x];
        var[threadIdx.x] = s * s;
    }
    __syncthreads();
    const long long pairs = (long long)q.nd * q.ng;
    for (long long p = (long long)blockIdx.y * blockDim.x + threadIdx.x; p < pairs; p += (long long)gridDim.y * blockDim.x) {
        const size_t d = (size_t)(q.det0 + (int)(p / q.ng)), g = (size_t)(q.gt0 + (int)(p % q.ng));
        const float* D = det_kps + 2 * (size_t)J * d;
        const float* Gt = gt_kps + 2 * (size_t)J * g;
        const unsigned char* V = gt_vis + (size_t)J * g;
        int k1 = 0;
        for (int j = 0; j < J; ++j) k1 += V[j] > 0;
        const double scale = gt_area[g] + 0x1p-52;
        double sum = 0.0;
        if (k1 > 0) {
            for (int j = 0; j < J; ++j) {
                if (V[j] == 0) continue;
                const double dx = (double)D[2 * j] - (double)Gt[2 * j], dy = (double)D[2 * j + 1] - (double)Gt[2 * j + 1];
                sum += exp(-((dx * dx + dy * dy) / var[j] / scale / 2.0));
            }
        } else {      // no labelled joint: the distance to the ground-truth box doubled about its centre, over all joints
            const double bx = gt_box[4 * g], by = gt_box[4 * g + 1], bw = gt_box[4 * g + 2], bh = gt_box[4 * g + 3];
            const double x0 = bx - bw, x1 = bx + 2.0 * bw, y0 = by - bh, y1 = by + 2.0 * bh;
            for (int j = 0; j < J; ++j) {
                const double xd = D[2 * j], yd = D[2 * j + 1];
                const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
                sum += exp(-((dx * dx + dy * dy) / var[j] / scale / 2.0));
            }
        }
        oks[q.pair0 + p] = sum / (double)(k1 > 0 ? k1 : J);
    }
}

struct MatchTables {
    double thr[kMaxThresholds], lo[kAreaRanges], hi[kAreaRanges];
    int T;
};

// One wave per (group, area range): detections in score order, one after the other; for each of the T thresholds the
// arg-max over the still unmatched ground truths across the lanes.  Key: (not ignored, IoU, index), so a non-ignored
// candidate beats every ignored one, the larger IoU wins, and a tie goes to the later ground truth.
// gt_flags (may be null): a flagged ground truth is ignored in every area range.
// lds: per ground truth, bit t = matched at threshold t, bit 31 = ignored in this range.
__global__ __launch_bounds__(64) void eval_match_kernel(const double* __restrict__ iou, const int* __restrict__ groups,
                                                        int ND, int NGT, long long num_pairs,
                                                        const double* __restrict__ det_area,
                                                        const double* __restrict__ gt_area,
                                                        const unsigned char* __restrict__ gt_flags, MatchTables mt,
                                                        unsigned* __restrict__ det_bits,
                                                        unsigned char* __restrict__ gt_ignore) {
    extern __shared__ unsigned gstate[];
    Group q;
    if (!load_group(groups, blockIdx.x, ND, NGT, num_pairs, q)) return;
    const int lane = threadIdx.x, a = blockIdx.y;
    const double lo = mt.lo[a], hi = mt.hi[a];
    for (int j = lane; j < q.ng; j += 64) {
        const double ar = gt_area[q.gt0 + j];
        const unsigned ig = (ar < lo || ar > hi || (gt_flags && gt_flags[q.gt0 + j])) ? 1u : 0u;
        gstate[j] = ig << 31;
        gt_ignore[(size_t)(q.gt0 + j) * kAreaRanges + a] = (unsigned char)ig;
    }
    __syncthreads();
    const unsigned all_t = mt.T >= 32 ? 0xffffffffu : ((1u << mt.T) - 1u);
    for (int d = 0; d < q.nd; ++d) {
        const double* row = iou + q.pair0 + (size_t)d * q.ng;
        unsigned matched = 0, ignored = 0;
        for (int t = 0; t < mt.T; ++t) {
            const double thr = fmin(mt.thr[t], 1.0 - 1e-10);
            int cls = -1, best = -1;
            double v = 0.0;
            for (int j = lane; j < q.ng; j += 64) {
                const unsigned s = gstate[j];
                if ((s >> t) & 1u) continue;
                const double o = row[j];
                if (o < thr) continue;
                const int c = (s >> 31) ? 0 : 1;
                if (c > cls || (c == cls && o >= v)) cls = c, v = o, best = j;      // j ascends: >= keeps the later one
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int c2 = __shfl_xor(cls, off, 64), b2 = __shfl_xor(best, off, 64);
                const double v2 = __shfl_xor(v, off, 64);
                if (c2 > cls || (c2 == cls && (v2 > v || (v2 == v && b2 > best)))) cls = c2, v = v2, best = b2;
            }
            if (best >= 0) {
                matched |= 1u << t;
                if (cls == 0) ignored |= 1u << t;
                if (lane == 0) gstate[best] |= 1u << t;
            }
            __syncthreads();
        }
        const double ad = det_area[q.det0 + d];
        if (ad < lo || ad > hi) ignored |= ~matched & all_t;
        if (lane == 0) det_bits[(size_t)(q.det0 + d) * kAreaRanges + a] = matched | (ignored << 16);
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;
using namespace cnuda::evalcoco;

extern "C" size_t cnuda_eval_workspace_bytes(int num_boxes, int H) { return spans_workspace_bytes(num_boxes, H); }

extern "C" int cnuda_eval_box_spans(const int* verts, int num_boxes, int H, int W, int* rows, double* area,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "cnuda_eval_box_spans";
    CNUDA_REQUIRE(num_boxes >= 0, "%s: negative box count", who);
    const char* bad = image_error(H, W);
    CNUDA_REQUIRE(!bad, "%s: %s (H %d, W %d)", who, bad, H, W);
    if (num_boxes == 0) return 0;
    CNUDA_REQUIRE(verts && rows && area && workspace, "%s: null pointer", who);
    CNUDA_REQUIRE(workspace_bytes >= spans_workspace_bytes(num_boxes, H), "%s: workspace of %zu bytes, need %zu", who,
                  workspace_bytes, spans_workspace_bytes(num_boxes, H));
    CNUDA_LAUNCH(eval_box_spans_kernel, dim3((unsigned)num_boxes), dim3(kSpanThreads), sizeof(int) * 2 * H,
                 (hipStream_t)stream, verts, H, W, (int2*)workspace, rows, area);
    return check_launch(who);
}

extern "C" int cnuda_eval_iou_rotated(const int* groups, int num_groups, int num_det, int num_gt, long long num_pairs,
                                      const int* rows, const double* area, int H, double* iou, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const char* who = "cnuda_eval_iou_rotated";
    const char* bad = groups_error(num_groups, num_det, num_gt, num_pairs);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    bad = image_error(H, 1);
    CNUDA_REQUIRE(!bad, "%s: %s (H %d)", who, bad, H);
    CNUDA_REQUIRE((long long)num_det + num_gt < (1ll << 31), "%s: too many boxes", who);
    if (num_groups == 0 || num_pairs == 0) return 0;
    CNUDA_REQUIRE(groups && rows && area && iou && workspace, "%s: null pointer", who);
    CNUDA_REQUIRE(workspace_bytes >= spans_workspace_bytes(num_det + num_gt, H),
                  "%s: workspace of %zu bytes does not hold the spans of %d boxes", who, workspace_bytes, num_det + num_gt);
    CNUDA_LAUNCH(eval_iou_rotated_kernel, dim3((unsigned)num_groups, kPairChunks), dim3(256), 0, (hipStream_t)stream,
                 groups, num_det, num_gt, num_pairs, (const int2*)workspace, rows, area, H, iou);
    return check_launch(who);
}

extern "C" int cnuda_eval_iou_axis(const float* det_boxes, const float* gt_boxes, const int* groups, int num_groups,
                                   int num_det, int num_gt, long long num_pairs, double* iou, void* stream) {
    const char* who = "cnuda_eval_iou_axis";
    const char* bad = groups_error(num_groups, num_det, num_gt, num_pairs);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    if (num_groups == 0 || num_pairs == 0) return 0;
    CNUDA_REQUIRE(det_boxes && gt_boxes && groups && iou, "%s: null pointer", who);
    CNUDA_LAUNCH(eval_iou_axis_kernel, dim3((unsigned)num_groups, kPairChunks), dim3(256), 0, (hipStream_t)stream, groups,
                 num_det, num_gt, num_pairs, det_boxes, gt_boxes, iou);
    return check_launch(who);
}

extern "C" int cnuda_eval_iou_quads(const float* quads, const int* groups, int num_groups, int num_det, int num_gt,
                                    long long num_pairs, double* iou, double* area, void* stream) {
    const char* who = "cnuda_eval_iou_quads";
    const char* bad = groups_error(num_groups, num_det, num_gt, num_pairs);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    const long long boxes = (long long)num_det + num_gt;
    CNUDA_REQUIRE(boxes < (1ll << 31), "%s: too many boxes", who);
    if (boxes == 0) return 0;
    const bool any_pair = num_groups > 0 && num_pairs > 0;
    CNUDA_REQUIRE(quads && area && (!any_pair || (groups && iou)), "%s: null pointer", who);
    const int groups_run = any_pair ? num_groups : 0;
    const unsigned area_columns = (unsigned)((boxes + 256ll * kPairChunks - 1) / (256ll * kPairChunks));
    CNUDA_LAUNCH(eval_iou_quads_kernel, dim3((unsigned)groups_run + area_columns, kPairChunks), dim3(256), 0,
                 (hipStream_t)stream, groups, groups_run, num_det, num_gt, num_pairs, quads, iou, area);
    return check_launch(who);
}

static int eval_match(const char* who, const double* iou, const int* groups, int num_groups, const double* det_area,
                      const double* gt_area, const unsigned char* gt_flags, bool flagged, int num_det, int num_gt,
                      long long num_pairs, const double* thresholds, int num_thresholds, const double* area_ranges,
                      unsigned* det_bits, unsigned char* gt_ignore, void* stream) {
    const char* bad = groups_error(num_groups, num_det, num_gt, num_pairs);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    bad = match_error(thresholds, num_thresholds, area_ranges);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    CNUDA_REQUIRE(num_gt <= 8192 * 2, "%s: more than 16384 ground truths in one call", who);
    if (num_groups == 0) return 0;
    CNUDA_REQUIRE(groups && (det_area || num_det == 0) && (gt_area || num_gt == 0) && (iou || num_pairs == 0) &&
                      (det_bits || num_det == 0) && (gt_ignore || num_gt == 0) && (gt_flags || !flagged || num_gt == 0),
                  "%s: null pointer", who);
    MatchTables mt;
    mt.T = num_thresholds;
    for (int t = 0; t < kMaxThresholds; ++t) mt.thr[t] = t < num_thresholds ? thresholds[t] : 2.0;
    for (int a = 0; a < kAreaRanges; ++a) mt.lo[a] = area_ranges[2 * a], mt.hi[a] = area_ranges[2 * a + 1];
    // a group's ground truths never outnumber num_gt: the kernel skips a group that says otherwise
    CNUDA_LAUNCH(eval_match_kernel, dim3((unsigned)num_groups, kAreaRanges), dim3(kWave), sizeof(unsigned) * num_gt,
                 (hipStream_t)stream, iou, groups, num_det, num_gt, num_pairs, det_area, gt_area, gt_flags, mt, det_bits,
                 gt_ignore);
    return check_launch(who);
}

extern "C" int cnuda_eval_match(const double* iou, const int* groups, int num_groups, const double* det_area,
                                const double* gt_area, int num_det, int num_gt, long long num_pairs,
                                const double* thresholds, int num_thresholds, const double* area_ranges,
                                unsigned* det_bits, unsigned char* gt_ignore, void* stream) {
    return eval_match("cnuda_eval_match", iou, groups, num_groups, det_area, gt_area, nullptr, false, num_det, num_gt,
                      num_pairs, thresholds, num_thresholds, area_ranges, det_bits, gt_ignore, stream);
}

extern "C" int cnuda_eval_match_flagged(const double* iou, const int* groups, int num_groups, const double* det_area,
                                        const double* gt_area, const unsigned char* gt_flags, int num_det, int num_gt,
                                        long long num_pairs, const double* thresholds, int num_thresholds,
                                        const double* area_ranges, unsigned* det_bits, unsigned char* gt_ignore,
                                        void* stream) {
    return eval_match("cnuda_eval_match_flagged", iou, groups, num_groups, det_area, gt_area, gt_flags, true, num_det,
                      num_gt, num_pairs, thresholds, num_thresholds, area_ranges, det_bits, gt_ignore, stream);
}

extern "C" int cnuda_eval_oks(const float* det_kps, const float* gt_kps, const unsigned char* gt_vis, const double* gt_area,
                              const float* gt_box, const double* sigmas, int num_joints, const int* groups, int num_groups,
                              int num_det, int num_gt, long long num_pairs, double* oks, double* det_area,
                              unsigned char* gt_flags, void* stream) {
    const char* who = "cnuda_eval_oks";
    const char* bad = groups_error(num_groups, num_det, num_gt, num_pairs);
    CNUDA_REQUIRE(!bad, "%s: %s", who, bad);
    CNUDA_REQUIRE(num_joints >= 1 && num_joints <= kMaxJoints, "%s: J = %d joints, between 1 and %d are supported", who,
                  num_joints, kMaxJoints);
    if (num_det == 0 && num_gt == 0) return 0;
    CNUDA_REQUIRE((det_kps && det_area) || num_det == 0, "%s: null pointer (detections)", who);
    CNUDA_REQUIRE((gt_vis && gt_flags) || num_gt == 0, "%s: null pointer (ground truths)", who);
    const bool any_pair = num_groups > 0 && num_pairs > 0;
    CNUDA_REQUIRE(!any_pair || (groups && gt_kps && gt_area && gt_box && sigmas && oks), "%s: null pointer (pairs)", who);
    CNUDA_LAUNCH(eval_kps_prepare_kernel, dim3((unsigned)(((long long)num_det + num_gt + 255) / 256)), dim3(256), 0,
                 (hipStream_t)stream, det_kps, gt_vis, num_det, num_gt, num_joints, det_area, gt_flags);
    int rc = check_launch(who);
    if (rc != 0 || !any_pair) return rc;
    CNUDA_LAUNCH(eval_oks_kernel, dim3((unsigned)num_groups, kPairChunks), dim3(256), 0, (hipStream_t)stream, groups,
                 num_det, num_gt, num_pairs, det_kps, gt_kps, gt_vis, gt_area, gt_box, sigmas, num_joints, oks);
    return check_launch(who);
}
