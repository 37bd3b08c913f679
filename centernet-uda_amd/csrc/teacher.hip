// Mean teacher (uda/mean_teacher.py): the two device steps between a student network and the pseudo-labelled batch its
// exponential-moving-average copy produces.
//
//   EMA update      cnuda_ema_update walks a device-resident table of (dst, src, count, kind) segments in ONE launch:
//                   the teacher's flat parameter buffer against the student's arena, every BatchNorm running statistic,
//                   every integer buffer -- instead of one small launch per tensor.
//   pseudo-labels   cnuda_pseudo_labels filters the teacher's decoded detection table (class, per-class score
//                   threshold, finite geometry, minimum extent), compacts the survivors to the front in their input
//                   order, optionally mirrors the geometry, and leaves what datasets.targets.encode_targets takes.
//                   cnuda_pseudo_labels_kps (uda.KeypointTeacher) is the same body with the rows' decoded joints in tow.
//
// Both are element-wise or tiny.  The EMA is two rounded float32 products and one rounded sum (spelled with the
// never-contracted intrinsics, on top of the build's -ffp-contract=off); the filter's order is decided by wave ballots
// and prefix counts alone.  No atomics anywhere: every result is independent of scheduling.
#include "common.h"

#include <math.h>

namespace cnuda {
namespace {

// One table entry (32 bytes; hip_runtime.ops.EmaPlan builds the table with the same layout).
struct EmaSegment {
    void* dst;
    const void* src;
    long long count;          // kind 0: float32 elements; kind 1: bytes
    int kind;                 // 0: dst = dst * d + src * omd;  1: dst = src, byte for byte
    unsigned block0;          // first workgroup of this segment; it owns ceil(count / kEmaPerBlock) of them
};
static_assert(sizeof(EmaSegment) == 32, "EmaPlan's table layout");

constexpr int kEmaThreads = 256;
constexpr int kEmaPerBlock = 4096;        // elements (kind 0) or bytes (kind 1) per workgroup: 16 per thread

__device__ __forceinline__ float ema(float t, float s, float d, float omd) {
    return __fadd_rn(__fmul_rn(t, d), __fmul_rn(s, omd));
}

__global__ __launch_bounds__(kEmaThreads) void ema_update_kernel(const EmaSegment* __restrict__ table, int nseg, float d,
                                                                 float omd) {
    // the segment whose workgroup range holds blockIdx.x: the last one with block0 <= blockIdx.x (segments of no
    // workgroups share their successor's block0 and are never the last)
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const EmaSegment seg = table[lo];
    const long long n = seg.count;
    const long long base = (long long)(blockIdx.x - seg.block0) * kEmaPerBlock;
    const int tid = threadIdx.x;
    const uintptr_t da = (uintptr_t)seg.dst, sa = (uintptr_t)seg.src;
    if (seg.kind == 0) {
        float* __restrict__ t = static_cast<float*>(seg.dst);
        const float* __restrict__ s = static_cast<const float*>(seg.src);
        if (((da ^ sa) & 15) == 0) {
            // the two pointers are 16-byte aligned at the same elements: a scalar head up to the first of them (this
            // segment's first workgroup), 16-byte accesses from there, a scalar tail
            long long head = (long long)(((16 - (da & 15)) & 15) >> 2);
            if (head > n) head = n;
            if (base == 0 && tid < head) t[tid] = ema(t[tid], s[tid], d, omd);
#pragma unroll
            for (int v = 0; v < kEmaPerBlock / (4 * kEmaThreads); ++v) {
                const long long i = head + base + 4LL * (v * kEmaThreads + tid);
                if (i + 3 < n) {
                    float4 a = *reinterpret_cast<const float4*>(t + i);
                    const float4 b = *reinterpret_cast<const float4*>(s + i);
                    a.x = ema(a.x, b.x, d, omd);
                    a.y = ema(a.y, b.y, d, omd);
                    a.z = ema(a.z, b.z, d, omd);
                    a.w = ema(a.w, b.w, d, omd);
                    *reinterpret_cast<float4*>(t + i) = a;
                } else {
                    for (long long j = i; j < n; ++j) t[j] = ema(t[j], s[j], d, omd);
                }
            }
        } else {
#pragma unroll
            for (int v = 0; v < kEmaPerBlock / kEmaThreads; ++v) {
                const long long i = base + v * kEmaThreads + tid;
                if (i < n) t[i] = ema(t[i], s[i], d, omd);
            }
        }
    } else {
        unsigned char* __restrict__ t = static_cast<unsigned char*>(seg.dst);
        const unsigned char* __restrict__ s = static_cast<const unsigned char*>(seg.src);
        if (((da | sa) & 15) == 0) {
            const long long i = base + 16LL * tid;
            if (i + 15 < n) {
                *reinterpret_cast<uint4*>(t + i) = *reinterpret_cast<const uint4*>(s + i);
            } else {
                for (long long j = i; j < n; ++j) t[j] = s[j];
            }
        } else {
#pragma unroll
            for (int v = 0; v < kEmaPerBlock / kEmaThreads; ++v) {
                const long long i = base + v * kEmaThreads + tid;
                if (i < n) t[i] = s[i];
            }
        }
    }
}

// One wave per image (images strided over the workgroup's waves): rows in chunks of 64, a ballot of the survivors, each
// survivor's place from the count of survivors below its lane -- the input order, whatever the scheduling.
constexpr int kPseudoMaxThreads = 1024;

// What the keypoint form (cnuda_pseudo_labels_kps) carries beside the boxes; the box form passes an empty record.
struct PseudoJoints {
    const float* kps;         // [B, K, J, 2]
    const int* perm;          // [J] or null
    double* keypoints;        // [B, K, J, 2]
    int* visibility;          // [B, K, J]
    float* joints;
    int J, map_height;
};

// kKps: the joints of a chunk's survivors follow their rows.  The chunk's 64 row -> slot entries (-1: dropped) go to this
// wave's part of LDS, then the whole wave walks the chunk's (row, joint) pairs in memory order -- lane t takes pair t,
// t + 64, ... -- so that a row's 2 J values never sit in a lane's registers and loads and stores are contiguous.
template <bool kKps>
__device__ __forceinline__ void pseudo_labels_body(
    const float* __restrict__ dets, const float* __restrict__ thresholds, double* __restrict__ geometry,
    int* __restrict__ classes, int* __restrict__ counts, float* __restrict__ kept, int B, int K, int C, int rotated,
    int mirror, int map_width, float min_size, PseudoJoints jt) {
    __shared__ int red[16];
    long long visible = 0;                            // this lane's joints with v = 2 (kKps)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ncol = rotated ? 7 : 6, gcol = rotated ? 8 : 4;
    const double Wd = (double)map_width, smin = (double)min_size;
    int total = 0;                                    // survivors of this wave's images (equal in all its lanes)
    for (int b = wid; b < B; b += nw) {
        int base = 0;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int k = k0 + lane;
            bool keep = false;
            int cls = 0;
            double g[8];
            if (k < K) {
                const float* d = dets + ((size_t)b * K + k) * ncol;
                const float cf = d[ncol - 1], score = d[ncol - 2];
                keep = cf >= 0.0f && cf < (float)C && cf == floorf(cf);
                if (keep) {
                    cls = (int)cf;
                    keep = score >= thresholds[cls];
                }
                const float a0 = d[0], a1 = d[1], a2 = d[2], a3 = d[3];
                keep = keep && isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(a3);
                if (rotated) {
                    const float ang = d[4];
                    keep = keep && isfinite(ang) && (double)a2 >= smin && (double)a3 >= smin;
                    if (keep) {
                        const double rad = (double)ang * (M_PI / 180.0);
                        const double c = cos(rad), s = sin(rad);
                        const double hw = (double)a2 / 2.0, hh = (double)a3 / 2.0;
                        const double ox[4] = {-hw, hw, hw, -hw}, oy[4] = {-hh, -hh, hh, hh};
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const double px = (double)a0 + (ox[v] * c + oy[v] * (-s));
                            g[2 * v] = mirror ? Wd - px : px;
                            g[2 * v + 1] = (double)a1 + (ox[v] * s + oy[v] * c);
                        }
                    }
                } else {
                    const double x1 = (double)a0, y1 = (double)a1, x2 = (double)a2, y2 = (double)a3;
                    keep = keep && (x2 - x1) >= smin && (y2 - y1) >= smin;
                    g[0] = mirror ? Wd - x2 : x1;
                    g[1] = y1;
                    g[2] = mirror ? Wd - x1 : x2;
                    g[3] = y2;
                }
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                const size_t row = (size_t)b * K + at;
                classes[row] = cls;
                double* o = geometry + row * gcol;
                for (int q = 0; q < gcol; ++q) o[q] = g[q];
            }
            if constexpr (kKps) {
                __shared__ int slots[kPseudoMaxThreads];
                int* slot = slots + 64 * wid;
                slot[lane] = keep ? base + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
                wave_lds_sync();
                const int J = jt.J, n = min(64, K - k0);
                const double Hd = (double)jt.map_height;
                // pair t = r J + j without a division per step: (r, j) advances by 64 = qstep J + jstep
                const int qstep = 64 / J, jstep = 64 % J;
                for (int r = lane / J, j = lane % J; r < n;) {
                    const int at = slot[r];
                    if (at >= 0) {
                        const int p = jt.perm ? jt.perm[j] : j;
                        float fx = NAN, fy = NAN;             // (an entry of perm outside [0, J) reads nothing)
                        if ((unsigned)p < (unsigned)J) {
                            const float* src = jt.kps + (((size_t)b * K + (k0 + r)) * J + p) * 2;
                            fx = src[0], fy = src[1];
                        }
                        double x = 0.0, y = 0.0;
                        int v = 0;
                        if (isfinite(fx) && isfinite(fy)) {
                            x = mirror ? Wd - (double)fx : (double)fx, y = (double)fy;
                            v = (x >= 0.0 && x < Wd && y >= 0.0 && y < Hd) ? 2 : 0;
                        }
                        const size_t o = ((size_t)b * K + at) * J + j;
                        jt.keypoints[2 * o] = x, jt.keypoints[2 * o + 1] = y;
                        jt.visibility[o] = v;
                        visible += v == 2;
                    }
                    r += qstep, j += jstep;
                    if (j >= J) j -= J, ++r;
                }
                wave_lds_sync();                              // the next chunk rewrites the slots
            }
            base += __popcll(mask);
        }
        // (rows below `base` were each written by exactly one survivor; the rest of every output is zero)
        for (int k = base + lane; k < K; k += 64) {
            const size_t row = (size_t)b * K + k;
            classes[row] = 0;
            double* o = geometry + row * gcol;
            for (int q = 0; q < gcol; ++q) o[q] = 0.0;
        }
        if constexpr (kKps) {
            const size_t end = ((size_t)b * K + K) * jt.J;
            for (size_t o = ((size_t)b * K + base) * jt.J + lane; o < end; o += 64) {
                jt.keypoints[2 * o] = 0.0, jt.keypoints[2 * o + 1] = 0.0;
                jt.visibility[o] = 0;
            }
        }
        if (lane == 0) counts[b] = base;
        total += base;
    }
    total = block_sum(lane == 0 ? total : 0, red);
    if (threadIdx.x == 0) *kept = (float)((double)total / (double)B);
    if constexpr (kKps) {
        __shared__ long long red_joints[16];
        visible = block_sum(visible, red_joints);
        if (threadIdx.x == 0) *jt.joints = (float)((double)visible / (double)B);
    }
}

__global__ __launch_bounds__(kPseudoMaxThreads) void pseudo_labels_kernel(
    const float* __restrict__ dets, const float* __restrict__ thresholds, double* __restrict__ geometry,
    int* __restrict__ classes, int* __restrict__ counts, float* __restrict__ kept, int B, int K, int C, int rotated,
    int mirror, int map_width, float min_size) {
    pseudo_labels_body<false>(dets, thresholds, geometry, classes, counts, kept, B, K, C, rotated, mirror, map_width,
                              min_size, PseudoJoints{});
}

__global__ __launch_bounds__(kPseudoMaxThreads) void pseudo_labels_kps_kernel(
    const float* __restrict__ dets, const float* __restrict__ thresholds, double* __restrict__ geometry,
    int* __restrict__ classes, int* __restrict__ counts, float* __restrict__ kept, int B, int K, int C, int rotated,
    int mirror, int map_width, float min_size, PseudoJoints jt) {
    pseudo_labels_body<true>(dets, thresholds, geometry, classes, counts, kept, B, K, C, rotated, mirror, map_width,
                             min_size, jt);
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_ema_update(const void* table, int segments, unsigned blocks, float decay, float one_minus_decay,
                                cnuda_stream_t stream) {
    CNUDA_REQUIRE(segments >= 0, "cnuda_ema_update: segments=%d", segments);
    if (segments == 0 || blocks == 0) return 0;
    CNUDA_REQUIRE(table, "cnuda_ema_update: null table");
    CNUDA_REQUIRE(((uintptr_t)table & 7) == 0, "cnuda_ema_update: the table must be 8-byte aligned");
    CNUDA_REQUIRE(decay >= 0.0f && decay < 1.0f, "cnuda_ema_update: decay=%g outside [0, 1)", (double)decay);
    CNUDA_REQUIRE(one_minus_decay == 1.0f - decay, "cnuda_ema_update: one_minus_decay=%g is not float32(1) - decay",
                  (double)one_minus_decay);
    CNUDA_LAUNCH(ema_update_kernel, dim3(blocks), dim3(kEmaThreads), 0, (hipStream_t)stream,
                 static_cast<const EmaSegment*>(table), segments, decay, one_minus_decay);
    return check_launch("cnuda_ema_update");
}

extern "C" int cnuda_pseudo_labels(const float* dets, const float* thresholds, double* geometry, int* classes, int* counts,
                                   float* kept, int B, int K, int C, int rotated, int mirror, int map_width,
                                   float min_size, cnuda_stream_t stream) {
    CNUDA_REQUIRE(dets && thresholds && geometry && classes && counts && kept, "cnuda_pseudo_labels: null pointer");
    CNUDA_REQUIRE(B > 0 && K > 0 && C > 0, "cnuda_pseudo_labels: bad sizes (B=%d, K=%d, C=%d)", B, K, C);
    CNUDA_REQUIRE(map_width > 0, "cnuda_pseudo_labels: map_width=%d", map_width);
    CNUDA_REQUIRE(min_size == min_size, "cnuda_pseudo_labels: min_size is NaN");
    const int waves = B < kPseudoMaxThreads / 64 ? B : kPseudoMaxThreads / 64;
    CNUDA_LAUNCH(pseudo_labels_kernel, dim3(1), dim3(64 * waves), 0, (hipStream_t)stream, dets, thresholds, geometry,
                 classes, counts, kept, B, K, C, rotated ? 1 : 0, mirror ? 1 : 0, map_width, min_size);
    return check_launch("cnuda_pseudo_labels");
}

extern "C" int cnuda_pseudo_labels_kps(const float* dets, const float* kps, const float* thresholds, const int* perm,
                                       double* geometry, int* classes, int* counts, float* kept, double* keypoints,
                                       int* visibility, float* joints, int B, int K, int C, int J, int rotated, int mirror,
                                       int map_height, int map_width, float min_size, cnuda_stream_t stream) {
    CNUDA_REQUIRE(dets && kps && thresholds && geometry && classes && counts && kept && keypoints && visibility && joints,
                  "cnuda_pseudo_labels_kps: null pointer");
    CNUDA_REQUIRE(B > 0 && K > 0 && C > 0 && J > 0, "cnuda_pseudo_labels_kps: bad sizes (B=%d, K=%d, C=%d, J=%d)", B, K,
                  C, J);
    CNUDA_REQUIRE(map_height > 0 && map_width > 0, "cnuda_pseudo_labels_kps: bad map (map_height=%d, map_width=%d)",
                  map_height, map_width);
    CNUDA_REQUIRE(min_size == min_size, "cnuda_pseudo_labels_kps: min_size is NaN");
    CNUDA_REQUIRE(((uintptr_t)keypoints & 7) == 0
                      && (((uintptr_t)kps | (uintptr_t)perm | (uintptr_t)visibility | (uintptr_t)joints) & 3) == 0,
                  "cnuda_pseudo_labels_kps: arrays must be aligned to their element size");
    const int waves = B < kPseudoMaxThreads / 64 ? B : kPseudoMaxThreads / 64;
    const PseudoJoints jt{kps, perm, keypoints, visibility, joints, J, map_height};
    CNUDA_LAUNCH(pseudo_labels_kps_kernel, dim3(1), dim3(64 * waves), 0, (hipStream_t)stream, dets, thresholds, geometry,
                 classes, counts, kept, B, K, C, rotated ? 1 : 0, mirror ? 1 : 0, map_width, min_size, jt);
    return check_launch("cnuda_pseudo_labels_kps");
}
