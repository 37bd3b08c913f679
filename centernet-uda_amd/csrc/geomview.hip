// The student's geometric view for self-training (uda/mean_teacher.py, GeometricTeacher; datasets/geometric_view.py;
// DESIGN.md, "Geometric view"): a similarity transform -- rotation, isotropic scale, shift, mirror -- of a normalised
// float32 batch as it sits on the device, and of the teacher's pseudo-labels at output-map resolution.
//
//   warp_bilinear_kernel      one 64 x 16 tile of one image per workgroup, four consecutive pixels of one row per thread.
//                             The image comes from the block index: the six matrix entries are wave-uniform.  The source
//                             position and the two weights of a pixel are computed once, in float64, and serve every
//                             channel; the four taps are gathered through L2 (no LDS: at a rotation the source rows of a
//                             wave form a slanted line, and neighbouring tiles share them there).  An image whose matrix is
//                             exactly the identity is copied.
//   labels_transform_kernel   one workgroup (one wave) per image: every row's corners mapped in float64, the visible
//                             fraction from the exact convex clip of polyiou.cuh against the map's rectangle, survivors
//                             compacted in input order by a ballot and a prefix count;
//   labels_totals_kernel      the two means over the batch (`kept`, `dropped`) from the integer counts.
//   labels_transform_kps_kernel, labels_totals_kps_kernel
//                             the same two with the rows' joints in tow (uda.KeypointTeacher; DESIGN.md, "Keypoint
//                             teacher"): mapped by the same matrix, visible while inside the map, and counted.
//
// No atomics: every result is the same from run to run.  The float32 arithmetic of the warp is one IEEE operation per step
// in the order of include/centernet_uda_hip.h (-ffp-contract=off): numpy's float32 bit for bit (tests/
// geometric_view_oracle.py).
#include "common.h"
#include "polyiou.cuh"

namespace cnuda {
namespace {

constexpr int kGvThreads = 256;
constexpr int kGvPer = 4;                                        // pixels per thread
constexpr int kGvTW = 64, kGvTH = 16;                            // the output tile: 16 threads x 16 rows

struct Tap {                                                     // one output pixel's four taps
    int at[4];                                                   // offsets into a plane: (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1)
    bool in[4];
    float fx, fy;
};

// x, y [B, C, H, W]; inverse [B, 6] float64 (row-major 2 x 3: output pixel centres -> source positions).
// blockIdx.x = (image, tile row, tile column).
__global__ __launch_bounds__(kGvThreads) void warp_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                   const double* __restrict__ inverse, float fill, int C,
                                                                   int H, int W, int tiles_x, int tiles_y) {
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const double* m = inverse + 6 * (size_t)b;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const int row = ty * kGvTH + (int)(threadIdx.x / (kGvTW / kGvPer));
    const int col = tx * kGvTW + kGvPer * (int)(threadIdx.x % (kGvTW / kGvPer));
    if (row >= H || col >= W) return;
    const long long HW = (long long)H * W;
    const float* xb = x + (long long)b * C * HW;
    float* yrow = y + (long long)b * C * HW + (long long)row * W + col;
    const int n = min(kGvPer, W - col);                           // pixels of this thread inside the row

    if (m0 == 1.0 && m1 == 0.0 && m2 == 0.0 && m3 == 0.0 && m4 == 1.0 && m5 == 0.0) {         // the image's own bits
        const float* xrow = xb + (long long)row * W + col;
        for (int c = 0; c < C; ++c) {
            const float* src = xrow + c * HW;
            float* dst = yrow + c * HW;
            if (n == kGvPer && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0) {
                *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
            } else {
                for (int j = 0; j < n; ++j) dst[j] = src[j];
            }
        }
        return;
    }

    Tap tap[kGvPer];
    const double dy = (double)row + 0.5;
#pragma unroll
    for (int j = 0; j < kGvPer; ++j) {
        const double dx = (double)(col + j) + 0.5;
        const double u = ((m0 * dx + m1 * dy) + m2) - 0.5, v = ((m3 * dx + m4 * dy) + m5) - 0.5;
        const double fu = floor(u), fv = floor(v);
        tap[j].fx = (float)(u - fu), tap[j].fy = (float)(v - fv);
        // (a position far outside, or one that is not a number, is outside: the clamp keeps the conversion defined)
        const int x0 = (int)fmin(fmax(fu, -2.0), (double)W), y0 = (int)fmin(fmax(fv, -2.0), (double)H);
        const bool cx0 = x0 >= 0 && x0 < W, cx1 = x0 + 1 >= 0 && x0 + 1 < W;
        const bool ry0 = y0 >= 0 && y0 < H, ry1 = y0 + 1 >= 0 && y0 + 1 < H;
        tap[j].in[0] = ry0 && cx0, tap[j].in[1] = ry0 && cx1, tap[j].in[2] = ry1 && cx0, tap[j].in[3] = ry1 && cx1;
        const int base = y0 * W + x0;                             // (read only where the tap is inside: |base| < 2^31)
        tap[j].at[0] = base, tap[j].at[1] = base + 1, tap[j].at[2] = base + W, tap[j].at[3] = base + W + 1;
    }
    for (int c = 0; c < C; ++c) {
        const float* plane = xb + c * HW;
        float out[kGvPer];
#pragma unroll
        for (int j = 0; j < kGvPer; ++j) {
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = (j < n && tap[j].in[q]) ? plane[tap[j].at[q]] : fill;
            const float top = t[0] + tap[j].fx * (t[1] - t[0]);
            const float bot = t[2] + tap[j].fx * (t[3] - t[2]);
            out[j] = top + tap[j].fy * (bot - top);
        }
        float* dst = yrow + c * HW;
        if (n == kGvPer && (((uintptr_t)dst) & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kGvPer; ++j)
                if (j < n) dst[j] = out[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// labels
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_finite(double v) { return v - v == 0.0; }

// geometry_in / geometry_out [B, K, gcol] float64 (gcol 8: four (x, y) corners; 4: x1, y1, x2, y2); forward [B, 6] float64.
// One wave per image: rows in chunks of 64, a ballot of the survivors, each survivor's place from the count of survivors
// below its lane -- the input order, whatever the scheduling.
//
// kKps (cnuda_labels_transform_kps): the joints of a chunk's survivors follow their rows.  The chunk's 64 row -> slot
// entries (-1: dropped) go to LDS, then the whole wave walks the chunk's (row, joint) pairs in memory order -- lane t takes
// pair t, t + 64, ... -- so that a row's 2 J values never sit in a lane's registers and loads and stores are contiguous.
struct ViewJoints {
    const double* keypoints_in;      // [B, K, J, 2]
    const int* visibility_in;        // [B, K, J]
    double* keypoints_out;
    int* visibility_out;
    int J;
};

template <bool kKps>
__device__ __forceinline__ void labels_transform_body(
    const double* __restrict__ geometry_in, const int* __restrict__ classes_in, const int* __restrict__ counts_in,
    const double* __restrict__ forward, double* __restrict__ geometry_out, int* __restrict__ classes_out,
    int* __restrict__ counts_out, int K, int rotated, double map_w, double map_h, double min_size, double min_visible,
    ViewJoints jt) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int gcol = rotated ? 8 : 4;
    const double* m = forward + 6 * (size_t)b;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const bool identity = m0 == 1.0 && m1 == 0.0 && m2 == 0.0 && m3 == 0.0 && m4 == 1.0 && m5 == 0.0;
    const int count = min(max(counts_in[b], 0), K);
    polyiou::Quad map;
    map.x[0] = 0.0, map.y[0] = 0.0, map.x[1] = map_w, map.y[1] = 0.0;
    map.x[2] = map_w, map.y[2] = map_h, map.x[3] = 0.0, map.y[3] = map_h;
    const double a2map = polyiou::orient(map);
    int base = 0;
    for (int k0 = 0; k0 < count; k0 += 64) {
        const int k = k0 + lane;
        bool keep = false;
        int cls = 0;
        double g[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = 0.0;
        if (k < count) {
            const size_t row = (size_t)b * K + k;
            const double* src = geometry_in + row * gcol;
            cls = classes_in[row];
            if (identity) {                                       // the identity view keeps every row as it is
                for (int q = 0; q < gcol; ++q) g[q] = src[q];
                keep = true;
            } else if (rotated) {
                polyiou::Quad quad;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double px = src[2 * v], py = src[2 * v + 1];
                    quad.x[v] = (m0 * px + m1 * py) + m2, quad.y[v] = (m3 * px + m4 * py) + m5;
                    g[2 * v] = quad.x[v], g[2 * v + 1] = quad.y[v];
                }
                const double ax = quad.x[1] - quad.x[0], ay = quad.y[1] - quad.y[0];
                const double bx = quad.x[2] - quad.x[1], by = quad.y[2] - quad.y[1];
                const double e0 = sqrt(ax * ax + ay * ay), e1 = sqrt(bx * bx + by * by);
                if (polyiou::finite(quad)) {
                    const double a2 = polyiou::orient(quad);
                    if (a2 > 0.0 && is_finite(a2) && e0 >= min_size && e1 >= min_size) {
                        const double visible = polyiou::clipped_doubled_area(quad, map, a2, a2map) / a2;
                        keep = visible >= min_visible;
                    }
                }
            } else {
                const double cx[4] = {src[0], src[2], src[2], src[0]}, cy[4] = {src[1], src[1], src[3], src[3]};
                double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
                bool fin = true;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double qx = (m0 * cx[v] + m1 * cy[v]) + m2, qy = (m3 * cx[v] + m4 * cy[v]) + m5;
                    fin = fin && is_finite(qx) && is_finite(qy);
                    x1 = v == 0 ? qx : fmin(x1, qx), x2 = v == 0 ? qx : fmax(x2, qx);
                    y1 = v == 0 ? qy : fmin(y1, qy), y2 = v == 0 ? qy : fmax(y2, qy);
                }
                g[0] = x1, g[1] = y1, g[2] = x2, g[3] = y2;
                const double w = x2 - x1, h = y2 - y1, area = w * h;
                if (fin && area > 0.0 && is_finite(area) && w >= min_size && h >= min_size) {
                    const double iw = fmax(fmin(x2, map_w) - fmax(x1, 0.0), 0.0);
                    const double ih = fmax(fmin(y2, map_h) - fmax(y1, 0.0), 0.0);
                    keep = (iw * ih) / area >= min_visible;
                }
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
            const size_t row = (size_t)b * K + at;
            classes_out[row] = cls;
            double* o = geometry_out + row * gcol;
            for (int q = 0; q < gcol; ++q) o[q] = g[q];
        }
        if constexpr (kKps) {
            __shared__ int slot[64];
            slot[lane] = keep ? base + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
            wave_lds_sync();
            const int J = jt.J, n = min(64, count - k0);
            // pair t = r J + j without a division per step: (r, j) advances by 64 = qstep J + jstep
            const int qstep = 64 / J, jstep = 64 % J;
            for (int r = lane / J, j = lane % J; r < n;) {
                const int at = slot[r];
                if (at >= 0) {
                    const size_t i = ((size_t)b * K + (k0 + r)) * J + j, o = ((size_t)b * K + at) * J + j;
                    double x = jt.keypoints_in[2 * i], y = jt.keypoints_in[2 * i + 1];
                    int v = jt.visibility_in[i];
                    if (!identity) {
                        const double qx = (m0 * x + m1 * y) + m2, qy = (m3 * x + m4 * y) + m5;
                        const bool fin = is_finite(qx) && is_finite(qy);
                        v = (v == 2 && fin && qx >= 0.0 && qx < map_w && qy >= 0.0 && qy < map_h) ? 2 : 0;
                        x = fin ? qx : 0.0, y = fin ? qy : 0.0;
                    }
                    jt.keypoints_out[2 * o] = x, jt.keypoints_out[2 * o + 1] = y;
                    jt.visibility_out[o] = v;
                }
                r += qstep, j += jstep;
                if (j >= J) j -= J, ++r;
            }
            wave_lds_sync();                                      // the next chunk rewrites the slots
        }
        base += __popcll(mask);
    }
    // (rows below `base` were each written by exactly one survivor; the rest of every output is zero)
    for (int k = base + lane; k < K; k += 64) {
        const size_t row = (size_t)b * K + k;
        classes_out[row] = 0;
        double* o = geometry_out + row * gcol;
        for (int q = 0; q < gcol; ++q) o[q] = 0.0;
    }
    if constexpr (kKps) {
        const size_t end = ((size_t)b * K + K) * jt.J;
        for (size_t o = ((size_t)b * K + base) * jt.J + lane; o < end; o += 64) {
            jt.keypoints_out[2 * o] = 0.0, jt.keypoints_out[2 * o + 1] = 0.0;
            jt.visibility_out[o] = 0;
        }
    }
    if (lane == 0) counts_out[b] = base;
}

__global__ __launch_bounds__(64) void labels_transform_kernel(
    const double* __restrict__ geometry_in, const int* __restrict__ classes_in, const int* __restrict__ counts_in,
    const double* __restrict__ forward, double* __restrict__ geometry_out, int* __restrict__ classes_out,
    int* __restrict__ counts_out, int K, int rotated, double map_w, double map_h, double min_size, double min_visible) {
    labels_transform_body<false>(geometry_in, classes_in, counts_in, forward, geometry_out, classes_out, counts_out, K,
                                 rotated, map_w, map_h, min_size, min_visible, ViewJoints{});
}

__global__ __launch_bounds__(64) void labels_transform_kps_kernel(
    const double* __restrict__ geometry_in, const int* __restrict__ classes_in, const int* __restrict__ counts_in,
    const double* __restrict__ forward, double* __restrict__ geometry_out, int* __restrict__ classes_out,
    int* __restrict__ counts_out, int K, int rotated, double map_w, double map_h, double min_size, double min_visible,
    ViewJoints jt) {
    labels_transform_body<true>(geometry_in, classes_in, counts_in, forward, geometry_out, classes_out, counts_out, K,
                                rotated, map_w, map_h, min_size, min_visible, jt);
}

// kept = float32(double(sum counts_out) / B); dropped = float32(double(sum min(max(counts_in, 0), K) - sum counts_out) / B)
__global__ __launch_bounds__(64) void labels_totals_kernel(const int* __restrict__ counts_in,
                                                           const int* __restrict__ counts_out, float* __restrict__ kept,
                                                           float* __restrict__ dropped, int B, int K) {
    long long before = 0, after = 0;
    for (int b = threadIdx.x; b < B; b += 64) {
        before += min(max(counts_in[b], 0), K);
        after += counts_out[b];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64), after += __shfl_xor(after, o, 64);
    if (threadIdx.x == 0) {
        *kept = (float)((double)after / (double)B);
        *dropped = (float)((double)(before - after) / (double)B);
    }
}

// labels_totals_kernel's two means, and joints = float32(double(number of v = 2 among the surviving rows) / B): one
// workgroup, the rows below each image's count read in memory order, integer sums.
constexpr int kJointsThreads = 256;

__global__ __launch_bounds__(kJointsThreads) void labels_totals_kps_kernel(
    const int* __restrict__ counts_in, const int* __restrict__ counts_out, const int* __restrict__ visibility_out,
    float* __restrict__ kept, float* __restrict__ dropped, float* __restrict__ joints, int B, int K, int J) {
    __shared__ long long red[16];
    long long before = 0, after = 0, visible = 0;
    for (int b = threadIdx.x; b < B; b += kJointsThreads) {
        before += min(max(counts_in[b], 0), K);
        after += counts_out[b];
    }
    for (int b = 0; b < B; ++b) {
        const int* v = visibility_out + (size_t)b * K * J;
        const size_t n = (size_t)counts_out[b] * J;
        for (size_t i = threadIdx.x; i < n; i += kJointsThreads) visible += v[i] == 2;
    }
    before = block_sum(before, red), after = block_sum(after, red), visible = block_sum(visible, red);
    if (threadIdx.x == 0) {
        *kept = (float)((double)after / (double)B);
        *dropped = (float)((double)(before - after) / (double)B);
        *joints = (float)((double)visible / (double)B);
    }
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_warp_bilinear(const float* x, float* y, const double* inverse, float fill, int B, int C, int H, int W,
                                   cnuda_stream_t stream) {
    CNUDA_REQUIRE(x && y && inverse, "cnuda_warp_bilinear: null pointer");
    CNUDA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "cnuda_warp_bilinear: bad sizes (B=%d, C=%d, H=%d, W=%d)", B, C, H, W);
    CNUDA_REQUIRE((long long)H * W + W + 1 < (1ll << 31), "cnuda_warp_bilinear: plane too large (H=%d, W=%d)", H, W);
    const long long total = (long long)B * C * H * W;
    CNUDA_REQUIRE(!(x < y + total && y < x + total), "cnuda_warp_bilinear: x and y overlap");
    CNUDA_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0 && ((uintptr_t)inverse & 7) == 0,
                  "cnuda_warp_bilinear: arrays must be aligned to their element size");
    const int tiles_x = ceil_div(W, kGvTW), tiles_y = ceil_div(H, kGvTH);
    const long long tiles = (long long)tiles_x * tiles_y * B;
    CNUDA_REQUIRE(tiles < (1ll << 31), "cnuda_warp_bilinear: batch too large (%lld tiles)", tiles);
    CNUDA_LAUNCH(warp_bilinear_kernel, dim3((unsigned)tiles), dim3(kGvThreads), 0, (hipStream_t)stream, x, y, inverse,
                 fill, C, H, W, tiles_x, tiles_y);
    return check_launch("cnuda_warp_bilinear");
}

extern "C" int cnuda_labels_transform(const double* geometry_in, const int* classes_in, const int* counts_in,
                                      const double* forward, double* geometry_out, int* classes_out, int* counts_out,
                                      float* kept, float* dropped, int B, int K, int rotated, int map_h, int map_w,
                                      double min_size, double min_visible, cnuda_stream_t stream) {
    CNUDA_REQUIRE(geometry_in && classes_in && counts_in && forward && geometry_out && classes_out && counts_out && kept
                      && dropped, "cnuda_labels_transform: null pointer");
    CNUDA_REQUIRE(B > 0 && K > 0, "cnuda_labels_transform: bad sizes (B=%d, K=%d)", B, K);
    CNUDA_REQUIRE(map_h > 0 && map_w > 0, "cnuda_labels_transform: bad map (map_h=%d, map_w=%d)", map_h, map_w);
    CNUDA_REQUIRE(min_size == min_size && min_visible == min_visible, "cnuda_labels_transform: a threshold is NaN");
    CNUDA_REQUIRE((((uintptr_t)geometry_in | (uintptr_t)geometry_out | (uintptr_t)forward) & 7) == 0
                      && (((uintptr_t)classes_in | (uintptr_t)classes_out | (uintptr_t)counts_in | (uintptr_t)counts_out
                           | (uintptr_t)kept | (uintptr_t)dropped) & 3) == 0,
                  "cnuda_labels_transform: arrays must be aligned to their element size");
    CNUDA_REQUIRE(geometry_in != geometry_out && classes_in != classes_out && counts_in != counts_out,
                  "cnuda_labels_transform: the outputs must not be the inputs");
    hipStream_t st = (hipStream_t)stream;
    CNUDA_LAUNCH(labels_transform_kernel, dim3((unsigned)B), dim3(64), 0, st, geometry_in, classes_in, counts_in, forward,
                 geometry_out, classes_out, counts_out, K, rotated ? 1 : 0, (double)map_w, (double)map_h, min_size,
                 min_visible);
    CNUDA_LAUNCH(labels_totals_kernel, dim3(1), dim3(64), 0, st, counts_in, counts_out, kept, dropped, B, K);
    return check_launch("cnuda_labels_transform");
}

extern "C" int cnuda_labels_transform_kps(const double* geometry_in, const int* classes_in, const int* counts_in,
                                          const double* keypoints_in, const int* visibility_in, const double* forward,
                                          double* geometry_out, int* classes_out, int* counts_out, double* keypoints_out,
                                          int* visibility_out, float* kept, float* dropped, float* joints, int B, int K,
                                          int J, int rotated, int map_h, int map_w, double min_size, double min_visible,
                                          cnuda_stream_t stream) {
    CNUDA_REQUIRE(geometry_in && classes_in && counts_in && keypoints_in && visibility_in && forward && geometry_out
                      && classes_out && counts_out && keypoints_out && visibility_out && kept && dropped && joints,
                  "cnuda_labels_transform_kps: null pointer");
    CNUDA_REQUIRE(B > 0 && K > 0 && J > 0, "cnuda_labels_transform_kps: bad sizes (B=%d, K=%d, J=%d)", B, K, J);
    CNUDA_REQUIRE(map_h > 0 && map_w > 0, "cnuda_labels_transform_kps: bad map (map_h=%d, map_w=%d)", map_h, map_w);
    CNUDA_REQUIRE(min_size == min_size && min_visible == min_visible, "cnuda_labels_transform_kps: a threshold is NaN");
    CNUDA_REQUIRE((((uintptr_t)geometry_in | (uintptr_t)geometry_out | (uintptr_t)forward | (uintptr_t)keypoints_in
                    | (uintptr_t)keypoints_out) & 7) == 0
                      && (((uintptr_t)classes_in | (uintptr_t)classes_out | (uintptr_t)counts_in | (uintptr_t)counts_out
                           | (uintptr_t)visibility_in | (uintptr_t)visibility_out | (uintptr_t)kept | (uintptr_t)dropped
                           | (uintptr_t)joints) & 3) == 0,
                  "cnuda_labels_transform_kps: arrays must be aligned to their element size");
    CNUDA_REQUIRE(geometry_in != geometry_out && classes_in != classes_out && counts_in != counts_out
                      && keypoints_in != keypoints_out && visibility_in != visibility_out,
                  "cnuda_labels_transform_kps: the outputs must not be the inputs");
    hipStream_t st = (hipStream_t)stream;
    const ViewJoints jt{keypoints_in, visibility_in, keypoints_out, visibility_out, J};
    CNUDA_LAUNCH(labels_transform_kps_kernel, dim3((unsigned)B), dim3(64), 0, st, geometry_in, classes_in, counts_in,
                 forward, geometry_out, classes_out, counts_out, K, rotated ? 1 : 0, (double)map_w, (double)map_h, min_size,
                 min_visible, jt);
    CNUDA_LAUNCH(labels_totals_kps_kernel, dim3(1), dim3(kJointsThreads), 0, st, counts_in, counts_out, visibility_out, kept,
                 dropped, joints, B, K, J);
    return check_launch("cnuda_labels_transform_kps");
}
