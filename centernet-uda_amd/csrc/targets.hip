// CenterNet target encoding on the GPU: the per-image loop of datasets/coco.py:191-221 and
// the gaussian splat of utils/image.py:8-57, for a whole batch in one launch.
//
// One workgroup per (image, object slot).  Box arithmetic in double exactly like the reference's numpy code
// (clip, ceil, gaussian_radius, centre -> float32 -> int truncation), so `ind`, `reg_mask` and the peak cells are
// identical; the splat is exp() in double, cast to float32 and merged with an integer atomicMax (non-negative
// floats order like their bit patterns), which makes overlapping objects order-independent like np.maximum.
//
// encode_targets_kernel<ROT> covers the whole batch schema: the plain boxes above and (coco.py:176-184,217-233 and
// 303-376) keypoint targets, the annotation's own `area`, and rotated boxes from four corner points.  The enclosing
// rectangle of the four points (the reference's cv2.minAreaRect) is defined geometrically: the least-area rectangle
// with a side along an edge of the convex hull, in double from the float32 points ("Target modes").
#include "common.h"

namespace cnuda {
namespace {

__device__ __forceinline__ double gaussian_radius(double height, double width) {
    const double min_overlap = 0.7;
    const double b1 = height + width;
    const double c1 = width * height * (1 - min_overlap) / (1 + min_overlap);
    const double r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2;
    const double b2 = 2 * (height + width);
    const double c2 = (1 - min_overlap) * width * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
    const double a3 = 4 * min_overlap;
    const double b3 = -2 * min_overlap * (height + width);
    const double c3 = (min_overlap - 1) * width * height;
    const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
    return fmin(r1, fmin(r2, r3));
}

// draw_umich_gaussian (utils/image.py:42-57) by the whole workgroup: window [cx-left, cx+right) x [cy-top, cy+bottom),
// sigma = diameter / 6
__device__ __forceinline__ void splat_gaussian(float* __restrict__ hm, int b, int cls, int cx, int cy, int radius,
                                               int C, int H, int W) {
    const int left = min(cx, radius), right = min(W - cx, radius + 1);
    const int top = min(cy, radius), bottom = min(H - cy, radius + 1);
    const int ww = left + right, hh = top + bottom;
    if (ww <= 0 || hh <= 0) return;
    const double sigma = (2 * radius + 1) / 6.0;
    const double eps_cut = 2.220446049250313e-16;           // np.finfo(float64).eps * h.max(), h.max() == 1
    int* plane = reinterpret_cast<int*>(hm + ((size_t)b * C + cls) * H * W);
    for (int i = threadIdx.x; i < ww * hh; i += blockDim.x) {
        const int yy = i / ww, xx = i - yy * ww;
        const double dx = (double)(xx - left), dy = (double)(yy - top);
        double gv = exp(-(dx * dx + dy * dy) / (2 * sigma * sigma));
        if (gv < eps_cut) gv = 0.0;
        const float f = (float)gv;
        if (f > 0.0f) atomicMax(plane + (size_t)(cy - top + yy) * W + (cx - left + xx), __float_as_int(f));
    }
}

// The enclosing rectangle with a side along the line through points I and J, if that line carries an edge of the
// convex hull (every point on one closed side of it) and the rectangle is smaller than the best so far.  Projections
// stay unnormalised (dot and cross with d = pJ - pI), so collinear points give a cross extent of exactly 0: the
// differences of float32 coordinates and their pairwise products are exact in double.
struct EdgeRect {
    double area, cx, cy, lu, lv, dx, dy;      // extents lu along d = (dx, dy), lv across it
    bool found;
};

template <int I, int J>
__device__ __forceinline__ void try_edge(const double (&x)[4], const double (&y)[4], EdgeRect& best) {
    const double dx = x[J] - x[I], dy = y[J] - y[I];
    const double l2 = dx * dx + dy * dy;
    if (!(l2 > 0)) return;                                  // coincident points have no direction
    double dmin = 0, dmax = 0, cmin = 0, cmax = 0;          // point I projects to (0, 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double qx = x[k] - x[I], qy = y[k] - y[I];
        const double d = qx * dx + qy * dy, c = dx * qy - dy * qx;
        dmin = fmin(dmin, d); dmax = fmax(dmax, d);
        cmin = fmin(cmin, c); cmax = fmax(cmax, c);
    }
    if (cmin < 0 && cmax > 0) return;                       // points on both sides: a diagonal, not a hull edge
    const double area = (dmax - dmin) * (cmax - cmin) / l2;
    if (best.found && !(area < best.area)) return;          // ties keep the first edge in the fixed order
    const double md = (dmax + dmin) / 2, mc = (cmax + cmin) / 2, l = sqrt(l2);
    best.found = true; best.area = area;
    best.cx = x[I] + (md * dx - mc * dy) / l2; best.cy = y[I] + (md * dy + mc * dx) / l2;
    best.lu = (dmax - dmin) / l; best.lv = (cmax - cmin) / l;
    best.dx = dx; best.dy = dy;
}

// One workgroup per (image, slot).  ROT: the object is four corner points
// (coco.py:329-358) instead of a box (coco.py:191-215).  kps / areas may be null (J == 0: no keypoints).
template <bool ROT>
__global__ __launch_bounds__(256) void encode_targets_kernel(
    const double* __restrict__ geom, const int* __restrict__ classes, const int* __restrict__ counts,
    const double* __restrict__ keypoints, const int* __restrict__ visibility, const float* __restrict__ areas,
    float* __restrict__ hm, unsigned char* __restrict__ reg_mask, long long* __restrict__ ind,
    float* __restrict__ wh, float* __restrict__ reg, float* __restrict__ gt_dets, float* __restrict__ gt_areas,
    float* __restrict__ kps, float* __restrict__ gt_kps, unsigned char* __restrict__ kp_reg_mask,
    int C, int H, int W, int M, int J) {
    const int b = blockIdx.y, k = blockIdx.x;
    if (k >= min(counts[b], M)) return;
    const size_t o = (size_t)b * M + k;
    const int cls = classes[o];
    if (cls < 0 || cls >= C) return;
    float ctx, cty, area;
    double rh, rw;                                          // what the radius is computed from
    float wh3[3], det4[4];
    if (ROT) {
        // clip, then points.astype(np.float32) (coco.py:333-337); the geometry in double from those
        double x[4], y[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            x[p] = (double)(float)fmin(fmax(geom[o * 8 + 2 * p], 0.0), (double)(W - 1));
            y[p] = (double)(float)fmin(fmax(geom[o * 8 + 2 * p + 1], 0.0), (double)(H - 1));
        }
        EdgeRect r;
        r.found = false; r.area = 0; r.cx = r.cy = r.lu = r.lv = r.dx = r.dy = 0;
        try_edge<0, 1>(x, y, r); try_edge<1, 2>(x, y, r); try_edge<2, 3>(x, y, r);
        try_edge<3, 0>(x, y, r); try_edge<0, 2>(x, y, r); try_edge<1, 3>(x, y, r);
        if (!r.found) return;                               // four coincident points
        const float fu = (float)r.lu, fv = (float)r.lv;
        if (fu == 0.0f || fv == 0.0f) return;               // the reference's `continue` (coco.py:340-341)
        // utils/box.py get_annotation_with_angle on the float32 values: w the short side, the angle its direction
        const bool along = fu <= fv;
        float w = along ? fu : fv, h = along ? fv : fu;
        const double sx = along ? r.dx : -r.dy, sy = along ? r.dy : r.dx;
        double deg = atan2(sy, sx) * (180.0 / 3.141592653589793);
        if (deg >= 90.0) deg -= 180.0;                      // a direction is a line: fold into [-90, 90)
        if (deg < -90.0) deg += 180.0;
        float angle = (float)deg;
        if (w == h) h += 1.0f;                              // "force that w < h"
        if (angle == 90.0f) angle = -90.0f;
        ctx = (float)r.cx; cty = (float)r.cy;
        wh3[0] = w; wh3[1] = h; wh3[2] = angle;
        det4[0] = ctx; det4[1] = cty; det4[2] = w; det4[3] = h;
        area = w * h;
        rh = ceil((double)h); rw = ceil((double)w);
    } else {
        const double* bx = geom + o * 4;
        const double x1 = fmin(fmax(bx[0], 0.0), (double)(W - 1)), x2 = fmin(fmax(bx[2], 0.0), (double)(W - 1));
        const double y1 = fmin(fmax(bx[1], 0.0), (double)(H - 1)), y2 = fmin(fmax(bx[3], 0.0), (double)(H - 1));
        const double h = y2 - y1, w = x2 - x1;
        if (!(h > 0 && w > 0)) return;
        ctx = (float)((x1 + x2) / 2); cty = (float)((y1 + y2) / 2);
        wh3[0] = (float)w; wh3[1] = (float)h; wh3[2] = 0.0f;
        // gt_det is assigned as a float64 tuple and cast to float32 (coco.py:219-220)
        det4[0] = (float)((double)ctx - w / 2); det4[1] = (float)((double)cty - h / 2);
        det4[2] = (float)((double)ctx + w / 2); det4[3] = (float)((double)cty + h / 2);
        area = (float)(w * h);
        rh = ceil(h); rw = ceil(w);
    }
    int radius = (int)gaussian_radius(rh, rw);              // int(): truncation (the radius is never negative)
    if (radius < 0) radius = 0;
    const int cx = (int)ctx, cy = (int)cty;
    if (threadIdx.x == 0) {
        constexpr int NW = ROT ? 3 : 2, ND = ROT ? 7 : 6;
#pragma unroll
        for (int i = 0; i < NW; ++i) wh[o * NW + i] = wh3[i];
        ind[o] = (long long)cy * W + cx;
        reg[o * 2] = ctx - (float)cx; reg[o * 2 + 1] = cty - (float)cy;
        reg_mask[o] = 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) gt_dets[o * ND + i] = det4[i];
        if (ROT) gt_dets[o * ND + 4] = wh3[2];
        gt_dets[o * ND + ND - 2] = 1.0f; gt_dets[o * ND + ND - 1] = (float)cls;
        if (areas) {                                        // NaN: the annotation has no "area" (coco.py:230-233)
            const float a = areas[o];
            if (a == a) area = a;
        }
        gt_areas[o] = area;
    }
    // keypoints of a valid object (coco.py:217-228): offsets from the integer centre, subtracted in double; the
    // reference tests y against the WIDTH too (is_out_of_image((output_w, output_w))), restated as it is
    for (int i = threadIdx.x; i < J; i += blockDim.x) {
        const double px = keypoints[(o * J + i) * 2], py = keypoints[(o * J + i) * 2 + 1];
        kps[o * 2 * J + 2 * i] = (float)(px - (double)cx);
        kps[o * 2 * J + 2 * i + 1] = (float)(py - (double)cy);
        gt_kps[(o * J + i) * 2] = (float)px; gt_kps[(o * J + i) * 2 + 1] = (float)py;
        const bool inside = px >= 0 && px < (double)W && py >= 0 && py < (double)W;
        const unsigned char m = (visibility[o * J + i] == 2 && inside) ? 1 : 0;
        kp_reg_mask[o * 2 * J + 2 * i] = m; kp_reg_mask[o * 2 * J + 2 * i + 1] = m;
    }
    splat_gaussian(hm, b, cls, cx, cy, radius, C, H, W);
}

}  // namespace
}  // namespace cnuda

using namespace cnuda;

extern "C" int cnuda_encode_targets(const double* boxes, const int* classes, const int* counts, float* hm,
                                    unsigned char* reg_mask, long long* ind, float* wh, float* reg, float* gt_dets,
                                    float* gt_areas, int B, int C, int H, int W, int M, cnuda_stream_t stream) {
    return cnuda_encode_targets_modes(boxes, nullptr, classes, counts, nullptr, nullptr, nullptr, hm, reg_mask, ind, wh, reg,
                                      gt_dets, gt_areas, nullptr, nullptr, nullptr, B, C, H, W, M, 0, stream);
}

extern "C" int cnuda_encode_targets_modes(const double* boxes, const double* corners, const int* classes,
                                          const int* counts, const double* keypoints, const int* visibility,
                                          const float* areas, float* hm, unsigned char* reg_mask, long long* ind,
                                          float* wh, float* reg, float* gt_dets, float* gt_areas, float* kps,
                                          float* gt_kps, unsigned char* kp_reg_mask, int B, int C, int H, int W,
                                          int M, int J, cnuda_stream_t stream) {
    CNUDA_REQUIRE((boxes != nullptr) != (corners != nullptr),
                  "cnuda_encode_targets_modes: exactly one of boxes and corners must be given");
    CNUDA_REQUIRE(classes && counts && hm && reg_mask && ind && wh && reg && gt_dets && gt_areas,
                  "cnuda_encode_targets_modes: null pointer");
    CNUDA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && M > 0 && J >= 0 && B <= 65535,
                  "cnuda_encode_targets_modes: bad sizes");
    CNUDA_REQUIRE(J > 0 ? (keypoints && visibility && kps && gt_kps && kp_reg_mask)
                        : (!keypoints && !visibility && !kps && !gt_kps && !kp_reg_mask),
                  "cnuda_encode_targets_modes: keypoints, visibility, kps, gt_kps and kp_reg_mask go with J > 0 only");
    hipStream_t st = (hipStream_t)stream;
    const bool rot = corners != nullptr;
    const size_t BM = (size_t)B * M;
    // the outputs start from zeros like the reference's np.zeros (coco.py:168-174)
    (void)hipMemsetAsync(hm, 0, (size_t)B * C * H * W * sizeof(float), st);
    (void)hipMemsetAsync(reg_mask, 0, BM, st);
    (void)hipMemsetAsync(ind, 0, BM * sizeof(long long), st);
    (void)hipMemsetAsync(wh, 0, BM * (rot ? 3 : 2) * sizeof(float), st);
    (void)hipMemsetAsync(reg, 0, BM * 2 * sizeof(float), st);
    (void)hipMemsetAsync(gt_dets, 0, BM * (rot ? 7 : 6) * sizeof(float), st);
    (void)hipMemsetAsync(gt_areas, 0, BM * sizeof(float), st);
    if (J > 0) {                                            // coco.py:176-184
        (void)hipMemsetAsync(kps, 0, BM * 2 * J * sizeof(float), st);
        (void)hipMemsetAsync(gt_kps, 0, BM * 2 * J * sizeof(float), st);
        (void)hipMemsetAsync(kp_reg_mask, 0, BM * 2 * J, st);
    }
    if (rot)
        CNUDA_LAUNCH(encode_targets_kernel<true>, dim3(M, B), dim3(256), 0, st, corners, classes, counts,
                     keypoints, visibility, areas, hm, reg_mask, ind, wh, reg, gt_dets, gt_areas, kps, gt_kps,
                     kp_reg_mask, C, H, W, M, J);
    else
        CNUDA_LAUNCH(encode_targets_kernel<false>, dim3(M, B), dim3(256), 0, st, boxes, classes, counts,
                     keypoints, visibility, areas, hm, reg_mask, ind, wh, reg, gt_dets, gt_areas, kps, gt_kps,
                     kp_reg_mask, C, H, W, M, J);
    return check_launch("cnuda_encode_targets_modes");
}
