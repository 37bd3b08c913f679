// Exact IoU of two convex quadrilaterals in float64 ("Rotated IoU"): the one device function behind
// cnuda_quad_iou_pairs, cnuda_eval_iou_quads (evalcoco.hip) and cnuda_soft_nms_merge_rotated (predict.hip), and what the
// stand-alone host program of the tests (tests/polyiou_host.cpp) runs on the CPU.
// Its clipping (steps 3 and 4, clipped_doubled_area) also gives cnuda_labels_transform (geomview.hip) the visible part of a
// pseudo-label, with the output map's rectangle as the clipper.
//
// The definition is normative: the tests demand the bits of a Python float64 restatement (tests/polyiou_oracle.py).
// Only + - * / and comparisons occur, every one rounded once: no fused multiply-add (the pragma below; the Makefile
// says so too), no reassociation.
//   1. a coordinate that is not finite: IoU 0, both areas 0;
//   2. per quad the doubled signed area a2 = sum_i (x_i y_{i+1} - x_{i+1} y_i), ascending i into one accumulator that
//      starts at 0; a2 < 0: the vertex order is reversed (3, 2, 1, 0) and a2 negated; area = a2 / 2; a2 not > 0: IoU 0;
//   3. Sutherland-Hodgman, subject A, clipper B, edges k = 0..3 of B with a = B_k, e = B_{k+1} - a,
//      d(p) = e.x (p.y - a.y) - e.y (p.x - a.x); per vertex p_j with successor q: emit p when d(p) >= 0, then, when
//      d(p) and d(q) have strictly opposite signs, p + t (q - p) with t = d(p) / (d(p) - d(q));
//   4. i2 = the doubled area of the result by the sum of 2 (0 below three vertices), clamped to [0, min(a2A, a2B)];
//      u2 = a2A + a2B - i2; IoU = i2 / u2 when u2 > 0, else 0.
// A convex subject never exceeds 8 vertices.  A non-convex or self-crossing quad can; what would be emitted past the
// eighth vertex is dropped, and the clamps of 4 keep the value finite and inside [0, 1]: it is otherwise unspecified.
//
// Register form.  The polygon lives in two sets of eight (x, y) doubles that only ever see compile-time indices: every
// loop below is fully unrolled, the successor of the last live vertex and the slot an emitted vertex lands in are
// picked by chains of selects (predicated compaction).  A privately indexed array would go to scratch memory on this
// compiler; this form uses none, needs no LDS and no barrier, and is the same code in all three kernels.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef CNUDA_HD
#if defined(__HIPCC__)
#define CNUDA_HD __host__ __device__
#else
#define CNUDA_HD
#endif
#endif

#pragma clang fp contract(off)

namespace cnuda {
namespace polyiou {

constexpr int kMaxVertices = 8;

struct Quad {
    double x[4], y[4];
};
struct QuadIou {
    double iou, area_a, area_b;
};

// q: eight float32 (x0, y0, ..., x3, y3), widened
CNUDA_HD inline Quad load_quad(const float* q) {
    Quad r;
#pragma unroll
    for (int v = 0; v < 4; ++v) r.x[v] = (double)q[2 * v], r.y[v] = (double)q[2 * v + 1];
    return r;
}

CNUDA_HD inline bool finite(const Quad& q) {
    bool ok = true;
#pragma unroll
    for (int v = 0; v < 4; ++v) ok = ok && (q.x[v] - q.x[v] == 0.0) && (q.y[v] - q.y[v] == 0.0);      // inf - inf, nan - nan: nan
    return ok;
}

// Step 2: counter-clockwise order in place; -> the doubled area (>= 0, or nan never: the input is finite).
CNUDA_HD inline double orient(Quad& q) {
    double a2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) a2 = a2 + (q.x[i] * q.y[(i + 1) & 3] - q.x[(i + 1) & 3] * q.y[i]);
    if (a2 < 0.0) {
        double t;
        t = q.x[0], q.x[0] = q.x[3], q.x[3] = t;
        t = q.y[0], q.y[0] = q.y[3], q.y[3] = t;
        t = q.x[1], q.x[1] = q.x[2], q.x[2] = t;
        t = q.y[1], q.y[1] = q.y[2], q.y[2] = t;
        a2 = -a2;
    }
    return a2;
}

// The area of one quad alone, by steps 1 and 2: what convex_quad_iou reports for it beside any partner.
CNUDA_HD inline double quad_area(Quad q) {
    if (!finite(q)) return 0.0;
    return orient(q) / 2.0;
}

namespace detail {
// out[n] = (vx, vy) when `on` and a slot is left: n is a run-time value, the slots are not
CNUDA_HD inline void put(double (&ox)[kMaxVertices], double (&oy)[kMaxVertices], int n, bool on, double vx, double vy) {
#pragma unroll
    for (int s = 0; s < kMaxVertices; ++s) {
        const bool here = on && n == s;
        ox[s] = here ? vx : ox[s];
        oy[s] = here ? vy : oy[s];
    }
}
}  // namespace detail

// Steps 3 and 4's i2: the doubled area of A clipped by B, both counter-clockwise (orient) with doubled areas a2a, a2b > 0.
// The one clipping routine of the library: convex_quad_iou below and the survivor filter of cnuda_labels_transform
// (geomview.hip), whose clipper is the map's rectangle.
CNUDA_HD inline double clipped_doubled_area(const Quad& A, const Quad& B, double a2a, double a2b) {
    double px[kMaxVertices], py[kMaxVertices];
#pragma unroll
    for (int s = 0; s < kMaxVertices; ++s) px[s] = s < 4 ? A.x[s] : 0.0, py[s] = s < 4 ? A.y[s] : 0.0;
    int m = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double ax = B.x[k], ay = B.y[k], ex = B.x[(k + 1) & 3] - ax, ey = B.y[(k + 1) & 3] - ay;
        double d[kMaxVertices];
#pragma unroll
        for (int s = 0; s < kMaxVertices; ++s) d[s] = ex * (py[s] - ay) - ey * (px[s] - ax);
        double ox[kMaxVertices], oy[kMaxVertices];
#pragma unroll
        for (int s = 0; s < kMaxVertices; ++s) ox[s] = 0.0, oy[s] = 0.0;
        int n = 0;
#pragma unroll
        for (int j = 0; j < kMaxVertices; ++j) {
            const bool live = j < m, wrap = j + 1 == m;
            const double dp = d[j], dq = wrap ? d[0] : d[(j + 1) & 7];
            const double qx = wrap ? px[0] : px[(j + 1) & 7], qy = wrap ? py[0] : py[(j + 1) & 7];
            const bool keep = live && dp >= 0.0;
            detail::put(ox, oy, n, keep, px[j], py[j]);
            n += keep ? 1 : 0;
            const bool cross = live && ((dp > 0.0 && dq < 0.0) || (dp < 0.0 && dq > 0.0));
            const double t = dp / (cross ? dp - dq : 1.0);
            detail::put(ox, oy, n, cross, px[j] + t * (qx - px[j]), py[j] + t * (qy - py[j]));
            n += cross ? 1 : 0;
        }
        m = n < kMaxVertices ? n : kMaxVertices;
#pragma unroll
        for (int s = 0; s < kMaxVertices; ++s) px[s] = ox[s], py[s] = oy[s];
        if (m == 0) break;
    }
    double i2 = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxVertices; ++j) {
        const bool wrap = j + 1 == m;
        const double qx = wrap ? px[0] : px[(j + 1) & 7], qy = wrap ? py[0] : py[(j + 1) & 7];
        const double term = px[j] * qy - qx * py[j];
        i2 = j < m ? i2 + term : i2;
    }
    if (m < 3) i2 = 0.0;
    if (i2 < 0.0) i2 = 0.0;
    if (i2 > a2a) i2 = a2a;
    if (i2 > a2b) i2 = a2b;
    return i2;
}

CNUDA_HD inline QuadIou convex_quad_iou(Quad A, Quad B) {
    QuadIou r = {0.0, 0.0, 0.0};
    if (!finite(A) || !finite(B)) return r;
    const double a2a = orient(A), a2b = orient(B);
    r.area_a = a2a / 2.0, r.area_b = a2b / 2.0;
    if (!(a2a > 0.0) || !(a2b > 0.0)) return r;
    const double i2 = clipped_doubled_area(A, B, a2a, a2b);
    const double u2 = a2a + a2b - i2;
    r.iou = u2 > 0.0 ? i2 / u2 : 0.0;
    return r;
}

}  // namespace polyiou
}  // namespace cnuda
