// The rasterisation rule of the COCO evaluator's rotated mode in closed form, shared by the kernels of evalcoco.hip and
// by the stand-alone host program of the tests (tests/evalcoco_host.cpp runs it on the CPU under the sanitizers).
//
// The rule is utils/image.py::_fill_convex_poly on the four integer vertices of a rotated box shifted to 16-bit fixed
// point: the 8-connected outline of the four edges (_line8, after _clip_line), then the scanlines between the two edge
// chains that walk down from the topmost vertex.  Both advance by a constant integer step per pixel / per row, so the
// position at step k is start + k * step: every outline pixel and every scanline is independent of the others, and the
// sequential part shrinks to a set-up of four `Line` records and at most `kMaxScanIntervals` `ScanInterval` records.
// All fixed-point arithmetic is 64-bit: (xe - xs) * 2 and dy << 16 pass 2^31 for boxes a few thousand pixels outside.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CNUDA_HD __host__ __device__
#else
#define CNUDA_HD
#endif

namespace cnuda {
namespace evalcoco {

typedef long long i64;
constexpr int kShift = 16;
constexpr i64 kOne = 1ll << kShift;
constexpr i64 kHalf = kOne >> 1;
constexpr int kMaxScanIntervals = 6;
constexpr int kMaxImageSide = 8192;        // two ints of LDS per image row
constexpr int kMaxThresholds = 16;         // matched / ignored bits of one detection share a 32-bit word
constexpr int kAreaRanges = 4;

// One edge of the outline after clipping.  count < 0: nothing visible.  Pixel k (0 <= k <= count) is
// (major0 + k, (minor0 + k * step) >> 16) along the major axis; (end_x, end_y) is drawn as well.
struct Line {
    int x_major, count, end_x, end_y;
    i64 major0, minor0, step;
};

// Rows [row_begin, row_end): chain c is at x0[c] + (row - row0[c]) * dx[c] (fixed point).
struct ScanInterval {
    int row_begin, row_end, row0[2];
    i64 x0[2], dx[2];
};

CNUDA_HD inline int outcode(i64 x, i64 y, i64 right, i64 bottom) {
    return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8;
}

// _clip_line on the image scaled to fixed point; the intersections are the double-precision products and quotients of
// the Python rule, truncated toward zero, in its order (the second end point sees the moved first one).
CNUDA_HD inline bool clip_line(i64 w, i64 h, i64& x1, i64& y1, i64& x2, i64& y2) {
    const i64 right = w - 1, bottom = h - 1;
    int c1 = outcode(x1, y1, right, bottom), c2 = outcode(x2, y2, right, bottom);
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const i64 a = c1 < 8 ? 0 : bottom;
            x1 += (i64)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const i64 a = c2 < 8 ? 0 : bottom;
            x2 += (i64)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const i64 a = c1 == 1 ? 0 : right;
                y1 += (i64)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const i64 a = c2 == 1 ? 0 : right;
                y2 += (i64)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

CNUDA_HD inline i64 iabs(i64 v) { return v < 0 ? -v : v; }

// _line8 from integer vertex (ax, ay) to (bx, by) on a W x H image
CNUDA_HD inline Line line_setup(int ax, int ay, int bx, int by, int W, int H) {
    Line l;
    l.x_major = 0, l.count = -1, l.end_x = l.end_y = 0, l.major0 = l.minor0 = l.step = 0;
    i64 x1 = (i64)ax * kOne, y1 = (i64)ay * kOne, x2 = (i64)bx * kOne, y2 = (i64)by * kOne;
    if (!clip_line((i64)W * kOne, (i64)H * kOne, x1, y1, x2, y2)) return l;
    i64 dx = x2 - x1, dy = y2 - y1;
    l.x_major = iabs(dx) > iabs(dy);
    if (l.x_major) {
        if (dx < 0) {
            i64 t = x1; x1 = x2; x2 = t;
            t = y1; y1 = y2; y2 = t;
            dy = -dy;
        }
        l.step = dy * kOne / (iabs(dx) | 1);
        l.count = (int)((x2 - x1) >> kShift);
    } else {
        if (dy < 0) {
            i64 t = x1; x1 = x2; x2 = t;
            t = y1; y1 = y2; y2 = t;
            dx = -dx;
        }
        l.step = dx * kOne / (iabs(dy) | 1);
        l.count = (int)((y2 - y1) >> kShift);
    }
    x1 += kHalf;
    y1 += kHalf;
    l.end_x = (int)((x2 + kHalf) >> kShift);
    l.end_y = (int)((y2 + kHalf) >> kShift);
    if (l.x_major) {
        l.major0 = x1 >> kShift;
        l.minor0 = y1;
    } else {
        l.major0 = y1 >> kShift;
        l.minor0 = x1;
    }
    return l;
}

CNUDA_HD inline void line_pixel(const Line& l, int k, int& x, int& y) {
    const int major = (int)(l.major0 + k), minor = (int)((l.minor0 + (i64)k * l.step) >> kShift);
    x = l.x_major ? major : minor;
    y = l.x_major ? minor : major;
}

// The scanline part of _fill_convex_poly for four integer vertices: its two-chain walk, advanced from one change of
// edge to the next instead of row by row.  -> number of intervals written to `out` (rows below 0 are not cut off here).
CNUDA_HD inline int scan_setup(const int* vx, const int* vy, int W, int H, ScanInterval* out) {
    int xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0], imin = 0;
    for (int i = 1; i < 4; ++i) {
        if (vy[i] < ymin) ymin = vy[i], imin = i;
        if (vy[i] > ymax) ymax = vy[i];
        if (vx[i] > xmax) xmax = vx[i];
        if (vx[i] < xmin) xmin = vx[i];
    }
    if (xmax < 0 || ymax < 0 || xmin >= W || ymin >= H) return 0;
    if (ymax > H - 1) ymax = H - 1;
    int edges = 4, n = 0, y = ymin;
    int idx[2] = {imin, imin}, ye[2] = {ymin, ymin}, row0[2] = {ymin, ymin};
    const int di[2] = {1, 3};
    i64 x[2] = {-kOne, -kOne}, dx[2] = {0, 0};
    for (;;) {
        for (int c = 0; c < 2; ++c) {
            if (y < ye[c]) continue;
            int i0 = idx[c], i1 = (i0 + di[c]) & 3;
            bool found = false;
            while (edges > 0) {
                --edges;
                const int ty = vy[i1];
                if (ty > y) {
                    const i64 xs = (i64)vx[i0] * kOne, xe = (i64)vx[i1] * kOne;
                    ye[c] = ty;
                    dx[c] = ((xe - xs) * 2 + (ty - y)) / (2 * (i64)(ty - y));
                    x[c] = xs;
                    idx[c] = i1;
                    row0[c] = y;
                    found = true;
                    break;
                }
                i0 = i1;
                i1 = (i1 + di[c]) & 3;
            }
            if (!found) --edges;
        }
        if (edges < 0) break;
        const int next = ye[0] < ye[1] ? ye[0] : ye[1];
        if (n < kMaxScanIntervals) {
            ScanInterval& s = out[n++];
            s.row_begin = y;
            s.row_end = next < ymax + 1 ? next : ymax + 1;
            for (int c = 0; c < 2; ++c) s.row0[c] = row0[c], s.x0[c] = x[c], s.dx[c] = dx[c];
        }
        if (next > ymax) break;
        y = next;
    }
    return n;
}

// span [left, right] of a scanline clipped to the image; false: nothing inside
CNUDA_HD inline bool scan_row(const ScanInterval& s, int row, int W, int& left, int& right) {
    const i64 a = s.x0[0] + (i64)(row - s.row0[0]) * s.dx[0], b = s.x0[1] + (i64)(row - s.row0[1]) * s.dx[1];
    const i64 lo = a > b ? b : a, hi = a > b ? a : b;
    const i64 xx1 = (lo + kHalf) >> kShift, xx2 = (hi + kHalf) >> kShift;
    if (xx2 < 0 || xx1 >= W) return false;
    left = (int)(xx1 < 0 ? 0 : xx1);
    right = (int)(xx2 > W - 1 ? W - 1 : xx2);
    return true;
}

// ---- host-only: argument checks and workspace sizes of the cnuda_eval_* entry points (no device involved) ----
inline size_t spans_workspace_bytes(int num_boxes, int H) {
    if (num_boxes < 0 || H <= 0 || H > kMaxImageSide) return 0;
    return (size_t)num_boxes * (size_t)H * 2 * sizeof(int) + 256;
}

// nullptr: fine; else what is wrong
inline const char* image_error(int H, int W) {
    if (H <= 0 || W <= 0) return "image height and width must be positive";
    if (H > kMaxImageSide || W > kMaxImageSide) return "image side above 8192";
    return nullptr;
}

inline const char* groups_error(int G, int ND, int NGT, long long num_pairs) {
    if (G < 0 || ND < 0 || NGT < 0 || num_pairs < 0) return "negative count";
    if (num_pairs >= (1ll << 31) || (long long)ND * 4 >= (1ll << 31) || (long long)NGT * 4 >= (1ll << 31))
        return "problem too large (2^31 pairs or more)";
    if (G >= (1 << 24)) return "too many (image, category) groups";
    return nullptr;
}

inline const char* match_error(const double* thresholds, int T, const double* ranges) {
    if (!thresholds || !ranges) return "null threshold or area-range table";
    if (T <= 0 || T > kMaxThresholds) return "between 1 and 16 IoU thresholds";
    for (int t = 0; t < T; ++t)
        if (!(thresholds[t] >= 0.0 && thresholds[t] <= 1.0)) return "an IoU threshold outside [0, 1]";
    for (int a = 0; a < kAreaRanges; ++a)
        if (!(ranges[2 * a] <= ranges[2 * a + 1])) return "an area range with lo > hi";
    return nullptr;
}

}  // namespace evalcoco
}  // namespace cnuda
