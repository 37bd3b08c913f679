"""numpy restatements of csrc/geomview.hip (include/centernet_uda_hip.h, "Geometric view"): the bilinear warp in the
kernel's own float64 / float32 steps -- bit for bit --, and the label transform in float64 with a convex clip written
independently of the kernel's (the kernel's is Sutherland-Hodgman in csrc/polyiou.cuh; this one intersects half-planes
one at a time on Python lists and takes the shoelace area)."""
import math

import numpy as np

F = np.float32
D = np.float64


def _six(m):
    m = np.asarray(m, dtype=D)
    if m.shape[-2:] == (3, 3):
        m = m[..., :2, :]
    return m.reshape(m.shape[0], 6)


# ---------------------------------------------------------------------------------------------------------------------
# the warp
# ---------------------------------------------------------------------------------------------------------------------
def warp(x, inverse, fill=0.0):
    """x [B, C, H, W] float32, inverse [B, 3, 3] / [B, 2, 3] / [B, 6] float64 -> cnuda_warp_bilinear's result."""
    x = np.asarray(x)
    assert x.dtype == F and x.ndim == 4
    B, C, H, W = x.shape
    m = _six(inverse)
    fill = F(fill)
    out = np.empty_like(x)
    dx = (np.arange(W, dtype=D) + 0.5)[None, :]
    dy = (np.arange(H, dtype=D) + 0.5)[:, None]
    for b in range(B):
        m0, m1, m2, m3, m4, m5 = m[b]
        if (m[b] == D([1, 0, 0, 0, 1, 0])).all():
            out[b] = x[b]
            continue
        u = ((m0 * dx + m1 * dy) + m2) - 0.5
        v = ((m3 * dx + m4 * dy) + m5) - 0.5
        fu, fv = np.floor(u), np.floor(v)
        fx, fy = (u - fu).astype(F), (v - fv).astype(F)
        x0 = np.clip(fu, -2.0, float(W)).astype(np.int64)
        y0 = np.clip(fv, -2.0, float(H)).astype(np.int64)

        def tap(yy, xx):
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            got = x[b][:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            return np.where(inside[None], got, fill).astype(F)
        a, bb, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        top = a + fx[None] * (bb - a)
        bot = c + fx[None] * (d - c)
        out[b] = top + fy[None] * (bot - top)
        assert out[b].dtype == F
    return out


def centroid(img):
    """The intensity centroid (x, y) of a [H, W] array in pixel-centre coordinates, float64."""
    img = np.asarray(img, dtype=D)
    H, W = img.shape
    total = img.sum()
    return ((img.sum(0) * (np.arange(W) + 0.5)).sum() / total, (img.sum(1) * (np.arange(H) + 0.5)).sum() / total)


# ---------------------------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------------------------
def shoelace(poly):
    """The signed area of a polygon given as a list of (x, y)."""
    return 0.5 * math.fsum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                           for i in range(len(poly)))


def _cut(poly, inside, cross):
    """The part of a convex polygon inside one half-plane: `inside(p)` -> bool, `cross(p, q)` -> the edge's point on the
    boundary."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        if inside(p):
            out.append(p)
            if not inside(q):
                out.append(cross(p, q))
        elif inside(q):
            out.append(cross(p, q))
    return out


def clip_area(poly, w, h):
    """The area of a convex polygon (list of (x, y), either winding) inside the rectangle [0, w] x [0, h]."""
    def at_x(x0):
        return lambda p, q: (x0, p[1] + (q[1] - p[1]) * (x0 - p[0]) / (q[0] - p[0]))

    def at_y(y0):
        return lambda p, q: (p[0] + (q[0] - p[0]) * (y0 - p[1]) / (q[1] - p[1]), y0)
    poly = [(float(px), float(py)) for px, py in poly]
    for inside, cross in ((lambda p: p[0] >= 0.0, at_x(0.0)), (lambda p: p[0] <= w, at_x(float(w))),
                          (lambda p: p[1] >= 0.0, at_y(0.0)), (lambda p: p[1] <= h, at_y(float(h)))):
        if len(poly) < 3:
            return 0.0
        poly = _cut(poly, inside, cross)
    return abs(shoelace(poly)) if len(poly) >= 3 else 0.0


def visible_fraction(poly, w, h):
    area = abs(shoelace([(float(px), float(py)) for px, py in poly]))
    return clip_area(poly, w, h) / area if area > 0.0 else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the labels
# ---------------------------------------------------------------------------------------------------------------------
def _map(m, px, py):
    return (m[0] * px + m[1] * py) + m[2], (m[3] * px + m[4] * py) + m[5]


def row(m, g, rotated, map_h, map_w):
    """One row's (label as a flat list, extent pair, area, visible) under the six entries m."""
    if rotated:
        quad = [_map(m, g[2 * v], g[2 * v + 1]) for v in range(4)]
        extent = (math.hypot(quad[1][0] - quad[0][0], quad[1][1] - quad[0][1]),
                  math.hypot(quad[2][0] - quad[1][0], quad[2][1] - quad[1][1]))
        area = abs(shoelace(quad))
        label = [t for p in quad for t in p]
    else:
        pts = [_map(m, px, py) for px, py in ((g[0], g[1]), (g[2], g[1]), (g[2], g[3]), (g[0], g[3]))]
        x1, x2 = min(p[0] for p in pts), max(p[0] for p in pts)
        y1, y2 = min(p[1] for p in pts), max(p[1] for p in pts)
        extent, area, label = (x2 - x1, y2 - y1), (x2 - x1) * (y2 - y1), [x1, y1, x2, y2]
        quad = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    finite = all(math.isfinite(t) for t in label) and math.isfinite(area)
    visible = visible_fraction(quad, map_w, map_h) if finite and area > 0.0 else 0.0
    return label, extent, area if finite else float('nan'), visible


def transform_labels(labels, forward_map, map_h, map_w, rotated=False, min_size=0.0, min_visible=0.5):
    """numpy dict in (geometry float64, classes int32, counts int32) -> (the dict cnuda_labels_transform gives, a list of
    (visible, extent0, extent1) of every row that went through the filter)."""
    key = 'corners' if rotated else 'boxes'
    geom = np.asarray(labels[key], dtype=D)
    B, K = geom.shape[:2]
    flat = geom.reshape(B, K, -1)
    m = _six(forward_map)
    out_g = np.zeros_like(flat)
    out_c = np.zeros((B, K), dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    judged = []
    before = 0
    for b in range(B):
        n = min(max(int(labels['counts'][b]), 0), K)
        before += n
        identity = (m[b] == D([1, 0, 0, 0, 1, 0])).all()
        at = 0
        for k in range(n):
            if identity:
                label, keep = list(flat[b, k]), True
            else:
                label, extent, area, visible = row(m[b], flat[b, k], rotated, map_h, map_w)
                judged.append((visible, extent[0], extent[1]))
                keep = (extent[0] >= min_size and extent[1] >= min_size and area > 0.0 and math.isfinite(area)
                        and visible >= min_visible)
            if keep:
                out_g[b, at], out_c[b, at] = label, labels['classes'][b, k]
                at += 1
        counts[b] = at
    after = int(counts.sum())
    return {'classes': out_c, 'counts': counts, 'kept': F(D(after) / D(B)), key: out_g.reshape(geom.shape),
            'dropped': F(D(before - after) / D(B))}, judged
