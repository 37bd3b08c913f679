"""numpy painter for the preview kernel's pixel rules (include/centernet_uda_hip.h, "Detection previews"; DESIGN.md
section 23), written from those rules and not from the kernel.  The kernel gathers: every pixel walks the primitives.
This painter scatters: it denormalises the image into two panels and then, primitive by primitive in list order,
works out that primitive's pixel set and blends it into its panel.  The QUAD rule runs in Python integers.
tests/test_host_visualize.py pins it by answers worked out by hand."""
import numpy as np

RECORD = 16
RING, FILL, QUAD, GLYPH = 0, 1, 2, 3


def rec(kind, panel, color, alpha, t, geometry):
    """one record, spelled out here independently of utils.visualize.record"""
    r = np.zeros(RECORD, np.int32)
    r[0], r[1], r[2] = kind, panel, color[0] + (color[1] << 8) + (color[2] << 16)
    r[3] = np.array([alpha], np.float32).view(np.int32)[0]
    r[4] = t
    r[5:5 + len(geometry)] = geometry
    return r


def base_pixels(chw, mean, std):
    """[3, H, W] float32 normalised -> [H, W, 3] uint8: (x * std + mean) * 255 in float32, clamped, truncated"""
    x = np.asarray(chw, np.float32).transpose(1, 2, 0)
    v = (x * np.asarray(std, np.float32) + np.asarray(mean, np.float32)) * np.float32(255)
    assert v.dtype == np.float32
    return np.trunc(np.clip(v, 0, 255)).astype(np.uint8)


def blend(v, a, c):
    """bytes v over colour byte c with alpha a: rint(v + a * (c - v)), every step float32, half to even"""
    v, a, c = np.asarray(v).astype(np.float32), np.float32(a), np.float32(c)
    d = (c - v).astype(np.float32)
    m = (a * d).astype(np.float32)
    s = (v + m).astype(np.float32)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def _near(x, y, p, q, t):
    """4 d^2 <= t^2 for the distance from (x, y) to the segment pq, in Python integers"""
    ex, ey, wx, wy = q[0] - p[0], q[1] - p[1], x - p[0], y - p[1]
    L, s = ex * ex + ey * ey, wx * ex + wy * ey
    if s <= 0:
        return 4 * (wx * wx + wy * wy) <= t * t
    if s >= L:
        return 4 * ((x - q[0]) ** 2 + (y - q[1]) ** 2) <= t * t
    return 4 * (wx * ey - wy * ex) ** 2 <= t * t * L


def _grid(y_lo, y_hi, x_lo, x_hi):
    """the integer points of [x_lo, x_hi] x [y_lo, y_hi] as flat (ys, xs); none when a range is empty"""
    ys, xs = np.meshgrid(np.arange(y_lo, y_hi + 1), np.arange(x_lo, x_hi + 1), indexing='ij')
    return ys.reshape(-1), xs.reshape(-1)


def pixel_set(r, H, W, atlas=None):
    """-> (ys, xs, alphas): the pixels of an H x W panel that record r covers, and the alpha at each"""
    kind, t = int(r[0]), int(r[4])
    g = [int(v) for v in r[5:13]]
    alpha = np.array([r[3]], np.int32).view(np.float32)[0]
    if kind in (RING, FILL):
        x1, y1, x2, y2 = g[:4]
        grow = t - 1 if kind == RING else 0
        ys, xs = _grid(max(y1 - grow, 0), min(y2 + grow, H - 1), max(x1 - grow, 0), min(x2 + grow, W - 1))
        if kind == RING:
            out = ~((x1 < xs) & (xs < x2) & (y1 < ys) & (ys < y2))
            ys, xs = ys[out], xs[out]
        return ys, xs, np.full(ys.shape, alpha, np.float32)
    if kind == QUAD:
        pts = [(g[0], g[1]), (g[2], g[3]), (g[4], g[5]), (g[6], g[7])]
        lo_x, hi_x = min(p[0] for p in pts) - t, max(p[0] for p in pts) + t
        lo_y, hi_y = min(p[1] for p in pts) - t, max(p[1] for p in pts) + t
        ys, xs = [], []
        for y in range(max(lo_y, 0), min(hi_y, H - 1) + 1):
            for x in range(max(lo_x, 0), min(hi_x, W - 1) + 1):
                if any(_near(x, y, pts[k], pts[(k + 1) % 4], t) for k in range(4)):
                    ys.append(y), xs.append(x)
        ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
        return ys, xs, np.full(ys.shape, alpha, np.float32)
    if kind == GLYPH:
        x0, y0 = g[:2]
        if atlas is None or not 0 <= t < atlas.shape[0]:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
        gh, gw = atlas.shape[1:]
        ys, xs = _grid(max(y0, 0), min(y0 + gh - 1, H - 1), max(x0, 0), min(x0 + gw - 1, W - 1))
        return ys, xs, atlas[t, ys - y0, xs - x0].astype(np.float32) / np.float32(255)
    raise ValueError("unknown primitive kind %d" % kind)


def paint_panels(chw, prims, mean, std, atlas=None):
    """-> [3, H, 2W] uint8: one image's two panels with its primitives painted in list order"""
    base = base_pixels(chw, mean, std)
    H, W = base.shape[:2]
    panels = [base.copy(), base.copy()]
    for r in np.asarray(prims, np.int32).reshape(-1, RECORD):
        ys, xs, alphas = pixel_set(r, H, W, atlas)
        panel = panels[int(r[1])]
        for c in range(3):
            panel[ys, xs, c] = blend(panel[ys, xs, c], alphas, (int(r[2]) >> (8 * c)) & 255)
    return np.ascontiguousarray(np.hstack(panels).transpose(2, 0, 1))


def paint(input, index, first, prims, mean, std, atlas=None):
    """the whole call: input [B, 3, H, W], index [n], first [n + 1], prims [N, RECORD] -> [n, 3, H, 2W] uint8"""
    prims = np.asarray(prims, np.int32).reshape(-1, RECORD)
    return np.stack([paint_panels(input[b], prims[first[i]:first[i + 1]], mean, std, atlas)
                     for i, b in enumerate(index)])
