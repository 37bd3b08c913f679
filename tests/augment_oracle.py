"""numpy restatement of the augmentation kernels' definitions ("Augmentation on the device"), written from
the definitions and pinned in tests/test_host_augment.py by answers that do not come from it: exact identities, PIL's
bilinear resize and affine transform, colorsys.  Every float32 step is one numpy operation in the documented order."""
import numpy as np

f = np.float32


def warp(src, inverse, out_h, out_w, taps=((0.0, 0.0, 1.0),), size=None):
    """src [H_max, W_max, 3] uint8 with valid size (h, w) (default: all of it); inverse: six values, output -> source
    coordinates; taps: (offset x, offset y, weight) rows -> [out_h, out_w, 3] uint8.  No noise."""
    hs, ws = src.shape[:2] if size is None else (int(size[0]), int(size[1]))
    a = np.asarray(inverse, dtype=np.float32).reshape(6)
    j, i = np.meshgrid(np.arange(out_w, dtype=np.float32), np.arange(out_h, dtype=np.float32))
    x, y = j + f(0.5), i + f(0.5)
    u = (a[0] * x + a[1] * y) + a[2]
    v = (a[3] * x + a[4] * y) + a[5]
    inside = (u >= 0) & (u <= ws) & (v >= 0) & (v <= hs)
    s = src.astype(np.float32)
    one = f(1)
    acc = np.zeros((out_h, out_w, 3), np.float32)
    for ox, oy, w in np.asarray(taps, dtype=np.float32).reshape(-1, 3):
        pu, pv = (u + ox) - f(0.5), (v + oy) - f(0.5)
        x0, y0 = np.floor(pu), np.floor(pv)
        fx, fy = (pu - x0)[..., None], (pv - y0)[..., None]
        # outside pixels are zeroed below; keep their indices finite and in range all the same
        xa, xb = np.clip(x0, 0, ws - 1).astype(np.int64), np.clip(x0 + one, 0, ws - 1).astype(np.int64)
        ya, yb = np.clip(y0, 0, hs - 1).astype(np.int64), np.clip(y0 + one, 0, hs - 1).astype(np.int64)
        top = (one - fx) * s[ya, xa] + fx * s[ya, xb]
        bot = (one - fx) * s[yb, xa] + fx * s[yb, xb]
        acc = acc + w * ((one - fy) * top + fy * bot)
    assert acc.dtype == np.float32
    out = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    out[~inside] = 0
    return out


def warp_batch(images, params, sizes=None):
    """images [B, H_max, W_max, 3] uint8 and a datasets.augment.AugmentParams record (its noise is ignored)."""
    sizes = params.sizes if sizes is None else sizes
    W_in, H_in = params.input_size
    return np.stack([warp(images[b], params.inverse[b], H_in, W_in, params.taps[b, :params.ntaps[b]], sizes[b])
                     for b in range(images.shape[0])])


def color(img, alpha, hue_deg, add):
    """Grayscale blend, RGB -> HSV (hue in sextants), hue rotation by hue_deg, V + add clamped, HSV -> RGB, rint,
    clamp; float32, only + - * / floor min max."""
    x = img.astype(np.float32)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    gray = (f(0.299) * r + f(0.587) * g) + f(0.114) * b
    keep = f(1) - f(alpha)
    r, g, b = keep * r + f(alpha) * gray, keep * g + f(alpha) * gray, keep * b + f(alpha) * gray
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    c = mx - mn
    safe = np.where(c > 0, c, f(1))
    h = np.where(mx == r, (g - b) / safe, np.where(mx == g, (b - r) / safe + f(2), (r - g) / safe + f(4)))
    h = np.where(c > 0, h, f(0))
    h = h + f(hue_deg) / f(60)
    h = h - f(6) * np.floor(h / f(6))
    s = np.where(mx > 0, c / np.where(mx > 0, mx, f(1)), f(0))
    v = np.clip(mx + f(add), f(0), f(255))

    def channel(n):
        k = f(n) + h
        k = k - f(6) * np.floor(k / f(6))
        t = np.clip(np.minimum(k, f(4) - k), f(0), f(1))
        return v - (v * s) * t

    out = np.stack([channel(5), channel(3), channel(1)], -1)
    assert out.dtype == np.float32
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def points(forward, pts):
    """forward: six float64 values; pts [N, 2] -> (m0 u + m1 v) + m2, (m3 u + m4 v) + m5"""
    m = np.asarray(forward, dtype=np.float64).reshape(6)
    u, v = pts[..., 0], pts[..., 1]
    return np.stack([(m[0] * u + m[1] * v) + m[2], (m[3] * u + m[4] * v) + m[5]], -1)


def boxes(forward, bxs):
    """bxs [M, 4] (x1, y1, x2, y2) -> the bounding box of the four mapped corners"""
    x1, y1, x2, y2 = (bxs[..., k] for k in range(4))
    c = points(forward, np.stack([np.stack([x1, y1], -1), np.stack([x2, y1], -1), np.stack([x2, y2], -1),
                                  np.stack([x1, y2], -1)], -2))
    return np.concatenate([c.min(-2), c.max(-2)], -1)
