"""numpy float32 restatement of the strong view (include/centernet_uda_hip.h, "Strong view"; csrc/strongview.hip), in
whole-array operations: every line below is one float32 numpy operation per IEEE step of the definition, the blur pads
with np.pad(mode='edge'), Philox4x32-10 runs in uint64 arithmetic and the pivot comes from np.rint.  Used by
tests/test_host_strong_view.py (pinned there by hand-worked pictures) and tests/test_gpu_strong_view.py (bit for bit)."""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)


def _c3(a):
    return np.asarray(a, dtype=F).reshape(3, 1, 1)


def luma(v):
    """v [3, H, W] float32 -> [H, W]: (0.299 R + 0.587 G) + 0.114 B"""
    return (F(0.299) * v[0] + F(0.587) * v[1]) + F(0.114) * v[2]


def denormalise(x, mean, std):
    return np.clip(x * _c3(std) + _c3(mean), F(0), F(1))


def pivot(x, mean, std):
    """x [B, 3, H, W] float32 -> [B] float32: the mean luma of every un-augmented image from an exact integer sum."""
    x = np.asarray(x, dtype=F)
    out = np.zeros(x.shape[0], dtype=F)
    for b in range(x.shape[0]):
        q = np.rint(luma(denormalise(x[b], mean, std)) * F(65536.0)).astype(np.uint64)
        out[b] = F(np.float64(int(q.sum())) / (65536.0 * x.shape[2] * x.shape[3]))
    return out


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words, key: two 32-bit ints -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & M32 for c in counter]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2       # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def fill(H, W, seed, image_id):
    """-> [3, H, W] float32: the value every pixel of an image takes inside a rectangle."""
    pixel = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    image_id = int(image_id) & 0xFFFFFFFFFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((pixel & M32, pixel >> np.uint64(32), np.full((H, W), image_id & 0xFFFFFFFF, dtype=np.uint64),
                           np.full((H, W), image_id >> 32, dtype=np.uint64)), (seed & 0xFFFFFFFF, seed >> 32))
    u = ((np.stack(words[:3]) >> np.uint64(9)).astype(F) + F(0.5)) * F(1.0 / 8388608.0)
    return (u * F(2.0) - F(1.0)) * F(1.7320508)


def blur(v, taps, radius):
    """v [3, H, W] -> the separable blur with replicated edges: horizontal pass, its float32 result kept, then vertical."""
    R = int(radius)
    if R == 0:
        return v
    H, W = v.shape[1:]
    w = np.asarray(taps, dtype=F)
    padded = np.pad(v, ((0, 0), (0, 0), (R, R)), mode='edge')
    acc = np.zeros_like(v)
    for k in range(2 * R + 1):
        acc = acc + w[k] * padded[:, :, k:k + W]
    padded = np.pad(acc, ((0, 0), (R, R), (0, 0)), mode='edge')
    acc = np.zeros_like(v)
    for k in range(2 * R + 1):
        acc = acc + w[k] * padded[:, k:k + H, :]
    return acc


def rect_mask(rects, H, W):
    """rects [3, 4] (x0, y0, x1, y1) half-open -> [H, W] bool: inside any non-empty rectangle"""
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), dtype=bool)
    for x0, y0, x1, y1 in np.asarray(rects).reshape(-1, 4):
        if x1 > x0 and y1 > y0:
            mask |= (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
    return mask


def photometric(x, mean, std, photo, m):
    """One image [3, H, W] through steps 1-4 -> v in [0, 1]; a factor of exactly 1 skips its step."""
    fb, fc, fs, gray = [F(t) for t in photo]
    v = denormalise(x, mean, std)
    if fb != 1:
        v = np.minimum(v * fb, F(1))
    if fc != 1:
        v = np.clip((v - F(m)) * fc + F(m), F(0), F(1))
    if fs != 1:
        g = luma(v)
        v = np.clip((v - g) * fs + g, F(0), F(1))
    if gray != 0:
        v = np.broadcast_to(luma(v), v.shape).copy()
    return v


def strong_view(x, mean, std, photo, taps, radius, rects, ids, seed, pivots=None):
    """x [B, 3, H, W] float32 and the tables of cnuda_strong_view -> y [B, 3, H, W] float32.  pivots: [B], default
    pivot(x, mean, std)."""
    x = np.asarray(x, dtype=F)
    B, _, H, W = x.shape
    pivots = pivot(x, mean, std) if pivots is None else pivots
    y = np.empty_like(x)
    for b in range(B):
        fb, fc, fs, gray = [F(t) for t in photo[b]]
        if fb == 1 and fc == 1 and fs == 1 and gray == 0 and int(radius[b]) == 0:
            y[b] = x[b]
        else:
            v = blur(photometric(x[b], mean, std, photo[b], pivots[b]), taps[b], radius[b])
            y[b] = (v - _c3(mean)) / _c3(std)
        mask = rect_mask(rects[b], H, W)
        if mask.any():
            y[b] = np.where(mask[None], fill(H, W, seed, ids[b]), y[b])
    return y
