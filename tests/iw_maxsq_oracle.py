"""float64 numpy statement of image-wise class-balanced max-squares (Chen, Xue, Cai, ICCV 2019), for its tests.

    v = softmax(x, 1);   a[b, p] = argmax_c x[b, c, p] on the logits, lowest channel on a tie (np.argmax)
    hist[b, c] = #{p : a[b, p] == c};   w[b, c] = 1 / max(hist[b, c]^ratio * HW^(1 - ratio), 1)
    loss = -sum_{b,c,p} v^2 w[b, a[b, p]] / (2 B C)

the published -sum(prob^2 * weight[argpred]) / (batch * num_class), divided by 2 as MaxSquareLoss is.  The weights are
constants of the gradient:  dx_j = k v_j (2 v_j - sum_i 2 v_i^2),  k = -w[b, a] / (2 B C)."""
import numpy as np


def hist(x):
    """x [B, C, H, W] -> int64 [B, C]"""
    B, C = x.shape[:2]
    a = np.argmax(np.asarray(x).reshape(B, C, -1), axis=1)
    return np.stack([np.bincount(a[b], minlength=C) for b in range(B)]).astype(np.int64)


def weights(x, ratio):
    """-> float64 [B, C]"""
    h = hist(x).astype(np.float64)
    hw = float(np.prod(x.shape[2:]))
    return 1.0 / np.maximum(h ** ratio * hw ** (1.0 - ratio), 1.0)


def _parts(x, ratio):
    B, C = x.shape[:2]
    z = np.asarray(x, np.float64).reshape(B, C, -1)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    v = e / e.sum(axis=1, keepdims=True)
    a = np.argmax(np.asarray(x).reshape(B, C, -1), axis=1)                  # on the input's own dtype
    wp = np.take_along_axis(weights(x, ratio), a, axis=1)[:, None, :]       # [B, 1, HW]: the pixel's weight
    return v, wp, -1.0 / (2.0 * B * C)


def loss(x, ratio):
    v, wp, scale = _parts(x, ratio)
    return float((v * v * wp).sum() * scale)


def grad(x, ratio):
    """d loss / d x, float64, shaped like x"""
    v, wp, scale = _parts(x, ratio)
    dot = (2.0 * v * v).sum(axis=1, keepdims=True)
    return (scale * wp * v * (2.0 * v - dot)).reshape(x.shape)
