"""Float64 numpy statement of the dense teacher's definitions (include/centernet_uda_hip.h, "Dense teacher"):
the per-image selection on the teacher's LOGITS with every tie included, the quality focal loss of the heat map and the
score-weighted L1 of the sizes, with their gradients.  Independent of the library: plain sorting, no keys, no kernels.

Conventions the kernels share: the score is the channel maximum and is NaN as soon as one channel is; a NaN score orders
below every number and is never selected; with fewer than k numbers in an image tau is -inf (all numbers selected); a
zero tau is +0 (-0 and +0 are one value)."""
import numpy as np


def k_of(ratio, HW):
    return max(1, int(np.floor(float(ratio) * HW)))


def scores(t_hm):
    """[B, C, H, W] -> [B, H, W] float32: np.max propagates NaN."""
    return np.max(np.asarray(t_hm, np.float32), axis=1)


def select(t_hm, ratio):
    """-> (tau [B] float32, count [B] int32, mask [B, H, W] bool)"""
    s = scores(t_hm)
    B, H, W = s.shape
    k = k_of(ratio, H * W)
    tau = np.empty(B, np.float32)
    for b in range(B):
        v = s[b].ravel()
        v = np.sort(v[~np.isnan(v)])[::-1]          # descending, NaNs dropped
        tau[b] = v[k - 1] + np.float32(0) if v.size >= k else -np.inf      # (-0) + 0 = +0
    with np.errstate(invalid='ignore'):
        mask = s >= tau[:, None, None]              # NaN >= anything is False
    return tau, mask.reshape(B, -1).sum(1).astype(np.int32), mask


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


def _student_frame(a, mirror):
    """A teacher-side [..., H, W] array as the student sees it."""
    return a[..., ::-1] if mirror else a


def _terms(x_hm, x_wh, t_hm, t_wh, mask, mirror):
    x_hm, x_wh, t_hm, t_wh = (np.asarray(a, np.float64) for a in (x_hm, x_wh, t_hm, t_wh))
    m = _student_frame(mask, mirror)[:, None]                                   # [B, 1, H, W]
    with np.errstate(invalid='ignore'):
        y = np.where(m, _sigmoid(_student_frame(t_hm, mirror)), 0.0)
        s = np.max(_student_frame(t_hm, mirror), axis=1, keepdims=True)
        u = np.where(m, _sigmoid(s), 0.0)                                       # [B, 1, H, W]
    # (off the selection the teacher's sizes take no part, whatever they hold)
    twh = np.where(m, _student_frame(t_wh, mirror), 0.0)
    q = _sigmoid(x_hm)
    bce = np.maximum(x_hm, 0) - x_hm * y + np.log1p(np.exp(-np.abs(x_hm)))
    return x_hm, x_wh, y, q, bce, u, twh


def loss(x_hm, x_wh, t_hm, t_wh, ratio, mirror, hm_weight=1.0, wh_weight=0.1):
    """-> (dense_loss, hm_loss, wh_loss, N, sum u) as Python numbers"""
    _, count, mask = select(t_hm, ratio)
    x_hm, x_wh, y, q, bce, u, twh = _terms(x_hm, x_wh, t_hm, t_wh, mask, mirror)
    N = int(count.sum())
    hm_loss = float(((y - q) ** 2 * bce).sum() / max(N, 1))
    su = float(u.sum())
    wh_loss = float((u * np.abs(x_wh - twh)).sum() / (su + 1e-4))
    return hm_weight * hm_loss + wh_weight * wh_loss, hm_loss, wh_loss, N, su


def grad(x_hm, x_wh, t_hm, t_wh, ratio, mirror, hm_weight=1.0, wh_weight=0.1, upstream=1.0):
    """-> (d dense_loss / d x_hm, d dense_loss / d x_wh) * upstream, float64"""
    _, count, mask = select(t_hm, ratio)
    x_hm, x_wh, y, q, bce, u, twh = _terms(x_hm, x_wh, t_hm, t_wh, mask, mirror)
    N = int(count.sum())
    d = q - y
    g_hm = d * (d * d + 2 * q * (1 - q) * bce) / max(N, 1)
    g_wh = u * np.sign(x_wh - twh) / (u.sum() + 1e-4)
    return upstream * hm_weight * g_hm, upstream * wh_weight * g_wh
