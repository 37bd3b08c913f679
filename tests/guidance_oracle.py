"""float64 numpy statement of multi-level self-produced guidance (the max-squares paper's third part, as this project
defines it: README, "Multi-level self-produced guidance"), for its tests.

    x = logits of the final heat map, z = logits of the low-level one, both [B, C, H, W]
    p = softmax(x, 1), q = softmax(z, 1), e = (p + q) / 2, m = max_c e, a = argmax_c e (lowest channel on a tie)
    guided = m > threshold;   N = number of guided pixels of the batch
    loss = sum_{guided} (logsumexp_c z - z[a]) / max(N, 1)
    d loss / d z_c = guided * (q_c - [c == a]) / max(N, 1);   x has no gradient

and the margins of the oracle's own decisions, so that a test can show that a last-bit difference cannot flip one."""
import numpy as np


def _softmax(t):
    t = np.asarray(t, np.float64)
    t = t.reshape(t.shape[0], t.shape[1], -1)
    e = np.exp(t - t.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _mean_prob(x, z):
    return (_softmax(x) + _softmax(z)) / 2.0        # [B, C, HW]


def labels(x, z, threshold):
    """-> int64 shaped [B, H, W]: the guided pixels' class, -1 elsewhere"""
    e = _mean_prob(x, z)
    a = np.argmax(e, axis=1)                        # the first maximum: the lowest channel on a tie
    a[e.max(axis=1) <= threshold] = -1
    return a.reshape((x.shape[0],) + tuple(x.shape[2:]))


def count(x, z, threshold):
    return int((labels(x, z, threshold) >= 0).sum())


def _lse(z):
    z = np.asarray(z, np.float64).reshape(z.shape[0], z.shape[1], -1)
    mx = z.max(axis=1)
    return mx + np.log(np.exp(z - mx[:, None, :]).sum(axis=1)), z


def loss(x, z, threshold):
    a = labels(x, z, threshold).reshape(x.shape[0], -1)
    lse, zz = _lse(z)
    guided = a >= 0
    za = np.take_along_axis(zz, np.maximum(a, 0)[:, None, :], axis=1)[:, 0, :]
    return float(((lse - za) * guided).sum() / max(int(guided.sum()), 1))


def grad(x, z, threshold):
    """d loss / d z, float64, shaped like z"""
    a = labels(x, z, threshold).reshape(x.shape[0], -1)
    guided = a >= 0
    q = _softmax(z)
    onehot = (np.arange(z.shape[1])[None, :, None] == a[:, None, :])
    return ((q - onehot) * guided[:, None, :] / max(int(guided.sum()), 1)).reshape(z.shape)


def margins(x, z, threshold):
    """-> {'threshold': the smallest |m - threshold|,
           'gap': the smallest RELATIVE gap (e1 - e2) / e1 between the two largest e of a pixel, over all pixels whose
                  two largest differ (inf: none, or C = 1),
           'ties': the number of pixels whose two largest e are exactly equal, 'guided_ties': those of them that are
                   guided (where the tie rule decides a label that is used)}"""
    e = _mean_prob(x, z)
    m = e.max(axis=1)
    out = {'threshold': float(np.abs(m - threshold).min()), 'gap': float('inf'), 'ties': 0, 'guided_ties': 0}
    if e.shape[1] > 1:
        top = np.sort(e, axis=1)[:, -2:, :]         # [B, 2, HW]: second largest, largest
        e2, e1 = top[:, 0], top[:, 1]
        tie = e1 == e2
        out['ties'] = int(tie.sum())
        out['guided_ties'] = int((tie & (m > threshold)).sum())
        if (~tie).any():
            out['gap'] = float(((e1 - e2) / e1)[~tie].min())
    return out
