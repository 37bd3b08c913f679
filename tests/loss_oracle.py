"""fp64 restatement of every loss operator of hip_runtime.ops, and the inputs it is compared on (CPU only).

The oracle is oracle/losses.py, which is dtype-generic: it is called with float64 tensors made from the SAME float32
inputs, and autograd supplies the gradients.  Only what it lacks is added here: the eta-weighted entropy
(tests/fda_oracle.py) and the in-place after-images (`target * mask`, and the sigmoid of the masked angle channel of a
3-channel non-periodic loss).  `gt == 1` / `gt < 1` are decided on the float32 values (float32 -> float64 is exact).
Every `*_ref` takes a dtype, so that tests/test_host_loss_oracle.py can run the same restatement in float32 and show
that a float32 implementation meets the GPU bounds with room to spare.  The upstream gradient is 0.3 and no loss weight
is 1 (0.8 / 0.7 / 1.3 / 0.1, as in tests/test_gpu_loss_bits.py).

Why the inputs are built and not just drawn: almost every loss has a kink at which float32 and float64 may take
different branches (a clamped sigmoid switches its gradient between 0 and the map's largest value at |x| = ln 9999; an
L1 term switches sign at 0; the periodic residual wraps at +-pi/2).  Each builder below is pure numpy and seeded,
returns float32 / uint8 / int64 arrays, takes a `margin`, moves every value that lies nearer than `margin` to a kink to
the far side of it (it never drops one) and returns how many it moved.  The margin is 1e-3 in the quantity's own unit:
about 1e3 float32 ulps at these magnitudes.  `*_kinks` returns the distances, so that the host test can assert them.
Exempt from a kink are only the structures that are EXACTLY on it by construction and whose gradient is exactly 0 on
both sides: rows built with feat == target, a pair (j, j), a pair whose four coordinates are all masked out, an angle
whose prediction is clamped (no gradient passes, and the value is continuous).

A case's seed is the first one whose inputs pass accepted(): little moved, and the reference's own float32 arithmetic
within a tenth of the bounds of its float64 self.  Neither looks at a kernel."""
import functools
import math

import numpy as np
import torch

import fda_oracle
from oracle import losses as ol

UP = 0.3
W_FOCAL, W_L1, W_ANGLE, W_DIST = 0.8, 0.7, 1.3, 0.1
MARGIN = 1e-3
MOVED_SHARE = 1e-3
LN9999 = math.log(9999.0)
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))
ABOVE_ONE = np.nextafter(np.float32(1), np.float32(2))
F64, F32 = torch.float64, torch.float32


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _np(t):
    return t.detach().double().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def softmax_ref(kind, logits, dtype=F64, eta=None, gmap=None):
    """kind: 'entropy' | 'maxsq' | 'eta' (needs eta) -> {loss, grad} with the upstream UP; 'map' (needs gmap, the full
    upstream tensor) -> {out, grad}"""
    x = _t(logits, dtype).requires_grad_(True)
    if kind == 'map':
        out = ol.entropy_map(x)
        out.backward(_t(gmap, dtype))
        return {'out': _np(out), 'grad': _np(x.grad)}
    if kind == 'eta' and dtype == F64:
        loss, grad = fda_oracle.entropy_eta_loss(_t(logits), eta)
        return {'loss': loss.item(), 'grad': _np(grad) * UP}
    if kind == 'eta':
        v = torch.softmax(x, dim=1)
        e = -(v * torch.log2(v + 1e-30)).sum(dim=1) / math.log2(x.shape[1])
        loss = ((e ** 2 + 1e-30) ** eta).mean()
    else:
        loss = {'entropy': ol.entropy_loss, 'maxsq': ol.max_square_loss}[kind](x)
    (loss * UP).backward()
    return {'loss': loss.item(), 'grad': _np(x.grad)}


def focal_ref(logits, gt, dtype=F64):
    x = _t(logits, dtype).requires_grad_(True)
    prob = ol.clamped_sigmoid(x)
    loss = ol.focal(prob, _t(gt, dtype), W_FOCAL)
    (loss * UP).backward()
    return {'loss': loss.item(), 'prob': _np(prob), 'num_pos': float((gt == 1).sum()), 'grad': _np(x.grad)}


def l1_den(mask, ch=None):
    """the divisor the kernels keep: float32(expanded-mask sum) + float32(1e-4)"""
    n = int(mask.sum()) * (1 if mask.ndim == 3 else ch)
    return np.float32(n) + np.float32(1e-4)


def reg_target_after(mask, target, periodic):
    """`target` after the call: masked, and (3 channels, not periodic) the angle replaced by its sigmoid -> float64"""
    after = (target * mask[:, :, None].astype(np.float32)).astype(np.float64)
    if target.shape[2] == 3 and not periodic:
        after[:, :, 2] = _np(torch.sigmoid(_t(after[:, :, 2])))
    return after


def reg_l1_ref(feat, mask, ind, target, periodic, dtype=F64):
    x = _t(feat, dtype).requires_grad_(True)
    fn = ol.periodic_reg_l1 if periodic else ol.reg_l1
    loss = fn(x, _t(mask), _t(ind), _t(target, dtype), W_L1, W_ANGLE)
    (loss * UP).backward()
    return {'loss': loss.item(), 'grad': _np(x.grad), 'target_after': reg_target_after(mask, target, periodic)}


def kps_l1_ref(feat, mask, ind, target, pairs, use_l1, dtype=F64):
    x = _t(feat, dtype).requires_grad_(True)
    loss = ol.kps_l1(x, _t(mask), _t(ind), _t(target, dtype), W_L1, [tuple(p) for p in pairs] or None, W_DIST, use_l1)
    (loss * UP).backward()
    return {'loss': loss.item(), 'grad': _np(x.grad),
            'target_after': (target * mask.astype(np.float32)).astype(np.float64)}


def bce_ref(logits, label, dtype=F64):
    x = _t(logits, dtype).requires_grad_(True)
    loss = ol.advent_loss(x, label)
    (loss * UP).backward()
    return {'loss': loss.item(), 'grad': _np(x.grad)}


def detection_ref(out, batch, weights, dtype=F64):
    """DetectionLoss(**weights)(out, batch) -> {loss, stats, grads, hm_after, wh_after, reg_after[, kps_after]}"""
    leaves = {k: _t(v, dtype).requires_grad_(True) for k, v in out.items()}
    b = {k: _t(v, dtype) if v.dtype == np.float32 else _t(v) for k, v in batch.items()}
    periodic = weights.get('periodic', False)
    loss, stats, prob = ol.detection_loss(leaves, b, weights['hm_weight'], weights['wh_weight'], weights['off_weight'],
                                          weights.get('angle_weight', 1.0), periodic)
    res = {}
    if 'kps' in out:
        kp = ol.kps_l1(leaves['kps'], b['kp_reg_mask'], b['ind'], b['kps'], weights['kp_weight'],
                       [tuple(p) for p in weights['kp_indices']], weights['kp_distance_weight'],
                       weights['kp_distance_weight_l1'])
        loss = loss + kp
        stats = dict(stats, centernet_loss=loss, kp_loss=kp)
        res['kps_after'] = (batch['kps'] * batch['kp_reg_mask'].astype(np.float32)).astype(np.float64)
    (loss * UP).backward()
    res.update(loss=loss.item(), stats={k: v.item() for k, v in stats.items()},
               grads={k: _np(v.grad) for k, v in leaves.items()}, hm_after=_np(prob),
               wh_after=reg_target_after(batch['reg_mask'], batch['wh'], periodic),
               reg_after=reg_target_after(batch['reg_mask'], batch['reg'], False))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# kinks
# ---------------------------------------------------------------------------------------------------------------------
def gate_distance(x):
    """distance of every value from the clamp gate of the sigmoid, | |x| - ln 9999 |"""
    return np.abs(np.abs(np.asarray(x, np.float64)) - LN9999)


def _clear_gate(x, margin):
    """in place on a float32 array -> the elements moved (to 2 * margin OUTSIDE the bound, the sign kept)"""
    bad = gate_distance(x) < margin
    x[bad] = (np.sign(x[bad]) * (LN9999 + 2 * margin)).astype(np.float32)
    return bad


def _gather(feat, ind):
    """float64 [B, M, ch]"""
    B, ch = feat.shape[:2]
    flat = feat.reshape(B, ch, -1).astype(np.float64)
    return np.stack([flat[b][:, ind[b]].T for b in range(B)])


def _sig(x):
    return np.clip(1.0 / (1.0 + np.exp(-x)), 1e-4, 1 - 1e-4)


def _periodic_residual(pred_a, tg_a):
    pa = _sig(pred_a) * 2 * math.pi - math.pi
    return np.remainder((pa - np.deg2rad(tg_a)) - math.pi / 2, math.pi) - math.pi / 2


def _rows(plan_rows, shape):
    m = np.zeros(shape, bool)
    for b, r in plan_rows:
        m[b, r] = True
    return m


def reg_kinks(c):
    """-> {kink: distances (float64, 1-d) of the elements it applies to}"""
    feat, mask, ind, target, ch, periodic = c['feat'], c['mask'], c['ind'], c['target'], c['ch'], c['periodic']
    pred, tg = _gather(feat, ind), target.astype(np.float64)
    live = mask.astype(bool) & ~_rows(c['plan']['equal'], mask.shape)       # masked in, not built exactly equal
    nl = 2 if ch == 3 else ch
    out = {'l1': np.abs(pred[..., :nl] - tg[..., :nl])[live].ravel()}
    if ch == 3:
        on = mask.astype(bool)
        pa, ta = pred[..., 2], tg[..., 2]
        out['gate_pred'] = gate_distance(pa[on])
        passes = np.abs(pa) < LN9999
        if periodic:
            r = _periodic_residual(pa[on], ta[on])
            out['periodic_zero'], out['periodic_wrap'] = np.abs(r), math.pi / 2 - np.abs(r)
        else:
            out['gate_target'] = gate_distance(ta[on])
            out['angle'] = np.abs(_sig(pa) - _sig(ta))[live & passes]
    return out


def kps_pair_state(c):
    """-> (pd - td, dx, dy, which pairs count) as float64 [B, M, P]; a pair counts unless it is (j, j), lies in a row
    built exactly equal, or has its four coordinates masked out"""
    feat, mask, ind, target, pairs, use_l1 = c['feat'], c['mask'], c['ind'], c['target'], c['pairs'], c['use_l1']
    m = mask.astype(np.float64)
    pred, tg = _gather(feat, ind) * m, target.astype(np.float64) * m
    a, b = np.array(pairs)[:, 0], np.array(pairs)[:, 1]
    dx, dy = pred[..., 2 * a] - pred[..., 2 * b], pred[..., 2 * a + 1] - pred[..., 2 * b + 1]
    tx, ty = tg[..., 2 * a] - tg[..., 2 * b], tg[..., 2 * a + 1] - tg[..., 2 * b + 1]
    if use_l1:
        pd, td = np.abs(dx) + np.abs(dy), np.abs(tx) + np.abs(ty)
    else:
        pd, td = np.sqrt(dx * dx + dy * dy + 1e4), np.sqrt(tx * tx + ty * ty + 1e4)
    any_in = (m[..., 2 * a] + m[..., 2 * a + 1] + m[..., 2 * b] + m[..., 2 * b + 1]) > 0
    counts = any_in & (a != b)[None, None, :] & ~_rows(c['plan']['equal'], mask.shape[:2])[:, :, None]
    x_in, y_in = (m[..., 2 * a] + m[..., 2 * b]) > 0, (m[..., 2 * a + 1] + m[..., 2 * b + 1]) > 0
    return pd - td, dx, dy, counts, x_in, y_in


def kps_kinks(c):
    pred, tg = _gather(c['feat'], c['ind']), c['target'].astype(np.float64)
    live = c['mask'].astype(bool) & ~_rows(c['plan']['equal'], c['mask'].shape[:2])[:, :, None]
    out = {'l1': np.abs(pred - tg)[live].ravel()}
    if c['pairs']:
        diff, dx, dy, counts, x_in, y_in = kps_pair_state(c)
        out['pair'] = np.abs(diff)[counts]
        if c['use_l1']:
            out['pair_dx'] = np.concatenate([np.abs(dx)[counts & x_in], np.abs(dy)[counts & y_in]])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softmax_case(shape, seed):
    """The pixels are, a quarter each (pixel number mod 4 after a shuffle): ordinary N(0, 3^2); one channel ahead by
    60..120, so that the others underflow; all channels equal; ordinary plus a common offset of 1e4.  `gmap` is the full
    upstream tensor of entropy_map, a tenth of it zeros.  No kink: nothing is moved."""
    B, C, H, W = shape
    rs = np.random.RandomState(seed)
    n = B * H * W
    x = (rs.standard_normal((n, C)) * 3).astype(np.float32)
    kind = rs.permutation(n) % 4
    ahead = np.nonzero(kind == 1)[0]
    x[ahead, rs.randint(0, C, ahead.size)] += rs.uniform(60, 120, ahead.size).astype(np.float32)
    x[kind == 2] = x[kind == 2][:, :1]
    x[kind == 3] += np.float32(1e4)
    gmap = (rs.standard_normal(shape) * UP).astype(np.float32)
    gmap[rs.random_sample(shape) < 0.1] = 0
    logits = np.ascontiguousarray(x.reshape(B, H, W, C).transpose(0, 3, 1, 2))
    return {'logits': logits, 'gmap': gmap, 'kind': kind.reshape(B, H, W), 'moved': 0, 'total': logits.size}


PLANTED_LOGITS = (9.3, -9.3, 20.0, -20.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def focal_case(shape, peaks, seed, margin=MARGIN):
    """logits N(0, 4^2) with +-9.3, +-20, +-100 planted; gt uniform in [0, 1) with 0, the float just below 1, the float
    just above 1 and `peaks` exact 1.0 planted.  One peak sits on the +20 logit and one on the -100 logit (clamped: no
    gradient), the value above 1 on an ordinary logit (neither branch: no loss, no gradient)."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    logits = (rs.standard_normal(n) * 4).astype(np.float32)
    gt = rs.random_sample(n).astype(np.float32)
    gt[gt >= 1.0] = 0.5                                   # a double just below 1 may round up to 1.0f
    order = rs.permutation(n)
    at = {}
    if n >= 12:
        logits[order[:6]] = PLANTED_LOGITS
        gt[order[0]], gt[order[3]], gt[order[6]], gt[order[7]], gt[order[8]] = 0.0, BELOW_ONE, ABOVE_ONE, BELOW_ONE, 0.0
        gt[order[[9, 2, 5, 10, 11][:peaks]]] = 1.0
        at = {'above_one': int(order[6]), 'below_one': int(order[7]), 'planted': order[:6].copy()}
    else:
        assert peaks <= n
        gt[order[:peaks]] = 1.0
    moved = int(_clear_gate(logits, margin).sum())
    assert int((gt == 1.0).sum()) == peaks
    return {'logits': logits.reshape(shape), 'gt': gt.reshape(shape), 'peaks': peaks, 'at': at, 'moved': moved,
            'total': n}


def plant_rows(rs, B, HW, M, mask_kind, per_channel=0):
    """`ind` drawn with replacement, and (from M = 4) planted: image 0 rows 0 and 1 share cell 0, image 0 rows 2 and 3 are
    the rows built with feat == target, three rows share cell HW - 1 (image 1 rows 0..2, or image 0 rows 4..6 when there
    is one image).  The mask ('third': a third zeros, the planted rows in; 'ones'; 'zeros') is [B, M], or with
    per_channel = ch [B, M, ch] with row (0, 1) half masked (its second channel out)."""
    ind = rs.randint(0, HW, (B, M)).astype(np.int64)
    plan = {'pair': [], 'triple': [], 'equal': []}
    if M >= 4:
        ind[0, 0] = ind[0, 1] = 0
        plan['pair'], plan['equal'] = [(0, 0), (0, 1)], [(0, 2), (0, 3)]
        b, r = (1, 0) if B > 1 else (0, 4)
        if r + 3 <= M:
            ind[b, r:r + 3] = HW - 1
            plan['triple'] = [(b, r), (b, r + 1), (b, r + 2)]
    shape = (B, M, per_channel) if per_channel else (B, M)
    if mask_kind == 'third':
        mask = (rs.random_sample(shape) > 1.0 / 3).astype(np.uint8)
        for b, r in plan['pair'] + plan['triple'] + plan['equal']:
            mask[b, r] = 1
        if per_channel and plan['pair']:
            mask[0, 1, 1] = 0
        if M >= 4 and (B - 1, M - 1) not in plan['pair'] + plan['triple'] + plan['equal']:
            mask[B - 1, M - 1] = 0                          # (with M = 4 it is the one row that is not planted)
    else:
        mask = np.full(shape, 1 if mask_kind == 'ones' else 0, np.uint8)
    return ind, mask, plan


def _finish(c, kinks, fix, margin):
    """the loop every masked-L1 builder ends with: while a kink is nearer than margin, fix(c) moves the offenders (it
    returns how many); -> c with 'moved' and 'total'"""
    moved = 0
    for _ in range(16):
        n = fix(c)
        if not n:
            break
        moved += n
    short = {k: float(d.min()) for k, d in kinks(c).items() if d.size and d.min() < margin}
    assert not short, short
    c['moved'], c['total'] = moved, c['target'].size
    return c


def _cell(c, b, r):
    return np.unravel_index(c['ind'][b, r], c['feat'].shape[2:])


def _fix_l1(c, channels, margin, live):
    """L1 elements nearer than margin to pred == target: the target goes to 2 * margin from the prediction, on its side"""
    pred = _gather(c['feat'], c['ind'])[..., channels]
    d = pred - c['target'].astype(np.float64)[..., channels]
    bad = (np.abs(d) < margin) & live
    tgt = c['target'][..., channels]
    tgt[bad] = (pred[bad] - np.where(d[bad] >= 0, 1.0, -1.0) * 2 * margin).astype(np.float32)
    c['target'][..., channels] = tgt
    return int(bad.sum())


@functools.lru_cache(maxsize=None)
def reg_case(geom, ch, periodic, mask_kind, seed, margin=MARGIN):
    return reg_case_on(geom, ch, periodic, mask_kind, seed, margin)


def reg_case_on(geom, ch, periodic, mask_kind, seed, margin=MARGIN, rows=None):
    """feat N(0, 5^2), target N(0, 40^2); 3 channels: angle predictions N(0, 3^2) with 9.3, -9.3, 20, -20 at the cells of
    the last image's last masked-in rows that are not planted, angle targets N(0, 3^2) with +-12 on the two rows of cell 0
    (plain) or uniform in +-720 degrees (periodic).  The two rows of cell 0 have opposite signs of pred - target in
    channel 0.  `rows`: (ind, mask, plan) of another loss of the same batch."""
    B, H, W, M = geom
    rs = np.random.RandomState(seed)
    ind, mask, plan = rows if rows is not None else plant_rows(rs, B, H * W, M, mask_kind)
    feat = (rs.standard_normal((B, ch, H, W)) * 5).astype(np.float32)
    target = (rs.standard_normal((B, M, ch)) * 40).astype(np.float32)
    c = {'feat': feat, 'mask': mask, 'ind': ind, 'target': target, 'ch': ch, 'periodic': periodic, 'plan': plan,
         'geom': geom, 'mask_kind': mask_kind}
    planted = set(plan['pair'] + plan['triple'] + plan['equal'])
    if ch == 3:
        feat[:, 2] = (rs.standard_normal((B, H, W)) * 3).astype(np.float32)
        target[:, :, 2] = rs.uniform(-720, 720, (B, M)) if periodic else rs.standard_normal((B, M)) * 3
        free = [(B - 1, r) for r in range(M - 1, -1, -1) if (B - 1, r) not in planted and mask[B - 1, r]][:4]
        free = free if M > 1 else []
        if not free and plan['triple'] and mask_kind != 'zeros':
            free = plan['triple'][:1]                       # M = 4: the shared cell's angle is clamped, its sizes are not
        for (b, r), v in zip(free, (9.3, -9.3, 20.0, -20.0)):
            feat[(b, 2) + _cell(c, b, r)] = v
        c['extreme_rows'] = free
    if plan['pair']:
        p0 = feat[(0, 0) + _cell(c, 0, 0)]
        target[0, 0, 0], target[0, 1, 0] = p0 + 3, p0 - 3
        if ch == 3 and not periodic:
            target[0, 0, 2], target[0, 1, 2] = 12.0, -12.0
    nl = 2 if ch == 3 else ch
    for b, r in plan['equal']:
        target[b, r, :nl if periodic else ch] = feat[(b, slice(0, nl if periodic else ch)) + _cell(c, b, r)]
    live = mask.astype(bool) & ~_rows(plan['equal'], mask.shape)

    def fix(c):
        n = _fix_l1(c, slice(0, nl), margin, live[:, :, None])
        if ch < 3:
            return n
        on = mask.astype(bool)
        pa = _gather(feat, ind)[..., 2]
        for b, r in zip(*np.nonzero(on & (gate_distance(pa) < margin))):        # the prediction at the clamp gate
            cell = (b, 2) + _cell(c, b, r)
            if gate_distance(feat[cell]) < margin:                              # (a shared cell is moved once)
                feat[cell] = np.sign(feat[cell]) * (LN9999 + 2 * margin)
                n += 1
        pa, ta = _gather(feat, ind)[..., 2], target[..., 2].astype(np.float64)
        if periodic:
            r = _periodic_residual(pa, ta)
            bad = on & ((np.abs(r) < margin) | (math.pi / 2 - np.abs(r) < margin))
            target[..., 2][bad] += np.float32(1.0)                              # one degree: 17 margins
        else:
            gate = on & (gate_distance(ta) < margin)
            target[..., 2][gate] = (np.sign(ta[gate]) * (LN9999 + 2 * margin)).astype(np.float32)
            ta = target[..., 2].astype(np.float64)
            bad = live & (np.abs(pa) < LN9999) & (np.abs(_sig(pa) - _sig(ta)) < margin)
            target[..., 2][bad] = (pa[bad] - 3 * np.where(pa[bad] >= 0, 1.0, -1.0)).astype(np.float32)
            bad = bad | gate
        return n + int(bad.sum())

    return _finish(c, reg_kinks, fix, margin)


def pairs_for(J, P):
    """P = 1: the pair (0, J - 1).  P = 5: joint 0 in three of the pairs, one pair (j, j).  J = 1 has the pair (0, 0) only."""
    if P == 0:
        return ()
    if J == 1:
        return ((0, 0),) * P
    if P == 1:
        return ((0, J - 1),)
    return ((0, 1), (0, J - 1), (J // 2 + 1 if J > 3 else J - 1, 0), (1, 1), (1, J - 1))[:P]


@functools.lru_cache(maxsize=None)
def kps_case(geom, J, P, use_l1, seed, margin=MARGIN):
    return kps_case_on(geom, J, P, use_l1, seed, margin)


def kps_case_on(geom, J, P, use_l1, seed, margin=MARGIN, rows=None):
    """feat N(0, 8^2), target N(0, 10^2) (the two pair lengths are of one size: pd - td takes both signs); the mask is
    per channel with a third zeros, so joints are half masked; the rows of plant_rows.  `rows`: (ind, [B, M] mask, plan)
    of the batch's other losses -- the keypoint mask is then drawn inside those rows."""
    B, H, W, M = geom
    ch = 2 * J
    rs = np.random.RandomState(seed)
    if rows is None:
        ind, mask, plan = plant_rows(rs, B, H * W, M, 'third', ch)
    else:
        ind, row_mask, plan = rows
        mask = ((rs.random_sample((B, M, ch)) > 1.0 / 3) & row_mask[:, :, None].astype(bool)).astype(np.uint8)
        for b, r in plan['pair'] + plan['triple'] + plan['equal']:
            mask[b, r] = 1
    feat = (rs.standard_normal((B, ch, H, W)) * 8).astype(np.float32)
    target = (rs.standard_normal((B, M, ch)) * 10).astype(np.float32)
    c = {'feat': feat, 'mask': mask, 'ind': ind, 'target': target, 'pairs': pairs_for(J, P), 'use_l1': use_l1,
         'plan': plan, 'geom': geom, 'J': J}
    if plan['pair']:
        p0 = feat[(0, 0) + _cell(c, 0, 0)]
        target[0, 0, 0], target[0, 1, 0] = p0 + 3, p0 - 3
    for b, r in plan['equal']:
        target[b, r] = feat[(b, slice(None)) + _cell(c, b, r)]
    live = mask.astype(bool) & ~_rows(plan['equal'], mask.shape[:2])[:, :, None]
    turn = [0]

    def fix(c):
        n = _fix_l1(c, slice(None), margin, live)
        if not c['pairs']:
            return n
        pa = np.array(c['pairs'])
        diff, dx, dy, counts, x_in, y_in = kps_pair_state(c)
        for b, r, p in zip(*np.nonzero(counts & (np.abs(diff) < margin))):       # pd == td: a masked-in target moves
            cs = [2 * pa[p, 0], 2 * pa[p, 0] + 1, 2 * pa[p, 1], 2 * pa[p, 1] + 1]
            cs = [k for k in cs if mask[b, r, k]]
            target[b, r, cs[turn[0] % len(cs)]] += np.float32(0.5)
            n += 1
        if use_l1:                                                              # |dx|, |dy| at 0: a masked-in prediction
            for d, d_in, off in ((dx, x_in, 0), (dy, y_in, 1)):
                for b, r, p in zip(*np.nonzero(counts & d_in & (np.abs(d) < margin))):
                    k = 2 * pa[p, 0] + off if mask[b, r, 2 * pa[p, 0] + off] else 2 * pa[p, 1] + off
                    feat[(b, k) + _cell(c, b, r)] += np.float32(8 * margin * (1 + turn[0]))
                    n += 1
        turn[0] += 1
        return n

    return _finish(c, kps_kinks, fix, margin)


@functools.lru_cache(maxsize=None)
def bce_case(n, seed):
    """logits N(0, 3^2) with +-50, +-100 and 0 planted (from n = 70).  No kink: max(x, 0) - x * label + log1p(exp(-|x|))
    has none at 0."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal(n) * 3).astype(np.float32)
    if n >= 70:
        x[rs.permutation(n)[:5]] = (50.0, -50.0, 100.0, -100.0, 0.0)
    return {'logits': x.reshape(n, 1, 1, 1), 'moved': 0, 'total': n}


def detection_case(name, seed=0):
    """One batch for the DetectionLoss module: (2, 6, 5, 4) geometry, 3 classes, every loss on the same planted rows
    (two rows on cell 0, three on cell HW - 1).  name: 'plain' | 'rotated' | 'periodic' | 'keypoints'
    -> (head outputs, batch, DetectionLoss kwargs, the cases it was put together from)"""
    geom = (2, 6, 5, 4)
    B, H, W, M = geom
    wh_ch, periodic = (3, name == 'periodic') if name in ('rotated', 'periodic') else (2, False)
    rows = plant_rows(np.random.RandomState(900 + seed), B, H * W, M, 'third')
    wh = reg_case_on(geom, wh_ch, periodic, 'third', 901 + seed, rows=rows)
    reg = reg_case_on(geom, 2, False, 'third', 902 + seed, rows=rows)
    hm = focal_case((B, 3, H, W), 5, 903 + seed)
    out = {'hm': hm['logits'], 'wh': wh['feat'], 'reg': reg['feat']}
    batch = {'hm': hm['gt'], 'reg_mask': rows[1], 'ind': rows[0], 'wh': wh['target'], 'reg': reg['target']}
    weights = dict(hm_weight=W_FOCAL, wh_weight=W_L1, off_weight=1.1, angle_weight=W_ANGLE, periodic=periodic)
    parts = {'hm': hm, 'wh': wh, 'reg': reg}
    if name == 'keypoints':
        kp = kps_case_on(geom, 3, 5, False, 904 + seed, rows=rows)
        out['kps'], batch['kps'], batch['kp_reg_mask'] = kp['feat'], kp['target'], kp['mask']
        weights.update(kp_weight=0.6, kp_indices=[list(p) for p in kp['pairs']], kp_distance_weight=W_DIST,
                       kp_distance_weight_l1=False)
        parts['kps'] = kp
    return out, batch, weights, parts


# ---------------------------------------------------------------------------------------------------------------------
# the cases (the smallest shapes that reach each hazard) -- shared by the host file, the GPU file and the fuzz test
# ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_SHAPES = ((1, 2, 1, 1), (2, 3, 5, 7), (3, 80, 9, 31), (1, 2, 725, 725))     # 725^2: past both grid caps
ETAS = (1.0, 1.5, 2.0)
FOCAL_CASES = tuple((shape, peaks) for shape in ((1, 1, 1, 1), (2, 1, 5, 7), (3, 1, 9, 31), (1, 1, 725, 725))
                    for peaks in (0, 1, 5) if peaks <= shape[0] * shape[2] * shape[3])
L1_GEOMS = ((1, 1, 1, 1), (2, 6, 5, 4), (3, 12, 11, 100))                            # 300 rows: two trips of one workgroup
REG_CASES = tuple((g, ch, periodic, mk) for g in L1_GEOMS for ch, periodic in ((1, False), (2, False), (3, False), (3, True))
                  for mk in ('third', 'ones', 'zeros'))
KPS_CASES = tuple((g, J, P, use_l1) for g in ((2, 6, 5, 4), (3, 12, 11, 20)) for J in (1, 3, 17) for P in (0, 1, 5)
                  for use_l1 in (False, True))
BCE_NS = (1, 70, 1600, 100003)
BCE_LABELS = (0, 1, 0.9)
DETECTION_CASES = ('plain', 'rotated', 'periodic', 'keypoints')


def misses(got, want, share=1.0, log=None, what=''):
    """The project's bounds, scalars |a - b| <= 1e-5 * max(1, |b|), gradients and maps max|a - b| <= 1e-4 * max|b|, times
    `share` -> [(key, error, allowed)] of the entries of `got` that miss them (nested dicts are walked).  log(text)
    receives every entry's error as a share of what the bound allows at share = 1."""
    out = []
    for k, b in want.items():
        a = got[k]
        if isinstance(b, dict):
            out += misses(a, b, share, log, what + k + '.')
            continue
        if np.ndim(b) == 0:
            err, allowed = abs(float(a) - float(b)), 1e-5 * max(1.0, abs(float(b)))
        else:
            a = np.asarray(a, np.float64)
            assert a.shape == b.shape, (what + k, a.shape, b.shape)
            err, allowed = np.abs(a - b).max(), 1e-4 * np.abs(b).max()
        if log:
            log('%s%s: error %.3e, the bound allows %.3e (%s of it)'
                % (what, k, err, allowed, '%.4f' % (err / allowed) if allowed else 'exact'))
        if not err <= share * allowed:
            out.append((what + k, err, share * allowed))
    return out


def case_seed(*key):
    import zlib
    return zlib.crc32(repr(key).encode()) % 1000003


def accepted(build, ref, *key):
    """The first seed from case_seed(key) on whose inputs (1) needed at most MOVED_SHARE of their elements moved and (2)
    let the reference's own arithmetic in float32 (`ref(c, F32)`) stay within a TENTH of the bounds of its float64 self.
    Both depend on the inputs and the reference alone.  (2) is about conditioning, not about a kink: float32 keeps
    1 - sigmoid(x) to 6e-8 absolute, which for x in (5, ln 9999) is up to 6e-4 of its value -- on 70 pixels one such
    logit under a heavy (1 - gt)^4 moves the focal loss by 1e-5 of itself, in the reference as in any float32 kernel
    that returns the probabilities in float32."""
    seed = case_seed(*key)
    for k in range(64):
        c = build(seed + k)
        if c['moved'] > MOVED_SHARE * c['total']:
            continue
        want = ref(c, F64)
        if not misses(ref(c, F32), want, 0.1):
            c['seed'], c['want'] = seed + k, want            # the float64 reference, computed once
            return c
    raise AssertionError('no acceptable seed for %r' % (key,))


def softmax_refs(c, dtype=F64):
    r = {k: softmax_ref(k, c['logits'], dtype) for k in ('entropy', 'maxsq')}
    r['map'] = softmax_ref('map', c['logits'], dtype, gmap=c['gmap'])
    r.update({'eta%g' % e: softmax_ref('eta', c['logits'], dtype, eta=e) for e in ETAS})
    return r


def focal_refs(c, dtype=F64):
    return focal_ref(c['logits'], c['gt'], dtype)


def reg_refs(c, dtype=F64):
    return reg_l1_ref(c['feat'], c['mask'], c['ind'], c['target'], c['periodic'], dtype)


def kps_refs(c, dtype=F64):
    return kps_l1_ref(c['feat'], c['mask'], c['ind'], c['target'], c['pairs'], c['use_l1'], dtype)


def bce_refs(c, dtype=F64):
    return {'label%g' % l: bce_ref(c['logits'], l, dtype) for l in BCE_LABELS}


@functools.lru_cache(maxsize=None)
def softmax(shape):
    return accepted(lambda s: softmax_case(shape, s), softmax_refs, 'softmax', shape)


@functools.lru_cache(maxsize=None)
def focal(shape, peaks):
    return accepted(lambda s: focal_case(shape, peaks, s), focal_refs, 'focal', shape, peaks)


@functools.lru_cache(maxsize=None)
def reg(geom, ch, periodic, mask_kind):
    return accepted(lambda s: reg_case(geom, ch, periodic, mask_kind, s), reg_refs, 'reg', geom, ch, periodic, mask_kind)


@functools.lru_cache(maxsize=None)
def kps(geom, J, P, use_l1):
    return accepted(lambda s: kps_case(geom, J, P, use_l1, s), kps_refs, 'kps', geom, J, P, use_l1)


@functools.lru_cache(maxsize=None)
def bce(n):
    return accepted(lambda s: bce_case(n, s), bce_refs, 'bce', n)


@functools.lru_cache(maxsize=None)
def detection(name):
    """detection_case(name, seed) at the first seed that needs nothing moved and passes accepted()'s float32 check"""
    for seed in range(64):
        out, batch, w, parts = detection_case(name, seed)
        if any(c['moved'] for c in parts.values()):
            continue
        want = detection_ref(out, batch, w)
        if not misses(detection_ref(out, batch, w, F32), want, 0.1):
            parts['want'] = want
            return out, batch, w, parts
    raise AssertionError('no acceptable seed for %r' % name)


def fuzz_id(case):
    return '%s-B%dC%dH%dW%dM%d-%d' % case


def fuzz_case(case):
    """-> (the family's reference function, the built inputs) of one draw of fuzz_cases()"""
    mode, B, C, H, W, M, s = case
    if mode == 'softmax':
        return softmax_refs, softmax_case((B, C, H, W), s)
    if mode == 'focal':
        return focal_refs, focal_case((B, C, H, W), M, s)
    if mode == 'kps':
        return kps_refs, kps_case((B, H, W, M), C, 5, bool(s & 1), s)
    return reg_refs, reg_case((B, H, W, M), C, mode == 'periodic', 'third', s)


@functools.lru_cache(maxsize=None)
def fuzz_cases(n=20, seed=4242):
    """n seeded draws (mode, B, C or ch or J, H, W, M or peaks, seed) for tests/test_gpu_fuzz.py, four of each mode; a
    draw that accepted() would not take is drawn again (that depends on the inputs and the reference alone)."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        mode = ('softmax', 'focal', 'reg', 'periodic', 'kps')[len(out) % 5]
        B, H, W = int(rs.randint(1, 4)), int(rs.randint(1, 24)), int(rs.randint(1, 24))
        M, s = int(rs.randint(1, 40)), int(rs.randint(1 << 20))
        if mode == 'softmax':
            case = (mode, B, int(rs.choice([2, 3, 6, 20, 80])), H, W, 0, s)
        elif mode == 'focal':
            case = (mode, B, int(rs.randint(1, 7)), H, W, int(rs.randint(0, 6)), s)
            if case[5] > B * case[2] * H * W:
                continue
        elif mode == 'kps':
            case = (mode, B, int(rs.choice([1, 2, 3, 5, 17])), H, W, M, s)
        else:
            case = (mode, B, 3 if mode == 'periodic' else int(rs.randint(1, 4)), H, W, M, s)
        refs, c = fuzz_case(case)
        if c['moved'] > MOVED_SHARE * c['total'] or misses(refs(c, F32), refs(c, F64), 0.1):
            continue
        out.append(case)
    return out
