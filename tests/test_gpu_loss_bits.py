"""Bit pins of every loss operator of hip_runtime.ops, forward and backward.

tests/golden/loss_bits.npz was recorded by run_all() below with the library and ops.py of the commit BEFORE the loss
kernels were folded onto one softmax walk, one reduction tail and one masked-L1 scaffold (profiles/loss_dedupe_ab.txt),
in two separate processes whose recordings were equal.  The library is built with -ffp-contract=off, so a helper that
keeps the order of operations gives the same bits: a difference here means an expression was reordered.  Find it; never
re-record from the code under test.

Beyond the golden sizes of tests/test_gpu_losses.py the cases reach: partial blocks and idle lanes, the 1024 x 256
(forward) and 2048 x 256 (backward) grid caps, more rows than one trip of the single-workgroup kernels, the bad-index
rule (loss NaN, row absent from the gradient, no fault) and the focal num_pos == 0 branch.  Scatter targets are distinct
within an image and a keypoint cell gets at most two addends, so no result depends on the order of atomics."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loss_bits.npz')
FAMILIES = ('softmax', 'focal', 'regl1', 'kpsl1', 'bce', 'sigmoid')
SHAPES = ((2, 2, 5, 7), (3, 6, 9, 31), (1, 2, 725, 725))      # 70 / 837 / 525,625 pixels: see the module docstring
DIGEST_ABOVE = 1 << 16                                          # larger arrays are stored as head, tail and bit sum
UP = 0.3                                                        # the upstream gradient is not 1


def _put(res, key, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    if a.size <= DIGEST_ABOVE:
        res[key] = a
        return
    flat = a.reshape(-1)
    res[key + '.head'], res[key + '.tail'] = flat[:16].copy(), flat[-16:].copy()
    res[key + '.bitsum'] = np.array([flat.view(np.int32).astype(np.int64).sum()], np.int64)


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _masked_l1_batch(rs, B, H, W, M, ch, mask_per_channel, bad_ind):
    """feat, mask (u8, about a third zero), ind (a permutation prefix per image: distinct cells), target"""
    HW = H * W
    feat = (rs.standard_normal((B, ch, H, W)) * 5).astype(np.float32)
    mask = (rs.random_sample((B, M, ch) if mask_per_channel else (B, M)) > 1.0 / 3).astype(np.uint8)
    ind = np.stack([rs.permutation(HW)[:M] for _ in range(B)]).astype(np.int64)
    target = (rs.standard_normal((B, M, ch)) * 40).astype(np.float32)
    if bad_ind:
        ind[0, 1], ind[1, 2] = HW, -1
        mask[0, 1], mask[1, 2] = 1, 1
    return feat, mask, ind, target


def run_all(families=FAMILIES, inputs=None):
    """Builds every input from seeded RandomStates, runs every loss operator forward and backward (targets cloned per
    call: the operators mask them in place) -> {name: array}.  `inputs`, a dict, receives mask and ind of the masked-L1
    cases (they are not part of the recording)."""
    from hip_runtime import ops
    res = {}
    if 'softmax' in families:
        for shape in SHAPES:
            tag = 'softmax/%dx%dx%dx%d/' % shape
            rs = np.random.RandomState(101 + shape[1] * shape[3])
            logits = (rs.standard_normal(shape) * 3).astype(np.float32)
            gmap = (rs.standard_normal(shape) * UP).astype(np.float32)
            for name, fn in (('entropy', ops.entropy_loss), ('maxsq', ops.max_square_loss),
                             ('eta', lambda t: ops.entropy_eta_loss(t, 1.5))):
                x = _dev(logits, True)
                loss = fn(x)
                (loss * UP).backward()
                _put(res, tag + name + '.loss', loss.reshape(1))
                _put(res, tag + name + '.grad', x.grad)
            x = _dev(logits, True)
            em = ops.entropy_map(x)
            em.backward(_dev(gmap))                              # the map's backward takes a full upstream tensor
            _put(res, tag + 'map.out', em)
            _put(res, tag + 'map.grad', x.grad)
    if 'focal' in families:
        for shape, peaks in [(s, 5) for s in SHAPES] + [(SHAPES[0], 0)]:
            tag = 'focal/%dx%dx%dx%d/peaks%d/' % (shape + (peaks,))
            rs = np.random.RandomState(202 + shape[1] * shape[3] + peaks)
            logits = (rs.standard_normal(shape) * 4).astype(np.float32)     # |x| > 9.2 occurs: both clamp bounds bite
            gt = rs.random_sample(shape).astype(np.float32)
            gt[gt >= 1.0] = 0.5                                             # a double just below 1 may round up to 1.0f
            gt.reshape(-1)[rs.permutation(gt.size)[:peaks]] = 1.0
            assert int((gt == 1.0).sum()) == peaks
            x = _dev(logits, True)
            loss, prob, num_pos = ops.focal_loss(x, _dev(gt), weight=0.8, return_den=True)
            (loss * UP).backward()
            _put(res, tag + 'loss', loss.reshape(1))
            _put(res, tag + 'num_pos', num_pos.reshape(1))
            _put(res, tag + 'prob', prob)
            _put(res, tag + 'grad', x.grad)
    if 'regl1' in families:
        cases = [(2, False, (2, 6, 5, 4), False), (2, False, (2, 6, 5, 4), True)]
        cases += [(3, periodic, g, False) for periodic in (False, True) for g in ((2, 6, 5, 4), (3, 12, 11, 100))]
        for n, (ch, periodic, (B, H, W, M), bad) in enumerate(cases):
            tag = 'regl1/ch%d_%s_%dx%dx%dx%d%s/' % (ch, 'periodic' if periodic else 'plain', B, H, W, M,
                                                   '_badind' if bad else '')
            feat, mask, ind, target = _masked_l1_batch(np.random.RandomState(303 + n), B, H, W, M, ch, False, bad)
            if inputs is not None:
                inputs[tag + 'mask'], inputs[tag + 'ind'] = mask, ind
            x, tg = _dev(feat, True), _dev(target)
            loss, den = ops.reg_l1_loss(x, _dev(mask), _dev(ind), tg, periodic=periodic, weight=0.7, angle_weight=1.3,
                                        return_den=True)
            (loss * UP).backward()
            _put(res, tag + 'loss', loss.reshape(1))
            _put(res, tag + 'den', den.reshape(1))
            _put(res, tag + 'target_after', tg)
            _put(res, tag + 'grad', x.grad)
    if 'kpsl1' in families:
        J = 3
        cases = [(g, P, use_l1, False) for g in ((2, 6, 5, 4), (3, 12, 11, 20)) for P in (0, 1) for use_l1 in (False, True)]
        cases.append(((2, 6, 5, 4), 1, False, True))
        for n, ((B, H, W, M), P, use_l1, bad) in enumerate(cases):
            tag = 'kpsl1/%dx%dx%dx%d_P%d_%s%s/' % (B, H, W, M, P, 'l1' if use_l1 else 'l2', '_badind' if bad else '')
            feat, mask, ind, target = _masked_l1_batch(np.random.RandomState(404 + n), B, H, W, M, 2 * J, True, bad)
            # one pair: no joint is in two pairs, so a cell gets at most two addends (two floats onto zero commute)
            pairs = torch.tensor([[0, 2]], dtype=torch.int32, device=DEV) if P else None
            if inputs is not None:
                inputs[tag + 'mask'], inputs[tag + 'ind'] = mask, ind
            x, tg = _dev(feat, True), _dev(target)
            loss, den = ops.kps_l1_loss(x, _dev(mask), _dev(ind), tg, pairs=pairs, use_l1=use_l1, weight=0.7,
                                        distance_weight=0.1, return_den=True)
            (loss * UP).backward()
            _put(res, tag + 'loss', loss.reshape(1))
            _put(res, tag + 'den', den.reshape(1))
            _put(res, tag + 'target_after', tg)
            _put(res, tag + 'grad', x.grad)
    if 'bce' in families:
        for shape in ((2, 1, 5, 7), (4, 1, 20, 20)):
            logits = (np.random.RandomState(505 + shape[0]).standard_normal(shape) * 3).astype(np.float32)
            for label in (0, 1):
                tag = 'bce/%dx%dx%dx%d/label%d/' % (shape + (label,))
                x = _dev(logits, True)
                loss = ops.bce_with_logits_const(x, label)
                (loss * UP).backward()
                _put(res, tag + 'loss', loss.reshape(1))
                _put(res, tag + 'grad', x.grad)
    if 'sigmoid' in families:
        x = torch.tensor([-20.0, -9.3, -1.0, 0.0, 3.0, 9.3, 20.0], device=DEV)
        y = ops.sigmoid_clamp_(x)
        _put(res, 'sigmoid/in_place', x)
        _put(res, 'sigmoid/clamped', y)
    torch.cuda.synchronize()
    return res


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.int32), b.view(np.int32)) if a.dtype == np.float32 else np.array_equal(a, b)


@pytest.mark.parametrize('family', FAMILIES)
def test_loss_bits_are_those_of_the_recording(family):
    want = np.load(FIXTURE, allow_pickle=False)
    keys = sorted(k for k in want.files if k.startswith(family + '/'))
    got = run_all((family,))
    assert keys and sorted(got) == keys, (sorted(set(got) ^ set(keys)))
    differ = [k for k in keys if not _same_bits(got[k], want[k])]
    assert not differ, ('%d of %d arrays differ in bits from the recording (%s): %s'
                        % (len(differ), len(keys), str(want['recorded_with']), differ))


def test_bad_index_poisons_the_loss_and_skips_the_row():
    """An `ind` outside [0, HW): the forward reads cell 0 and returns NaN, the backward leaves the row out."""
    inputs = {}
    got = run_all(('regl1', 'kpsl1'), inputs)
    for tag in ('regl1/ch2_plain_2x6x5x4_badind/', 'kpsl1/2x6x5x4_P1_l2_badind/'):
        assert np.isnan(got[tag + 'loss']).all() and np.isfinite(got[tag + 'den']).all()
        grad, mask, ind = got[tag + 'grad'], inputs[tag + 'mask'], inputs[tag + 'ind']
        assert np.isfinite(grad).all()
        valid = (ind >= 0) & (ind < 30)
        assert (~valid).sum() == 2 and all(mask[b, m].all() for b, m in zip(*np.nonzero(~valid)))
        ch = grad.shape[1]
        per_row = mask.astype(bool) if mask.ndim == 3 else np.repeat(mask.astype(bool)[:, :, None], ch, 2)
        # `ind` is distinct within an image and no addend is 0: one gradient cell per masked-in channel of a valid row
        assert np.count_nonzero(grad) == (per_row & valid[:, :, None]).sum()


def test_focal_without_a_peak_divides_by_nothing():
    got = run_all(('focal',))
    tag = 'focal/2x2x5x7/peaks0/'
    assert got[tag + 'num_pos'][0] == 0.0 and np.isfinite(got[tag + 'loss']).all() and got[tag + 'loss'][0] > 0
    assert np.isfinite(got[tag + 'grad']).all() and np.count_nonzero(got[tag + 'grad'])
