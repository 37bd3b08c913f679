"""CPU: what tests/test_gpu_loss_forms.py stands on.

1. tests/loss_oracle.py in float64 reproduces the reference's golden vectors (tests/golden/losses_*.npz) at the bounds
   tests/test_gpu_losses.py holds, 1e-5 / 1e-4: the oracle is pinned to the reference, not to the kernels.
2. Every case's inputs keep MARGIN from every kink, no builder moved more than MOVED_SHARE of its elements, and the
   structures each case is about are there (duplicate cells, exactly equal rows, an all-zero mask, saturated pixels, gt
   just below and just above 1).
3. The bounds are attainable: oracle/losses.py in float32 stays within a TENTH of the GPU bounds of its float64 self on
   every case."""
import numpy as np
import pytest
import torch

import inputs as gin
import loss_oracle as lo

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _scalar(a, b, tol, what=''):
    err = abs(float(a) - float(b))
    print('%s: |a - b| %.3e, reference %.6g' % (what, err, float(b)))
    assert err <= tol * max(1.0, abs(float(b))), (what, float(a), float(b))


def _close(a, b, tol, what=''):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    print('%s: max abs err %.3e, reference max %.3e' % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the oracle against the reference's golden vectors
# ---------------------------------------------------------------------------------------------------------------------
def _golden_detection(g, out_np, batch_np, w, extra=()):
    ref = lo.detection_ref(out_np, batch_np, w)
    _scalar(ref['loss'], g['loss'], 1e-5, 'loss')
    assert set(ref['stats']) == {'centernet_loss', 'hm_loss', 'wh_loss', 'off_loss'} | set(extra)
    for k, v in ref['stats'].items():
        _scalar(v, g['stat_' + k], 1e-5, k)
    for k, v in ref['grads'].items():                      # the golden gradients have the upstream 1
        _close(v / lo.UP, g['grad_' + k], 1e-4, 'grad ' + k)
    return ref


@pytest.mark.parametrize('name', sorted(gin.LOSS_CASES))
def test_oracle_reproduces_the_detection_golden_vectors(golden, name):
    out_np, batch_np, w = gin.loss_inputs(name)
    g = golden('losses_det_' + name)
    ref = _golden_detection(g, out_np, batch_np, w)
    np.testing.assert_allclose(ref['hm_after'], g['hm_after'], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(ref['wh_after'], g['wh_target_after'], rtol=1e-6, atol=1e-7)
    assert np.array_equal(ref['reg_after'], g['reg_target_after'])


@pytest.mark.parametrize('name', sorted(gin.KPS_CASES))
def test_oracle_reproduces_the_keypoint_golden_vectors(golden, name):
    out_np, batch_np, w = gin.kps_inputs(name)
    w = dict(w, kp_indices=w['kp_indices'] or [])
    g = golden('losses_kps_' + name)
    ref = _golden_detection(g, out_np, batch_np, w, ('kp_loss',))
    assert np.array_equal(ref['kps_after'], g['kps_target_after'])


def test_oracle_reproduces_the_uda_golden_vectors(golden):
    g = golden('losses_uda')
    for kind, tag in (('entropy', 'entropy'), ('maxsq', 'maxsq')):
        ref = lo.softmax_ref(kind, g['hm'])
        _scalar(ref['loss'], g[tag + '_loss'], 1e-5, tag)
        _close(ref['grad'] / lo.UP, g[tag + '_grad'], 1e-4, tag + ' grad')
    ref = lo.softmax_ref('map', g['hm'], gmap=np.ones_like(g['hm']))
    np.testing.assert_allclose(ref['out'], g['entropy_map'], rtol=1e-4, atol=1e-7)
    _close(ref['grad'], g['entropy_map_grad_of_sum'], 1e-4, 'map grad')
    for label in (0, 1):
        ref = lo.bce_ref(g['advent_logits'], label)
        _scalar(ref['loss'], g['advent_loss_%d' % label], 1e-5, 'advent')
        np.testing.assert_allclose(ref['grad'] / lo.UP, g['advent_grad_%d' % label], rtol=1e-4, atol=1e-8)


def test_eta_restatement_in_float32_is_the_fda_oracle_formula():
    c = lo.softmax((2, 3, 5, 7))
    for eta in lo.ETAS:
        a, b = lo.softmax_ref('eta', c['logits'], lo.F32, eta=eta), lo.softmax_ref('eta', c['logits'], eta=eta)
        _scalar(a['loss'], b['loss'], 1e-6, 'eta %g' % eta)
        _close(a['grad'], b['grad'], 1e-5, 'eta %g grad' % eta)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the builders
# ---------------------------------------------------------------------------------------------------------------------
def _moved_little(c):
    print('moved %d of %d' % (c['moved'], c['total']))
    assert c['moved'] <= lo.MOVED_SHARE * c['total'], (c['moved'], c['total'])


def _kinks_clear(kinks):
    for name, d in kinks.items():
        print('%s: %d elements, nearest %.3e' % (name, d.size, d.min() if d.size else float('inf')))
        assert d.size == 0 or d.min() >= lo.MARGIN, (name, d.min())


@pytest.mark.parametrize('shape', lo.SOFTMAX_SHAPES, ids=str)
def test_softmax_inputs(shape):
    c = lo.softmax(shape)
    x = c['logits'].astype(np.float64)
    kind = c['kind']
    assert c['moved'] == 0 and x.shape == shape
    if kind.size < 4:
        return
    top2 = np.sort(x, axis=1)[:, -2:]
    lead = top2[:, 1] - top2[:, 0]
    for k in range(4):
        assert (kind == k).sum() >= kind.size // 4
    assert (lead[kind == 1] > 40).all() and (lead[kind == 1] > 104).any() == (kind.size > 8)   # exp(-104) is 0 in float32
    assert (x.max(1) == x.min(1))[kind == 2].all() and (x.min(1) > 9900)[kind == 3].all()
    assert ((c['gmap'] == 0).mean() > 0.03) == (kind.size > 8)
    # the gradient's scale is set by ordinary pixels: the largest entropy gradient lies on an ordinary or an offset pixel
    g = np.abs(lo.softmax_ref('entropy', c['logits'])['grad']).max(1)
    assert kind.reshape(-1)[g.argmax()] in (0, 3)


@pytest.mark.parametrize('shape,peaks', lo.FOCAL_CASES, ids=str)
def test_focal_inputs(shape, peaks):
    c = lo.focal(shape, peaks)
    x, gt = c['logits'].reshape(-1), c['gt'].reshape(-1)
    _moved_little(c)
    _kinks_clear({'gate': lo.gate_distance(x)})
    assert (gt == 1).sum() == peaks
    if x.size >= 12:
        assert (gt == 0).sum() >= 2 and (gt == lo.BELOW_ONE).sum() >= 2 and (gt == lo.ABOVE_ONE).sum() == 1
        assert lo.BELOW_ONE < 1 < lo.ABOVE_ONE and (gt > 1).sum() == 1
        assert np.array_equal(x[c['at']['planted']], np.float32(lo.PLANTED_LOGITS))
        grad = np.abs(lo.focal_ref(c['logits'], c['gt'])['grad']).reshape(-1)
        assert np.abs(x[grad.argmax()]) < lo.LN9999 and grad.max() > 0              # an ordinary logit sets the scale


def _rows_there(c, HW):
    ind, plan = c['ind'], c['plan']
    M = ind.shape[1]
    if M < 4:
        assert not (plan['pair'] or plan['triple'] or plan['equal'])
        return
    assert [ind[b, r] for b, r in plan['pair']] == [0, 0] and len(plan['equal']) == 2
    assert [ind[b, r] for b, r in plan['triple']] == [HW - 1] * 3
    if c.get('mask_kind', 'third') == 'third':
        assert all(c['mask'][b, r].any() for b, r in plan['pair'] + plan['triple'] + plan['equal'])


@pytest.mark.parametrize('geom,ch,periodic,mask_kind', lo.REG_CASES, ids=str)
def test_reg_l1_inputs(geom, ch, periodic, mask_kind):
    c = lo.reg(geom, ch, periodic, mask_kind)
    B, H, W, M = geom
    _moved_little(c)
    _kinks_clear(lo.reg_kinks(c))
    _rows_there(c, H * W)
    mask = c['mask']
    assert {'ones': mask.all(), 'zeros': not mask.any(), 'third': M < 4 or 0 < mask.mean() < 1}[mask_kind]
    pred = lo._gather(c['feat'], c['ind'])
    if M >= 4:
        (b0, r0), (b1, r1) = c['plan']['pair']
        d0, d1 = pred[b0, r0, 0] - c['target'][b0, r0, 0], pred[b1, r1, 0] - c['target'][b1, r1, 0]
        assert d0 * d1 < 0                                                       # opposite signs on the shared cell
        n_eq = 2 if ch == 3 and periodic else ch
        for b, r in c['plan']['equal']:
            assert np.array_equal(pred[b, r, :n_eq], c['target'][b, r, :n_eq].astype(np.float64))
        if ch == 3 and mask_kind != 'zeros':
            assert {float(pred[b, r, 2]) for b, r in c['extreme_rows']} >= {np.float64(np.float32(9.3))}
            assert np.abs(pred[..., 2][mask.astype(bool)]).max() > 9.3 - 1e-6
            if periodic:
                assert c['target'][..., 2].max() > 360 and c['target'][..., 2].min() < -360
            else:
                assert np.abs(c['target'][..., 2]).max() > lo.LN9999


@pytest.mark.parametrize('geom,J,P,use_l1', lo.KPS_CASES, ids=str)
def test_kps_l1_inputs(geom, J, P, use_l1):
    c = lo.kps(geom, J, P, use_l1)
    B, H, W, M = geom
    _moved_little(c)
    _kinks_clear(lo.kps_kinks(c))
    _rows_there(c, H * W)
    pairs, mask = c['pairs'], c['mask'].reshape(B, M, J, 2)
    assert len(pairs) == P
    assert (mask[..., 0] != mask[..., 1]).any()                                  # half-masked joints
    assert c['mask'][0, 1, 0] == 1 and c['mask'][0, 1, 1] == 0
    if P == 5 and J > 1:
        assert sum(0 in p for p in pairs) == 3 and sum(a == b for a, b in pairs) == 1
    if P and J > 1:
        diff, _, _, counts, _, _ = lo.kps_pair_state(c)
        assert (diff[counts] > 0).any() and (diff[counts] < 0).any()             # both signs of pd - td


@pytest.mark.parametrize('name', lo.DETECTION_CASES)
def test_detection_inputs(name):
    out, batch, w, parts = lo.detection(name)
    for k in out:
        assert parts[k]['moved'] == 0, (k, parts[k]['moved'])
    _kinks_clear({'gate': lo.gate_distance(parts['hm']['logits'])})
    _kinks_clear(lo.reg_kinks(parts['wh']))
    _kinks_clear(lo.reg_kinks(parts['reg']))
    if name == 'keypoints':
        _kinks_clear(lo.kps_kinks(parts['kps']))
        assert not (batch['kp_reg_mask'].any(2) & ~batch['reg_mask'].astype(bool)).any()
    _rows_there(parts['wh'], 30)


def test_fuzz_draws_move_little():
    cases = lo.fuzz_cases()
    assert len(cases) == 20 and {c[0] for c in cases} == {'softmax', 'focal', 'reg', 'periodic', 'kps'}
    assert cases == lo.fuzz_cases()
    for case in cases:
        c = lo.fuzz_case(case)[1]
        _moved_little(c)


# ---------------------------------------------------------------------------------------------------------------------
# 3. float32 against float64, at a tenth of the GPU bounds
# ---------------------------------------------------------------------------------------------------------------------
def _attainable(refs, c):
    assert not lo.misses(refs(c, lo.F32), refs(c, lo.F64), 0.1, print)


@pytest.mark.parametrize('shape', lo.SOFTMAX_SHAPES, ids=str)
def test_softmax_bounds_are_attainable_in_float32(shape):
    _attainable(lo.softmax_refs, lo.softmax(shape))


@pytest.mark.parametrize('shape,peaks', lo.FOCAL_CASES, ids=str)
def test_focal_bounds_are_attainable_in_float32(shape, peaks):
    _attainable(lo.focal_refs, lo.focal(shape, peaks))


@pytest.mark.parametrize('geom,ch,periodic,mask_kind', lo.REG_CASES, ids=str)
def test_reg_l1_bounds_are_attainable_in_float32(geom, ch, periodic, mask_kind):
    _attainable(lo.reg_refs, lo.reg(geom, ch, periodic, mask_kind))


@pytest.mark.parametrize('geom,J,P,use_l1', lo.KPS_CASES, ids=str)
def test_kps_l1_bounds_are_attainable_in_float32(geom, J, P, use_l1):
    _attainable(lo.kps_refs, lo.kps(geom, J, P, use_l1))


@pytest.mark.parametrize('n', lo.BCE_NS)
def test_bce_bounds_are_attainable_in_float32(n):
    _attainable(lo.bce_refs, lo.bce(n))


@pytest.mark.parametrize('name', lo.DETECTION_CASES)
def test_detection_bounds_are_attainable_in_float32(name):
    out, batch, w, _ = lo.detection(name)
    assert not lo.misses(lo.detection_ref(out, batch, w, lo.F32), lo.detection_ref(out, batch, w), 0.1, print)


@pytest.mark.parametrize('case', lo.fuzz_cases(), ids=lo.fuzz_id)
def test_fuzz_bounds_are_attainable_in_float32(case):
    refs, c = lo.fuzz_case(case)
    _attainable(refs, c)
