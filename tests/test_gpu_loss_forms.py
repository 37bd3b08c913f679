"""MI355X: every loss operator of csrc/loss.hip against tests/loss_oracle.py -- oracle/losses.py run in float64 on the
same float32 inputs, pinned to the reference's golden vectors by tests/test_host_loss_oracle.py.

The inputs reach what the golden sizes and the bit pins (tests/test_gpu_loss_bits.py) leave out: two and three
detections in one cell, rows with pred == target, an all-zero mask, softmax pixels whose other channels underflow or
that carry an offset of 1e4, C = 80, a keypoint in several pairs and a pair (j, j), half-masked joints, logits far past
the clamp, gt just below and just above 1, more pixels than both grid caps.  Every tensor mixes these with ordinary
values, so that the largest reference magnitude, which scales the bound, is an ordinary element's.

Almost every loss has a kink where float32 and float64 may take different branches; the inputs keep 1e-3 from each
(loss_oracle.py says how, the host file asserts it), so the bounds are the project's own and hold for EVERY element:
scalars |a - b| <= 1e-5 * max(1, |b|), gradients and maps max|a - b| <= 1e-4 * max|b|.  Where the math is exact the
check is exact: zeros of the gradient (clamped logits, rows masked out, gt > 1, an all-zero mask), `target` after the
call == target * mask, inputs untouched, num_pos and the L1 divisor.  Every case asserts by name, from the library's
launch log, that the kernels it means were launched; every comparison prints its error as a share of its bound."""
import numpy as np
import pytest
import torch

import loss_oracle as lo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _host(t):
    return t.detach().cpu().numpy()


def _same(t, a):
    """a device tensor still holds the array it was made from, bit for bit"""
    return np.array_equal(_host(t).view(np.int32 if a.dtype == np.float32 else a.dtype), a.view(
        np.int32 if a.dtype == np.float32 else a.dtype))


class _launches:
    """with _launches('focal_fwd_kernel', ...): the block must launch every kernel named (short names of
    tests/test_zz_kernel_coverage.py)"""

    def __init__(self, *kernels):
        self.kernels = kernels

    def __enter__(self):
        import hip_runtime as hr
        self.log = hr.launch_log()
        self.log.__enter__()

    def __exit__(self, *exc):
        from test_zz_kernel_coverage import short
        self.log.__exit__(*exc)
        if exc[0] is None:
            names = {short(k) for k in self.log.counts}
            assert names >= set(self.kernels), (sorted(set(self.kernels) - names), sorted(names))


def _check(family, got, want):
    """every entry of `want` (scalars, arrays, nested) against `got` at the project's bounds; prints each error"""
    missed = lo.misses(got, want, 1.0, lambda text: print('LOSSFORMS %s %s' % (family, text)))
    assert not missed, (family, missed)


# ---------------------------------------------------------------------------------------------------------------------
# the families: run_* -> the results in the layout of loss_oracle's *_refs, check_* -> everything asserted of a case
# ---------------------------------------------------------------------------------------------------------------------
SOFTMAX_KERNELS = ('softmax_reduce_kernel<EntropyTerm>', 'softmax_grad_kernel<EntropyTerm>',
                   'softmax_reduce_kernel<MaxSquareTerm>', 'softmax_grad_kernel<MaxSquareTerm>',
                   'softmax_reduce_kernel<EtaEntropyTerm>', 'softmax_grad_kernel<EtaEntropyTerm>',
                   'finalize_kernel<ScaleEpilogue>', 'entropy_map_fwd_kernel', 'entropy_map_bwd_kernel')


def _scalar_loss(fn, leaf, view=None):
    """`leaf` is what the gradient is read from; the operator sees view(leaf) (the leaf itself by default)"""
    loss = fn(leaf if view is None else view(leaf))
    (loss * lo.UP).backward()
    got = {'loss': loss.item(), 'grad': _host(leaf.grad).astype(np.float64)}
    leaf.grad = None
    return got


def run_softmax(c, leaf=None, view=None):
    from hip_runtime import ops
    x = _dev(c['logits'], True) if leaf is None else leaf
    got = {'entropy': _scalar_loss(ops.entropy_loss, x, view), 'maxsq': _scalar_loss(ops.max_square_loss, x, view)}
    em = ops.entropy_map(x if view is None else view(x))
    em.backward(_dev(c['gmap']))
    got['map'] = {'out': _host(em).astype(np.float64), 'grad': _host(x.grad).astype(np.float64)}
    x.grad = None
    for eta in lo.ETAS:
        got['eta%g' % eta] = _scalar_loss(lambda t: ops.entropy_eta_loss(t, eta), x, view)
    return got, x


def check_softmax(c, want):
    with _launches(*SOFTMAX_KERNELS):
        got, x = run_softmax(c)
    assert _same(x, c['logits'])
    _check('softmax', got, want)
    flat = c['kind'] == 2                                   # all channels equal: the entropy is exactly log2(C) / log2(C)
    if flat.any():
        assert (np.abs(got['map']['out'].transpose(0, 2, 3, 1)[flat].sum(1) - 1) < 1e-6).all()
    assert not got['map']['grad'].transpose(0, 2, 3, 1)[(c['gmap'] == 0).all(1)].any()    # no upstream, no gradient


def run_focal(c, leaf=None, view=None, gt=None):
    from hip_runtime import ops
    x = _dev(c['logits'], True) if leaf is None else leaf
    gt = _dev(c['gt']) if gt is None else gt
    loss, prob, num_pos = ops.focal_loss(x if view is None else view(x), gt, weight=lo.W_FOCAL, return_den=True)
    (loss * lo.UP).backward()
    return {'loss': loss.item(), 'prob': _host(prob).astype(np.float64), 'num_pos': num_pos.item(),
            'grad': _host(x.grad).astype(np.float64)}, x, gt


def check_focal(c, want):
    with _launches('focal_fwd_kernel', 'finalize_kernel<FocalEpilogue>', 'focal_bwd_kernel'):
        got, x, gt = run_focal(c)
    assert _same(x, c['logits']) and _same(gt, c['gt'])
    assert got['num_pos'] == c['peaks']
    _check('focal', got, want)
    clamped = (np.abs(c['logits']) > lo.LN9999) | (c['gt'] > 1)
    assert not got['grad'][clamped].any()
    assert np.count_nonzero(got['grad']) == (~clamped).sum()          # and nowhere else: no ordinary logit has gradient 0
    p = got['prob'][np.abs(c['logits']) > lo.LN9999]
    assert np.isin(p.astype(np.float32), np.float32([1e-4, 1 - 1e-4])).all()


def _touched_cells(c, ch):
    """[B, ch, H, W] bool: the cells a masked-in row gathers"""
    B, _, H, W = c['feat'].shape
    hit = np.zeros((B, ch, H * W), bool)
    m = c['mask'].astype(bool)
    for b, r in zip(*np.nonzero(m if m.ndim == 2 else m.any(2))):
        hit[b, :, c['ind'][b, r]] |= True if m.ndim == 2 else m[b, r]
    return hit.reshape(B, ch, H, W)


def _l1_common(c, got, tensors, ch):
    for t, name in zip(tensors, ('feat', 'mask', 'ind')):
        assert _same(t, c[name]), name
    assert got['den'] == lo.l1_den(c['mask'], ch), (got['den'], lo.l1_den(c['mask'], ch))
    assert not got['grad'][~_touched_cells(c, c['feat'].shape[1])].any()
    if not c['mask'].any():
        assert got['loss'] == 0 and not got['grad'].any()


def _after_image(got_after, mask, target, periodic, family):
    """`target` after the call: target * mask exactly; the angle of a 3-channel plain loss is its sigmoid, at the bound"""
    if mask.ndim == 2:
        want, sig = lo.reg_target_after(mask, target, periodic), target.shape[2] == 3 and not periodic
    else:
        want, sig = (target * mask.astype(np.float32)).astype(np.float64), False
    n = 2 if sig else target.shape[2]
    assert np.array_equal(got_after[..., :n].astype(np.float64), want[..., :n])
    if sig:
        _check(family, {'angle target after': got_after[..., 2].astype(np.float64)}, {'angle target after': want[..., 2]})


def run_reg(c, leaf=None, view=None):
    from hip_runtime import ops
    x = _dev(c['feat'], True) if leaf is None else leaf
    mask, ind, tg = _dev(c['mask']), _dev(c['ind']), _dev(c['target'])
    loss, den = ops.reg_l1_loss(x if view is None else view(x), mask, ind, tg, periodic=c['periodic'], weight=lo.W_L1, angle_weight=lo.W_ANGLE,
                                return_den=True)
    (loss * lo.UP).backward()
    return {'loss': loss.item(), 'grad': _host(x.grad).astype(np.float64), 'den': den.item(),
            'target_after': _host(tg)}, (x, mask, ind)


def check_reg(c, want):
    with _launches('regl1_fwd_kernel', 'regl1_bwd_kernel'):
        got, tensors = run_reg(c)
    _l1_common(c, got, tensors, c['ch'])
    _after_image(got['target_after'], c['mask'], c['target'], c['periodic'], 'reg_l1')
    _check('reg_l1', got, {k: want[k] for k in ('loss', 'grad')})
    for b, r in c['plan']['equal']:                         # pred == target: the row adds nothing, and alone it leaves 0
        alone = (c['ind'][b] == c['ind'][b, r]).sum() == 1
        cell = np.unravel_index(c['ind'][b, r], c['feat'].shape[2:])
        if alone and not (c['ch'] == 3 and c['periodic']):
            assert not got['grad'][(b, slice(None)) + cell].any()


def run_kps(c):
    from hip_runtime import ops
    x, mask, ind, tg = _dev(c['feat'], True), _dev(c['mask']), _dev(c['ind']), _dev(c['target'])
    pairs = torch.tensor(c['pairs'], dtype=torch.int32, device=DEV) if c['pairs'] else None
    loss, den = ops.kps_l1_loss(x, mask, ind, tg, pairs=pairs, use_l1=c['use_l1'], weight=lo.W_L1,
                                distance_weight=lo.W_DIST, return_den=True)
    (loss * lo.UP).backward()
    return {'loss': loss.item(), 'grad': _host(x.grad).astype(np.float64), 'den': den.item(),
            'target_after': _host(tg)}, (x, mask, ind)


def check_kps(c, want):
    with _launches('kpsl1_fwd_kernel', 'kpsl1_bwd_kernel'):
        got, tensors = run_kps(c)
    _l1_common(c, got, tensors, None)
    _after_image(got['target_after'], c['mask'], c['target'], False, 'kps_l1')
    _check('kps_l1', got, {k: want[k] for k in ('loss', 'grad')})


def check_bce(c, want):
    from hip_runtime import ops
    x = _dev(c['logits'], True)
    for label in lo.BCE_LABELS:
        with _launches('bce_const_fwd_kernel', 'bce_const_bwd_kernel'):
            got = _scalar_loss(lambda t: ops.bce_with_logits_const(t, label), x)
        _check('bce', got, want['label%g' % label])
    assert _same(x, c['logits'])


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', lo.SOFTMAX_SHAPES, ids=str)
def test_softmax_family(shape):
    c = lo.softmax(shape)
    check_softmax(c, c['want'])


@pytest.mark.parametrize('shape,peaks', lo.FOCAL_CASES, ids=str)
def test_focal(shape, peaks):
    c = lo.focal(shape, peaks)
    check_focal(c, c['want'])


@pytest.mark.parametrize('geom,ch,periodic,mask_kind', lo.REG_CASES, ids=str)
def test_reg_l1(geom, ch, periodic, mask_kind):
    c = lo.reg(geom, ch, periodic, mask_kind)
    check_reg(c, c['want'])


@pytest.mark.parametrize('geom,J,P,use_l1', lo.KPS_CASES, ids=str)
def test_kps_l1(geom, J, P, use_l1):
    c = lo.kps(geom, J, P, use_l1)
    check_kps(c, c['want'])


@pytest.mark.parametrize('n', lo.BCE_NS)
def test_bce_with_logits_const(n):
    c = lo.bce(n)
    check_bce(c, c['want'])


def check_fuzz(case):
    """one draw of loss_oracle.fuzz_cases() (tests/test_gpu_fuzz.py)"""
    refs, c = lo.fuzz_case(case)
    {lo.softmax_refs: check_softmax, lo.focal_refs: check_focal, lo.reg_refs: check_reg, lo.kps_refs: check_kps}[refs](
        c, refs(c))


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_sigmoid_clamp_in_place():
    from hip_runtime import ops
    c = lo.focal((3, 1, 9, 31), 5)                          # N(0, 4^2) with +-9.3, +-20, +-100, clear of the clamp gate
    x = _dev(c['logits'])
    with _launches('sigmoid_clamp_kernel'):
        y = ops.sigmoid_clamp_(x)
    s = 1.0 / (1.0 + np.exp(-c['logits'].astype(np.float64)))
    _check('sigmoid_clamp_', {'in place': _host(x).astype(np.float64), 'clamped': _host(y).astype(np.float64)},
           {'in place': s, 'clamped': c['want']['prob']})
    out = np.abs(c['logits']) > lo.LN9999
    assert out.sum() >= 6 and np.isin(_host(y)[out], np.float32([1e-4, 1 - 1e-4])).all()
    assert np.array_equal(_host(y)[~out], _host(x)[~out])


def test_gather_feat_and_the_index_out_of_range():
    from hip_runtime import ops
    c = lo.reg((3, 12, 11, 100), 3, False, 'third')
    ind = c['ind'].copy()
    ind[0, 5], ind[2, 99], ind[1, 0] = 12 * 11, -1, 1 << 40
    with _launches('gather_feat_kernel'):
        got = _host(ops.gather_feat(_dev(c['feat']), _dev(ind)))
    bad = (ind < 0) | (ind >= 12 * 11)
    assert bad.sum() == 3 and np.isnan(got[bad]).all()
    want = lo._gather(c['feat'], np.where(bad, 0, ind))
    assert np.array_equal(got[~bad].astype(np.float64), want[~bad])


def _views(a):
    """a [B, C, H, W] float32 -> [(leaf, the view of it that holds a, the same view of a numpy array)]: channels 1..C of
    a wider tensor, and a permuted NHWC tensor"""
    B, C, H, W = a.shape
    big = torch.zeros(B, C + 2, H, W, device=DEV)
    big[:, 1:C + 1] = _dev(a)
    nhwc = _dev(np.ascontiguousarray(a.transpose(0, 2, 3, 1)))
    return [(big.requires_grad_(True), lambda t: t[:, 1:C + 1]), (nhwc.requires_grad_(True), lambda t: t.permute(0, 3, 1, 2))]


def _same_results(got, plain, view, what):
    for k, v in plain.items():
        if isinstance(v, dict):
            _same_results(got[k], v, view, what + (k,))
        elif k == 'grad':
            assert np.array_equal(view(torch.from_numpy(got[k])).numpy(), v), what + (k,)
        else:
            assert np.array_equal(got[k], v), what + (k,)


def test_views_give_the_contiguous_calls_bits():
    """channels cut out of a wider tensor (`big[:, 1:4]`) and a permuted view into the softmax losses, focal_loss and
    reg_l1_loss: value and gradient equal the contiguous call's bit for bit"""
    sm, fo = lo.softmax((2, 3, 5, 7)), lo.focal_case((2, 3, 5, 7), 5, 11)
    rg = lo.reg((2, 6, 5, 4), 2, False, 'third')            # (sizes only: every addend of a cell has one magnitude, so
    #                                                          any order of the atomics gives the same sum)
    plain_sm, plain_fo, plain_rg = run_softmax(sm)[0], run_focal(fo)[0], run_reg(rg)[0]
    for i in (0, 1):
        leaf, view = _views(sm['logits'])[i]
        assert not view(leaf).is_contiguous()
        _same_results(run_softmax(sm, leaf, view)[0], plain_sm, view, (i, 'softmax'))
        leaf, view = _views(fo['logits'])[i]
        gleaf, gview = _views(fo['gt'])[i]
        _same_results(run_focal(fo, leaf, view, gview(gleaf.detach()))[0], plain_fo, view, (i, 'focal'))
        leaf, view = _views(rg['feat'])[i]
        _same_results(run_reg(rg, leaf, view)[0], plain_rg, view, (i, 'reg_l1'))


# ---------------------------------------------------------------------------------------------------------------------
# the modules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', lo.DETECTION_CASES)
def test_detection_loss_module(name):
    from losses.centernet import DetectionLoss
    out_np, batch_np, w, parts = lo.detection(name)
    want = parts['want']
    leaves = {k: _dev(v, True) for k, v in out_np.items()}
    out, batch = dict(leaves), {k: _dev(v) for k, v in batch_np.items()}
    kernels = ['focal_fwd_kernel', 'focal_bwd_kernel', 'regl1_fwd_kernel', 'regl1_bwd_kernel']
    with _launches(*kernels + (['kpsl1_fwd_kernel', 'kpsl1_bwd_kernel'] if name == 'keypoints' else [])):
        loss, stats = DetectionLoss(**w)(out, batch)
        (loss * lo.UP).backward()
    assert set(stats) == set(want['stats'])
    got = {'loss': loss.item(), 'stats': {k: v.item() for k, v in stats.items()},
           'grads': {k: _host(v.grad).astype(np.float64) for k, v in leaves.items()},
           'hm_after': _host(out['hm']).astype(np.float64)}
    _check('DetectionLoss', got, {k: want[k] for k in got})
    for k, v in leaves.items():
        assert _same(v, out_np[k]), k
    _after_image(_host(batch['wh']), batch_np['reg_mask'], batch_np['wh'], w['periodic'], 'DetectionLoss')
    _after_image(_host(batch['reg']), batch_np['reg_mask'], batch_np['reg'], False, 'DetectionLoss')
    if name == 'keypoints':
        _after_image(_host(batch['kps']), batch_np['kp_reg_mask'], batch_np['kps'], False, 'DetectionLoss')
    for k in ('hm', 'reg_mask', 'ind'):
        assert _same(batch[k], batch_np[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the one guard the masked-L1 pair did not share
# ---------------------------------------------------------------------------------------------------------------------
def test_reg_l1_refuses_a_batch_of_another_shape():
    """mask [B, M], ind [B, M] and target [B, M, ch] are walked by one index: a mismatch would read out of bounds, so it
    is an error before any launch"""
    import hip_runtime as hr
    from hip_runtime import ops
    c = lo.reg((2, 6, 5, 4), 2, False, 'ones')
    feat, mask, ind, tg = c['feat'], c['mask'], c['ind'], c['target']
    wrong = [(mask[:, :3], ind, tg), (mask, ind[:, :3], tg), (mask, ind, tg[:, :3]), (mask, ind, tg[:, :, :1]),
             (mask[:1], ind[:1], tg[:1]), (mask, ind, np.concatenate([tg, tg], 2)), (mask.reshape(-1), ind, tg)]
    with hr.launch_log() as log:
        for m, i, t in wrong:
            with pytest.raises(RuntimeError, match='reg_l1: output'):
                ops.reg_l1_loss(_dev(feat, True), _dev(m), _dev(i), _dev(t))
    assert not log.counts, log.counts
