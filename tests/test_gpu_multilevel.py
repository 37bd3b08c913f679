"""Multi-level self-produced guidance on the GPU against tests/guidance_oracle.py: the labels as exact integers, loss and
gradient at the tolerances tests/test_gpu_iw_max_squares.py holds max-squares to, the exact zeros of a batch without a
guided pixel, the bits from run to run, a non-default stream, the launch counts of DESIGN.md section 31, the `[B:]`
slices of a batched step, and one step through the plugin on DLA-34 in both step forms.

The inputs are made so that no decision of the oracle hangs on a last bit, and that is asserted on the oracle alone
(`_want`): every pixel's max_c e is more than 1e-3 away from the threshold, and its two largest e differ by more than
1e-5 relative unless they are exactly equal.  Random logits of 5 N(0, 1) cannot promise that over 270400 pixels, so
`_settle` overwrites the pixels that miss either margin (both maps then agree on one class there)."""
import ast
import functools

import numpy as np
import pytest
import torch

import guidance_oracle as go
import inputs as gin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs below are read-only
UPSTREAM = 0.3
THRESHOLD_MARGIN, GAP_MARGIN = 1e-3, 1e-5

# name: (shape, threshold).  sub_wave: 70 pixels in all, idle lanes; partial_group: the project's class count, 837 pixels =
# three full workgroups and a partial fourth; many_classes: COCO's 80 channels per pixel; single_class: every pixel guided,
# zero loss; grid_cap: 270400 pixels > 1024 workgroups x 256 threads, every thread walks a second pixel; extremes:
# partial_group's shape with logits of +-80; none: small logits under a threshold of 0.999, no guided pixel
CASES = {'sub_wave': ((2, 2, 5, 7), 0.8), 'partial_group': ((3, 6, 9, 31), 0.6), 'many_classes': ((2, 80, 16, 16), 0.55),
         'single_class': ((2, 1, 4, 4), 0.95), 'grid_cap': ((1, 2, 520, 520), 0.9), 'extremes': ((3, 6, 9, 31), 0.45),
         'none': ((3, 6, 9, 31), 0.999), 'ties': ((2, 4, 6, 11), 0.3)}
NAMES = sorted(CASES)
MIXED = ('sub_wave', 'partial_group', 'many_classes', 'grid_cap', 'extremes')      # some pixels guided, some not


def _settle(x, z, threshold):
    """Overwrite every pixel that misses a margin (twice the asserted ones) in both maps: +5 on channel (pixel mod C),
    -5 elsewhere -- m > 0.996 for up to 80 classes, far from every threshold used here, the runner-up far below."""
    B, C = x.shape[:2]
    e = (go._softmax(x) + go._softmax(z)) / 2.0
    m = e.max(axis=1)
    bad = np.abs(m - threshold) <= 2 * THRESHOLD_MARGIN
    if C > 1:
        top = np.sort(e, axis=1)[:, -2:, :]
        bad |= (top[:, 1] != top[:, 0]) & ((top[:, 1] - top[:, 0]) <= 2 * GAP_MARGIN * top[:, 1])
    xf, zf = x.reshape(B, C, -1), z.reshape(B, C, -1)
    for b, p in zip(*np.nonzero(bad)):
        xf[b, :, p] = zf[b, :, p] = -5.0
        xf[b, p % C, p] = zf[b, p % C, p] = 5.0
    return int(bad.sum())


def _ties():
    """[2, 4, 66] pairs of maps.  At four pixels of image 0 the SAME channels carry the SAME winning logit in both maps, so
    their e are equal to the bit in any precision: {1, 3} -> 1, {0, 3} -> 0, {0, 1, 3} -> 0, {2, 3} -> 2."""
    rs = np.random.RandomState(77)
    x = (rs.standard_normal((2, 4, 66)) * 5).astype(np.float32)
    z = (rs.standard_normal((2, 4, 66)) * 5).astype(np.float32)
    for pixel, channels in ((3, (1, 3)), (20, (0, 3)), (41, (0, 1, 3)), (60, (2, 3))):
        top_x = np.abs(x[0, :, pixel]).max() + np.float32(1.5)
        top_z = np.abs(z[0, :, pixel]).max() + np.float32(2.5)
        for c in channels:
            x[0, c, pixel], z[0, c, pixel] = top_x, top_z
    return x.reshape(2, 4, 6, 11), z.reshape(2, 4, 6, 11)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """-> (x: the final map's logits, z: the low-level map's, threshold), read-only"""
    shape, threshold = CASES[case]
    rs = np.random.RandomState(200 + NAMES.index(case))
    if case == 'ties':
        x, z = _ties()
    else:
        scale = 0.1 if case == 'none' else 5.0
        x = (rs.standard_normal(shape) * scale).astype(np.float32)
        z = (rs.standard_normal(shape) * scale).astype(np.float32)
    if case == 'extremes':
        # p = onehot(0), q_0 = e^-80 / 5: e = (1/2, 1/10, ...), guided to 0 at a cost of 80 + ln 5, q_0 below float32's range
        x[0, :, 0, 0], z[0, :, 0, 0] = (80, 0, 0, 0, 0, 0), (-80, 0, 0, 0, 0, 0)
        x[1, :, 4, 17], z[1, :, 4, 17] = (-80, -80, 80, -80, -80, -80), (-80, -80, 80, -80, -80, -80)   # agreed: cost 0
        x[2, :, 8, 30], z[2, :, 8, 30] = (0, 0, 0, -80, 0, 80), (80, 0, 0, 0, 0, -80)     # e = (1/2, .., 1/2): an exact tie -> 0
    _settle(x, z, threshold)
    x.setflags(write=False), z.setflags(write=False)
    return x, z, threshold


@functools.lru_cache(maxsize=None)
def _want(case):
    """The oracle, once per case, with its margins asserted: (labels, loss, grad of UPSTREAM * loss, count)."""
    x, z, threshold = _inputs(case)
    m = go.margins(x, z, threshold)
    assert m['threshold'] > THRESHOLD_MARGIN and m['gap'] > GAP_MARGIN, (case, m)
    labels, n = go.labels(x, z, threshold), go.count(x, z, threshold)
    if case in MIXED:
        assert 0 < n < labels.size, (case, n)
    if case == 'ties':
        assert m['ties'] == 4 and m['guided_ties'] == 4, m
        assert [int(labels[0].reshape(-1)[p]) for p in (3, 20, 41, 60)] == [1, 0, 0, 2]
    elif case == 'extremes':
        assert m['ties'] == 1 and m['guided_ties'] == 1 and labels[2, 8, 30] == 0 and labels[0, 0, 0] == 0
    else:
        assert m['ties'] == 0, (case, m)
    if case == 'none':
        assert n == 0
    if case == 'single_class':
        assert n == labels.size
    return labels, go.loss(x, z, threshold), UPSTREAM * go.grad(x, z, threshold), n


def _run(x, z, threshold, weight=UPSTREAM):
    """-> (weighted loss [1], d / d low, d / d high (None or a tensor), count) -- the weight in place, as the plugin does"""
    from hip_runtime import ops
    low, high = z.detach().requires_grad_(True), x.detach().requires_grad_(True)
    loss, count = ops.guidance_loss(low, high, threshold, return_count=True)
    loss *= weight
    loss.backward()
    return loss.detach().reshape(1), low.grad, high.grad, count


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('case', NAMES)
def test_the_labels_are_exact(case):
    from hip_runtime import ops
    x, z, threshold = _inputs(case)
    want = _want(case)[0]
    high, low = T(x).to(DEV).requires_grad_(True), T(z).to(DEV).requires_grad_(True)
    got = ops.guidance_labels(high, low, threshold)
    assert got.dtype == torch.int32 and tuple(got.shape) == (x.shape[0],) + x.shape[2:] and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() != want).sum()
    again = ops.guidance_labels(high, low, threshold)           # a fresh result every call
    assert again.data_ptr() != got.data_ptr() and torch.equal(again, got)


@pytest.mark.parametrize('case', NAMES)
def test_loss_and_gradient_vs_oracle(case):
    x, z, threshold = _inputs(case)
    _, want_loss, want_grad, n = _want(case)
    loss, grad, ghigh, count = _run(T(x).to(DEV), T(z).to(DEV), threshold)
    got_loss, got_grad = loss.item(), grad.cpu().numpy()
    err = np.abs(got_grad - want_grad).max()
    print(case, 'guided', int(count.item()), 'of', x.size // x.shape[1], 'loss', got_loss, UPSTREAM * want_loss,
          'grad err', err, 'of', np.abs(want_grad).max())
    assert count.item() == n and not count.requires_grad
    assert np.isfinite(got_loss) and np.isfinite(got_grad).all()
    assert abs(got_loss - UPSTREAM * want_loss) <= 1e-5 * abs(UPSTREAM * want_loss)
    assert err <= 1e-4 * np.abs(want_grad).max()
    assert ghigh is None or not ghigh.any()                   # the labels are constants: nothing for the final map
    if case in ('none', 'single_class'):                      # exact zeros, not small numbers and not NaN
        assert got_loss == 0.0 and not got_grad.any() and want_loss == 0.0
    if case == 'extremes':                                    # 80 + ln 5 from one pixel alone
        assert got_loss * n / UPSTREAM > 80.0


def test_the_module_returns_the_loss_it_logs():
    from losses.max_square import GuidanceLoss
    x, z, _ = _inputs('partial_group')
    outputs = {'hm': T(x).to(DEV).requires_grad_(True), 'hm_low': T(z).to(DEV).requires_grad_(True)}
    loss, stats = GuidanceLoss(0.6)(outputs, None)
    assert list(stats) == ['guidance_loss'] and stats['guidance_loss'] is loss
    want = _want('partial_group')[1]
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    loss.backward()
    assert outputs['hm'].grad is None and outputs['hm_low'].grad is not None


@pytest.mark.parametrize('case', ['grid_cap', 'many_classes'])
def test_two_runs_give_the_same_bits(case):
    x, z, threshold = _inputs(case)
    x, z = T(x).to(DEV), T(z).to(DEV)
    (l1, g1, _, _), (l2, g2, _, _) = _run(x, z, threshold), _run(x, z, threshold)
    assert np.array_equal(_bits(l1), _bits(l2)) and np.array_equal(_bits(g1), _bits(g2))


def test_a_non_default_stream_and_the_launch_counts():
    """Nothing in the call waits for the device: on a side stream the result is there after ONE synchronize of that
    stream.  Launches: forward = the walk + finalize, backward = one; the labels alone = forward."""
    import hip_runtime as hr
    from test_zz_kernel_coverage import short
    from hip_runtime import ops
    x, z, threshold = _inputs('partial_group')
    _, want_loss, want_grad, _ = _want('partial_group')
    high, low = T(x).to(DEV), T(z).to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with hr.launch_log() as fwd:
            loss = ops.guidance_loss(low, high, threshold)
        loss *= UPSTREAM
        with hr.launch_log() as bwd:
            loss.backward()
    side.synchronize()
    assert abs(loss.item() - UPSTREAM * want_loss) <= 1e-5 * abs(UPSTREAM * want_loss)
    assert np.abs(low.grad.cpu().numpy() - want_grad).max() <= 1e-4 * np.abs(want_grad).max()
    forward = {'guidance_fwd_kernel': 1, 'finalize_kernel<GuidanceEpilogue>': 1}
    assert {short(k): v for k, v in fwd.counts.items()} == forward
    assert {short(k): v for k, v in bwd.counts.items()} == {'guidance_grad_kernel': 1}
    with hr.launch_log() as lab:
        ops.guidance_labels(high, low, threshold)
    assert {short(k): v for k, v in lab.counts.items()} == forward


def test_the_trailing_slices_of_a_batched_step_are_taken_as_they_are():
    """forward_domains returns y[B:] of one [2B, C, H, W] tensor: contiguous, so the op reads it where it lies."""
    import hip_runtime as hr
    x, z, threshold = _inputs('partial_group')
    B = x.shape[0]
    rs = np.random.RandomState(9)
    lead = lambda: (rs.standard_normal(x.shape) * 5).astype(np.float32)
    both_x, both_z = T(np.concatenate([lead(), x])).to(DEV), T(np.concatenate([lead(), z])).to(DEV)
    sx, sz = both_x[B:], both_z[B:]
    assert hr.f32c(sx) is sx and hr.f32c(sz) is sz and sx.data_ptr() != both_x.data_ptr()
    loss, grad, _, count = _run(sx, sz, threshold)
    ref_loss, ref_grad, _, ref_count = _run(T(x).to(DEV), T(z).to(DEV), threshold)
    assert np.array_equal(_bits(loss), _bits(ref_loss)) and np.array_equal(_bits(grad), _bits(ref_grad))
    assert count.item() == ref_count.item() == _want('partial_group')[3]
    # ... and through autograd, from a tensor that requires grad: the gradient lands in the trailing half only
    from hip_runtime import ops
    whole = both_z.clone().requires_grad_(True)
    ops.guidance_loss(whole[B:], both_x[B:], threshold).backward()
    unit_grad = _run(T(x).to(DEV), T(z).to(DEV), threshold, weight=1.0)[1]
    assert not whole.grad[:B].any() and np.array_equal(_bits(whole.grad[B:]), _bits(unit_grad))


# -- one step through the plugin on DLA-34 (the wiring of tests/test_gpu_batched_domains.py::_plugin) -------------------
PLUGIN_THRESHOLD = 0.2      # the filled weights give nearly flat heat maps (m around 1/6): a threshold that splits them


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _plugin(golden, batched, multilevel=True, aux_weight=0.1, seed=5):
    import uda
    from backends import dla
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    shapes = dict(ast.literal_eval(str(golden('dla_axis')['shapes_json'])))
    model = dla.build(num_classes=6)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gin.fill_state(shapes, 0.1).items()})
    plugin = uda.MultiLevelMaxSquaresMinimization(0.3, aux_weight=aux_weight, threshold=PLUGIN_THRESHOLD) if multilevel \
        else uda.MaxSquaresMinimization(0.3)
    plugin.cfg = _Cfg(model=_Cfg(backend=_Cfg(name='dla', params=_Cfg(num_classes=6))))
    plugin.batch_domains = batched
    plugin.backend = model.to(DEV)
    plugin.device = torch.device(DEV)
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    torch.manual_seed(seed)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    return plugin, model


def _data(B=2, S=64, M=8):
    data = {k: T(v) for k, v in gin.detection_batch(B, 6, S // 4, S // 4, M, (3, 2), 2, 51).items()}
    data['input'] = T(gin.image_batch(B, S, S, 60))
    data['target_domain_input'] = T(gin.image_batch(B, S, S, 70))
    return data


def _grads(module):
    return {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}


def _compare(ga, gb, label):
    """Every gradient of `ga` against `gb` at 2e-4 of its maximum.  A DCN bias in front of a BatchNorm has an analytically
    zero gradient (tests/test_gpu_batched_domains.py): what is left there is rounding noise, which is held to 2e-4 of its
    own layer's weight gradient instead of to itself."""
    assert sorted(ga) == sorted(gb), label
    worst = 0.0
    for n in gb:
        if n.endswith('.conv.bias') and 'ida' in n:
            scale = gb[n[:-len('bias')] + 'weight'].abs().max().item()
            r = (ga[n].double() - gb[n].double()).abs().max().item() / scale
        else:
            r = _rel(ga[n], gb[n])
        worst = max(worst, r)
        assert r <= 2e-4, (label, n, r)
    return worst


def test_one_step_through_the_plugin_in_both_step_forms(golden):
    B, S = 2, 64
    res = []
    for batched in (True, False):
        plugin, model = _plugin(golden, batched)
        head = plugin.low_level_head
        before = {n: p.detach().clone() for n, p in head.named_parameters()}
        out = plugin.step(_data(B, S))
        res.append((out, _grads(model), _grads(head)))
        assert sorted(res[-1][2]) == sorted(before) and len(before) == 4
        for n, p in head.named_parameters():                  # the head's own optimizer stepped
            assert not torch.equal(p.detach(), before[n]), n
    for out, _, _ in res:
        stats = {k: float(v) for k, v in out['stats'].items()}
        assert set(stats) == {'centernet_loss', 'hm_loss', 'wh_loss', 'off_loss', 'max_square_loss', 'aux_hm_loss',
                              'guidance_loss', 'guidance_pixels', 'total_loss'}
        total = stats['centernet_loss'] + stats['aux_hm_loss'] + stats['max_square_loss'] + stats['guidance_loss']
        assert abs(stats['total_loss'] - total) <= 1e-5 * abs(total), stats
        for dom in ('source_domain', 'target_domain'):
            assert list(out[dom]) == ['hm', 'wh', 'reg', 'hm_low']
            assert out[dom]['hm_low'].shape == out[dom]['hm'].shape == (B, 6, S // 4, S // 4)
        hm = out['target_domain']['hm'].detach().cpu().numpy()
        low = out['target_domain']['hm_low'].detach().cpu().numpy()
        n = go.count(hm, low, PLUGIN_THRESHOLD)
        print('guided', n, 'of', B * (S // 4) ** 2, 'margins', go.margins(hm, low, PLUGIN_THRESHOLD), stats)
        assert 0 < n < B * (S // 4) ** 2                      # the guidance term is really there
        assert stats['guidance_pixels'] == n / B
        want = 0.3 * 0.1 * go.loss(hm, low, PLUGIN_THRESHOLD)
        assert abs(stats['guidance_loss'] - want) <= 1e-4 * abs(want), (stats, want)
    (_, gb, hb), (_, gs, hs) = res
    assert len(gs) > 60
    print('batched vs two-pass: backbone', _compare(gb, gs, 'backbone'), 'head', _compare(hb, hs, 'low-level head'))


def test_without_the_auxiliary_weight_the_backbone_trains_as_plain_max_squares(golden):
    plugin, model = _plugin(golden, True, aux_weight=0.0)
    out = plugin.step(_data())
    got = _grads(model)
    plain, plain_model = _plugin(golden, True, multilevel=False)
    ref = plain.step(_data())
    assert float(out['stats']['aux_hm_loss']) == 0.0 and float(out['stats']['guidance_loss']) == 0.0
    assert abs(float(out['stats']['total_loss']) - float(ref['stats']['total_loss'])) <= 1e-6 * abs(float(ref['stats']['total_loss']))
    print('aux_weight = 0 against MaxSquaresMinimization: worst relative gradient difference',
          _compare(got, _grads(plain_model), 'aux_weight=0'))


def test_checkpoints_carry_the_head_and_its_optimizer(golden, tmp_path):
    import export
    plugin, model = _plugin(golden, True)
    plugin.step(_data())
    plugin.step(_data())
    path = str(tmp_path / 'model_last.pth')
    plugin.save_model(path, 4, True)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['epoch', 'low_level_head_optimizer', 'low_level_head_state_dict', 'optimizer', 'state_dict']
    assert list(ckpt['state_dict']) == list(model.state_dict())                 # the backend's entries as they were
    fresh, fresh_model = _plugin(golden, True, seed=9)
    assert any(not torch.equal(a, b) for a, b in zip(fresh.low_level_head.parameters(), plugin.low_level_head.parameters()))
    assert fresh.load_model(path, resume=True) == 5
    for (n, a), b in zip(fresh.low_level_head.state_dict().items(), plugin.low_level_head.state_dict().values()):
        assert torch.equal(a, b), n
    for a, b in zip(fresh_model.state_dict().values(), model.state_dict().values()):
        assert torch.equal(a, b)

    def flat(state):
        if torch.is_tensor(state):
            return [state.detach().cpu()]
        if isinstance(state, dict):
            return [t for k in sorted(state, key=str) for t in flat(state[k])]
        if isinstance(state, (list, tuple)):
            return [t for v in state for t in flat(v)]
        return [torch.tensor(float(state))] if isinstance(state, (int, float)) else []
    mine, theirs = flat(fresh.low_level_optimizer.state_dict()), flat(plugin.low_level_optimizer.state_dict())
    assert len(mine) == len(theirs) > 0 and all(torch.equal(a, b) for a, b in zip(mine, theirs))
    a, b = fresh.step(_data()), plugin.step(_data())          # and both train on from there, alike
    ta, tb = float(a['stats']['total_loss']), float(b['stats']['total_loss'])
    assert abs(ta - tb) <= 1e-6 * abs(tb), (ta, tb)
    # without the optimizer: the head alone travels; predict's loader takes the file and ignores the extra entries
    plugin.save_model(path, 5)
    assert sorted(torch.load(path, map_location='cpu', weights_only=False)) == ['epoch', 'low_level_head_state_dict', 'state_dict']
    spec = {'name': 'dla', 'params': {'num_classes': 6}}
    loaded = export.build_model(str(tmp_path), spec, True, 100)
    for (n, a), b in zip(loaded.state_dict().items(), model.state_dict().values()):
        assert torch.equal(a, b.cpu()), n
