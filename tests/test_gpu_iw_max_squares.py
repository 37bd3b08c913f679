"""Image-wise class-balanced max-squares on the GPU against tests/iw_maxsq_oracle.py: the argmax histogram as exact
integers, loss and gradient at the tolerances test_gpu_losses.py::test_uda_losses_golden holds MaxSquareLoss to, the
ratio = 0 identity, the bits from run to run, a non-default stream, the launch counts of DESIGN.md section 28 and one
step through the plugin."""
import functools

import numpy as np
import pytest
import torch

import inputs as gin
import iw_maxsq_oracle as iwo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs below are read-only
RATIOS = (0.0, 0.2, 1.0)
UPSTREAM = 0.3

# sub_wave: 35 pixels, idle lanes; partial_group: the project's class count, 279 pixels = 2 workgroups per image, the
# second one partial; coco: the LDS-atomic path, most classes empty; many_groups: 352 workgroups on one image;
# grid_cap: 270400 pixels > 1024 workgroups x 256 threads, every thread walks a second pixel
SHAPES = {'sub_wave': (2, 2, 5, 7), 'partial_group': (3, 6, 9, 31), 'coco': (2, 80, 16, 16),
          'many_groups': (1, 3, 300, 300), 'grid_cap': (1, 2, 520, 520)}
CASES = sorted(SHAPES) + ['ties']


def _ties():
    """[2, 4, 6, 11].  Image 0: channel 0 wins every pixel, at pixels 3 / 20 / 41 only through the tie rule (equal
    logits in channels {0, 3}, {0, 1} and {0, 1, 3}).  Image 1: channel 2 wins exactly pixel 17; ties at the maximum
    between channels {1, 3} (-> 1), {0, 3} (-> 0) and {0, 1, 3} (-> 0)."""
    rs = np.random.RandomState(77)
    x = (rs.standard_normal((2, 4, 66)) * 5).astype(np.float32)
    x[0, 0] = np.abs(x[0]).max(0) + np.float32(1.5)
    x[0, 3, 3] = x[0, 0, 3]
    x[0, 1, 20] = x[0, 0, 20]
    x[0, 1, 41] = x[0, 3, 41] = x[0, 0, 41]
    x[1, 2] = -50.0
    x[1, 2, 17] = 50.0
    top = np.float32(30.0)
    x[1, 1, 5] = x[1, 3, 5] = top
    x[1, 0, 29] = x[1, 3, 29] = top
    x[1, 0, 60] = x[1, 1, 60] = x[1, 3, 60] = top
    return x.reshape(2, 4, 6, 11)


@functools.lru_cache(maxsize=None)
def _logits(case):
    x = _ties() if case == 'ties' else \
        (np.random.RandomState(100 + CASES.index(case)).standard_normal(SHAPES[case]) * 5).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(case, ratio):
    """the oracle, once per (case, ratio): (loss, grad of UPSTREAM * loss)"""
    x = _logits(case)
    return iwo.loss(x, ratio), UPSTREAM * iwo.grad(x, ratio)


def _run(x, ratio, weight=UPSTREAM, loss_fn=None):
    """-> (weighted loss [1] and gradient as device tensors), the weight applied in place as the plugins do"""
    from hip_runtime import ops
    x = x.detach().requires_grad_(True)
    loss = ops.iw_max_square_loss(x, ratio) if loss_fn is None else loss_fn(x)
    loss *= weight
    loss.backward()
    return loss.detach().reshape(1), x.grad


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('case', CASES)
def test_class_histogram_is_exact(case):
    from hip_runtime import ops
    x = _logits(case)
    got = ops.class_histogram(T(x).to(DEV))
    assert got.dtype == torch.int32 and tuple(got.shape) == x.shape[:2]
    got = got.cpu().numpy()
    assert np.array_equal(got, iwo.hist(x)), (got, iwo.hist(x))
    assert (got.sum(1) == x.shape[2] * x.shape[3]).all()
    if case == 'ties':
        assert got[0].tolist() == [66, 0, 0, 0] and got[1, 2] == 1


def test_class_histogram_detaches_and_clears_its_output():
    from hip_runtime import ops
    x = T(_logits('partial_group')).to(DEV).requires_grad_(True)
    a = ops.class_histogram(x)
    b = ops.class_histogram(x)                       # a second call starts from zero again
    assert not a.requires_grad and torch.equal(a, b)


@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('case', CASES)
def test_loss_and_gradient_vs_oracle(case, ratio):
    want_loss, want_grad = _want(case, ratio)
    loss, grad = _run(T(_logits(case)).to(DEV), ratio)
    got_loss, got_grad = loss.item(), grad.cpu().numpy()
    err = np.abs(got_grad - want_grad).max()
    print(case, ratio, 'loss', got_loss, UPSTREAM * want_loss, 'grad err', err, 'of', np.abs(want_grad).max())
    assert abs(got_loss - UPSTREAM * want_loss) <= 1e-5 * abs(UPSTREAM * want_loss)
    assert err <= 1e-4 * np.abs(want_grad).max()


@pytest.mark.parametrize('case', CASES)
def test_ratio_zero_is_max_square_loss(case):
    from hip_runtime import ops
    x = T(_logits(case)).to(DEV)
    loss, grad = _run(x, 0.0)
    ref_loss, ref_grad = _run(x, None, loss_fn=ops.max_square_loss)
    print(case, loss.item(), ref_loss.item())
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * abs(ref_loss.item())
    assert (grad - ref_grad).abs().max().item() <= 1e-5 * ref_grad.abs().max().item()


def test_the_module_returns_the_loss_it_logs():
    from losses.max_square import IWMaxSquareLoss
    x = T(_logits('partial_group')).to(DEV).requires_grad_(True)
    loss, stats = IWMaxSquareLoss(0.2)({'hm': x}, None)
    assert list(stats) == ['iw_max_square_loss'] and stats['iw_max_square_loss'] is loss
    want = iwo.loss(_logits('partial_group'), 0.2)
    assert abs(loss.item() - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize('case', ['many_groups', 'coco'])
def test_two_runs_give_the_same_bits(case):
    x = T(_logits(case)).to(DEV)
    (l1, g1), (l2, g2) = _run(x, 0.2), _run(x, 0.2)
    assert np.array_equal(_bits(l1), _bits(l2)) and np.array_equal(_bits(g1), _bits(g2))


def test_a_non_default_stream_and_the_launch_counts():
    """Nothing in the call waits for the device: on a side stream the result is there after ONE synchronize of that
    stream.  Launches: forward = histogram + reduction + finalize, backward = one."""
    import hip_runtime as hr
    from test_zz_kernel_coverage import short
    from hip_runtime import ops
    want_loss, want_grad = _want('partial_group', 0.2)
    x = T(_logits('partial_group')).to(DEV).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with hr.launch_log() as fwd:
            loss = ops.iw_max_square_loss(x, 0.2)
        loss *= UPSTREAM
        with hr.launch_log() as bwd:
            loss.backward()
    side.synchronize()
    assert abs(loss.item() - UPSTREAM * want_loss) <= 1e-5 * abs(UPSTREAM * want_loss)
    assert np.abs(x.grad.cpu().numpy() - want_grad).max() <= 1e-4 * np.abs(want_grad).max()
    assert {short(k): v for k, v in fwd.counts.items()} == {
        'argmax_hist_kernel<true>': 1, 'iw_max_square_reduce_kernel': 1, 'finalize_kernel<ScaleEpilogue>': 1}
    assert {short(k): v for k, v in bwd.counts.items()} == {'iw_max_square_grad_kernel': 1}
    with hr.launch_log() as coco:                    # above 16 classes the histogram counts with LDS atomics
        ops.class_histogram(T(_logits('coco')).to(DEV))
    assert {short(k): v for k, v in coco.counts.items()} == {'argmax_hist_kernel<false>': 1}


def test_more_classes_than_the_table_holds_are_refused():
    from hip_runtime import ops
    x = torch.zeros(1, 1025, 2, 2, device=DEV)
    with pytest.raises(RuntimeError, match='1024'):
        ops.class_histogram(x)
    with pytest.raises(RuntimeError, match='1024'):
        ops.iw_max_square_loss(x)
    assert ops.class_histogram(torch.zeros(1, 1024, 2, 2, device=DEV))[0, 0].item() == 4   # all ties: channel 0


# -- one step through the plugin (the wiring of tests/test_gpu_batched_domains.py::_plugin, on ResNet-18) -------------
def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def _plugin(batched):
    import uda
    from backends import resnet
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    torch.manual_seed(5)
    model = resnet.build(num_layers=18, num_classes=6, pretrained=False)
    plugin = uda.IWMaxSquaresMinimization(0.3, ratio=0.2)
    plugin.batch_domains = batched
    plugin.backend = model.to(DEV)
    plugin.device = torch.device(DEV)
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    return plugin, model


def test_one_step_through_the_plugin():
    B, S, M = 2, 64, 8
    res = []
    for batched in (True, False):
        plugin, model = _plugin(batched)
        data = {k: T(v) for k, v in gin.detection_batch(B, 6, S // 4, S // 4, M, (3, 2), 2, 51).items()}
        data['input'] = T(gin.image_batch(B, S, S, 60))
        data['target_domain_input'] = T(gin.image_batch(B, S, S, 70))
        out = plugin.step(data)
        res.append((out, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (ob, gb), (os_, gs) = res
    for out in (ob, os_):
        stats = {k: float(v) for k, v in out['stats'].items()}
        assert set(stats) == {'centernet_loss', 'hm_loss', 'wh_loss', 'off_loss', 'iw_max_square_loss', 'total_loss'}
        total = stats['centernet_loss'] + stats['iw_max_square_loss']
        assert abs(stats['total_loss'] - total) <= 1e-5 * abs(total), stats
        hm = out['target_domain']['hm'].detach().cpu().numpy()
        assert hm.shape == (B, 6, S // 4, S // 4)
        want = 0.3 * iwo.loss(hm, 0.2)
        assert abs(stats['iw_max_square_loss'] - want) <= 1e-4 * abs(want), (stats, want)
    assert sorted(gb) == sorted(gs) and len(gs) > 60
    for n in gs:
        assert _rel(gb[n], gs[n]) <= 2e-4, (n, _rel(gb[n], gs[n]))
