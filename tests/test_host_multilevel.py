"""No-GPU checks of multi-level self-produced guidance: the float64 oracle on hand-worked cases and against an
independent torch statement, the plugin as the driver sees it, the backend's low-level tap in the alias plan, and the C
ABI's refusals."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import guidance_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cnuda_guidance_forward', 'cnuda_guidance_backward')
OVERRIDE = "model.uda={MultiLevelMaxSquaresMinimization: {max_squares_weight: 0.3, aux_weight: 0.1}}"


def _logits(shape, seed):
    return (np.random.RandomState(seed).standard_normal(shape) * 5).astype(np.float32)


# -- the oracle -----------------------------------------------------------------------------------------------------------
def test_the_oracle_on_the_hand_worked_pixel():
    """C = 2, one pixel, x = (ln 3, 0), z = (0, 0): p = (3/4, 1/4), q = (1/2, 1/2), e = (5/8, 3/8)."""
    x = np.array([math.log(3.0), 0.0]).reshape(1, 2, 1, 1)
    z = np.zeros((1, 2, 1, 1))
    assert go.labels(x, z, 0.6).tolist() == [[[0]]] and go.count(x, z, 0.6) == 1
    assert abs(go.loss(x, z, 0.6) - math.log(2.0)) < 1e-15
    assert np.allclose(go.grad(x, z, 0.6).reshape(2), [-0.5, 0.5], rtol=0, atol=1e-15)
    m = go.margins(x, z, 0.6)
    assert abs(m['threshold'] - 0.025) < 1e-12 and abs(m['gap'] - 0.4) < 1e-12 and m['ties'] == 0
    # threshold 0.7: unguided
    assert go.labels(x, z, 0.7).tolist() == [[[-1]]] and go.count(x, z, 0.7) == 0
    assert go.loss(x, z, 0.7) == 0.0 and not go.grad(x, z, 0.7).any()


def test_the_oracle_on_a_second_hand_worked_batch():
    """Two pixels, C = 3.  Pixel 0: x = z = (0, 0, ln 2): e = (1/4, 1/4, 1/2) -> label 2 above 0.4, -log q_2 = ln 2.
    Pixel 1: x = (ln 2, 0, 0), z = (0, ln 2, 0): e = (3/8, 3/8, 1/4): a tie, the lowest channel -> label 0 above 0.3,
    -log q_0 = ln 4.  N = 2: loss = (ln 2 + ln 4) / 2, gradients (q - onehot) / 2."""
    l2 = math.log(2.0)
    x = np.array([[0, 0, l2], [l2, 0, 0]], np.float64).T.reshape(1, 3, 1, 2)
    z = np.array([[0, 0, l2], [0, l2, 0]], np.float64).T.reshape(1, 3, 1, 2)
    assert go.labels(x, z, 0.3).tolist() == [[[2, 0]]]
    assert abs(go.loss(x, z, 0.3) - (l2 + 2 * l2) / 2) < 1e-15
    want = np.array([[0.25, 0.25, -0.5], [-0.75, 0.5, 0.25]]).T.reshape(1, 3, 1, 2) / 2
    assert np.abs(go.grad(x, z, 0.3) - want).max() < 1e-15
    m = go.margins(x, z, 0.3)
    assert m['ties'] == 1 and m['guided_ties'] == 1 and abs(m['gap'] - 0.5) < 1e-12
    # threshold 0.4: only pixel 0 is guided, N = 1
    assert go.labels(x, z, 0.4).tolist() == [[[2, -1]]] and abs(go.loss(x, z, 0.4) - l2) < 1e-15
    assert go.margins(x, z, 0.4)['guided_ties'] == 0


def test_a_single_class_guides_every_pixel_to_a_zero_loss():
    x, z = _logits((2, 1, 4, 4), 3), _logits((2, 1, 4, 4), 4)
    assert (go.labels(x, z, 0.95) == 0).all() and go.count(x, z, 0.95) == 32
    assert go.loss(x, z, 0.95) == 0.0 and not go.grad(x, z, 0.95).any()
    assert go.margins(x, z, 0.95)['gap'] == float('inf')


@pytest.mark.parametrize('shape,threshold', [((2, 2, 5, 7), 0.8), ((3, 6, 9, 31), 0.6), ((2, 80, 16, 16), 0.5)])
def test_the_oracle_is_cross_entropy_against_its_own_labels(shape, threshold):
    """torch float64 with autograd: F.cross_entropy(z, labels, ignore_index=-1, reduction='sum') / max(N, 1)"""
    x, z = _logits(shape, 21), _logits(shape, 22)
    lab = go.labels(x, z, threshold)
    n = go.count(x, z, threshold)
    assert 0 < n < lab.size
    zt = torch.from_numpy(z).double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(zt, torch.from_numpy(lab), ignore_index=-1, reduction='sum') / max(n, 1)
    want.backward()
    assert abs(go.loss(x, z, threshold) - want.item()) <= 1e-12 * abs(want.item())
    got = go.grad(x, z, threshold)
    assert got.shape == z.shape and np.abs(got - zt.grad.numpy()).max() <= 1e-12 * zt.grad.abs().max().item()
    # the labels: argmax of the mean of the two softmaxes, in torch
    e = (torch.softmax(torch.from_numpy(x).double(), 1) + torch.softmax(torch.from_numpy(z).double(), 1)) / 2
    m, a = e.max(1)
    assert np.array_equal(lab, torch.where(m > threshold, a, torch.full_like(a, -1)).numpy())


def test_logits_of_eighty_stay_finite_in_the_oracle():
    x, z = _logits((1, 3, 2, 2), 5), _logits((1, 3, 2, 2), 6)
    x[0, 0, 0, 0] = 80.0
    z[0, :, 0, 0] = (-80.0, 0.0, 0.0)               # p = (1, 0, 0), q = (e^-80 / 2, 1/2, 1/2): e = (1/2, 1/4, 1/4)
    assert go.labels(x, z, 0.45)[0, 0, 0] == 0      # -log q_0 = 80 + ln 2, where q_0 itself is below float32's range
    n = go.count(x, z, 0.45)
    assert np.isfinite(go.loss(x, z, 0.45)) and go.loss(x, z, 0.45) >= (80.0 + math.log(2.0)) / n


# -- the plugin as the driver sees it -------------------------------------------------------------------------------------
def test_the_plugin_as_the_driver_sees_it():
    import importlib
    import train
    import uda
    cls = uda.MultiLevelMaxSquaresMinimization
    assert cls is importlib.import_module('uda.max_squares_minimization').MultiLevelMaxSquaresMinimization
    assert 'MultiLevelMaxSquaresMinimization' in dir(uda) and 'MultiLevelMaxSquaresMinimization' in uda.__all__
    assert issubclass(cls, uda.Model) and issubclass(cls, uda.MaxSquaresMinimization)
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[1:] == ['max_squares_weight', 'aux_weight', 'threshold', 'optimizer']
    assert (params['aux_weight'].default, params['threshold'].default, params['optimizer'].default) == (0.1, 0.95, None)
    # the pinned neighbours stay as they are
    assert list(inspect.signature(uda.MaxSquaresMinimization.__init__).parameters)[1:] == ['max_squares_weight']
    from backends import dla
    assert list(inspect.signature(dla.build).parameters) == ['num_classes', 'num_keypoints', 'head_conv', 'down_ratio',
                                                             'freeze_base', 'rotated_boxes']
    got, args = train.plugin_from_config({'MultiLevelMaxSquaresMinimization': {'max_squares_weight': 0.3}})
    assert got is cls and args == {'max_squares_weight': 0.3}
    plugin = got(**args)
    from losses.max_square import GuidanceLoss, MaxSquareLoss
    assert isinstance(plugin.max_squares_loss, MaxSquareLoss) and isinstance(plugin.guidance_loss, GuidanceLoss)
    assert plugin.guidance_loss.threshold == 0.95 and plugin.aux_weight == 0.1 and plugin.max_squares_weight == 0.3
    assert plugin.target_grad_heads == ('hm',) and plugin.low_level_head is None


def test_the_readme_override_resolves_through_the_config():
    import train
    import uda
    from utils.config import load_config
    cfg = load_config(os.path.join(ROOT, 'centernet-uda_amd', 'configs'), ['experiment=max_squares_minimization', OVERRIDE])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is uda.MultiLevelMaxSquaresMinimization and args == {'max_squares_weight': 0.3, 'aux_weight': 0.1}
    assert OVERRIDE in open(os.path.join(ROOT, 'README.md')).read()


@pytest.mark.parametrize('bad', [1.0, 1.5, -0.1, float('nan')])
def test_a_threshold_outside_the_half_open_unit_interval_is_refused(bad):
    import uda
    from hip_runtime import ops
    from losses.max_square import GuidanceLoss
    with pytest.raises(ValueError, match='threshold'):
        uda.MultiLevelMaxSquaresMinimization(0.3, threshold=bad)
    with pytest.raises(ValueError, match='threshold'):
        GuidanceLoss(bad)
    with pytest.raises(ValueError, match='threshold'):
        ops.guidance_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), bad)
    with pytest.raises(ValueError, match='threshold'):
        ops.guidance_labels(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), bad)


def test_the_accepted_arguments():
    import uda
    from losses.max_square import GuidanceLoss
    assert GuidanceLoss().threshold == 0.95 and GuidanceLoss(0).threshold == 0.0
    assert uda.MultiLevelMaxSquaresMinimization(0.3, aux_weight=0).aux_weight == 0.0
    with pytest.raises(ValueError, match='aux_weight'):
        uda.MultiLevelMaxSquaresMinimization(0.3, aux_weight=-1.0)


def test_no_cpu_fallback():
    from hip_runtime import ops
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.guidance_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.guidance_labels(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


def _cfg(name, **params):
    return types.SimpleNamespace(model=types.SimpleNamespace(backend=types.SimpleNamespace(
        name=name, params=types.SimpleNamespace(**params))))


def test_a_backend_without_the_tap_is_refused_by_name():
    import uda
    from backends import resnet
    plugin = uda.MultiLevelMaxSquaresMinimization(0.3)
    plugin.backend = resnet.build(num_layers=18, num_classes=6, pretrained=False)
    plugin.cfg = _cfg('resnet', num_classes=6, num_layers=18)
    with pytest.raises(ValueError, match='resnet'):
        plugin.init_done()
    assert plugin.low_level_head is None


def test_init_done_builds_the_head_and_its_optimizer_on_dla():
    import uda
    from backends import dla
    from hip_runtime import nn as hnn
    from hip_runtime import optim
    plugin = uda.MultiLevelMaxSquaresMinimization(0.3)
    plugin.backend = dla.DLASeg('dla34', {'hm': 6, 'wh': 2, 'reg': 2}, pretrained=False, down_ratio=4, final_kernel=1,
                                last_level=5, head_conv=64)
    before = list(plugin.backend.state_dict())
    plugin.cfg = _cfg('dla', num_classes=6, head_conv=64)
    plugin.init_done()
    head = plugin.low_level_head
    assert isinstance(head, hnn.Head) and list(head.state_dict()) == ['0.weight', '0.bias', '2.weight', '2.bias']
    assert tuple(head[0].weight.shape) == (64, 64, 3, 3) and tuple(head[2].weight.shape) == (6, 64, 1, 1)
    assert torch.equal(head[2].bias, torch.full((6,), -2.19))
    assert isinstance(plugin.low_level_optimizer, optim.Adam) and plugin.low_level_scheduler is None
    assert list(plugin.backend.state_dict()) == before               # the head is the plugin's, not the backend's
    assert plugin.backend.low_level_channels == 64


# -- the backend's tap ----------------------------------------------------------------------------------------------------
def _seg():
    from backends import dla
    return dla.DLASeg('dla34', {'hm': 3, 'wh': 2}, pretrained=False, down_ratio=4, final_kernel=1, last_level=5,
                      head_conv=64)


def test_the_tap_adds_exactly_one_read_to_the_alias_plan():
    from backends import dla
    seg = _seg()
    keys = list(seg.state_dict())
    off, on = dla._FanPlan(seg, 6), dla._FanPlan(seg, 6, low_level=True)
    assert off.n_ids == on.n_ids
    more = {k: on.reads[k] - off.reads[k] for k in set(on.reads) | set(off.reads) if on.reads[k] != off.reads[k]}
    assert list(more.values()) == [1], more
    (tap,) = more
    assert off.reads[tap] == 1                  # the final IDAUp's skip was its only reader
    # the default plan is what it was: the same counts as a plan that never heard of the tap
    assert dict(dla._FanPlan(seg, 6, low_level=False).reads) == dict(off.reads)
    assert sum(off.reads.values()) + 1 == sum(on.reads.values())
    assert list(seg.state_dict()) == keys and not any('low' in k for k in keys)
    # features() and forward() keep their signatures; the tap has methods of its own
    assert list(inspect.signature(seg.features).parameters) == ['x'] and list(inspect.signature(seg.forward).parameters) == ['x']
    assert list(inspect.signature(seg.features_with_low_level).parameters) == ['x']
    assert list(inspect.signature(seg.forward_low_level).parameters) == ['x', 'low_level_head']
    fd = inspect.signature(seg.forward_domains).parameters
    assert list(fd) == ['source', 'target', 'target_grad_heads', 'low_level_head'] and fd['low_level_head'].default is None


@pytest.mark.parametrize('low_level', [False, True])
def test_every_alias_has_one_reader_with_and_without_the_tap(low_level):
    """tests/test_host_fan_plan.py's walk (modules replaced by pass-throughs) with the tap on: no alias left over, no
    reader without one, and the tapped tensor is the finest map of the aggregation."""
    from unittest import mock
    from backends import dla
    from hip_runtime import nn as hnn
    seg = _seg()
    feats = [torch.zeros(1, c, 4, 4, requires_grad=True) for c in seg.base.channels]
    pools, fallbacks = [], []
    real_init, real_take = dla._Aliases.__init__, dla._Aliases.take

    def init(self, t, n):
        real_init(self, t, n)
        pools.append((self, n))

    def take(self):
        if self.pool is not None and not self.pool:
            fallbacks.append(self)
        return real_take(self)

    with mock.patch.object(dla.DeformConv, 'forward', lambda self, x: x), \
            mock.patch.object(hnn.DepthwiseConvTranspose2d, 'forward', lambda self, x, skip=None: x if skip is None else x + 0 * skip.sum()), \
            mock.patch.object(type(seg.base), 'forward', lambda self, x: list(feats)), \
            mock.patch.object(dla._Aliases, '__init__', init), mock.patch.object(dla._Aliases, 'take', take):
        x = torch.zeros(1, 3, 16, 16)
        got = seg.features_with_low_level(x) if low_level else seg.features(x)
    assert not fallbacks, 'a tensor had more readers than the plan gave it aliases'
    left = [(n, len(a.pool)) for a, n in pools if a.pool]
    assert not left, 'aliases without a reader: %s' % left
    if low_level:
        y, low = got
        assert y.requires_grad and low.requires_grad and low.shape == y.shape
        assert seg._fan_plan is None and seg._fan_plan_low is not None
    else:
        assert torch.is_tensor(got) and seg._fan_plan is not None and seg._fan_plan_low is None


# -- the C ABI ------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    import hip_runtime as hr
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(hr.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(lib, name), name
        restype, argtypes = getattr(hr._Sig, name)
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p, name
    assert len(hr._Sig.cnuda_guidance_forward[1]) == 11
    assert len(hr._Sig.cnuda_guidance_backward[1]) == 9
    assert hr.lib().cnuda_abi_version() == 2
    for name in SYMBOLS:
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read(), name


def test_bad_arguments_return_minus_one_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    one = ctypes.c_void_p(256)        # any non-null address: the refusals below come before anything reads it
    assert L.cnuda_guidance_forward(None, None, 0.95, None, None, 1, 3, 16, None, 0, None) == -1
    assert b'cnuda_guidance_forward' in L.cnuda_last_error()
    for missing in range(4):          # every pointer on its own
        ptrs = [None if k == missing else one for k in range(4)]
        assert L.cnuda_guidance_forward(ptrs[0], ptrs[1], 0.95, ptrs[2], ptrs[3], 1, 3, 16, one, 1 << 20, None) == -1
    assert L.cnuda_guidance_forward(one, one, 0.95, one, one, 0, 3, 16, one, 1 << 20, None) == -1
    assert L.cnuda_guidance_forward(one, one, 0.95, one, one, 1, 0, 16, one, 1 << 20, None) == -1
    assert L.cnuda_guidance_forward(one, one, 0.95, one, one, 1, 3, 0, one, 1 << 20, None) == -1
    assert L.cnuda_guidance_forward(one, one, 1.0, one, one, 1, 3, 16, one, 1 << 20, None) == -1
    assert b'threshold' in L.cnuda_last_error()
    assert L.cnuda_guidance_forward(one, one, -0.5, one, one, 1, 3, 16, one, 1 << 20, None) == -1
    assert L.cnuda_guidance_forward(one, one, 0.95, one, one, 1, 3, 16, None, 0, None) == -1
    assert b'workspace' in L.cnuda_last_error()
    assert L.cnuda_guidance_forward(one, one, 0.95, one, one, 1, 3, 16, one, 8, None) == -1
    assert L.cnuda_guidance_backward(None, None, None, None, None, 1, 3, 16, None) == -1
    assert b'cnuda_guidance_backward' in L.cnuda_last_error()
    for missing in range(5):
        ptrs = [None if k == missing else one for k in range(5)]
        assert L.cnuda_guidance_backward(*ptrs, 1, 3, 16, None) == -1
    assert L.cnuda_guidance_backward(one, one, one, one, one, 1, 3, 0, None) == -1
