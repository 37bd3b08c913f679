"""No-GPU checks of image-wise class-balanced max-squares: the float64 oracle against an independent torch statement
of the published form, the ratio = 0 identity with MaxSquareLoss, the plugin as the driver sees it, and the C ABI's
refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import iw_maxsq_oracle as iwo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cnuda_argmax_histogram', 'cnuda_iw_max_square_forward', 'cnuda_iw_max_square_backward')


def _logits(shape, seed):
    return (np.random.RandomState(seed).standard_normal(shape) * 5).astype(np.float32)


def _published(x, ratio):
    """The authors' IW_MaxSquareloss in torch float64 (softmax, torch.max, a bincount per image, the weights detached),
    divided by 2 -> (loss, d loss / d x)"""
    x = torch.from_numpy(x).double().requires_grad_(True)
    B, C = x.shape[:2]
    prob = torch.softmax(x, dim=1)
    _, argpred = torch.max(x, 1)                    # first maximum, like np.argmax
    weights = []
    for b in range(B):
        hist = torch.bincount(argpred[b].reshape(-1), minlength=C).double()
        weights.append(1 / torch.max(hist ** ratio * hist.sum() ** (1 - ratio), torch.ones(1, dtype=torch.float64)))
    weights = torch.stack(weights).detach()         # [B, C]
    wp = torch.gather(weights, 1, argpred.reshape(B, -1)).reshape(argpred.shape).unsqueeze(1)
    loss = -torch.sum(prob ** 2 * wp) / (B * C) / 2
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize('shape', [(2, 2, 5, 7), (3, 6, 9, 31), (2, 80, 16, 16)])
@pytest.mark.parametrize('ratio', [0.0, 0.2, 1.0])
def test_the_oracle_is_the_published_form(shape, ratio):
    x = _logits(shape, 11)
    want_loss, want_grad = _published(x, ratio)
    assert abs(iwo.loss(x, ratio) - want_loss) <= 1e-12 * abs(want_loss)
    got = iwo.grad(x, ratio)
    assert got.shape == x.shape and np.abs(got - want_grad).max() <= 1e-12 * np.abs(want_grad).max()
    h = iwo.hist(x)
    assert h.shape == shape[:2] and (h.sum(1) == shape[2] * shape[3]).all()


def test_the_oracle_counts_the_lowest_channel_on_a_tie():
    x = np.zeros((1, 3, 2, 2), np.float32)
    x[0, :, 0, 1] = (1, 3, 3)
    x[0, :, 1, 0] = (2, -1, 2)
    assert iwo.hist(x).tolist() == [[3, 1, 0]]
    assert iwo.weights(x, 1.0).tolist() == [[1 / 3, 1.0, 1.0]]          # the empty class: max(0, 1)


def test_ratio_zero_is_max_square_loss():
    from oracle import losses as ol
    x = _logits((3, 6, 9, 31), 12)
    want = ol.max_square_loss(torch.from_numpy(x).double()).item()
    assert abs(iwo.loss(x, 0.0) - want) <= 1e-12 * abs(want)


def test_the_plugin_as_the_driver_sees_it():
    import importlib
    import train
    import uda
    cls = uda.IWMaxSquaresMinimization
    assert cls is importlib.import_module('uda.max_squares_minimization').IWMaxSquaresMinimization
    assert 'IWMaxSquaresMinimization' in dir(uda) and 'IWMaxSquaresMinimization' in uda.__all__
    assert issubclass(cls, uda.Model) and issubclass(cls, uda.MaxSquaresMinimization)
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[1:] == ['max_squares_weight', 'ratio'] and params['ratio'].default == 0.2
    got, args = train.plugin_from_config({'IWMaxSquaresMinimization': {'max_squares_weight': 0.3}})
    assert got is cls and args == {'max_squares_weight': 0.3}
    plugin = got(**args)
    from losses.max_square import IWMaxSquareLoss
    assert isinstance(plugin.max_squares_loss, IWMaxSquareLoss) and plugin.max_squares_loss.ratio == 0.2
    assert plugin.max_squares_weight == 0.3 and plugin.target_grad_heads == ('hm',)
    assert got(0.3, ratio=1.0).max_squares_loss.ratio == 1.0 and got(0.3, ratio=0).max_squares_loss.ratio == 0.0


def test_the_readme_override_resolves_through_the_config():
    import train
    import uda
    from utils.config import load_config
    override = "model.uda={IWMaxSquaresMinimization: {max_squares_weight: 0.3, ratio: 0.2}}"
    cfg = load_config(os.path.join(ROOT, 'centernet-uda_amd', 'configs'), ['experiment=max_squares_minimization', override])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is uda.IWMaxSquaresMinimization and args == {'max_squares_weight': 0.3, 'ratio': 0.2}
    assert override in open(os.path.join(ROOT, 'README.md')).read()


@pytest.mark.parametrize('bad', [1.5, -0.1])
def test_a_ratio_outside_the_unit_interval_is_refused(bad):
    import uda
    from hip_runtime import ops
    from losses.max_square import IWMaxSquareLoss
    with pytest.raises(ValueError, match='ratio'):
        uda.IWMaxSquaresMinimization(0.3, ratio=bad)
    with pytest.raises(ValueError, match='ratio'):
        IWMaxSquareLoss(bad)
    with pytest.raises(ValueError, match='ratio'):
        ops.iw_max_square_loss(torch.zeros(1, 3, 4, 4), bad)


def test_no_cpu_fallback():
    from hip_runtime import ops
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.iw_max_square_loss(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.class_histogram(torch.zeros(1, 3, 4, 4))


def test_the_symbols_are_declared_exported_and_bound():
    import hip_runtime as hr
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(hr.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(lib, name), name
        restype, argtypes = getattr(hr._Sig, name)
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p, name
    assert len(hr._Sig.cnuda_argmax_histogram[1]) == 6
    assert len(hr._Sig.cnuda_iw_max_square_forward[1]) == 11
    assert len(hr._Sig.cnuda_iw_max_square_backward[1]) == 8
    assert hr.lib().cnuda_abi_version() == 2


def test_bad_arguments_return_minus_one_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    one = ctypes.c_void_p(256)        # any non-null address: the refusals below come before anything reads it
    assert L.cnuda_argmax_histogram(None, None, 1, 3, 16, None) == -1
    assert b'cnuda_argmax_histogram' in L.cnuda_last_error()
    assert L.cnuda_argmax_histogram(one, one, 1, 1025, 16, None) == -1
    assert b'1025' in L.cnuda_last_error() and b'1024' in L.cnuda_last_error()
    assert L.cnuda_argmax_histogram(one, one, 0, 3, 16, None) == -1
    assert L.cnuda_iw_max_square_forward(None, None, 0.2, None, None, 1, 3, 16, None, 0, None) == -1
    assert b'cnuda_iw_max_square_forward' in L.cnuda_last_error()
    assert L.cnuda_iw_max_square_forward(one, one, 0.2, one, one, 1, 1025, 16, one, 1 << 20, None) == -1
    assert b'1024' in L.cnuda_last_error()
    assert L.cnuda_iw_max_square_forward(one, one, 1.5, one, one, 1, 3, 16, one, 1 << 20, None) == -1
    assert b'ratio' in L.cnuda_last_error()
    assert L.cnuda_iw_max_square_forward(one, one, 0.2, one, one, 1, 3, 16, None, 0, None) == -1
    assert b'workspace' in L.cnuda_last_error()
    assert L.cnuda_iw_max_square_backward(None, None, None, None, 1, 3, 16, None) == -1
    assert b'cnuda_iw_max_square_backward' in L.cnuda_last_error()
