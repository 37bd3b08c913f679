"""No-GPU checks of the dense teacher: the float64 oracle against a hand-worked picture and against torch.autograd, its tie
rule, the plugin as the driver sees it, and the C ABI's refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_teacher_oracle as dto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cnuda_dense_select', 'cnuda_dense_teacher_forward', 'cnuda_dense_teacher_backward')
README_OVERRIDE = 'model.uda={DenseTeacher: {pseudo_weight: 1.0, ratio: 0.01, burn_in_steps: 2000}}'


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _bce(x, y):
    return max(x, 0.0) - x * y + np.log1p(np.exp(-abs(x)))


def test_the_oracle_on_a_hand_worked_picture():
    """B = 1, C = 2, a 2 x 3 map, ratio 0.4 -> k = floor(2.4) = 2.  Channel maxima (row-major): 0, 2, -1 / 1, -3, 0.5: the two
    largest are 2 at (0, 1) and 1 at (1, 0), tau = 1.  With the mirror the student's cells are (0, 1) (the middle column
    is its own mirror) and (1, 2).  Every student logit is 0 (q = 1/2, bce = ln 2 - 0 * y) and every student size 1."""
    t_hm = np.float32([[[[0, 2, -1], [1, -3, 0.5]],
                        [[-1, 0, -2], [-1, -4, -5]]]])
    t_wh = np.float32([[[[9, 3, 9], [0.5, 9, 9]],
                        [[9, 1, 9], [4, 9, 9]]]])
    x_hm, x_wh = np.zeros((1, 2, 2, 3), np.float32), np.ones((1, 2, 2, 3), np.float32)
    assert dto.k_of(0.4, 6) == 2 and dto.k_of(0.01, 6) == 1 and dto.k_of(1.0, 6) == 6
    tau, count, mask = dto.select(t_hm, 0.4)
    assert tau.dtype == np.float32 and tau.tolist() == [1.0] and count.dtype == np.int32 and count.tolist() == [2]
    assert mask.tolist() == [[[False, True, False], [True, False, False]]]
    ln2 = np.log(2.0)
    # the selected cells' four targets y, each against q = 1/2; the eight unselected entries have y = 0
    ys = [_sig(2.0), _sig(0.0), _sig(1.0), _sig(-1.0)]
    hm_sum = sum((y - 0.5) ** 2 * (ln2 - 0.0 * y) for y in ys) + 8 * 0.25 * ln2
    u = [_sig(2.0), _sig(1.0)]
    wh_sum = u[0] * (abs(1 - 3) + abs(1 - 1)) + u[1] * (abs(1 - 0.5) + abs(1 - 4))
    for mirror in (False, True):
        total, hm_loss, wh_loss, n, su = dto.loss(x_hm, x_wh, t_hm, t_wh, 0.4, mirror, hm_weight=2.0, wh_weight=0.5)
        assert n == 2 and abs(su - sum(u)) < 1e-14
        assert abs(hm_loss - hm_sum / 2) < 1e-14 and abs(wh_loss - wh_sum / (sum(u) + 1e-4)) < 1e-14
        assert abs(total - (2.0 * hm_loss + 0.5 * wh_loss)) < 1e-14
        g_hm, g_wh = dto.grad(x_hm, x_wh, t_hm, t_wh, 0.4, mirror, hm_weight=2.0, wh_weight=0.5, upstream=3.0)
        col = 2 if mirror else 0                      # where the student sees the teacher's (1, 0)
        # student (1, col), size channel 0: 1 - 0.5 > 0; channel 1: 1 - 4 < 0; (0, 1) channel 1: 1 - 1 = 0 -> sign 0
        k = 3.0 * 0.5 / (sum(u) + 1e-4)
        assert abs(g_wh[0, 0, 1, col] - k * u[1]) < 1e-14 and abs(g_wh[0, 1, 1, col] + k * u[1]) < 1e-14
        assert g_wh[0, 1, 0, 1] == 0.0 and abs(g_wh[0, 0, 0, 1] + k * u[0]) < 1e-14
        assert np.count_nonzero(g_wh) == 3
        # heat map at an unselected cell: y = 0, q = 1/2: (1/2) (1/4 + 2 (1/4) ln 2) / N
        assert abs(g_hm[0, 0, 0, 2 - col] - 3.0 * 2.0 * 0.5 * (0.25 + 0.5 * ln2) / 2) < 1e-14
        y = ys[2]                                     # channel 0 of the teacher's (1, 0)
        want = (0.5 - y) * ((0.5 - y) ** 2 + 0.5 * _bce(0.0, y)) / 2
        assert abs(g_hm[0, 0, 1, col] - 3.0 * 2.0 * want) < 1e-14


def _random_case(shape, seed, scale=3.0):
    rs = np.random.RandomState(seed)
    B, C, H, W = shape
    t_hm = (rs.standard_normal(shape) * scale).astype(np.float32)
    x_hm = (rs.standard_normal(shape) * scale).astype(np.float32)
    t_wh = rs.uniform(0.5, 9, (B, 2, H, W)).astype(np.float32)
    x_wh = rs.uniform(0.5, 9, (B, 2, H, W)).astype(np.float32)
    return x_hm, x_wh, t_hm, t_wh


@pytest.mark.parametrize('mirror', [False, True], ids=['plain', 'mirror'])
@pytest.mark.parametrize('shape, ratio', [((2, 4, 6, 11), 0.05), ((1, 80, 8, 12), 0.01), ((2, 3, 9, 8), 1.0)])
def test_the_oracles_gradient_is_autograds(shape, ratio, mirror):
    """The written-out derivatives against torch.autograd on the float64 formula, the selection taken from the oracle."""
    x_hm, x_wh, t_hm, t_wh = _random_case(shape, 5)
    _, count, mask = dto.select(t_hm, ratio)
    m = torch.from_numpy(mask)[:, None]
    flip = (lambda t: t.flip(-1)) if mirror else (lambda t: t)
    T, Twh = flip(torch.from_numpy(t_hm).double()), flip(torch.from_numpy(t_wh).double())
    m = flip(m)
    X = torch.from_numpy(x_hm).double().requires_grad_(True)
    Xwh = torch.from_numpy(x_wh).double().requires_grad_(True)
    y = torch.where(m, torch.sigmoid(T), torch.zeros_like(T))
    u = torch.where(m, torch.sigmoid(T.max(1, keepdim=True).values), torch.zeros_like(T[:, :1]))
    bce = torch.nn.functional.binary_cross_entropy_with_logits(X, y, reduction='none')
    hm_loss = ((y - torch.sigmoid(X)) ** 2 * bce).sum() / max(int(count.sum()), 1)
    wh_loss = (u * (Xwh - Twh).abs()).sum() / (u.sum() + 1e-4)
    total = 1.5 * hm_loss + 0.3 * wh_loss
    (0.7 * total).backward()
    got = dto.loss(x_hm, x_wh, t_hm, t_wh, ratio, mirror, hm_weight=1.5, wh_weight=0.3)
    assert abs(got[0] - total.item()) <= 1e-13 * abs(total.item())
    assert abs(got[1] - hm_loss.item()) <= 1e-13 * hm_loss.item() and abs(got[2] - wh_loss.item()) <= 1e-13 * wh_loss.item()
    g_hm, g_wh = dto.grad(x_hm, x_wh, t_hm, t_wh, ratio, mirror, hm_weight=1.5, wh_weight=0.3, upstream=0.7)
    assert np.abs(g_hm - X.grad.numpy()).max() <= 1e-13 * np.abs(X.grad.numpy()).max()
    assert np.abs(g_wh - Xwh.grad.numpy()).max() <= 1e-13 * np.abs(Xwh.grad.numpy()).max()


def test_the_oracles_tie_rule():
    # a plateau across the k-th rank selects all of it: k = 3, values 5, 4, 4, 4, 4, 1, ...
    t = np.full((1, 1, 4, 5), -2.0, np.float32)
    t[0, 0, 0, :5] = (4, 5, 4, 1, 4)
    t[0, 0, 3, 2] = 4
    tau, count, mask = dto.select(t, 0.16)
    assert dto.k_of(0.16, 20) == 3 and tau.tolist() == [4.0] and count.tolist() == [5]
    assert mask.sum() == 5 and mask[0, 0, :3].all() and mask[0, 0, 4] and mask[0, 3, 2] and not mask[0, 0, 3]
    # -0.0 and +0.0 are one value: both are selected, tau is +0
    t = np.full((1, 2, 2, 4), -1.0, np.float32)
    t[0, 0, 0, 0], t[0, 1, 0, 1], t[0, 0, 1, 3], t[0, 0, 1, 0] = 3.0, -0.0, 0.0, -0.0
    tau, count, mask = dto.select(t, 2 / 8)
    assert tau.tolist() == [0.0] and not np.signbit(tau[0]) and count.tolist() == [4]
    assert mask.tolist() == [[[True, True, False, False], [True, False, False, True]]]
    # a NaN is never selected, not even with ratio = 1; a NaN in ANY channel makes the position's score NaN
    t = np.float32([[[[1, np.nan, 3], [0, -1, 2]], [[5, 0, np.nan], [0, 0, 0]]]])
    tau, count, mask = dto.select(t, 1.0)
    assert tau.tolist() == [-np.inf] and count.tolist() == [4]
    assert mask.tolist() == [[[True, False, False], [True, True, True]]]
    tau, count, mask = dto.select(t, 0.5)             # k = 3 of the four numbers 5, 2, 0, 0: both zeros
    assert tau.tolist() == [0.0] and count.tolist() == [4]
    # a whole image of NaN selects nothing, its neighbour is untouched
    t = np.stack([np.full((2, 2, 3), np.nan, np.float32), np.arange(12, dtype=np.float32).reshape(2, 2, 3)])
    tau, count, mask = dto.select(t, 0.2)
    assert count.tolist() == [0, 1] and not mask[0].any() and tau[1] == 11.0
    total, hm_loss, wh_loss, n, su = dto.loss(np.zeros_like(t), np.ones((2, 2, 2, 3), np.float32), t,
                                              np.ones((2, 2, 2, 3), np.float32), 0.2, False)
    assert n == 1 and np.isfinite(total) and wh_loss == 0.0
    # +-inf logits order like any number
    t = np.float32([[[[np.inf, 1, -np.inf, 2]]]])
    assert dto.select(t, 0.25)[0].tolist() == [np.inf] and dto.select(t, 1.0)[0].tolist() == [-np.inf]
    assert dto.select(t, 1.0)[1].tolist() == [4]


def test_the_plugin_as_the_driver_sees_it():
    import importlib
    import train
    import uda
    from utils.config import load_config
    cls = uda.DenseTeacher
    assert cls is importlib.import_module('uda.mean_teacher').DenseTeacher
    assert 'DenseTeacher' in dir(uda) and 'DenseTeacher' in uda.__all__
    assert issubclass(cls, uda.Model) and issubclass(cls, uda.WeakStrongTeacher)
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[1:] == ['pseudo_weight', 'ratio', 'hm_weight', 'wh_weight', 'strong_view', 'decay',
                                'burn_in_steps', 'mirror_student', 'evaluate_teacher']
    assert [params[k].default for k in list(params)[2:]] == [0.01, 1.0, 0.1, None, 0.999, 0, True, False]
    assert cls.target_grad_heads == ('hm', 'wh')
    cfg = load_config(os.path.join(ROOT, 'centernet-uda_amd', 'configs'), ['experiment=dla_baseline', README_OVERRIDE])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is cls and args == {'pseudo_weight': 1.0, 'ratio': 0.01, 'burn_in_steps': 2000}
    plugin = got(**args)
    assert (plugin.pseudo_weight, plugin.ratio, plugin.hm_weight, plugin.wh_weight) == (1.0, 0.01, 1.0, 0.1)
    assert plugin.burn_in_steps == 2000 and plugin.mirror_student and plugin.strong_view is not None
    assert cls(1.0, strong_view=False).strong_view is None
    assert "'" + README_OVERRIDE + "'" in open(os.path.join(ROOT, 'README.md')).read()
    # what the parents' signatures were
    assert list(inspect.signature(uda.WeakStrongTeacher.__init__).parameters)[1:] == [
        'pseudo_weight', 'strong_view', 'mean_teacher_arguments']
    assert 'score_threshold' in inspect.signature(uda.MeanTeacher.__init__).parameters


def test_constructor_validation():
    import uda
    for name in ('score_threshold', 'min_size'):
        with pytest.raises(TypeError, match=name):
            uda.DenseTeacher(1.0, **{name: 0.5})
    for bad in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            uda.DenseTeacher(1.0, ratio=bad)
    with pytest.raises(ValueError, match='wh_weight'):
        uda.DenseTeacher(1.0, wh_weight=-1.0)
    with pytest.raises(ValueError, match='pseudo_weight'):
        uda.DenseTeacher(-1.0)
    with pytest.raises(ValueError, match='decay'):
        uda.DenseTeacher(1.0, decay=1.0)
    assert uda.DenseTeacher(1.0, ratio=1.0).ratio == 1.0


def test_the_ops_refuse_a_bad_ratio_and_cpu_tensors():
    from hip_runtime import ops
    z = torch.zeros
    for bad in (0.0, 1.5, -0.2):
        with pytest.raises(ValueError, match='ratio'):
            ops.dense_select(z(1, 3, 4, 4), bad)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.dense_select(z(1, 3, 4, 4), 0.1)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 4), z(1),
                               z(1, dtype=torch.int32), mirror=True)
    with pytest.raises(RuntimeError, match='teacher_hm requires grad'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4, requires_grad=True), z(1, 2, 4, 4), z(1),
                               z(1, dtype=torch.int32), mirror=True)
    with pytest.raises(RuntimeError, match='teacher_wh is'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 5), z(1),
                               z(1, dtype=torch.int32), mirror=True)


def test_the_symbols_are_declared_exported_and_bound():
    import hip_runtime as hr
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(hr.LIB_PATH)
    for name in SYMBOLS + ('cnuda_dense_select_workspace_bytes',):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(lib, name), name
        assert hasattr(hr._Sig, name), name
    for name in SYMBOLS:
        restype, argtypes = getattr(hr._Sig, name)
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p, name
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read(), name
    assert len(hr._Sig.cnuda_dense_select[1]) == 10 and hr._Sig.cnuda_dense_select[1][1] is ctypes.c_double
    assert len(hr._Sig.cnuda_dense_teacher_forward[1]) == 17
    assert len(hr._Sig.cnuda_dense_teacher_backward[1]) == 17
    assert hr.lib().cnuda_abi_version() == 2


def test_bad_arguments_return_minus_one_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    one = ctypes.c_void_p(256)        # any non-null address: the refusals below come before anything reads it
    big = 1 << 20
    assert L.cnuda_dense_select_workspace_bytes(2, 66) >= 2 * 66 * 4
    assert L.cnuda_dense_select_workspace_bytes(0, 66) == 0 and L.cnuda_dense_select_workspace_bytes(1, 0) == 0
    assert L.cnuda_dense_select(None, 0.01, None, None, 1, 3, 16, None, 0, None) == -1
    assert b'cnuda_dense_select' in L.cnuda_last_error()
    for B, C, HW in ((0, 3, 16), (1, 0, 16), (1, 3, 0), (1, 3, 1 << 31)):
        assert L.cnuda_dense_select(one, 0.01, one, one, B, C, HW, one, big, None) == -1, (B, C, HW)
    for bad in (0.0, -0.5, 1.0001, float('nan')):
        assert L.cnuda_dense_select(one, bad, one, one, 1, 3, 16, one, big, None) == -1, bad
        assert b'ratio' in L.cnuda_last_error()
    assert L.cnuda_dense_select(one, 0.01, one, one, 1, 1025, 16, one, big, None) == -1
    assert b'1025' in L.cnuda_last_error() and b'1024' in L.cnuda_last_error()
    assert L.cnuda_dense_select(one, 0.01, one, one, 1, 3, 16, one, 16, None) == -1
    assert b'workspace' in L.cnuda_last_error()
    fwd = lambda B, C, H, W, ws=big: L.cnuda_dense_teacher_forward(one, one, one, one, one, one, one, B, C, H, W, 1, 1.0,
                                                                    0.1, one, ws, None)
    bwd = lambda B, C, H, W: L.cnuda_dense_teacher_backward(one, one, one, one, one, one, one, one, one, B, C, H, W, 1,
                                                            1.0, 0.1, None)
    for call, name in ((fwd, b'cnuda_dense_teacher_forward'), (bwd, b'cnuda_dense_teacher_backward')):
        for shape in ((0, 3, 4, 4), (1, 0, 4, 4), (1, 3, 0, 4), (1, 3, 4, -1), (1, 3, 1 << 16, 1 << 16)):
            assert call(*shape) == -1, shape
            assert name in L.cnuda_last_error()
        assert call(1, 1025, 4, 4) == -1 and b'1024' in L.cnuda_last_error()
    assert fwd(1, 3, 4, 4, ws=16) == -1 and b'workspace' in L.cnuda_last_error()
    assert L.cnuda_dense_teacher_forward(None, one, one, one, one, one, one, 1, 3, 4, 4, 1, 1.0, 0.1, one, big, None) == -1
    assert L.cnuda_dense_teacher_backward(one, one, one, one, one, one, None, one, one, 1, 3, 4, 4, 1, 1.0, 0.1, None) == -1
