"""Dense teacher on the GPU: the kernels of csrc/dense.hip against the float64 oracle (tests/dense_teacher_oracle.py) -- the
selection exactly, the loss and its gradients at the tolerances of tests/test_gpu_iw_max_squares.py -- and the plugin
`uda.DenseTeacher` through its training step, burn-in, checkpoints and the driver."""
import ast
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import coco_fixture as fx
import dense_teacher_oracle as dto
import inputs as gin
import strong_view_helpers as sh
from strong_view_helpers import G, N, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

LOSS_RTOL = 1e-5            # tests/test_gpu_iw_max_squares.py: the loss, relative
GRAD_TOL = 1e-4             # ... and each gradient, of its own largest magnitude

# [B, C, H, W]: HW = 66 (no multiple of 4, 64 or 256); C = 1; COCO's classes on a tiny map; several workgroups per image;
# 43264 scores = 169 KiB, more than the 32768 keys the select keeps on chip.  W = 11 and 7 take the scalar walk of the loss,
# 12, 48 and 208 the 16-byte one.
SHAPES = [(2, 4, 6, 11), (2, 1, 5, 7), (1, 80, 8, 12), (2, 3, 32, 48), (1, 2, 208, 208)]
RATIOS = [1e-6, 0.01, 0.05, 1.0]          # k = 1; the default; five times it; everything
_CASES = {}


def _case(shape):
    """Logits of standard deviation 3 (the selected targets span (0, 1)), sizes in [0.5, 9); made once per shape."""
    if shape not in _CASES:
        rs = np.random.RandomState(sum(shape))
        B, C, H, W = shape
        c = {'t_hm': (rs.standard_normal(shape) * 3).astype(F), 'x_hm': (rs.standard_normal(shape) * 3).astype(F),
             't_wh': rs.uniform(0.5, 9, (B, 2, H, W)).astype(F), 'x_wh': rs.uniform(0.5, 9, (B, 2, H, W)).astype(F)}
        for v in c.values():
            v.setflags(write=False)
        _CASES[shape] = c
    return _CASES[shape]


def _select(t_hm, ratio):
    from hip_runtime import ops
    tau, count = ops.dense_select(G(t_hm), ratio)
    torch.cuda.synchronize()
    return N(tau), N(count)


def _check_select(t_hm, ratio):
    want_tau, want_count, want_mask = dto.select(t_hm, ratio)
    tau, count = _select(t_hm, ratio)
    assert count.dtype == np.int32 and count.tolist() == want_count.tolist(), (count, want_count)
    assert same_bits(tau, want_tau), (tau, want_tau)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(dto.scores(t_hm) >= tau[:, None, None], want_mask)
    return want_tau, want_count, want_mask


# ---------------------------------------------------------------------------------------------------------------------
# cnuda_dense_select
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ratio', RATIOS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dense_select_is_the_oracles_exactly(shape, ratio):
    tau, count, mask = _check_select(_case(shape)['t_hm'], ratio)
    k = dto.k_of(ratio, shape[2] * shape[3])
    assert (count >= k).all() and (ratio > 1e-6 or k == 1)
    if ratio == 1.0:
        assert mask.all()


@pytest.mark.parametrize('shape', [(2, 3, 6, 11), (1, 2, 208, 208)], ids=['on-chip', 'off-chip'])
def test_dense_select_on_constructed_inputs(shape):
    B, C, H, W = shape
    HW = H * W
    rs = np.random.RandomState(7)
    base = (-np.abs(rs.standard_normal(shape)) * 2 - 1).astype(F)      # everything below -0 to start with
    assert base.max() < -0.5
    # a plateau of equal maxima straddling rank k: 2 values above it, 7 equal ones, k = 5
    t = base.copy()
    cells = rs.choice(HW, 9, replace=False)
    flat = t.reshape(B, C, HW)
    flat[:, 0, cells[:2]] = (9.0, 8.0)
    flat[:, C - 1, cells[2:]] = 1.25
    ratio = 5.5 / HW
    assert dto.k_of(ratio, HW) == 5
    tau, count, _ = _check_select(t, ratio)
    assert tau.tolist() == [1.25] * B and count.tolist() == [9] * B
    # -0.0 beside +0.0 at the threshold: both are selected, tau is +0
    t = base.copy()
    flat = t.reshape(B, C, HW)
    flat[:, 0, cells[0]] = 3.0
    flat[:, 0, cells[1:4]] = (-0.0, 0.0, -0.0)
    tau, count, mask = _check_select(t, 2.5 / HW)
    assert count.tolist() == [4] * B and not np.signbit(tau).any() and (tau == 0).all()
    # +-inf logits
    t = base.copy()
    flat = t.reshape(B, C, HW)
    flat[:, 0, cells[0]], flat[:, :, cells[1]], flat[:, C - 1, cells[2]] = np.inf, -np.inf, np.inf
    tau, count, _ = _check_select(t, 1.5 / HW)
    assert np.isposinf(tau).all() and count.tolist() == [2] * B
    tau, count, _ = _check_select(t, 1.0)
    assert np.isneginf(tau).all() and count.tolist() == [HW] * B
    # one NaN pixel (in one channel): never selected, not even by ratio = 1, and not counted towards k
    t = _case(shape)['t_hm'].copy()
    t[0, C - 1, H // 2, W // 3] = np.nan
    for r in (1e-6, 0.05, 1.0):
        tau, count, mask = _check_select(t, r)
        assert not mask[0, H // 2, W // 3]
    assert count[0] == HW - 1 and np.isneginf(tau[0])
    # a whole image of NaN selects nothing
    t = _case(shape)['t_hm'].copy()
    t[0] = np.nan
    tau, count, mask = _check_select(t, 0.05)
    assert count[0] == 0 and not mask[0].any() and (B == 1 or count[1] >= dto.k_of(0.05, HW))
    # an all-equal image: every position, whatever k
    t = _case(shape)['t_hm'].copy()
    t[0] = -2.5
    for r in (1e-6, 0.05):
        tau, count, _ = _check_select(t, r)
        assert count[0] == HW and tau[0] == F(-2.5)


def test_a_second_dense_select_starts_clean_and_a_side_stream_needs_one_synchronise():
    from hip_runtime import ops
    a, b = _case((2, 3, 32, 48))['t_hm'], _case((2, 4, 6, 11))['t_hm']
    want = dto.select(a, 0.05)
    tau, count = ops.dense_select(G(a), 0.05)
    other = ops.dense_select(G(b), 1.0)                   # the same workspace, other sizes
    again = ops.dense_select(G(a), 0.05)
    torch.cuda.synchronize()
    for got in ((tau, count), again):
        assert same_bits(N(got[0]), want[0]) and N(got[1]).tolist() == want[1].tolist()
    assert N(other[1]).tolist() == [66, 66]
    # a non-default stream: the call enqueues on it and reads nothing back -- one synchronise of THAT stream is enough
    side = torch.cuda.Stream()
    x = G(a)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        tau, count = ops.dense_select(x, 0.05)
    side.synchronize()
    assert same_bits(N(tau), want[0]) and N(count).tolist() == want[1].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# cnuda_dense_teacher_forward / _backward
# ---------------------------------------------------------------------------------------------------------------------
def _run_loss(c, ratio, mirror, hm_weight=1.0, wh_weight=0.1, upstream=1.0, x_hm=None, x_wh=None):
    """-> (loss, stats [5], grad_hm, grad_wh) as numpy"""
    from hip_runtime import ops
    t_hm, t_wh = G(c['t_hm']), G(c['t_wh'])
    hm = G(c['x_hm'] if x_hm is None else x_hm).requires_grad_(True)
    wh = G(c['x_wh'] if x_wh is None else x_wh).requires_grad_(True)
    tau, count = ops.dense_select(t_hm, ratio)
    loss, stats = ops.dense_teacher_loss(hm, wh, t_hm, t_wh, tau, count, mirror=mirror, hm_weight=hm_weight,
                                         wh_weight=wh_weight)
    assert loss.dim() == 0 and stats.shape == (5,) and not stats.requires_grad
    (loss * upstream).backward()
    torch.cuda.synchronize()
    return N(loss), N(stats), N(hm.grad), N(wh.grad)


@pytest.mark.parametrize('mirror', [False, True], ids=['plain', 'mirror'])
@pytest.mark.parametrize('shape, ratio', list(zip(SHAPES, [0.05, 0.05, 0.01, 0.01, 0.01])) + [((2, 4, 6, 11), 1.0)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_loss_stats_and_gradients_against_the_oracle(shape, ratio, mirror):
    c = _case(shape)
    weights = dict(hm_weight=1.5, wh_weight=0.3)
    want = dto.loss(c['x_hm'], c['x_wh'], c['t_hm'], c['t_wh'], ratio, mirror, **weights)
    want_hm, want_wh = dto.grad(c['x_hm'], c['x_wh'], c['t_hm'], c['t_wh'], ratio, mirror, upstream=0.7, **weights)
    loss, stats, g_hm, g_wh = _run_loss(c, ratio, mirror, upstream=0.7, **weights)
    print('\nloss %.9g oracle %.9g; stats %s oracle %s' % (loss, want[0], stats.tolist(), want))
    print('grad_hm err %.3g of %.3g; grad_wh err %.3g of %.3g' % (
        np.abs(g_hm - want_hm).max(), np.abs(want_hm).max(), np.abs(g_wh - want_wh).max(), np.abs(want_wh).max()))
    assert abs(float(loss) - want[0]) <= LOSS_RTOL * abs(want[0])
    assert same_bits(stats[0], loss)
    for i in (1, 2, 4):
        assert abs(float(stats[i]) - want[i]) <= LOSS_RTOL * abs(want[i]), i
    assert float(stats[3]) == want[3]                                    # N, exactly
    assert np.abs(g_hm - want_hm).max() <= GRAD_TOL * np.abs(want_hm).max()
    assert np.abs(g_wh - want_wh).max() <= GRAD_TOL * np.abs(want_wh).max()
    # grad_wh is exactly zero off the (mirrored) selection, and nowhere else for these sizes
    mask = dto.select(c['t_hm'], ratio)[2]
    seen = mask[..., ::-1] if mirror else mask
    assert not g_wh[~np.broadcast_to(seen[:, None], g_wh.shape)].any()
    assert (g_wh[np.broadcast_to(seen[:, None], g_wh.shape)] != 0).all()


@pytest.mark.parametrize('mirror', [False, True], ids=['plain', 'mirror'])
def test_the_sign_of_zero_is_zero(mirror):
    """Where the student's size IS the teacher's (as the student sees it), its gradient is 0, not +-k."""
    shape = (2, 3, 32, 48)
    c = _case(shape)
    mask = dto.select(c['t_hm'], 0.05)[2]
    seen_t = c['t_wh'][..., ::-1] if mirror else c['t_wh']
    seen = mask[..., ::-1] if mirror else mask
    x_wh = c['x_wh'].copy()
    x_wh[:, 0] = np.where(seen, seen_t[:, 0], x_wh[:, 0])               # channel 0 coincides on the whole selection
    _, _, _, g_wh = _run_loss(c, 0.05, mirror, x_wh=x_wh)
    assert seen.sum() >= 2 * 76 and not g_wh[:, 0].any() and (g_wh[:, 1][seen] != 0).all()


@pytest.mark.parametrize('shape', [(2, 4, 6, 11), (2, 3, 32, 48)], ids=['scalar', 'vector'])
def test_the_mirror_is_the_plain_loss_of_mirrored_student_maps(shape):
    from predict import mirror_input
    c = _case(shape)
    loss_m, stats_m, ghm_m, gwh_m = _run_loss(c, 0.05, True, upstream=2.0)
    x_hm, x_wh = N(mirror_input(G(c['x_hm']))), N(mirror_input(G(c['x_wh'])))
    assert same_bits(x_hm, c['x_hm'][..., ::-1])
    loss_p, stats_p, ghm_p, gwh_p = _run_loss(c, 0.05, False, upstream=2.0, x_hm=x_hm, x_wh=x_wh)
    assert abs(float(loss_m) - float(loss_p)) <= LOSS_RTOL * abs(float(loss_p)) and stats_m[3] == stats_p[3]
    assert np.abs(ghm_m - ghm_p[..., ::-1]).max() <= GRAD_TOL * np.abs(ghm_p).max()
    assert np.abs(gwh_m - gwh_p[..., ::-1]).max() <= GRAD_TOL * np.abs(gwh_p).max()


def test_two_runs_give_the_same_bits():
    c = _case((2, 3, 32, 48))
    a, b = _run_loss(c, 0.05, True, upstream=0.7), _run_loss(c, 0.05, True, upstream=0.7)
    for x, y in zip(a, b):
        assert same_bits(x, y)


def _launched(log):
    """{bare kernel name: launches}, and the template arguments seen (a demangler may spell `<4>` as `<(int)4>`)"""
    names = {sh.short(k): v for k, v in log.counts.items()}
    return {k.split('<')[0]: v for k, v in names.items()}, ' '.join(names)


def test_launch_counts_are_the_documented_ones():
    """DESIGN.md, "Dense teacher": select 2 (scores, select), forward 2 (reduction, its tail), backward 1."""
    import hip_runtime as hr
    from hip_runtime import ops
    c = _case((2, 3, 32, 48))
    t_hm, t_wh = G(c['t_hm']), G(c['t_wh'])
    hm, wh = G(c['x_hm']).requires_grad_(True), G(c['x_wh']).requires_grad_(True)
    with hr.launch_log() as log:
        tau, count = ops.dense_select(t_hm, 0.01)
    counts, spelled = _launched(log)
    assert counts == {'dense_score_kernel': 1, 'dense_select_kernel': 1} and 'true' in spelled       # on chip
    with hr.launch_log() as log:
        loss, _ = ops.dense_teacher_loss(hm, wh, t_hm, t_wh, tau, count, mirror=True)
    counts, spelled = _launched(log)
    assert counts == {'dense_loss_kernel': 1, 'dense_finalize_kernel': 1} and '4>' in spelled         # 16-byte items
    with hr.launch_log() as log:
        loss.backward()
    counts, spelled = _launched(log)
    assert counts == {'dense_grad_kernel': 1} and '4>' in spelled
    torch.cuda.synchronize()
    big = G(_case((1, 2, 208, 208))['t_hm'])
    with hr.launch_log() as log:
        ops.dense_select(big, 0.01)
    counts, spelled = _launched(log)
    assert counts == {'dense_score_kernel': 1, 'dense_select_kernel': 1} and 'false' in spelled      # re-reads the scores
    torch.cuda.synchronize()


def test_refusals():
    import uda
    from hip_runtime import ops
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    tau, count = z(1), z(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='teacher_hm requires grad'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4, requires_grad=True), z(1, 2, 4, 4), tau, count,
                               mirror=True)
    with pytest.raises(RuntimeError, match='teacher_wh requires grad'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 4, requires_grad=True), tau, count,
                               mirror=True)
    with pytest.raises(RuntimeError, match='teacher_hm is'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 2, 4, 4), tau, count, mirror=True)
    with pytest.raises(RuntimeError, match='wh is'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 3, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 4), tau, count, mirror=True)
    with pytest.raises(RuntimeError, match='tau is'):
        ops.dense_teacher_loss(z(1, 3, 4, 4), z(1, 2, 4, 4), z(1, 3, 4, 4), z(1, 2, 4, 4), z(2), count, mirror=True)
    with pytest.raises(RuntimeError, match='1025 classes'):
        ops.dense_select(z(1, 1025, 2, 2), 0.5)
    with pytest.raises(RuntimeError, match='1025 classes'):
        ops.dense_teacher_loss(z(1, 1025, 2, 2), z(1, 2, 2, 2), z(1, 1025, 2, 2), z(1, 2, 2, 2), tau, count, mirror=False)
    with pytest.raises(RuntimeError, match='B, C, H, W'):
        ops.dense_select(z(3, 4, 4), 0.5)
    for key, params in (('rotated_boxes', dict(rotated_boxes=True, num_keypoints=0)),
                        ('num_keypoints', dict(rotated_boxes=False, num_keypoints=17))):
        plugin = uda.DenseTeacher(1.0)
        plugin.cfg = sh.cfg(3)
        plugin.cfg.model.backend.params.update(params)
        with pytest.raises(ValueError, match='model.backend.params.' + key):
            plugin.init_done()


# ---------------------------------------------------------------------------------------------------------------------
# the plugin on ResNet-18: 64 x 64, 2 + 2 images, 3 classes (the set-up of tests/test_gpu_teacher.py)
# ---------------------------------------------------------------------------------------------------------------------
SOURCE_STATS = ['centernet_loss', 'hm_loss', 'wh_loss', 'off_loss']
DENSE_STATS = ['dense_loss', 'dense_hm_loss', 'dense_wh_loss', 'dense_positions', 'dense_score']


def _resnet_plugin(target, seed=3, **kwargs):
    import uda
    from backends import resnet
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    torch.manual_seed(seed)
    model = resnet.build(18, num_classes=3, pretrained=False)
    sh.condition(model, target)
    plugin = uda.DenseTeacher(kwargs.pop('pseudo_weight', 0.5), **kwargs)
    plugin.cfg, plugin.device, plugin.backend = sh.cfg(3), torch.device(DEV), model
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    plugin.host_stats = False
    return plugin


def test_one_training_step_by_hand_and_the_ema_behind_it():
    import teacher_oracle as to
    from hip_runtime import ops
    data = sh.data()
    plugin = _resnet_plugin(data['target_domain_input'], pseudo_weight=0.5, ratio=0.05, hm_weight=1.0, wh_weight=0.2)
    teacher, student = plugin.teacher, plugin.backend
    target = data['target_domain_input']
    target_before = N(target).copy()
    with torch.no_grad():
        heads = teacher(target)                       # the UNmirrored batch, before the step moves the teacher
    t_hm, t_wh = heads['hm'].clone(), heads['wh'].clone()
    want_view = N(plugin.student_view(target))        # step 0's strong view of the mirror (the parent's, by the step number)
    old = sh.snapshot(teacher)
    cap = sh.Capture(plugin)
    out = plugin.step(data)
    torch.cuda.synchronize()
    stats = out['stats']
    assert list(stats) == SOURCE_STATS + DENSE_STATS + ['total_loss']
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 and math.isfinite(float(v)) for v in stats.values())
    assert data['target_domain_input'] is target and same_bits(N(target), target_before)
    assert same_bits(cap.teacher[0], target_before) and len(cap.student) == 2 and len(cap.teacher) == 1
    assert same_bits(cap.student[1], want_view)
    cap.remove()
    # by hand: the dense loss of the returned target outputs against the teacher's heads
    tau, count = ops.dense_select(t_hm, 0.05)
    loss, stats5 = ops.dense_teacher_loss(out['target_domain']['hm'].detach(), out['target_domain']['wh'].detach(), t_hm,
                                          t_wh, tau, count, mirror=True, hm_weight=1.0, wh_weight=0.2)
    by_hand = plugin.dense_stats(stats5, 2)
    assert list(by_hand) == DENSE_STATS
    for k, v in by_hand.items():
        assert same_bits(N(stats[k]), N(v)), k
    assert same_bits(N(by_hand['dense_positions']), N(stats5[3]) / F(2))
    assert same_bits(N(by_hand['dense_score']), N(stats5[4]) / N(stats5[3]))
    assert float(stats['dense_hm_loss']) > 0 and float(stats['dense_wh_loss']) > 0
    assert float(stats['dense_positions']) >= dto.k_of(0.05, 16 * 16) == 12 and 0 < float(stats['dense_score']) < 1
    assert same_bits(N(stats['total_loss']), N(stats['centernet_loss']) + N(loss) * F(0.5))
    # the EMA: decay_t(0) = 0.1 against the student's NEW values
    assert plugin.teacher_updates == 1
    new, now = sh.snapshot(student), sh.snapshot(teacher)
    moved = 0
    for k in old:
        if old[k].dtype == np.float32:
            assert same_bits(now[k], to.ema(old[k], new[k], 0.1)), k
            moved += int(not same_bits(now[k], old[k]))
        else:
            assert k.endswith('num_batches_tracked') and same_bits(now[k], new[k]) and int(now[k]) == 2, k
    assert moved > 50 and not teacher.training and all(not p.requires_grad for p in teacher.parameters())
    assert plugin.target_grad_heads == ('hm', 'wh')


def test_burn_in_trains_the_source_loss_only():
    data = sh.data()
    plugin = _resnet_plugin(data['target_domain_input'], burn_in_steps=1)
    names = [list(plugin.step(data)['stats']) for _ in range(2)]
    torch.cuda.synchronize()
    assert names[0] == SOURCE_STATS + ['total_loss'] and not any(k.startswith('dense_') for k in names[0])
    assert names[1] == SOURCE_STATS + DENSE_STATS + ['total_loss'] and plugin.teacher_updates == 2
    plugin.set_phase(False)
    with torch.no_grad():
        assert list(plugin.step(sh.data(), is_training=False)['stats']) == SOURCE_STATS + ['total_loss']
    assert plugin.teacher_updates == 2


def test_without_strong_view_and_mirror_the_student_sees_the_target_batch_itself():
    data = sh.data()
    target = data['target_domain_input']
    plugin = _resnet_plugin(target, strong_view=False, mirror_student=False)
    cap = sh.Capture(plugin)
    plugin.step(data)
    torch.cuda.synchronize()
    assert len(cap.student) == 2 and same_bits(cap.student[1], N(target)) and same_bits(cap.teacher[0], N(target))
    cap.remove()
    mirrored = _resnet_plugin(target, strong_view=False)
    cap = sh.Capture(mirrored)
    mirrored.step(data)
    torch.cuda.synchronize()
    assert same_bits(cap.student[1], N(target)[..., ::-1])
    cap.remove()


def test_checkpoints_carry_the_teacher(tmp_path):
    data = sh.data()
    plugin = _resnet_plugin(data['target_domain_input'])
    plugin.step(data)
    plugin.step(data)
    path = str(tmp_path / 'model_last.pth')
    plugin.save_model(path, 4, True)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['epoch', 'optimizer', 'state_dict', 'teacher_state_dict', 'teacher_updates']
    assert ckpt['teacher_updates'] == 2
    fresh = _resnet_plugin(data['target_domain_input'], seed=9)
    assert fresh.load_model(path, resume=True) == 5 and fresh.teacher_updates == 2
    want_t, got_t = sh.snapshot(plugin.teacher), sh.snapshot(fresh.teacher)
    want_s, got_s = sh.snapshot(plugin.backend), sh.snapshot(fresh.backend)
    assert all(same_bits(got_t[k], want_t[k]) for k in want_t) and all(same_bits(got_s[k], want_s[k]) for k in want_s)
    assert any(not same_bits(want_t[k], want_s[k]) for k in want_t)
    fresh.step(data)
    assert fresh.teacher_updates == 3


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def test_dla_batched_step_equals_the_sequential_step(golden):
    """tests/test_gpu_teacher.py::test_dla_batched_step_equals_the_sequential_step's comparison and tolerances (statistics
    and outputs 1e-5, gradients 2e-4, running statistics 1e-5, all relative) with the dense loss on hm and wh.  The plain
    mirror view: the comparison is of the two passes, not of the augmentation."""
    import uda
    from backends import dla
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    shapes = dict(ast.literal_eval(str(golden('dla_axis')['shapes_json'])))
    data0 = sh.data(B=2, S=128, C=6, seed=80)
    res = []
    for batched in (True, False):
        model = dla.build(num_classes=6)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in gin.fill_state(shapes, 0.1).items()})
        sh.condition(model, data0['target_domain_input'])
        plugin = uda.DenseTeacher(1.0, ratio=0.05, strong_view=False)
        plugin.batch_domains = batched
        plugin.cfg, plugin.device, plugin.backend = sh.cfg(6), torch.device(DEV), model
        plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
        plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
        plugin.init_done()
        plugin.to(DEV)
        plugin.set_phase(True)
        out = plugin.step(dict(data0))
        torch.cuda.synchronize()
        res.append((out, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                    {n: b.detach().clone() for n, b in model.named_buffers()}))
    (ob, gb, bb), (os_, gs, bs) = res
    assert list(ob['stats']) == list(os_['stats']) == SOURCE_STATS + DENSE_STATS + ['total_loss']
    assert float(ob['stats']['dense_positions']) >= dto.k_of(0.05, 32 * 32) and float(ob['stats']['dense_wh_loss']) > 0
    for k in ob['stats']:
        assert math.isfinite(float(ob['stats'][k]))
        assert abs(float(ob['stats'][k]) - float(os_['stats'][k])) <= 1e-5 * max(abs(float(os_['stats'][k])), 1e-9), k
    for dom in ('source_domain', 'target_domain'):
        assert list(ob[dom]) == list(os_[dom]) == ['hm', 'wh', 'reg']
        for k in ob[dom]:
            assert _rel(ob[dom][k].detach(), os_[dom][k].detach()) <= 1e-5, (dom, k)
    assert sorted(gb) == sorted(gs)
    for n in gs:
        if n.endswith('.conv.bias') and 'ida' in n:
            continue                                      # analytically zero (bias in front of a BatchNorm): noise
        assert _rel(gb[n], gs[n]) <= 2e-4, (n, _rel(gb[n], gs[n]))
    for n in bs:
        if bs[n].is_floating_point():
            assert _rel(bb[n], bs[n]) <= 1e-5, n
        else:
            assert int(bb[n]) == int(bs[n]) == 2, n


def test_the_driver_trains_logs_saves_and_predicts_with_the_dense_teacher(tmp_path, monkeypatch):
    """train.py for one epoch of two steps on the fixture dataset with the README's override -- its burn-in cut to one
    step --, then predict.py --teacher on its checkpoint."""
    import predict
    import train
    from utils import tensorboard
    monkeypatch.setattr(tensorboard, 'default_writer', lambda log_dir='logs': tensorboard.FileWriter(log_dir))
    root = tmp_path
    tr = fx.write_dataset(root, 8, name='train')
    val = fx.write_dataset(root, 4, name='val', first_seed=30)
    glob = fx.write_target_images(root, 3)
    cfg = root / 'configs'
    (cfg / 'experiment').mkdir(parents=True)
    with open(os.path.join(ROOT, 'centernet-uda_amd', 'configs', 'defaults.yaml')) as f:
        (cfg / 'defaults.yaml').write_text(f.read())

    def split(files, **extra):
        return {'name': 'coco', 'params': dict(image_folder=files[0], annotation_file=files[1], input_size=[128, 128],
                                               target_domain_glob=[glob], **extra)}
    experiment = {
        'experiment': 'tiny',
        'model': {'backend': {'name': 'resnet', 'params': {'num_layers': 18, 'pretrained': False, 'num_classes': 3,
                                                           'num_keypoints': 0, 'rotated_boxes': False}}, 'uda': None},
        'datasets': {'training': split(tr, augment_target_domain=True), 'validation': split(val)},
        'optimizer': {'name': 'Adam', 'params': {'lr': 0.00005}, 'scheduler': None},
        'tensorboard': {'num_visualizations': 0},
        'max_detections': 20, 'epochs': 1, 'batch_size': 4, 'num_workers': 0,
        'hydra': {'run': {'dir': str(root / 'runs') + '/${experiment}/'}},
    }
    (cfg / 'experiment' / 'tiny.yaml').write_text(yaml.safe_dump(experiment))
    summary = train.main(['--config-dir', str(cfg), 'experiment=tiny',
                          'model.uda={DenseTeacher: {pseudo_weight: 1.0, ratio: 0.01, burn_in_steps: 1}}'])
    assert summary['error'] is None and summary['epochs'] == [1]
    run = summary['run_dir']
    with open(os.path.join(run, 'logs', 'scalars.jsonl')) as f:
        logged = {r['name']: r['value'] for r in map(json.loads, f)}
    for name in ['training/total_loss', 'validation/total_loss'] + ['training/' + k for k in DENSE_STATS]:
        assert name in logged and math.isfinite(logged[name]), (name, sorted(logged))
    last = torch.load(os.path.join(run, 'model_last.pth'), map_location='cpu', weights_only=False)
    assert last['teacher_updates'] >= 1 and list(last['teacher_state_dict']) == list(last['state_dict'])
    assert any(not torch.equal(last['teacher_state_dict'][k], v) for k, v in last['state_dict'].items())
    out = root / 'teacher.json'
    got = predict.main([run, tr[0], '--teacher', '--out', str(out), '--score-threshold', '0.0', '--num-workers', '0'])
    assert got['images'] == 8 and isinstance(json.loads(out.read_text()), list) and got['detections'] > 0
