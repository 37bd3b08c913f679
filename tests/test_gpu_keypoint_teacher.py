"""The keypoint teacher on the GPU: cnuda_pseudo_labels_kps (csrc/teacher.hip) and cnuda_labels_transform_kps
(csrc/geomview.hip) against the numpy oracle (tests/keypoint_teacher_oracle.py) bit for bit -- the joints' arithmetic is
float64 in a written order under -ffp-contract=off, integers otherwise, so equality is the derived tolerance --, against
the two entry points they extend on the same inputs, from run to run, and `uda.KeypointTeacher` through its pseudo batch,
a training step and a checkpoint.

The one exception to "bit for bit": a rotated model's corners out of the score filter pass through cos and sin, where
the device's and numpy's libraries may differ in the last place; they are compared with the box-only entry bit for bit
and with the oracle to 1e-9 cells, the bound of tests/test_gpu_teacher.py.  Inputs: tests/keypoint_teacher_cases.py; what
they cover is asserted on the CPU in tests/test_host_keypoint_teacher.py."""
import math

import numpy as np
import pytest
import torch

import keypoint_teacher_cases as kc
import keypoint_teacher_oracle as ko
import strong_view_helpers as sh
from strong_view_helpers import DEV, F, G, N, same_bits

pytestmark = pytest.mark.gpu
_WANT = {}


def _once(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def _sync_numpy(d):
    torch.cuda.synchronize()
    return {k: N(v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the score filter with joints
# ---------------------------------------------------------------------------------------------------------------------
def _check_filter(rotated, mirror, perm, J, full=False):
    from hip_runtime import ops
    key = 'corners' if rotated else 'boxes'
    dets, kps = kc.dets(rotated, full), kc.kps(J)
    want = _once(('filter', rotated, mirror, perm is not None, J, full),
                 lambda: ko.pseudo_labels_kps(dets, kps, kc.THRESHOLDS, kc.MAP_W, kc.MAP_H, rotated=rotated, mirror=mirror,
                                              min_size=kc.MIN_SIZE, perm=perm))
    d, k, t = G(dets), G(kps), G(kc.THRESHOLDS)
    args = dict(rotated=rotated, mirror=mirror, min_size=kc.MIN_SIZE)
    got = ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H, flip_perm=None if perm is None else G(perm), **args)
    again = ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H,
                              flip_perm=None if perm is None else perm.tolist(), **args)
    old = ops.pseudo_labels(d, t, kc.MAP_W, **args)
    assert list(got) == ['classes', 'counts', 'kept', key, 'keypoints', 'visibility', 'joints']
    assert list(old) == ['classes', 'counts', 'kept', key]                     # without kps: exactly today's keys
    got, again, old = _sync_numpy(got), _sync_numpy(again), _sync_numpy(old)
    for name in old:                                                           # the box-only entry's bits
        assert same_bits(got[name], old[name]), name
    for name in got:                                                           # two calls, identical bytes
        assert same_bits(got[name], again[name]), name
    for name in ('classes', 'counts', 'kept', 'keypoints', 'visibility', 'joints'):
        assert same_bits(got[name], np.asarray(want[name])), name
    if rotated:
        assert got[key].dtype == np.float64 and np.abs(got[key] - want[key]).max() <= 1e-9
    else:
        assert same_bits(got[key], want[key])
    for b in range(kc.B):                                                      # zeros behind the survivors
        n = want['counts'][b]
        assert not got['keypoints'][b, n:].any() and not got['visibility'][b, n:].any() and not got[key][b, n:].any()
    assert same_bits(N(d), dets) and same_bits(N(k), kps)                      # the inputs are not written
    return want


@pytest.mark.parametrize('J', kc.JOINTS)
@pytest.mark.parametrize('perm', ['null', 'pairs'])
@pytest.mark.parametrize('mirror', [False, True], ids=['plain', 'mirror'])
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_pseudo_labels_with_joints_is_the_oracle_bit_for_bit(rotated, mirror, perm, J):
    want = _check_filter(rotated, mirror, kc.flip_perm(J) if perm == 'pairs' else None, J)
    assert want['counts'].tolist()[:2] == [0, 1] and 1 < want['counts'][2] < kc.K


@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_pseudo_labels_with_joints_when_every_row_of_an_image_survives(rotated):
    want = _check_filter(rotated, True, kc.flip_perm(4), 4, full=True)
    assert want['counts'].tolist() == [0, 1, kc.K]


def test_a_device_permutation_is_validated_once_and_a_bad_one_refused():
    from hip_runtime import ops
    d, k, t = G(kc.dets(False)), G(kc.kps(4)), G(kc.THRESHOLDS)
    bad = G(np.int32([0, 1, 1, 3]))
    with pytest.raises(RuntimeError, match='flip_perm'):
        ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H, flip_perm=bad)
    with pytest.raises(RuntimeError, match='flip_perm'):
        ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H, flip_perm=G(np.int64([0, 1, 2, 3])))
    perm = G(kc.flip_perm(4))
    ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H, flip_perm=perm)
    assert ops._CHECKED_PERMS[id(perm)][1] == perm._version
    perm[1] = 3                                             # written since: looked at again
    with pytest.raises(RuntimeError, match='flip_perm'):
        ops.pseudo_labels(d, t, kc.MAP_W, kps=k, map_height=kc.MAP_H, flip_perm=perm)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the view with joints
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('J', kc.JOINTS)
@pytest.mark.parametrize('view', kc.VIEWS)
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_transform_labels_with_joints_is_the_oracle_bit_for_bit(rotated, view, J):
    from hip_runtime import ops
    key = 'corners' if rotated else 'boxes'
    labels, fmap = kc.labels(rotated, J), np.array(kc.forward_maps(view))       # (a writable copy for the upload)
    args = dict(rotated=rotated, min_size=kc.MIN_SIZE, min_visible=0.5)
    want = _once(('view', rotated, view, J), lambda: ko.transform_labels_kps(labels, fmap, kc.MAP_H, kc.MAP_W, **args)[0])
    dl = {k: G(v) for k, v in labels.items()}
    got = ops.transform_labels(dl, fmap, kc.MAP_H, kc.MAP_W, **args)
    again = ops.transform_labels(dl, G(fmap), kc.MAP_H, kc.MAP_W, **args)
    old = ops.transform_labels({k: v for k, v in dl.items() if k not in ('keypoints', 'visibility', 'joints')}, fmap,
                               kc.MAP_H, kc.MAP_W, **args)
    assert list(got) == ['classes', 'counts', 'kept', key, 'dropped', 'keypoints', 'visibility', 'joints']
    assert list(old) == ['classes', 'counts', 'kept', key, 'dropped']          # without joints: exactly today's keys
    for name in got:                                                           # new tensors, never the inputs
        assert name not in dl or got[name].data_ptr() != dl[name].data_ptr()
    got, again, old = _sync_numpy(got), _sync_numpy(again), _sync_numpy(old)
    for name in old:                                                           # the box-only entry's bits
        assert same_bits(got[name], old[name]), name
    for name in got:
        assert same_bits(got[name], again[name]), name                         # two calls, identical bytes
        assert same_bits(got[name], np.asarray(want[name])), name              # the oracle, bit for bit
    for b in range(kc.B):                                                      # zeros behind the survivors
        n = want['counts'][b]
        assert not got['keypoints'][b, n:].any() and not got['visibility'][b, n:].any() and not got[key][b, n:].any()
    for name, v in labels.items():
        assert same_bits(N(dl[name]), np.asarray(v)), name                     # the inputs are not written
    if view == 'ident':                                                        # image 2 came through as it went in
        for name in (key, 'classes', 'keypoints', 'visibility'):
            assert same_bits(got[name][2], labels[name][2]), name


def test_transform_labels_refuses_a_table_with_half_the_joints():
    from hip_runtime import ops
    dl = {k: G(v) for k, v in kc.labels(False, 4).items()}
    shift = np.array(kc.forward_maps('shift'))                                # (a writable copy for the upload)
    for drop in ('keypoints', 'visibility'):
        with pytest.raises(RuntimeError, match='only one'):
            ops.transform_labels({k: v for k, v in dl.items() if k != drop}, shift, kc.MAP_H, kc.MAP_W)
    with pytest.raises(RuntimeError, match='visibility'):
        ops.transform_labels(dict(dl, visibility=dl['visibility'].long()), shift, kc.MAP_H, kc.MAP_W)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the plugin: ResNet-18 with J = 4, 64 x 64, B = 2, every score passes (thresholds 0)
# ---------------------------------------------------------------------------------------------------------------------
J4 = 4
PAIRS = [[0, 1], [2, 3]]
VIEW = {'rotate': [-20, 20], 'scale': None, 'translate_percent': [0.2, 0.3]}       # rows leave on two edges
OFF = {'rotate': None, 'scale': None, 'translate_percent': None}


def _data(rotated=False):
    rs = np.random.RandomState(5)
    data = {k: G(v) for k, v in sh.gin.detection_batch(2, 3, 16, 16, 8, (3, 2), 3 if rotated else 2, 61).items()}
    data['input'] = G(sh.gin.image_batch(2, 64, 64, 60))
    data['target_domain_input'] = G(sh.gin.image_batch(2, 64, 64, 70))
    data['kps'] = G(rs.uniform(-4, 4, (2, 8, 2 * J4)).astype(F))
    data['kp_reg_mask'] = G(np.repeat(N(data['reg_mask'])[..., None], 2 * J4, -1).astype(np.uint8))
    return data


def _plugin(target, seed=3, pseudo_weight=0.5, rotated=False, **kwargs):
    """uda.KeypointTeacher around a ResNet-18 with three classes and four joints, conditioned as
    strong_view_helpers.condition does (sizes around 5 cells, heat-map logits spread around -2.19), moved and in
    training phase."""
    import uda
    from backends import resnet
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    torch.manual_seed(seed)
    model = resnet.build(18, num_classes=3, num_keypoints=J4, pretrained=False, rotated_boxes=rotated).to(DEV)
    with torch.no_grad():
        sh._last_conv(model.wh).bias.fill_(5.0)
        sh._last_conv(model.hm).bias.fill_(-2.19)
        model.eval()
        sh._last_conv(model.hm).weight.mul_(1.5 / float(model(target)['hm'].std()))
    model.train()
    kwargs.setdefault('score_threshold', 0.0)
    kwargs.setdefault('flip_pairs', PAIRS)
    plugin = uda.KeypointTeacher(pseudo_weight, **kwargs)
    plugin.cfg = sh.cfg(3)
    plugin.cfg['model']['backend']['params'].update(num_keypoints=J4, rotated_boxes=rotated)
    plugin.device, plugin.backend = torch.device(DEV), model
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, kp_weight=1.0,
                                          **({'angle_weight': 1.0, 'periodic': True} if rotated else {}))
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    plugin.host_stats = False
    return plugin


def _finite(stats):
    return all(math.isfinite(float(v)) for v in stats.values())


def test_the_pseudo_batch_is_encode_targets_of_the_oracles_labels():
    from backends.decode import decode_detection
    from datasets.geometric_view import GeometricView
    from datasets.targets import encode_targets
    from hip_runtime import ops
    data = _data()
    target = data['target_domain_input']
    plugin = _plugin(target, geometric_view=VIEW)
    got = plugin.pseudo_batch(target)
    with torch.no_grad():
        heads = plugin.teacher(target)
        hm = ops.sigmoid_clamp_(heads['hm'])
        dets, kps = decode_detection(hm, heads['wh'], heads['reg'], kps=heads['kps'], K=sh.KDET)
    assert kps.shape == (2, sh.KDET, J4, 2)
    first = ko.pseudo_labels_kps(N(dets), N(kps), F([0, 0, 0]), 16, 16, mirror=True, min_size=plugin.min_size,
                                 perm=[1, 0, 3, 2])
    p = GeometricView(VIEW).sample(2, 64, 64, np.random.default_rng([42, 0x47454F, 0]))
    want, judged = ko.transform_labels_kps(first, p.forward_map(4), 16, 16, min_size=plugin.min_size, min_visible=0.5)
    assert all(abs(v[0] - 0.5) > 1e-6 and abs(v[1] - plugin.min_size) > 1e-6 and abs(v[2] - plugin.min_size) > 1e-6
               for v in judged)
    ref = encode_targets(G(want['boxes']), G(want['classes']), G(want['counts']), 3, 16, 16,
                         keypoints=G(want['keypoints']), visibility=G(want['visibility']))
    assert {'kps', 'gt_kps', 'kp_reg_mask'} <= set(ref)
    assert sorted(got) == sorted(list(ref) + ['kept', 'dropped', 'joints'])
    for k in ref:
        assert same_bits(N(got[k]), N(ref[k])), k
    for k in ('kept', 'dropped', 'joints'):
        assert same_bits(N(got[k]), np.asarray(want[k])), k
    # the tables are not empty: labels survive and labels leave, joints are taught and joints are masked
    assert float(got['kept']) > 0 and float(got['dropped']) > 0 and float(got['joints']) > 0
    mask = N(got['kp_reg_mask'])
    assert mask.any() and not mask.all() and (want['visibility'] == 2).any()
    # the permutation matters on this batch: without the pairs the joints land elsewhere
    other = _plugin(target, geometric_view=VIEW, flip_pairs=None).pseudo_batch(target)
    assert same_bits(N(other['hm']), N(got['hm'])) and not same_bits(N(other['kps']), N(got['kps']))


def test_one_training_step_logs_the_keypoint_statistics_and_launches_the_keypoint_kernels():
    import hip_runtime as hr
    data = _data()
    plugin = _plugin(data['target_domain_input'], geometric_view=VIEW)
    batch = plugin.pseudo_batch(data['target_domain_input'])
    with hr.launch_log() as log:
        out = plugin.step(data)
        torch.cuda.synchronize()
    stats = out['stats']
    assert {'kp_loss', 'pseudo_kp_loss', 'pseudo_joints', 'pseudo_boxes', 'pseudo_dropped', 'pseudo_hm_loss',
            'total_loss'} <= set(stats) and _finite(stats)
    assert list(stats)[-2:] == ['pseudo_joints', 'total_loss']
    assert float(stats['pseudo_joints']) == float(batch['joints']) > 0 and float(stats['pseudo_kp_loss']) > 0
    assert float(stats['pseudo_boxes']) == float(batch['kept']) and plugin.teacher_updates == 1
    counts = {sh.short(k): v for k, v in log.counts.items()}
    for name in ('pseudo_labels_kps_kernel', 'labels_transform_kps_kernel', 'labels_totals_kps_kernel'):
        assert counts.get(name) == 1, (name, counts.get(name))
    for name in ('pseudo_labels_kernel', 'labels_transform_kernel', 'labels_totals_kernel'):
        assert name not in counts, name


def test_the_target_halfs_keypoint_gradient_reaches_the_students_kps_head():
    """The same initial weights and the same draws, one step each: with pseudo_weight = 0 the target term is multiplied
    away, with 1 it is not; the source half is the same in both."""
    last = []
    for weight in (1.0, 0.0):
        data = _data()
        plugin = _plugin(data['target_domain_input'], pseudo_weight=weight, geometric_view=VIEW)
        conv = sh._last_conv(plugin.backend.kps)
        before = N(conv.weight).copy()
        out = plugin.step(data)
        torch.cuda.synchronize()
        assert float(out['stats']['pseudo_joints']) > 0 and float(out['stats']['pseudo_kp_loss']) > 0
        last.append((before, N(conv.weight).copy()))
    assert same_bits(last[0][0], last[1][0])                                   # the same start
    assert not same_bits(last[1][0], last[1][1])                               # the source half alone moves the head
    assert not same_bits(last[0][1], last[1][1])                               # and the target half moves it further


def test_a_step_with_every_geometric_component_null_and_a_checkpoint_round_trip(tmp_path):
    data = _data()
    target = data['target_domain_input']
    plugin = _plugin(target, geometric_view=OFF)
    out = plugin.step(data)
    torch.cuda.synchronize()
    assert _finite(out['stats']) and float(out['stats']['pseudo_dropped']) == 0.0
    assert float(out['stats']['pseudo_boxes']) > 0 and float(out['stats']['pseudo_joints']) > 0
    path = str(tmp_path / 'model_last.pth')
    plugin.save_model(path, 1, True)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['epoch', 'optimizer', 'state_dict', 'teacher_state_dict', 'teacher_updates']
    assert ckpt['teacher_updates'] == 1 and any(k.startswith('kps') for k in ckpt['teacher_state_dict'])
    fresh = _plugin(target, seed=9, geometric_view=OFF)
    assert fresh.teacher_updates == 0
    fresh.load_model(path, resume=True)
    assert fresh.teacher_updates == 1
    want = sh.snapshot(plugin.teacher)
    for k, v in sh.snapshot(fresh.teacher).items():
        assert same_bits(v, want[k]), k
    out = fresh.step(data)
    torch.cuda.synchronize()
    assert _finite(out['stats']) and fresh.teacher_updates == 2


def test_one_step_with_a_rotated_box_model():
    data = _data(rotated=True)
    plugin = _plugin(data['target_domain_input'], rotated=True, geometric_view={'rotate': [-180, 180]})
    batch = plugin.pseudo_batch(data['target_domain_input'])
    assert batch['wh'].shape[-1] == 3 and batch['kps'].shape[-1] == 2 * J4 and float(batch['kept']) > 0
    out = plugin.step(data)
    torch.cuda.synchronize()
    assert {'pseudo_kp_loss', 'pseudo_joints', 'pseudo_dropped'} <= set(out['stats']) and _finite(out['stats'])
    assert float(out['stats']['pseudo_joints']) == float(batch['joints'])
