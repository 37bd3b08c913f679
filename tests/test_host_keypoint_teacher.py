"""The keypoint teacher without a GPU: how the driver resolves `uda.KeypointTeacher`, its signature and refusals, the numpy
oracle of tests/keypoint_teacher_oracle.py pinned by two hand-worked cases, the argument checks of the two C entry points
and of the operators, and what the inputs of tests/test_gpu_keypoint_teacher.py (tests/keypoint_teacher_cases.py) cover
when they run through the oracle alone."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import keypoint_teacher_cases as kc
import keypoint_teacher_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'centernet-uda_amd', 'configs')
PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
OVERRIDE = ('model.uda={KeypointTeacher: {pseudo_weight: 1.0, score_threshold: 0.4, burn_in_steps: 2000, '
            'flip_pairs: [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]}}')
F = np.float32
D = np.float64


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(num_keypoints=17, num_classes=3):
    return Cfg(max_detections=20, seed=42, model=Cfg(backend=Cfg(params=Cfg(
        rotated_boxes=False, num_classes=num_classes, num_keypoints=num_keypoints))))


def _loss(kp_weight=1.0):
    from losses.centernet import DetectionLoss
    return DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, kp_weight=kp_weight)


# -- the plugin's front door --------------------------------------------------------------------------------------------
def test_the_driver_resolves_keypoint_teacher_from_the_readme_override():
    import train
    import uda
    from uda.mean_teacher import GeometricTeacher, KeypointTeacher
    from utils.config import load_config
    cls = train.resolve_plugin('KeypointTeacher')
    assert cls is uda.KeypointTeacher is KeypointTeacher and issubclass(cls, GeometricTeacher)
    assert 'KeypointTeacher' in dir(uda) and 'KeypointTeacher' in uda.__all__
    assert "'" + OVERRIDE + "'" in open(os.path.join(ROOT, 'README.md')).read()
    cfg = load_config(CONFIGS, ['experiment=dla_baseline', 'model.backend.params.num_keypoints=17',
                                'model.backend.loss.params.kp_weight=1.0', OVERRIDE,
                                'datasets.training.params.target_domain_glob=[/data/target/images/*.jpg]'])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is cls and sorted(args) == ['burn_in_steps', 'flip_pairs', 'pseudo_weight', 'score_threshold']
    plugin = got(**args)
    assert (plugin.pseudo_weight, plugin.score_threshold, plugin.burn_in_steps) == (1.0, 0.4, 2000)
    assert plugin.flip_pairs == [tuple(p) for p in PAIRS] and plugin.mirror_student and plugin.min_visible == 0.5
    plugin.cfg, plugin.centernet_loss = cfg, _loss()
    plugin.init_done()                                        # 17 joints, the keypoint term, disjoint pairs below 17
    assert plugin._flip_perm[0].tolist() == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def test_signature_and_defaults():
    import uda
    params = inspect.signature(uda.KeypointTeacher.__init__).parameters
    assert list(params)[1:] == ['pseudo_weight', 'flip_pairs', 'geometric_view', 'min_visible', 'strong_view',
                                'mean_teacher_arguments']
    assert [params[k].default for k in list(params)[2:6]] == [None, None, 0.5, None]
    assert params['mean_teacher_arguments'].kind is inspect.Parameter.VAR_KEYWORD
    assert uda.KeypointTeacher.target_grad_heads == ('hm', 'wh', 'reg', 'kps')
    plugin = uda.KeypointTeacher(1.0, decay=0.99, min_size=3.0)
    assert plugin.flip_pairs is None and plugin.decay == 0.99 and plugin.min_size == 3.0
    assert plugin.geometric_view.rotate == (-15.0, 15.0) and plugin.strong_view.blur is not None
    # the parents' refusals are inherited
    with pytest.raises(ValueError, match='min_visible'):
        uda.KeypointTeacher(1.0, min_visible=0)
    with pytest.raises(ValueError, match='decay'):
        uda.KeypointTeacher(1.0, decay=1.0)


def test_the_three_refusals_name_their_argument():
    import uda
    plugin = uda.KeypointTeacher(1.0)
    plugin.cfg, plugin.centernet_loss = _cfg(num_keypoints=0), _loss()
    with pytest.raises(ValueError, match=r'num_keypoints.*GeometricTeacher'):
        plugin.init_done()
    for bad in ([[1, 2], [2, 3]], [[1, 17]], [[4, 4]], [[1, 2, 3]], [[1.5, 2]]):
        plugin = uda.KeypointTeacher(1.0, flip_pairs=bad)
        plugin.cfg, plugin.centernet_loss = _cfg(), _loss()
        with pytest.raises(ValueError, match='flip_pairs'):
            plugin.init_done()
    plugin = uda.KeypointTeacher(1.0, flip_pairs=PAIRS)
    plugin.cfg, plugin.centernet_loss = _cfg(), _loss(kp_weight=None)
    assert not plugin.centernet_loss.with_keypoints
    with pytest.raises(ValueError, match='kp_weight'):
        plugin.init_done()
    plugin.centernet_loss = _loss()
    plugin.init_done()
    plugin = uda.KeypointTeacher(1.0, score_threshold=[0.3, 0.4])
    plugin.cfg, plugin.centernet_loss = _cfg(), _loss()
    with pytest.raises(ValueError, match='score_threshold'):
        plugin.init_done()


def test_the_other_teachers_still_refuse_keypoints():
    import uda
    for cls in (uda.MeanTeacher, uda.WeakStrongTeacher, uda.GeometricTeacher, uda.DenseTeacher):
        plugin = cls(1.0)
        plugin.cfg = _cfg(num_keypoints=4)
        with pytest.raises(ValueError, match='num_keypoints'):
            plugin.init_done()
        assert 'kps' not in cls.target_grad_heads
    assert uda.MeanTeacher.target_grad_heads == ('hm', 'wh', 'reg')


# -- the oracle, pinned by hand -----------------------------------------------------------------------------------------
def test_the_oracle_on_a_mirrored_pair_swap_by_hand():
    """A 24 x 16 map, J = 3, perm (0, 2, 1).  Row 0 is below its threshold; row 1 survives and lands in slot 0.  Its joints
    are (5, 3), (24, 4), (2, 16).  Mirrored, output joint 0 is input joint 0: (24 - 5, 3) = (19, 3), inside.  Output joint
    1 is input joint 2: (24 - 2, 16) = (22, 16), y = H is outside.  Output joint 2 is input joint 1: (24 - 24, 4) = (0, 4),
    inside (x' = 0), although x = 24 = W itself is outside without the mirror.  The box follows teacher_oracle:
    (24 - 9, 2, 24 - 3, 8)."""
    dets = F([[[1, 1, 6, 6, 0.1, 0], [3, 2, 9, 8, 0.9, 0]]])
    kps = F([[[[1, 1], [2, 2], [3, 3]], [[5, 3], [24, 4], [2, 16]]]])
    out = ko.pseudo_labels_kps(dets, kps, F([0.5]), 24, 16, mirror=True, perm=[0, 2, 1])
    assert out['counts'].tolist() == [1] and out['boxes'][0].tolist() == [[15, 2, 21, 8], [0] * 4]
    assert out['keypoints'].dtype == D and out['keypoints'][0].tolist() == [[[19, 3], [22, 16], [0, 4]], [[0, 0]] * 3]
    assert out['visibility'].dtype == np.int32 and out['visibility'][0].tolist() == [[2, 0, 2], [0, 0, 0]]
    assert out['joints'] == F(2) and out['joints'].dtype == F
    # without the mirror and the permutation: the joints as they are, x = W outside
    out = ko.pseudo_labels_kps(dets, kps, F([0.5]), 24, 16)
    assert out['keypoints'][0, 0].tolist() == [[5, 3], [24, 4], [2, 16]] and out['visibility'][0, 0].tolist() == [2, 0, 0]
    # a joint that is not finite is (0, 0) and invisible; the row stays
    kps[0, 1, 0, 1] = np.inf
    out = ko.pseudo_labels_kps(dets, kps, F([0.5]), 24, 16)
    assert out['counts'].tolist() == [1] and out['keypoints'][0, 0, 0].tolist() == [0, 0]
    assert out['visibility'][0, 0].tolist() == [0, 0, 0] and out['joints'] == F(0)


def test_the_oracle_on_a_quarter_turn_of_a_non_square_map_by_hand():
    """The 24 x 16 map turned by 90 degrees (clockwise on the y-down image) about its centre (12, 8):
    (x, y) -> (12 - (y - 8), 8 + (x - 12)) = (20 - y, x - 4), the matrix (0, -1, 20, 1, 0, -4).  The box (10, 6, 14, 9)
    becomes (11, 6, 14, 10), wholly inside.  Its joints: (12, 8) -> (12, 8), visible; (4, 8) -> (12, 0), on the top edge,
    visible; (3, 8) -> (12, -1), outside; (12, 8) with v = 1 -> (12, 8) with v = 0: only v = 2 stays visible.  The box
    (1, 6, 5, 9) becomes (11, -3, 14, 1): a quarter of it is visible, the row and its joints go."""
    labels = {'boxes': D([[[1, 6, 5, 9], [10, 6, 14, 9], [0, 0, 0, 0]]]), 'classes': np.int32([[1, 2, 0]]),
              'counts': np.int32([2]),
              'keypoints': D([[[[3, 7]] * 4, [[12, 8], [4, 8], [3, 8], [12, 8]], [[0, 0]] * 4]]),
              'visibility': np.int32([[[2, 2, 2, 2], [2, 2, 2, 1], [0, 0, 0, 0]]])}
    quarter = D([[0, -1, 20, 1, 0, -4]])
    out, judged = ko.transform_labels_kps(labels, quarter, 16, 24, min_size=1.0, min_visible=0.5)
    assert [v[0] for v in judged] == [0.25, 1.0]
    assert out['counts'].tolist() == [1] and out['classes'].tolist() == [[2, 0, 0]]
    assert out['boxes'][0].tolist() == [[11, 6, 14, 10], [0] * 4, [0] * 4]
    assert out['keypoints'][0].tolist() == [[[12, 8], [12, 0], [12, -1], [12, 8]], [[0, 0]] * 4, [[0, 0]] * 4]
    assert out['visibility'][0].tolist() == [[2, 2, 0, 0], [0] * 4, [0] * 4]
    assert out['kept'] == F(1) and out['dropped'] == F(1) and out['joints'] == F(2)
    # the identity keeps every row, every joint and every v as it is
    same, judged = ko.transform_labels_kps(labels, D([[1, 0, 0, 0, 1, 0]]), 16, 24, min_size=100.0, min_visible=1.0)
    assert judged == [] and same['counts'].tolist() == [2]
    assert np.array_equal(same['keypoints'], labels['keypoints']) and np.array_equal(same['visibility'], labels['visibility'])
    assert same['joints'] == F(7)


# -- what the GPU test's inputs cover -----------------------------------------------------------------------------------
def _both(vis, rows):
    seen = vis[:rows]
    return (seen == 2).any() and (seen != 2).any()


@pytest.mark.parametrize('J', kc.JOINTS)
@pytest.mark.parametrize('mirror', [False, True], ids=['plain', 'mirror'])
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_the_score_filters_inputs_cover_the_cases(rotated, mirror, J):
    """Image 0 empty, image 1 one survivor out of K, image 2 survivors on both sides of the 64-row chunk boundary beside
    dropped rows.  Every image that keeps at least two rows shows visible and invisible joints (one row of one joint
    cannot show both; the one row of image 1 does from J = 4 on), and joints that are not finite, on x' = 0 and on
    x' = W occur among the survivors."""
    dets, kps = kc.dets(rotated), kc.kps(J)
    perm = kc.flip_perm(J)
    assert (J == 1) == (perm.tolist() == list(range(J))) and sorted(perm.tolist()) == list(range(J))
    out = ko.pseudo_labels_kps(dets, kps, kc.THRESHOLDS, kc.MAP_W, kc.MAP_H, rotated=rotated, mirror=mirror,
                               min_size=kc.MIN_SIZE, perm=perm)
    rows = ko.surviving_rows(dets, kc.THRESHOLDS, rotated, kc.MIN_SIZE)
    counts = out['counts'].tolist()
    assert counts[:2] == [0, 1] and rows[1] == [kc.LONE] and 10 < counts[2] < kc.K - 10
    assert min(rows[2]) < 64 <= max(rows[2]) and not {3, 5, 66} & set(rows[2])
    assert _both(out['visibility'][2], counts[2]) and (J == 1 or _both(out['visibility'][1], 1))
    got = out['keypoints'][2, :counts[2]]
    src = kps[2, rows[2]][:, perm]
    assert (~np.isfinite(src)).any() and (got[~np.isfinite(src).all(-1)] == 0).all()
    assert ((got[..., 0] == 0) & (out['visibility'][2, :counts[2]] == 2)).any()                # x' = 0: inside
    assert ((got[..., 0] == kc.MAP_W) & (out['visibility'][2, :counts[2]] == 0)).any()         # x' = W: outside
    assert ((got[..., 1] == kc.MAP_H) & (out['visibility'][2, :counts[2]] == 0)).any()
    assert not out['keypoints'][0].any() and not out['visibility'][0].any() and out['joints'] > 0
    if J > 1:                                                 # the permutation and the mirror each change the result
        plain = ko.pseudo_labels_kps(dets, kps, kc.THRESHOLDS, kc.MAP_W, kc.MAP_H, rotated=rotated, mirror=mirror,
                                     min_size=kc.MIN_SIZE)
        assert not np.array_equal(plain['keypoints'], out['keypoints'])
    # the `full` table: every row of image 2 survives
    full = ko.surviving_rows(kc.dets(rotated, full=True), kc.THRESHOLDS, rotated, kc.MIN_SIZE)
    assert [len(r) for r in full] == [0, 1, kc.K]


@pytest.mark.parametrize('J', kc.JOINTS)
@pytest.mark.parametrize('view', kc.VIEWS)
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_the_views_inputs_cover_the_cases(rotated, view, J):
    """Counts (0, 1, K) going in.  Image 2 -- the one image that can show both -- keeps rows and drops rows, past the
    64-row chunk, and shows visible and invisible joints among its survivors (under 'ident' it keeps all K rows and
    every v, 1 included); the one row of image 1 survives, so its joints travel.  No row at a kink of the filter."""
    labels, fmap = kc.labels(rotated, J), kc.forward_maps(view)
    assert labels['counts'].tolist() == [0, 1, kc.K]
    out, judged = ko.transform_labels_kps(labels, fmap, kc.MAP_H, kc.MAP_W, rotated=rotated, min_size=kc.MIN_SIZE,
                                          min_visible=0.5)
    for visible, e0, e1 in judged:
        assert abs(visible - 0.5) > 1e-6 and abs(e0 - kc.MIN_SIZE) > 1e-6 and abs(e1 - kc.MIN_SIZE) > 1e-6
    counts = out['counts'].tolist()
    rows = ko.kept_rows(labels, fmap, kc.MAP_H, kc.MAP_W, rotated, kc.MIN_SIZE, 0.5)
    assert counts[:2] == [0, 1] and max(rows[2]) >= 64
    assert _both(out['visibility'][2], counts[2]) and not out['visibility'][0].any()
    if view == 'ident':
        assert counts[2] == kc.K and np.array_equal(out['visibility'][2], labels['visibility'][2])
        assert (out['visibility'][2] == 1).any() and np.isnan(out['keypoints'][2]).any()
        assert len(judged) == 1
    else:
        assert 10 < counts[2] < kc.K - 10 and len(judged) == kc.K + 1
        assert not (out['visibility'] == 1).any() and np.isfinite(out['keypoints']).all()
        src_v = labels['visibility'][2, rows[2]]
        assert ((src_v == 2) & (out['visibility'][2, :counts[2]] == 0)).any()        # left the map, or was not finite
    if view == 'shift':                                       # joints exactly on the right edge (outside) and on (0, 0)
        got, vis = out['keypoints'][2, :counts[2]], out['visibility'][2, :counts[2]]
        assert ((got[..., 0] == kc.MAP_W) & (vis == 0)).any() and ((got == 0).all(-1) & (vis == 2)).any()
    assert out['joints'] == F(D(int((out['visibility'] == 2).sum())) / D(kc.B)) and out['joints'] > 0


# -- argument checks ----------------------------------------------------------------------------------------------------
def test_the_entry_points_check_their_arguments_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 32 * 8)
    first = lambda **kw: [kw.get('d', p), p, p, None, q, q, q, q, q, q, q, kw.get('B', 1), 2, 1, kw.get('J', 3), 0, 1,
                          kw.get('h', 4), 4, kw.get('s', 0.0), None]
    assert L.cnuda_pseudo_labels_kps(*first(d=None)) == -1 and b'null' in L.cnuda_last_error()
    assert L.cnuda_pseudo_labels_kps(*first(J=0)) == -1 and b'bad sizes' in L.cnuda_last_error()
    assert L.cnuda_pseudo_labels_kps(*first(h=0)) == -1 and b'bad map' in L.cnuda_last_error()
    assert L.cnuda_pseudo_labels_kps(*first(s=float('nan'))) == -1 and b'NaN' in L.cnuda_last_error()
    second = lambda **kw: [kw.get('g', p), p, p, p, p, p, q, q, q, kw.get('o', q), q, q, q, q, 1, kw.get('K', 2),
                           kw.get('J', 3), 0, kw.get('h', 4), 4, kw.get('s', 0.0), 0.5, None]
    assert L.cnuda_labels_transform_kps(*second(g=None)) == -1 and b'null' in L.cnuda_last_error()
    assert L.cnuda_labels_transform_kps(*second(K=0)) == -1 and b'bad sizes' in L.cnuda_last_error()
    assert L.cnuda_labels_transform_kps(*second(J=0)) == -1 and b'bad sizes' in L.cnuda_last_error()
    assert L.cnuda_labels_transform_kps(*second(h=0)) == -1 and b'bad map' in L.cnuda_last_error()
    assert L.cnuda_labels_transform_kps(*second(s=float('nan'))) == -1 and b'NaN' in L.cnuda_last_error()
    assert L.cnuda_labels_transform_kps(*second(o=p)) == -1 and b'must not be the inputs' in L.cnuda_last_error()
    assert L.cnuda_abi_version() == hr.ABI_VERSION == 2


def test_the_operators_refuse_bad_arguments():
    from hip_runtime import ops
    dets, thr, kps = torch.zeros(1, 2, 6), torch.zeros(1), torch.zeros(1, 2, 3, 2)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.pseudo_labels(dets, thr, 4, kps=kps, map_height=4)
    with pytest.raises(RuntimeError, match='map_height'):
        ops.pseudo_labels(dets, thr, 4, kps=kps)
    with pytest.raises(RuntimeError, match='kps'):
        ops.pseudo_labels(dets, thr, 4, flip_perm=[0, 2, 1])
    for bad in ([0, 1], [0, 1, 1], [0, 1, 3], [0.0, 1.0, 2.0]):
        with pytest.raises(RuntimeError, match='flip_perm'):
            ops._flip_perm(bad, 3, dets.device)
    assert ops._flip_perm([0, 2, 1], 3, dets.device).tolist() == [0, 2, 1] and ops._flip_perm(None, 3, dets.device) is None
    labels = {'boxes': torch.zeros(1, 2, 4, dtype=torch.float64), 'classes': torch.zeros(1, 2, dtype=torch.int32),
              'counts': torch.zeros(1, dtype=torch.int32), 'keypoints': torch.zeros(1, 2, 3, 2, dtype=torch.float64),
              'visibility': torch.zeros(1, 2, 3, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.transform_labels(labels, np.eye(3)[None, :2], 4, 4)
    for key in ('keypoints', 'visibility'):
        with pytest.raises(RuntimeError, match="only one of 'keypoints' and 'visibility'"):
            ops.transform_labels({k: v for k, v in labels.items() if k != key}, np.eye(3)[None, :2], 4, 4)
