"""No-GPU checks that pin tests/targets_modes_oracle.py (the numpy restatement of the dataset loop's keypoint and
rotated modes) by answers that do not come from it, plus utils.box.get_annotation_with_angle and the argument checks
of the new C entry points."""
import itertools

import numpy as np
import pytest

import targets_modes_oracle as tmo
from oracle import targets as ot


def _rotated_corners(cx, cy, w, h, angle):
    """utils.box.rotate_bboxes' formula without the truncation to integers."""
    t = np.radians(angle)
    c, s = np.cos(t), np.sin(t)
    half = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return np.array([cx, cy]) + half @ np.array([[c, s], [-s, c]])


def _f32(points):
    return np.asarray(points, dtype=np.float64).astype(np.float32)


def test_upright_rectangle():
    got = tmo.rotated_annotation(_f32([(10, 20), (30, 20), (30, 70), (10, 70)]))
    np.testing.assert_array_equal(got, np.array([20, 45, 20, 50, 0], np.float32))


def test_lying_rectangle():
    got = tmo.rotated_annotation(_f32([(20, 10), (70, 10), (70, 30), (20, 30)]))
    np.testing.assert_array_equal(got, np.array([45, 20, 20, 50, -90], np.float32))


@pytest.mark.parametrize('angle', [30.0, -60.0, 75.0])
def test_rotated_rectangle_is_recovered(angle):
    got = tmo.rotated_annotation(_f32(_rotated_corners(64.3, 61.7, 20, 50, angle)))
    np.testing.assert_allclose(got, [64.3, 61.7, 20, 50, angle], rtol=0, atol=1e-4)
    # and utils.box.rotate_bboxes gives the rectangle back (to its integer truncation)
    from utils.box import rotate_bboxes
    want = _rotated_corners(64.3, 61.7, 20, 50, angle)
    back = rotate_bboxes(got[None].astype(np.float64))[0]
    assert np.abs(back - want).max() <= 1.0


def test_all_orderings_of_the_corners_agree():
    pts = _f32(_rotated_corners(64.3, 61.7, 20, 50, 30.0))
    want = tmo.rotated_annotation(pts)
    for perm in itertools.permutations(range(4)):
        np.testing.assert_allclose(tmo.rotated_annotation(pts[list(perm)]), want, rtol=0, atol=1e-5, err_msg=str(perm))


def test_corner_clipped_at_the_map_edge():
    H = W = 64
    pts = tmo.clip_points(_rotated_corners(8.0, 30.0, 20, 50, 30.0), H, W)
    assert (pts[:, 0] == 0).sum() == 1                                  # one corner was cut off by the edge
    cx, cy, w, h, angle = [float(v) for v in tmo.rotated_annotation(pts)]
    t = np.radians(angle)
    u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
    rel = pts.astype(np.float64) - [cx, cy]
    assert np.abs(rel @ u).max() <= w / 2 + 1e-4 and np.abs(rel @ v).max() <= h / 2 + 1e-4   # contains all four
    # sweep: the enclosing rectangle of every direction in 0.01 degree steps.  Each extent is at most the diameter D
    # and changes by at most D per radian, so the area changes by at most 2 D^2 per radian: no direction between two
    # samples can beat the best sample by more than 2 D^2 * step / 2.
    step = np.radians(0.01)
    th = np.arange(0, 18000) * step
    uu = np.stack([np.cos(th), np.sin(th)], 1)
    vv = np.stack([-np.sin(th), np.cos(th)], 1)
    a, c = pts.astype(np.float64) @ uu.T, pts.astype(np.float64) @ vv.T
    sweep = (a.max(0) - a.min(0)) * (c.max(0) - c.min(0))
    D = max(np.hypot(*(p - q)) for p in pts.astype(np.float64) for q in pts.astype(np.float64))
    assert w * h <= sweep.min() + 1e-3                                  # no sampled direction is better
    assert w * h >= sweep.min() - D * D * step                          # and it is a minimum, not merely a bound
    assert w < h and -90 <= angle < 90


def test_degenerate_points_are_skipped():
    H, W = 32, 48
    collinear = tmo.clip_points([(-5, 3), (-2, 10), (-8, 20), (-1, 30)], H, W)      # all clipped onto x = 0
    assert (collinear[:, 0] == 0).all() and tmo.rotated_annotation(collinear) is None
    pairs = _f32([(5, 5), (20, 9), (5, 5), (20, 9)])
    assert tmo.rotated_annotation(pairs) is None
    assert tmo.rotated_annotation(_f32([(7, 7)] * 4)) is None
    # in the loop: the slot's rows stay zero and the next slot is unaffected
    good = _rotated_corners(20.3, 15.6, 6, 12, 20.0)
    corners = np.stack([good, [(-5, 3), (-2, 10), (-8, 20), (-1, 30)], good + 9.0])
    out = tmo.encode_targets_modes([0, 1, 1], 2, H, W, 4, corners=corners)
    np.testing.assert_array_equal(out['reg_mask'], [1, 0, 1, 0])
    for key in ('wh', 'reg', 'gt_dets', 'gt_areas', 'ind'):
        assert not out[key][1].any(), key
    alone = tmo.encode_targets_modes([1], 2, H, W, 4, corners=corners[2:])
    for key in ('wh', 'reg', 'gt_dets', 'gt_areas', 'ind'):
        np.testing.assert_array_equal(out[key][2], alone[key][0])
    np.testing.assert_array_equal(out['hm'][1], alone['hm'][1])


def test_exact_square_gets_the_longer_h():
    got = tmo.rotated_annotation(_f32([(10, 10), (30, 10), (30, 30), (10, 30)]))
    assert got[2] == 20 and got[3] == 21 and tuple(got[:2]) == (20, 20)


def test_rotated_loop_on_a_known_rectangle():
    H, W = 96, 64
    out = tmo.encode_targets_modes([2], 3, H, W, 2, corners=np.array([[(10, 20), (30, 20), (30, 70), (10, 70)]], float),
                                   areas=np.array([123.5]))
    assert out['ind'][0] == 45 * W + 20 and out['reg_mask'][0] == 1
    np.testing.assert_array_equal(out['wh'][0], [20, 50, 0])
    np.testing.assert_array_equal(out['reg'][0], [0, 0])
    np.testing.assert_array_equal(out['gt_dets'][0], [20, 45, 20, 50, 0, 1, 2])
    assert out['gt_areas'][0] == np.float32(123.5)
    assert out['hm'][2, 45, 20] == 1 and (out['hm'] == 1).sum() == 1
    radius = int(ot.gaussian_radius((50.0, 20.0)))
    assert out['hm'][2, 45, 20 + radius] > 0 and out['hm'][2, 45, 20 + radius + 1] == 0
    nan = tmo.encode_targets_modes([2], 3, H, W, 2, corners=np.array([[(10, 20), (30, 20), (30, 70), (10, 70)]], float),
                                   areas=np.array([np.nan]))
    assert nan['gt_areas'][0] == 1000


def test_axis_mode_agrees_with_the_frozen_oracle():
    rs = np.random.RandomState(3)
    H, W, M, n = 24, 40, 8, 6
    c = rs.uniform(0, [W, H], (n, 2))
    s = rs.uniform(1, 20, (n, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], 1)
    classes = rs.randint(0, 3, n)
    got = tmo.encode_targets_modes(classes, 3, H, W, M, boxes=boxes)
    want = ot.encode_targets(boxes, classes, 3, H, W, M)
    for key, v in want.items():
        np.testing.assert_array_equal(got[key], v, err_msg=key)


def test_keypoints_y_is_tested_against_the_width_and_only_v2_counts():
    H, W = 24, 40                                                       # H != W: y = 30 is below the map but < W
    boxes = np.array([[10.0, 4.0, 21.0, 15.0], [5.0, 5.0, 5.0, 9.0]])   # the second box is empty: rows stay zero
    kpts = np.array([[(12.5, 30.0), (12.5, 40.0), (40.0, 3.0), (-0.5, 3.0), (39.75, 0.0), (3.0, 3.0), (3.0, 3.0)]] * 2)
    vis = np.array([[2, 2, 2, 2, 2, 1, 0]] * 2)
    out = tmo.encode_targets_modes([0, 0], 1, H, W, 3, boxes=boxes, keypoints=kpts, visibility=vis)
    np.testing.assert_array_equal(out['kp_reg_mask'][0], np.repeat([1, 0, 0, 0, 1, 0, 0], 2))
    ct_int = np.array([15, 9])                                          # centre (15.5, 9.5) truncated
    np.testing.assert_array_equal(out['kps'][0], (kpts[0] - ct_int).reshape(-1).astype(np.float32))
    np.testing.assert_array_equal(out['gt_kps'][0], kpts[0].astype(np.float32))
    for key in ('kps', 'gt_kps', 'kp_reg_mask'):
        assert not out[key][1:].any(), key
    assert out['kps'].shape == (3, 14) and out['gt_kps'].shape == (3, 7, 2) and out['kp_reg_mask'].dtype == np.uint8


def test_get_annotation_with_angle():
    from utils.box import get_annotation_with_angle as norm
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 20, 50, 30]}), np.array([10, 11, 20, 50, 30], np.float32))
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 50, 20, 30]}), np.array([10, 11, 20, 50, -60], np.float32))
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 50, 20, -30]}), np.array([10, 11, 20, 50, 60], np.float32))
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 20, 50, 90]}), np.array([10, 11, 20, 50, -90], np.float32))
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 50, 20, 0]}), np.array([10, 11, 20, 50, -90], np.float32))
    np.testing.assert_array_equal(norm({'rbbox': [10, 11, 20, 20, 5]}), np.array([10, 11, 20, 21, 5], np.float32))
    assert norm({'rbbox': (1, 2, 3, 4, 5)}).dtype == np.float32
    with pytest.raises(ValueError, match='rbbox'):
        norm({'bbox': [1, 2, 3, 4]})


def test_new_entry_points_reject_null_pointers_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    assert L.cnuda_encode_targets_modes(*[None] * 17, 1, 1, 4, 4, 2, 0, None) == -1
    assert b'cnuda_encode_targets_modes' in L.cnuda_last_error()
    assert L.cnuda_prepare_input(None, None, 1, 4, 4, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, None) == -1
    assert b'cnuda_prepare_input' in L.cnuda_last_error()


def test_python_entries_refuse_cpu_tensors():
    import torch
    from datasets import encode_targets, prepare_input
    z = torch.zeros
    with pytest.raises(RuntimeError, match='MI355X only'):
        encode_targets(None, z(1, 2, dtype=torch.int32), z(1, dtype=torch.int32), 2, 8, 8,
                       corners=z(1, 2, 4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='MI355X only'):
        prepare_input(z(1, 4, 4, 3, dtype=torch.uint8))


def test_rectangle_matches_cv2():
    cv2 = pytest.importorskip('cv2')
    from utils.box import get_annotation_with_angle
    rs = np.random.RandomState(11)
    for _ in range(50):
        w, h = rs.uniform(3, 30), rs.uniform(31, 60)
        pts = _f32(_rotated_corners(rs.uniform(40, 80), rs.uniform(40, 80), w, h, rs.uniform(-89, 89)))
        ct, size, angle = cv2.minAreaRect(pts)
        want = get_annotation_with_angle({'rbbox': np.array([ct[0], ct[1], size[0], size[1], angle])})
        got = tmo.rotated_annotation(pts)
        np.testing.assert_allclose(got[:4], want[:4], rtol=0, atol=1e-3)
        assert abs((got[4] - want[4] + 90) % 180 - 90) <= 1e-2
