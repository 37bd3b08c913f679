"""The geometric view on the GPU: csrc/geomview.hip against the numpy oracle (tests/geometric_view_oracle.py) -- the warp
bit for bit, the label transform in survivors, order and counts exactly and in geometry to 1e-9 cells --, known pictures
that do not pass through the oracle, the two kernels' common convention, the launch accounting, and
`uda.GeometricTeacher` through its training step, a resumed run and the driver."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import coco_fixture as fx
import geometric_view_oracle as go
import strong_view_helpers as sh
import strong_view_oracle as so
from strong_view_helpers import DEV, F, G, N, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (33, 65), (64, 96)]       # smaller than a tile; one past a tile edge, W % 4 = 1; whole tiles
SENTINEL = F(-777.25)
_CACHE = {}


def _matrices(H, W):
    """[4, 3, 3] inverses: the identity, the mirror, a half turn, a general similarity (33 degrees, 0.8, shifts of 0.13 W
    and -0.07 H)."""
    from datasets.augment import fliplr_matrix
    from datasets.geometric_view import similarity_matrices
    return np.stack([np.eye(3), fliplr_matrix(W), similarity_matrices(H, W, 180.0)[1],
                     similarity_matrices(H, W, 33.0, 0.8, (0.13, -0.07))[1]])


def _case(H, W, C):
    """(x, the inverses, the oracle's view), computed once per case and never written."""
    key = (H, W, C)
    if key not in _CACHE:
        x = np.random.default_rng(7 * H + W + C).uniform(-3, 3, (4, C, H, W)).astype(F)
        inv = _matrices(H, W)
        want = go.warp(x, inv)
        for a in (x, inv, want):
            a.setflags(write=False)
        _CACHE[key] = (x, inv, want)
    return _CACHE[key]


def _check_case(x, want, got):
    assert same_bits(got, want)
    # what the oracle must itself give, on its inputs alone
    assert same_bits(got[0], x[0])                                              # the identity: the input's bits
    assert same_bits(got[1], x[1][..., ::-1])                                   # the mirror
    assert same_bits(got[2], x[2][..., ::-1, ::-1])                             # the half turn
    assert (got[3] == 0).any() and (got[3] != 0).any()                          # the fill, and the picture


# ---------------------------------------------------------------------------------------------------------------------
# 1. the warp against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 5])
@pytest.mark.parametrize('H,W', SHAPES)
def test_warp_is_the_oracle_bit_for_bit(H, W, C):
    from datasets.geometric_view import warp_batch
    x, inv, want = _case(H, W, C)
    dx = G(x)
    got = warp_batch(dx, inv)
    assert got is not dx and got.is_contiguous() and got.dtype == torch.float32 and got.shape == dx.shape
    _check_case(x, want, N(got))
    assert same_bits(N(dx), x)                                                  # x is never written
    # the 2 x 3 and the flat layout of the matrices, and another fill
    assert same_bits(N(warp_batch(dx, inv[:, :2])), want) and same_bits(N(warp_batch(dx, inv[:, :2].reshape(4, 6))), want)
    filled = N(warp_batch(dx, inv, fill=-1.5))
    assert same_bits(filled, go.warp(x, inv, fill=-1.5)) and (filled[3] == -1.5).any() and not same_bits(filled, want)


@pytest.mark.parametrize('guard', [8, 5], ids=['y_aligned', 'y_off_by_one'])
def test_misaligned_input_and_guarded_output(guard):
    """(33, 65) with x one element into a 16-byte aligned buffer, y between `guard` sentinel elements on either side
    (5: y starts 4 bytes past a 16-byte boundary as well)."""
    from datasets.geometric_view import warp_batch
    x, inv, want = _case(33, 65, 3)
    n = x.size
    xbuf = torch.full((n + 2,), float(SENTINEL), dtype=torch.float32, device=DEV)
    assert xbuf.data_ptr() % 16 == 0
    xbuf[1:1 + n] = G(x).reshape(-1)
    dx = xbuf[1:1 + n].view(x.shape)
    assert dx.data_ptr() % 16 == 4 and dx.is_contiguous()
    ybuf = torch.full((n + 2 * guard,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dy = ybuf[guard:guard + n].view(x.shape)
    assert dy.data_ptr() % 16 == (4 * guard) % 16
    before = N(xbuf).copy()
    got = warp_batch(dx, inv, out=dy)
    assert got is dy
    _check_case(x, want, N(got))
    whole = N(ybuf)
    assert (whole[:guard] == SENTINEL).all() and (whole[guard + n:] == SENTINEL).all()
    assert same_bits(N(xbuf), before)
    # an aligned copy of a whole-tile shape takes the 16-byte stores: the same bits between the same guards
    x, inv, want = _case(64, 96, 3)
    ybuf = torch.full((x.size + 2 * guard,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dy = ybuf[guard:guard + x.size].view(x.shape)
    assert same_bits(N(warp_batch(G(x), inv, out=dy)), want)
    whole = N(ybuf)
    assert (whole[:guard] == SENTINEL).all() and (whole[guard + x.size:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. known pictures, without the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_known_pictures():
    import predict
    from datasets.augment import fliplr_matrix
    from datasets.geometric_view import similarity_matrices, warp_batch
    x = np.random.default_rng(3).uniform(-3, 3, (2, 3, 33, 33)).astype(F)
    dx = G(x)
    one = lambda m: np.tile(m, (2, 1, 1))
    assert same_bits(N(warp_batch(dx, one(similarity_matrices(33, 33, 180)[1]))), x[..., ::-1, ::-1])
    # positive = clockwise on the y-down image: np.rot90 turns counter-clockwise for positive k
    assert same_bits(N(warp_batch(dx, one(similarity_matrices(33, 33, 90)[1]))), np.rot90(x, -1, axes=(2, 3)))
    assert same_bits(N(warp_batch(dx, one(similarity_matrices(33, 33, -90)[1]))), np.rot90(x, 1, axes=(2, 3)))
    assert same_bits(N(warp_batch(dx, one(similarity_matrices(33, 33, 270)[1]))), np.rot90(x, 1, axes=(2, 3)))
    # the mirror is predict.mirror_input's
    assert same_bits(N(warp_batch(dx, one(fliplr_matrix(33)))), N(predict.mirror_input(dx)))
    assert same_bits(N(predict.mirror_input(dx)), x[..., ::-1])
    # five pixels to the right and three up, `fill` in the vacated bands
    wide = np.random.default_rng(4).uniform(-3, 3, (2, 5, 40, 70)).astype(F)
    y = N(warp_batch(G(wide), one(similarity_matrices(40, 70, 0, 1, (5 / 70, -3 / 40))[1]), fill=2.5))
    assert same_bits(y[..., :37, 5:], wide[..., 3:, :65])
    assert (y[..., 37:, :] == 2.5).all() and (y[..., :, :5] == 2.5).all()
    assert same_bits(N(dx), x)


# ---------------------------------------------------------------------------------------------------------------------
# 3. launch accounting
# ---------------------------------------------------------------------------------------------------------------------
def _logged(fn):
    import hip_runtime as hr
    with hr.launch_log() as log:
        out = fn()
        torch.cuda.synchronize()
    return out, {sh.short(k): v for k, v in log.counts.items()}


def test_a_neutral_batch_launches_nothing():
    from datasets.geometric_view import GeometricViewParams, similarity_matrices, warp_batch
    x = G(sh.images(2, 16, 24, 3))
    p = GeometricViewParams.identity(2)
    y, counts = _logged(lambda: warp_batch(x, p.inverse))
    assert y is x and counts == {}
    out = torch.empty_like(x)
    y, counts = _logged(lambda: warp_batch(x, p.inverse, out=out))              # asked for a buffer: a copy
    assert y is out and counts == {'warp_bilinear_kernel': 1} and same_bits(N(out), N(x))
    p.inverse[1] = similarity_matrices(16, 24, 10.0)[1]
    y, counts = _logged(lambda: warp_batch(x, p.inverse))
    assert y is not x and counts == {'warp_bilinear_kernel': 1}
    assert same_bits(N(y)[0], N(x)[0]) and same_bits(N(y), go.warp(N(x), p.inverse))
    # the mirrored student of a neutral draw: one launch, no mirror kernel
    y, counts = _logged(lambda: warp_batch(x, GeometricViewParams.identity(2).mirrored(24)[1]))
    assert counts == {'warp_bilinear_kernel': 1} and same_bits(N(y), N(x)[..., ::-1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the labels against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
MAP_H, MAP_W = 16, 24


def _labels(rotated, K, counts, seed):
    """Rows with centres all over (and a little outside) the map, sides of 0.6 to 8 cells, any angle."""
    rs = np.random.RandomState(seed)
    B = len(counts)
    cx, cy = rs.uniform(-1, MAP_W + 1, (B, K)), rs.uniform(-1, MAP_H + 1, (B, K))
    w, h = rs.uniform(0.6, 8, (B, K)), rs.uniform(0.6, 8, (B, K))
    if rotated:
        t = np.radians(rs.uniform(-90, 90, (B, K)))
        ox, oy = np.stack([-w, w, w, -w], -1) / 2, np.stack([-h, -h, h, h], -1) / 2
        geom = np.stack([cx[..., None] + ox * np.cos(t)[..., None] - oy * np.sin(t)[..., None],
                         cy[..., None] + ox * np.sin(t)[..., None] + oy * np.cos(t)[..., None]], -1)
    else:
        geom = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1)
    classes = rs.randint(0, 5, (B, K)).astype(np.int32)
    for b, n in enumerate(counts):                       # as pseudo_labels leaves the rows behind the count
        geom[b, n:], classes[b, n:] = 0, 0
    return {'corners' if rotated else 'boxes': geom.astype(np.float64), 'classes': classes,
            'counts': np.int32(counts), 'kept': F(sum(counts) / B)}


def _forward_maps(case):
    """[3, 6] at map resolution (the similarity of the 4 x larger input, its translation divided by 4)."""
    from datasets.geometric_view import GeometricViewParams, similarity_matrices
    H, W = 4 * MAP_H, 4 * MAP_W
    per_image = {'rot33': [(33.0, 0.8, (0.13, -0.07)), (33.0, 1.0, (0.0, 0.0)), (-33.0, 1.25, (-0.05, 0.1))],
                 'quarter': [(90.0, 1.0, (0.0, 0.0)), (90.0, 1.0, (0.0, 0.0)), (-90.0, 1.0, (0.0, 0.0))],
                 'shift': [(0.0, 1.0, (0.2, 0.2)), (0.0, 1.0, (-0.3, -0.35)), (0.0, 1.0, (0.3, 0.35))]}[case]
    p = GeometricViewParams.identity(3)
    for b, (angle, scale, shift) in enumerate(per_image):
        p.forward[b], p.inverse[b] = similarity_matrices(H, W, angle, scale, shift)
    return p.forward_map(4)


def _wanted(rotated, case, min_size, K, counts):
    """(the labels, the matrices, the oracle's result), with what the case must cover asserted on the oracle's values."""
    labels = _labels(rotated, K, counts, 2 if (K == 20 and not rotated) else 1)     # (tables that cover every demand below)
    fmap = _forward_maps(case)
    want, judged = go.transform_labels(labels, fmap, MAP_H, MAP_W, rotated=rotated, min_size=min_size, min_visible=0.5)
    # no row at a kink, on the oracle's values; no case filtered out
    assert len(judged) == sum(counts)
    for visible, e0, e1 in judged:
        assert abs(visible - 0.5) > 1e-6 and abs(e0 - min_size) > 1e-6 and abs(e1 - min_size) > 1e-6
    assert any(0.0 < v[0] < 0.5 for v in judged) and any(0.5 < v[0] < 1.0 for v in judged)
    assert want['counts'][0] == 0 and all(0 < want['counts'][b] < counts[b] for b in (1, 2))
    if min_size > 0:
        assert any(min(v[1], v[2]) < min_size and v[0] >= 0.5 for v in judged)          # dropped for its size alone
    return labels, fmap, want


def _check_labels(rotated, case, min_size, K, counts):
    from hip_runtime import ops
    key = 'corners' if rotated else 'boxes'
    labels, fmap, want = _wanted(rotated, case, min_size, K, counts)
    dl = {k: G(v) for k, v in labels.items()}
    got = ops.transform_labels(dl, fmap, MAP_H, MAP_W, rotated=rotated, min_size=min_size, min_visible=0.5)
    again = ops.transform_labels(dl, G(fmap), MAP_H, MAP_W, rotated=rotated, min_size=min_size, min_visible=0.5)
    torch.cuda.synchronize()
    assert list(got) == ['classes', 'counts', 'kept', key, 'dropped']
    for k in got:
        assert got[k].dtype == G(np.asarray(want[k])).dtype and tuple(got[k].shape) == np.shape(want[k]), k
        assert same_bits(N(got[k]), N(again[k])), k                                      # two runs, the same bits
        assert k not in dl or got[k].data_ptr() != dl[k].data_ptr()                      # a new dict of new tensors
    for k in ('classes', 'counts', 'kept', 'dropped'):
        assert same_bits(N(got[k]), np.asarray(want[k])), k
    assert np.abs(N(got[key]) - want[key]).max() <= 1e-9
    for b in range(len(counts)):
        assert not N(got[key])[b, want['counts'][b]:].any()                              # zeros behind the survivors
    assert int(N(got['counts']).sum()) + round(float(got['dropped']) * len(counts)) == sum(counts)
    for k, v in labels.items():
        assert same_bits(N(dl[k]), np.asarray(v)), k                                     # the inputs are not written
    return want


@pytest.mark.parametrize('min_size', [0.0, 2.0])
@pytest.mark.parametrize('case', ['rot33', 'quarter', 'shift'])
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_transform_labels_against_the_oracle(rotated, case, min_size):
    want = _check_labels(rotated, case, min_size, 20, (0, 7, 20))
    if case == 'shift':                                  # rows leave over every edge: the two images shift opposite ways
        assert want['counts'][1] < 7 and want['counts'][2] < 20


@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_transform_labels_over_more_than_one_ballot(rotated):
    """K = 200: four rounds of 64 rows per image, survivors placed across their boundaries."""
    want = _check_labels(rotated, 'rot33', 2.0, 200, (0, 70, 200))
    assert want['counts'][2] > 64


def test_the_identity_keeps_every_row_and_the_mirror_is_left_to_pseudo_labels():
    from hip_runtime import ops
    for rotated in (False, True):
        key = 'corners' if rotated else 'boxes'
        labels = _labels(rotated, 20, (0, 7, 20), 5)
        dl = {k: G(v) for k, v in labels.items()}
        got = ops.transform_labels(dl, np.tile(np.float64([1, 0, 0, 0, 1, 0]), (3, 1)), MAP_H, MAP_W, rotated=rotated,
                                   min_size=100.0, min_visible=1.0)
        for k in ('classes', 'counts', 'kept', key):
            assert same_bits(N(got[k]), np.asarray(labels[k])), k
        assert float(got['dropped']) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the two kernels agree on the convention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('angle,scale,shift', [(33.0, 1.0, (0.0, 0.0)), (33.0, 0.8, (0.1, -0.05)), (90.0, 1.0, (0.0, 0.0)),
                                               (0.0, 1.0, (0.15, -0.2))], ids=['rot33', 'similarity', 'quarter', 'shift'])
@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_a_bright_patch_lands_where_its_label_does(rotated, angle, scale, shift):
    """64 x 64 inputs, a 16 x 16 map: a 3 x 3 patch of ones on a zero (= fill) ground at a box centre; after the warp its
    intensity centroid lies within half an input pixel -- the resolution of the sampling grid -- of 4 x the centre of
    the transformed label."""
    from datasets.geometric_view import GeometricViewParams, similarity_matrices, warp_batch
    from hip_runtime import ops
    S, down = 64, 4
    rows, cols = (22, 40), (37, 25)                      # the patches' centre pixels, one image each
    x = np.zeros((2, 3, S, S), F)
    centres = []
    for b in range(2):
        x[b, :, rows[b] - 1:rows[b] + 2, cols[b] - 1:cols[b] + 2] = 1
        centres.append(((cols[b] + 0.5) / down, (rows[b] + 0.5) / down))
    p = GeometricViewParams.identity(2)
    for b in range(2):
        p.forward[b], p.inverse[b] = similarity_matrices(S, S, angle, scale, shift)
    y = N(warp_batch(G(x), p.inverse))
    if rotated:
        geom = np.float64([[[[cx - 1.5, cy - 1], [cx + 1.5, cy - 1], [cx + 1.5, cy + 1], [cx - 1.5, cy + 1]]]
                           for cx, cy in centres])
    else:
        geom = np.float64([[[cx - 1.5, cy - 1, cx + 1.5, cy + 1]] for cx, cy in centres])
    labels = {'corners' if rotated else 'boxes': G(geom), 'classes': G(np.zeros((2, 1), np.int32)),
              'counts': G(np.ones(2, np.int32))}
    got = ops.transform_labels(labels, p.forward_map(down), S // down, S // down, rotated=rotated, min_visible=0.5)
    assert N(got['counts']).tolist() == [1, 1]
    out = N(got['corners' if rotated else 'boxes'])
    for b in range(2):
        lx, ly = (out[b, 0].mean(0) if rotated else (out[b, 0, [0, 2]].mean(), out[b, 0, [1, 3]].mean()))
        assert same_bits(y[b, 0], y[b, 1]) and y[b].sum() > 0
        cx, cy = go.centroid(y[b, 0])
        assert abs(cx - down * lx) <= 0.5 and abs(cy - down * ly) <= 0.5, (cx, cy, down * lx, down * ly)
        assert math.hypot(down * lx - (cols[b] + 0.5), down * ly - (rows[b] + 0.5)) > 3          # it did move


# ---------------------------------------------------------------------------------------------------------------------
# 6. the plugin: ResNet-18, 64 x 64, B = 2
# ---------------------------------------------------------------------------------------------------------------------
STAT_NAMES = ['centernet_loss', 'hm_loss', 'wh_loss', 'off_loss', 'pseudo_centernet_loss', 'pseudo_hm_loss',
              'pseudo_wh_loss', 'pseudo_off_loss', 'pseudo_boxes', 'pseudo_dropped', 'total_loss']
VIEW = {'rotate': [-30, 30], 'scale': [0.8, 1.25], 'translate_percent': [-0.25, 0.25]}
OFF = {'rotate': None, 'scale': None, 'translate_percent': None}


def _params(target, n, seed=42, config=VIEW):
    from datasets.geometric_view import GeometricView
    B, _, H, W = target.shape
    return GeometricView(config).sample(B, H, W, np.random.default_rng([seed, 0x47454F, n]))


def _expected_view(target, n, seed=42, config=VIEW, mirror=True):
    """The oracle's warp of the target under the parameters the documented generator draws at step n (the mirror folded
    into the matrix), then the oracle's strong view under WeakStrongTeacher's own draws of step n."""
    from datasets.strong_view import StrongView
    B, _, H, W = target.shape
    p = _params(target, n, seed, config)
    warped = go.warp(target, p.mirrored(W)[1] if mirror else p.inverse)
    q = StrongView(None).sample(B, H, W, np.random.default_rng([seed, 0x57534B, n]), first_id=n * B)
    return sh.oracle_view(so, warped, q), p


def test_student_sees_the_warped_strong_view_and_the_teacher_the_batch_itself():
    import uda
    data = sh.data()
    target = data['target_domain_input']
    before = N(target).copy()
    plugin = sh.resnet_plugin(uda.GeometricTeacher, target, geometric_view=VIEW)
    cap = sh.Capture(plugin)
    seen = []
    for n in range(2):
        cap.clear()
        out = plugin.step(data)
        torch.cuda.synchronize()
        assert list(out['stats']) == STAT_NAMES
        assert all(math.isfinite(float(v)) for v in out['stats'].values())
        want, p = _expected_view(before, n)
        assert len(cap.student) == 2 and len(cap.teacher) == 1
        assert same_bits(cap.student[0], N(data['input'])) and same_bits(cap.student[1], want)
        assert same_bits(cap.teacher[0], before)                                 # the un-warped, un-mirrored target
        assert data['target_domain_input'] is target and same_bits(N(target), before)
        assert p.drawn.all() and not p.neutral.any() and plugin.teacher_updates == n + 1
        seen.append(want)
    assert not same_bits(seen[0], seen[1])
    # without the mirror the matrix is A's own inverse
    plain = sh.resnet_plugin(uda.GeometricTeacher, target, geometric_view=VIEW, mirror_student=False)
    assert same_bits(N(plain.student_view(target)), _expected_view(before, 0, mirror=False)[0])
    cap.remove()


def test_the_pseudo_batch_is_encode_targets_of_the_oracles_labels():
    import uda
    from backends.decode import decode_detection
    from datasets.targets import encode_targets
    from hip_runtime import ops
    data = sh.data()
    target = data['target_domain_input']
    shift = {'rotate': [-20, 20], 'scale': None, 'translate_percent': [0.2, 0.3]}        # rows leave on two edges
    plugin = sh.resnet_plugin(uda.GeometricTeacher, target, geometric_view=shift)
    got = plugin.pseudo_batch(target)
    with torch.no_grad():
        heads = plugin.teacher(target)
        hm = ops.sigmoid_clamp_(heads['hm'])
        dets = decode_detection(hm, heads['wh'], heads['reg'], K=sh.KDET)
        labels = ops.pseudo_labels(dets, plugin._thresholds, 16, mirror=True, min_size=plugin.min_size)
    host = {k: N(v) for k, v in labels.items()}
    p = _params(N(target), 0, config=shift)
    want, judged = go.transform_labels(host, p.forward_map(4), 16, 16, min_size=plugin.min_size, min_visible=0.5)
    assert all(abs(v[0] - 0.5) > 1e-6 and abs(v[1] - plugin.min_size) > 1e-6 and abs(v[2] - plugin.min_size) > 1e-6
               for v in judged)
    ref = encode_targets(G(want['boxes']), G(want['classes']), G(want['counts']), 3, 16, 16)
    assert sorted(got) == sorted(list(ref) + ['kept', 'dropped'])
    for k in ref:
        assert same_bits(N(got[k]), N(ref[k])), k
    assert same_bits(N(got['kept']), np.asarray(want['kept'])) and same_bits(N(got['dropped']), np.asarray(want['dropped']))
    # boxes + dropped is what the parent counts on the same batch
    parent = sh.resnet_plugin(uda.WeakStrongTeacher, target)                  # the same seed: the same model
    assert float(got['kept']) + float(got['dropped']) == float(labels['kept']) == float(parent.pseudo_batch(target)['kept'])
    assert float(got['kept']) > 0 and float(got['dropped']) > 0
    out = plugin.step(data)
    assert float(out['stats']['pseudo_boxes']) == float(got['kept'])
    assert float(out['stats']['pseudo_dropped']) == float(got['dropped'])


@pytest.mark.parametrize('config', [OFF, {'p': 0}], ids=['null', 'p0'])
def test_the_identity_configuration_is_weak_strong_teacher_bit_for_bit(config):
    import uda
    res = []
    for cls, kwargs in ((uda.WeakStrongTeacher, {}), (uda.GeometricTeacher, {'geometric_view': config})):
        data = sh.data()
        plugin = sh.resnet_plugin(cls, data['target_domain_input'], **kwargs)
        for _ in range(2):
            out = plugin.step(data)
        torch.cuda.synchronize()
        res.append(({k: N(v) for k, v in out['stats'].items()}, {k: N(v) for k, v in out['target_domain'].items()},
                    sh.snapshot(plugin.backend), sh.snapshot(plugin.teacher), plugin.teacher_updates))
    (stats_a, out_a, student_a, teacher_a, n_a), (stats_b, out_b, student_b, teacher_b, n_b) = res
    assert float(stats_b.pop('pseudo_dropped')) == 0.0 and n_a == n_b == 2
    assert float(stats_a['pseudo_boxes']) > 0
    for a, b in ((stats_a, stats_b), (out_a, out_b), (student_a, student_b), (teacher_a, teacher_b)):
        assert list(a) == list(b)
        for k in a:
            assert same_bits(a[k], b[k]), k


def test_a_resumed_run_continues_the_same_geometric_stream(tmp_path):
    import uda
    data = sh.data()
    target = data['target_domain_input']
    straight = sh.resnet_plugin(uda.GeometricTeacher, target, geometric_view=VIEW)
    cap = sh.Capture(straight)
    straight.step(data)
    cap.clear()
    straight.step(data)
    torch.cuda.synchronize()
    second = cap.student[1]
    first = sh.resnet_plugin(uda.GeometricTeacher, target, geometric_view=VIEW)
    first.step(data)
    path = str(tmp_path / 'model_last.pth')
    first.save_model(path, 1, True)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['epoch', 'optimizer', 'state_dict', 'teacher_state_dict', 'teacher_updates']    # no new entry
    fresh = sh.resnet_plugin(uda.GeometricTeacher, target, seed=9, geometric_view=VIEW)
    fresh.load_model(path, resume=True)
    assert fresh.teacher_updates == 1
    cap = sh.Capture(fresh)
    fresh.step(data)
    torch.cuda.synchronize()
    assert same_bits(cap.student[1], second) and same_bits(second, _expected_view(N(target), 1)[0])
    assert not same_bits(second, _expected_view(N(target), 0)[0])


def test_one_step_with_a_rotated_box_model_and_any_angle():
    import uda
    from backends import resnet
    from backends.decode import decode_detection
    from hip_runtime import ops, optim
    from losses.centernet import DetectionLoss
    data = {k: G(v) for k, v in sh.gin.detection_batch(2, 3, 16, 16, 8, (3, 2), 3, 61).items()}
    data['input'] = G(sh.gin.image_batch(2, 64, 64, 60))
    data['target_domain_input'] = target = G(sh.gin.image_batch(2, 64, 64, 70))
    torch.manual_seed(3)
    model = resnet.build(18, num_classes=3, pretrained=False, rotated_boxes=True).to(DEV)
    with torch.no_grad():                                # strong_view_helpers.condition, for the rotated decode
        sh._last_conv(model.wh).bias.fill_(5.0)
        sh._last_conv(model.hm).bias.fill_(-2.19)
        model.eval()
        sh._last_conv(model.hm).weight.mul_(1.5 / float(model(target)['hm'].std()))
        heads = model(target)
        dets = decode_detection(ops.sigmoid_clamp_(heads['hm']), heads['wh'], heads['reg'], K=sh.KDET, rotated=True)
    model.train()
    plugin = uda.GeometricTeacher(0.5, geometric_view={'rotate': [-180, 180]},
                                  score_threshold=sh.threshold_between(N(dets)[..., 5]))
    plugin.cfg = sh.cfg(3)
    plugin.cfg['model']['backend']['params']['rotated_boxes'] = True
    plugin.device, plugin.backend = torch.device(DEV), model
    plugin.optimizer = optim.Adam([q for q in model.parameters() if q.requires_grad], lr=1e-3)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, angle_weight=1.0, periodic=True)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    plugin.host_stats = False
    p = _params(N(target), 0, config={'rotate': [-180, 180]})
    assert (np.abs(p.rotate) > 30).any()
    batch = plugin.pseudo_batch(target)
    assert batch['wh'].shape[-1] == 3 and float(batch['kept']) > 0
    out = plugin.step(data)
    torch.cuda.synchronize()
    assert {'pseudo_boxes', 'pseudo_dropped', 'pseudo_hm_loss', 'total_loss'} <= set(out['stats'])
    assert all(math.isfinite(float(v)) for v in out['stats'].values())
    assert float(out['stats']['pseudo_boxes']) == float(batch['kept'])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the driver
# ---------------------------------------------------------------------------------------------------------------------
def test_the_driver_trains_logs_and_saves_with_the_geometric_teacher(tmp_path, monkeypatch):
    """train.py for two epochs of two steps on the fixture dataset with the README's override -- its burn-in cut to one
    step."""
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
        'max_detections': 20, 'epochs': 2, 'batch_size': 4, 'num_workers': 0,
        'hydra': {'run': {'dir': str(root / 'runs') + '/${experiment}/'}},
    }
    (cfg / 'experiment' / 'tiny.yaml').write_text(yaml.safe_dump(experiment))
    summary = train.main(['--config-dir', str(cfg), 'experiment=tiny',
                          'model.uda={GeometricTeacher: {pseudo_weight: 1.0, score_threshold: 0.4, burn_in_steps: 1, '
                          'geometric_view: {rotate: [-180, 180]}}}'])
    assert summary['error'] is None and summary['epochs'] == [1, 2]
    run = summary['run_dir']
    with open(os.path.join(run, 'logs', 'scalars.jsonl')) as f:
        logged = {r['name']: r['value'] for r in map(json.loads, f)}
    for name in ('training/total_loss', 'training/pseudo_hm_loss', 'training/pseudo_boxes', 'training/pseudo_dropped',
                 'validation/total_loss'):
        assert name in logged and math.isfinite(logged[name]), (name, sorted(logged))
    last = torch.load(os.path.join(run, 'model_last.pth'), map_location='cpu', weights_only=False)
    assert last['teacher_updates'] >= 3 and list(last['teacher_state_dict']) == list(last['state_dict'])
