"""The geometric view without a GPU: the sampler (datasets/geometric_view.py), every refusal, the two C entry points'
argument checks, how the driver resolves `uda.GeometricTeacher`, and the numpy oracle of tests/geometric_view_oracle.py
pinned by hand-worked cases."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import geometric_view_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERRIDE = ('model.uda={GeometricTeacher: {pseudo_weight: 1.0, score_threshold: 0.4, burn_in_steps: 2000, '
            'geometric_view: {rotate: [-180, 180]}}}')
F = np.float32
FIELDS = ('forward', 'inverse', 'drawn', 'rotate', 'scale', 'translate_percent')
OFF = {'rotate': None, 'scale': None, 'translate_percent': None}


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in FIELDS)


class _CountingRng:
    """A generator that counts what is asked of it."""

    def __init__(self, seed=0):
        self.rng, self.calls = np.random.default_rng(seed), 0

    def random(self):
        self.calls += 1
        return self.rng.random()

    def uniform(self, lo, hi):
        self.calls += 1
        return self.rng.uniform(lo, hi)


# -- the sampler --------------------------------------------------------------------------------------------------------
def test_sampling_is_a_function_of_its_arguments_alone():
    from datasets.geometric_view import DEFAULTS, GeometricView
    assert DEFAULTS == {'p': 1.0, 'rotate': [-15, 15], 'scale': [0.8, 1.25], 'translate_percent': [-0.1, 0.1]}
    view = GeometricView()
    a = view.sample(6, 48, 64, np.random.default_rng([42, 0x47454F, 3]))
    b = GeometricView(None).sample(6, 48, 64, np.random.default_rng([42, 0x47454F, 3]))
    assert _same(a, b) and a.batch == 6
    assert a.forward.shape == a.inverse.shape == (6, 3, 3) and a.forward.dtype == a.inverse.dtype == np.float64
    assert a.drawn.shape == (6,) and a.drawn.dtype == bool and a.drawn.all() and not a.neutral.any()
    assert ((-15 <= a.rotate) & (a.rotate <= 15)).all() and ((0.8 <= a.scale) & (a.scale <= 1.25)).all()
    assert (np.abs(a.translate_percent) <= 0.1).all() and len(set(a.rotate.tolist())) == 6
    for other in (view.sample(6, 48, 64, np.random.default_rng([42, 0x47454F, 4])),
                  view.sample(6, 48, 65, np.random.default_rng([42, 0x47454F, 3])),
                  GeometricView({'rotate': [-180, 180]}).sample(6, 48, 64, np.random.default_rng([42, 0x47454F, 3]))):
        assert not _same(a, other)
    # a given mapping is merged over the defaults
    merged = GeometricView({'rotate': [-180, 180], 'p': 0.5})
    assert merged.rotate == (-180.0, 180.0) and merged.scale == (0.8, 1.25) and merged.p == 0.5
    assert merged.translate_percent == (-0.1, 0.1)
    # the scale is isotropic and the linear part a rotation times it: rectangles stay rectangles
    lin = a.forward[:, :2, :2]
    assert np.allclose(lin @ lin.transpose(0, 2, 1), (a.scale ** 2)[:, None, None] * np.eye(2), atol=1e-12)
    assert (a.forward[:, 2] == (0, 0, 1)).all() and (a.inverse[:, 2] == (0, 0, 1)).all()


def test_inverse_times_forward_is_the_identity():
    from datasets.geometric_view import GeometricView, similarity_matrices
    p = GeometricView({'rotate': [-180, 180], 'scale': [0.5, 2.0], 'translate_percent': [-0.3, 0.3]}).sample(
        64, 512, 384, np.random.default_rng(7))
    eye = np.eye(3)
    assert np.abs(p.inverse @ p.forward - eye).max() <= 1e-12 and np.abs(p.forward @ p.inverse - eye).max() <= 1e-12
    fm, im = p.mirrored(384)
    assert np.abs(im @ fm - eye).max() <= 1e-12
    # the convention of datasets.augment.affine_matrix: positive = clockwise on the y-down image, about the centre
    from datasets.augment import affine_matrix, fliplr_matrix
    for angle, scale, shift in ((33.0, 0.8, (0.13, -0.07)), (-120.0, 1.3, (0.0, 0.2))):
        fwd, inv = similarity_matrices(48, 64, angle, scale, shift)
        assert np.abs(fwd - affine_matrix(48, 64, (scale, scale), shift, angle)).max() <= 1e-12
        assert np.abs(inv @ fwd - eye).max() <= 1e-12
    fwd, _ = similarity_matrices(10, 10, 90.0)
    assert (fwd @ [6.0, 5.0, 1.0]).tolist() == [5.0, 6.0, 1.0]          # right of the centre -> below it
    # the mirrored student: A . F, F's own inverse in front of A's
    q = GeometricView().sample(2, 8, 12, np.random.default_rng(1))
    fm, im = q.mirrored(12)
    assert np.array_equal(fm, q.forward @ fliplr_matrix(12) + 0.0) and np.array_equal(im, fliplr_matrix(12) @ q.inverse + 0.0)
    # map resolution: the same linear part, the translation divided
    six = q.forward_map(4)
    assert six.shape == (2, 6) and np.array_equal(six[:, [0, 1, 3, 4]], q.forward[:, :2, :2].reshape(2, 4))
    assert np.array_equal(six[:, [2, 5]], q.forward[:, :2, 2] / 4.0)


@pytest.mark.parametrize('angle', [-270, -180, -90, 0, 90, 180, 270, 360, 450])
def test_quarter_turns_are_exact(angle):
    from datasets.geometric_view import GeometricView, similarity_matrices
    for h, w in ((7, 9), (64, 96), (33, 65)):
        for m in similarity_matrices(h, w, angle):
            assert (m * 2 == np.round(m * 2)).all() and set(np.abs(m[:2, :2]).ravel().tolist()) == {0.0, 1.0}
            assert not np.signbit(m).any() or (m[np.signbit(m)] != 0).all()       # no negative zero
    p = GeometricView({'rotate': [angle, angle], 'scale': None, 'translate_percent': None}).sample(
        2, 8, 8, np.random.default_rng(0))
    assert (p.forward * 2 == np.round(p.forward * 2)).all() and (p.rotate == angle).all()
    assert p.neutral.all() == (angle % 360 == 0)


def test_a_null_component_draws_nothing():
    from datasets.geometric_view import GeometricView, GeometricViewParams
    ident = GeometricViewParams.identity(5)
    assert ident.neutral.all() and not ident.drawn.any() and ident.batch == 5
    rng = _CountingRng()
    off = GeometricView(OFF).sample(5, 16, 16, rng)
    assert rng.calls == 0 and _same(off, ident)
    for config, per_image in (({**OFF, 'rotate': [-10, 10]}, 2), ({**OFF, 'scale': [0.9, 1.1]}, 2),
                              ({**OFF, 'translate_percent': [-0.1, 0.1]}, 3), ({'scale': None}, 4), (None, 5)):
        rng = _CountingRng()
        p = GeometricView(config).sample(5, 16, 16, rng)
        assert rng.calls == 5 * per_image and p.drawn.all()
        if config and config.get('rotate', 1) is None:
            assert (p.rotate == 0).all()
        if config and config.get('scale', 1) is None:
            assert (p.scale == 1).all()
        if config and config.get('translate_percent', 1) is None:
            assert (p.translate_percent == 0).all()
    rng = _CountingRng()
    never = GeometricView({'p': 0}).sample(5, 16, 16, rng)
    assert rng.calls == 5 and never.neutral.all() and not never.drawn.any()
    some = GeometricView({'p': 0.5}).sample(64, 16, 16, np.random.default_rng(3))
    assert 10 < some.drawn.sum() < 54 and np.array_equal(some.neutral, ~some.drawn)


@pytest.mark.parametrize('config,names', [
    ({'rotation': [0, 1]}, 'rotation'), ({'rotate': [5, -5]}, 'rotate'), ({'rotate': 5}, 'rotate'),
    ({'scale': [1.2, 0.8]}, 'scale'), ({'scale': [0.0, 1.0]}, 'scale'), ({'scale': [-1.0, 1.0]}, 'scale'),
    ({'translate_percent': [0.2, 0.1]}, 'translate_percent'), ({'translate_percent': [0.1]}, 'translate_percent'),
    ({'p': 1.5}, 'p'), ({'p': -0.1}, 'p'), ({'p': 'often'}, 'p'), ({'rotate': [0, float('inf')]}, 'rotate'),
])
def test_every_refusal_names_its_key(config, names):
    from datasets.geometric_view import GeometricView
    with pytest.raises(ValueError, match=r'\b%s\b' % names):
        GeometricView(config)


def test_sample_and_warp_refuse_bad_arguments():
    from datasets.geometric_view import GeometricView, warp_batch
    with pytest.raises(ValueError, match='positive'):
        GeometricView().sample(0, 4, 4, np.random.default_rng(0))
    eye = np.tile(np.eye(3), (2, 1, 1))
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match='MI355X only'):
        warp_batch(x, eye)
    with pytest.raises(RuntimeError, match=r'float32 \[B, C, H, W\]'):
        warp_batch(x.double(), eye)
    with pytest.raises(RuntimeError, match='contiguous'):
        warp_batch(x.transpose(2, 3), eye)
    with pytest.raises(RuntimeError, match='requires grad'):
        warp_batch(x.clone().requires_grad_(), eye)
    with pytest.raises(RuntimeError, match='inverse must be'):
        warp_batch(x, eye[:1])
    with pytest.raises(RuntimeError, match='finite'):
        warp_batch(x, np.full((2, 2, 3), np.inf))
    with pytest.raises(RuntimeError, match='affine'):
        warp_batch(x, eye * 2)
    with pytest.raises(RuntimeError, match='out must be'):
        warp_batch(x, eye, out=torch.zeros(2, 3, 4, 5))


def test_the_entry_points_check_their_arguments_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 32 * 8)
    assert L.cnuda_warp_bilinear(None, None, None, 0.0, 1, 3, 4, 4, None) == -1 and b'null' in L.cnuda_last_error()
    assert L.cnuda_warp_bilinear(p, q, p, 0.0, 1, 0, 4, 4, None) == -1 and b'bad sizes' in L.cnuda_last_error()
    assert L.cnuda_warp_bilinear(p, p, p, 0.0, 1, 1, 2, 2, None) == -1 and b'overlap' in L.cnuda_last_error()
    assert L.cnuda_warp_bilinear(p, q, p, 0.0, 1, 1, 65536, 32768, None) == -1 and b'too large' in L.cnuda_last_error()
    args = lambda **kw: [kw.get('g', p), p, p, p, kw.get('o', q), q, q, q, q, kw.get('B', 1), kw.get('K', 2), 0,
                         kw.get('h', 4), 4, kw.get('s', 0.0), 0.5, None]
    assert L.cnuda_labels_transform(*args(g=None)) == -1 and b'null' in L.cnuda_last_error()
    assert L.cnuda_labels_transform(*args(K=0)) == -1 and b'bad sizes' in L.cnuda_last_error()
    assert L.cnuda_labels_transform(*args(h=0)) == -1 and b'bad map' in L.cnuda_last_error()
    assert L.cnuda_labels_transform(*args(s=float('nan'))) == -1 and b'NaN' in L.cnuda_last_error()
    assert L.cnuda_labels_transform(*args(o=p)) == -1 and b'must not be the inputs' in L.cnuda_last_error()


def test_transform_labels_refuses_bad_arguments():
    from hip_runtime import ops
    labels = {'boxes': torch.zeros(1, 2, 4, dtype=torch.float64), 'classes': torch.zeros(1, 2, dtype=torch.int32),
              'counts': torch.zeros(1, dtype=torch.int32), 'kept': torch.zeros(())}
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.transform_labels(labels, np.eye(3)[None, :2], 4, 4)
    with pytest.raises(RuntimeError, match="'corners'"):
        ops.transform_labels(labels, np.eye(3)[None, :2], 4, 4, rotated=True)


# -- the plugin's front door --------------------------------------------------------------------------------------------
def test_the_driver_resolves_geometric_teacher():
    import uda
    from uda.mean_teacher import GeometricTeacher, WeakStrongTeacher
    assert uda.GeometricTeacher is GeometricTeacher and issubclass(GeometricTeacher, WeakStrongTeacher)
    assert 'GeometricTeacher' in dir(uda) and 'GeometricTeacher' in uda.__all__
    assert list(inspect.signature(GeometricTeacher.__init__).parameters)[1:] == [
        'pseudo_weight', 'geometric_view', 'min_visible', 'strong_view', 'mean_teacher_arguments']
    plugin = GeometricTeacher(1.0, score_threshold=0.4, burn_in_steps=2000, geometric_view={'rotate': [-180, 180]})
    assert plugin.geometric_view.rotate == (-180.0, 180.0) and plugin.min_visible == 0.5 and plugin.burn_in_steps == 2000
    assert plugin.strong_view.blur is not None and plugin.mirror_student
    assert GeometricTeacher(1.0, min_visible=1).min_visible == 1.0
    for bad in (0, 0.0, -0.5, 1.01, 'half', None, True):
        with pytest.raises(ValueError, match='min_visible'):
            GeometricTeacher(1.0, min_visible=bad)
    with pytest.raises(ValueError, match='rotation'):
        GeometricTeacher(1.0, geometric_view={'rotation': [0, 1]})
    with pytest.raises(ValueError, match='decay'):
        GeometricTeacher(1.0, decay=1.0)


def test_the_documented_override_builds_the_plugin():
    """The README's run line, through the driver's own config composition."""
    import yaml
    import uda
    assert "'" + OVERRIDE + "'" in open(os.path.join(ROOT, 'README.md')).read()
    spec = yaml.safe_load(OVERRIDE.split('=', 1)[1])
    (name, kwargs), = spec.items()
    plugin = getattr(uda, name)(**kwargs)
    assert type(plugin).__name__ == 'GeometricTeacher' and plugin.pseudo_weight == 1.0 and plugin.score_threshold == 0.4
    assert plugin.geometric_view.rotate == (-180.0, 180.0) and plugin.geometric_view.scale == (0.8, 1.25)


# -- the oracle, pinned by hand -----------------------------------------------------------------------------------------
def test_the_oracles_clip_gives_the_hand_worked_areas():
    square = [(0, 0), (1, 0), (1, 1), (0, 1)]
    shift = lambda poly, dx, dy: [(px + dx, py + dy) for px, py in poly]
    assert go.clip_area(shift(square, -0.5, 3), 24, 16) == 0.5                     # half outside the left edge
    assert go.visible_fraction(shift(square, 23.5, 3), 24, 16) == 0.5              # ... the right edge
    assert go.visible_fraction(shift(square, 3, 15.5), 24, 16) == 0.5              # ... the bottom edge
    r = math.sqrt(0.5)
    diamond = [(r, 0), (0, r), (-r, 0), (0, -r)]                                    # the unit square at 45 degrees
    assert abs(abs(go.shoelace(diamond)) - 1.0) < 1e-15
    for cx, cy in ((0, 0), (24, 0), (24, 16), (0, 16)):                             # centred on every corner of the map
        assert abs(go.visible_fraction(shift(diamond, cx, cy), 24, 16) - 0.25) < 1e-15
    quad = [(3, 2), (9, 4), (8, 9), (2, 6)]
    assert go.visible_fraction(quad, 24, 16) == 1.0 and go.visible_fraction(quad[::-1], 24, 16) == 1.0
    assert go.clip_area(quad, 24, 16) == abs(go.shoelace(quad)) == 29.5
    assert go.visible_fraction(shift(quad, 30, 0), 24, 16) == 0.0 and go.visible_fraction(shift(quad, 0, -20), 24, 16) == 0.0
    assert go.visible_fraction([(1, 1), (2, 2), (3, 3), (4, 4)], 24, 16) == 0.0     # no area
    # a box larger than the map: the map's share of it
    assert go.visible_fraction([(-12, -8), (36, -8), (36, 24), (-12, 24)], 24, 16) == (24 * 16) / (48 * 32)


def test_the_oracles_warp_gives_the_known_pictures():
    """What the GPU tests demand of the kernel, asked of the restatement first."""
    from datasets.augment import fliplr_matrix
    from datasets.geometric_view import similarity_matrices
    rng = np.random.default_rng(5)
    x = rng.uniform(-3, 3, (1, 2, 6, 6)).astype(F)
    same = lambda a, b: a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes()
    assert same(go.warp(x, np.eye(3)[None]), x)
    assert same(go.warp(x, similarity_matrices(6, 6, 180)[1][None]), x[..., ::-1, ::-1])
    assert same(go.warp(x, similarity_matrices(6, 6, 90)[1][None]), np.rot90(x, -1, axes=(2, 3)))      # clockwise
    assert same(go.warp(x, similarity_matrices(6, 6, -90)[1][None]), np.rot90(x, 1, axes=(2, 3)))
    assert same(go.warp(x, fliplr_matrix(6)[None]), x[..., ::-1])
    y = go.warp(x, similarity_matrices(6, 6, 0, 1, (2 / 6, -1 / 6))[1][None], fill=7.5)                  # right 2, up 1
    assert same(y[..., :5, 2:], x[..., 1:, :4]) and (y[..., 5, :] == 7.5).all() and (y[..., :, :2] == 7.5).all()
    # halfway between four pixels: their mean, in the documented order
    half = np.float64([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]])
    y = go.warp(x, half[None])
    top = x[0, 0, 0, 0] + F(0.5) * (x[0, 0, 0, 1] - x[0, 0, 0, 0])
    bot = x[0, 0, 1, 0] + F(0.5) * (x[0, 0, 1, 1] - x[0, 0, 1, 0])
    assert y[0, 0, 0, 0] == top + F(0.5) * (bot - top)
    # the centroid of a bright patch follows the forward matrix
    img = np.zeros((1, 1, 32, 32), F)
    img[0, 0, 9:12, 19:22] = 1
    fwd, inv = similarity_matrices(32, 32, 33, 0.8, (0.05, -0.1))
    cx, cy = go.centroid(go.warp(img, inv[None])[0, 0])
    want = fwd @ [20.5, 10.5, 1.0]
    assert abs(cx - want[0]) < 0.5 and abs(cy - want[1]) < 0.5


def test_the_oracles_label_transform_on_hand_worked_rows():
    labels = {'boxes': np.float64([[[2, 2, 6, 4], [20, 2, 23, 5], [1, 1, 1.5, 6], [0, 0, 0, 0]]]),
              'classes': np.int32([[2, 0, 1, 0]]), 'counts': np.int32([3])}
    shift = np.float64([[1, 0, 3, 0, 1, 0]])                          # three cells to the right
    out, judged = go.transform_labels(labels, shift, 16, 24, min_size=1.0, min_visible=0.5)
    # row 0 moves; row 1 is [23, 26] x [2, 5]: one third visible; row 2 is half a cell wide
    assert out['counts'].tolist() == [1] and out['classes'].tolist() == [[2, 0, 0, 0]]
    assert out['boxes'][0].tolist() == [[5, 2, 9, 4], [0] * 4, [0] * 4, [0] * 4]
    assert out['kept'] == F(1) and out['dropped'] == F(2) and out['kept'].dtype == out['dropped'].dtype == F
    assert [round(v[0], 12) for v in judged] == [1.0, round(1 / 3, 12), 1.0]
    ident, judged = go.transform_labels(labels, np.float64([[1, 0, 0, 0, 1, 0]]), 16, 24, min_size=1.0)
    assert ident['counts'].tolist() == [3] and np.array_equal(ident['boxes'], labels['boxes']) and judged == []
    # a quarter turn about the centre of a 16 x 24 map swaps a box's sides; rotated labels keep their corner order
    quarter = np.float64([[0, -1, 20, 1, 0, -4]])
    out, _ = go.transform_labels(labels, quarter, 16, 24, min_size=0.0, min_visible=0.01)
    assert out['boxes'][0, 0].tolist() == [16, -2, 18, 2]
    corners = {'corners': np.float64([[[[2, 2], [6, 2], [6, 4], [2, 4]]]]), 'classes': np.int32([[1]]),
               'counts': np.int32([1])}
    out, judged = go.transform_labels(corners, quarter, 16, 24, rotated=True, min_visible=0.4)
    assert out['corners'][0, 0].tolist() == [[18, -2], [18, 2], [16, 2], [16, -2]] and judged == [(0.5, 4.0, 2.0)]
