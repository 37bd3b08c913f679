"""The strong view without a GPU: the sampler (datasets/strong_view.py), every refusal, the two C entry points' argument
checks, how the driver resolves `uda.WeakStrongTeacher`, and the numpy oracle of tests/strong_view_oracle.py pinned by two
hand-worked pictures."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import strong_view_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'centernet-uda_amd', 'configs')
OVERRIDE = 'model.uda={WeakStrongTeacher: {pseudo_weight: 1.0, score_threshold: 0.4, burn_in_steps: 2000}}'
F = np.float32
OFF = {'color_jitter': None, 'grayscale': None, 'blur': None, 'erase': None}
FIELDS = ('photo', 'taps', 'radius', 'rects', 'ids', 'sigma')


def _same(a, b):
    return a.seed == b.seed and all(np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) for k in FIELDS)


# -- the sampler --------------------------------------------------------------------------------------------------------
def test_sampling_is_a_function_of_its_arguments_alone():
    from datasets.strong_view import StrongView
    view = StrongView()
    a = view.sample(6, 48, 64, np.random.default_rng([42, 0x57534B, 3]), first_id=18)
    b = StrongView(None).sample(6, 48, 64, np.random.default_rng([42, 0x57534B, 3]), first_id=18)
    assert _same(a, b) and a.ids.tolist() == list(range(18, 24)) and a.ids.dtype == np.int64
    assert (a.photo.dtype, a.taps.dtype, a.radius.dtype, a.rects.dtype) == (F, F, np.int32, np.int32)
    assert a.photo.shape == (6, 4) and a.taps.shape == (6, 13) and a.radius.shape == (6,) and a.rects.shape == (6, 3, 4)
    assert 0 <= a.seed < 2 ** 64
    for other in (view.sample(6, 48, 64, np.random.default_rng([42, 0x57534B, 4]), first_id=18),
                  view.sample(6, 48, 65, np.random.default_rng([42, 0x57534B, 3]), first_id=18),
                  view.sample(6, 48, 64, np.random.default_rng([42, 0x57534B, 3]), first_id=19),
                  StrongView({'blur': {'sigma': [0.5, 0.6]}}).sample(6, 48, 64, np.random.default_rng([42, 0x57534B, 3]),
                                                                    first_id=18)):
        assert not _same(a, other)
    # a given mapping is merged over the defaults key by key
    merged = StrongView({'blur': {'sigma': [0.5, 0.6]}, 'erase': [{'p': 1.0}]})
    assert merged.blur == {'p': 0.5, 'sigma': (0.5, 0.6)} and merged.grayscale == {'p': 0.2}
    assert merged.erase == [{'p': 1.0, 'scale': (0.05, 0.2), 'ratio': (0.3, 3.3)}]
    assert merged.color_jitter == {'p': 0.8, 'brightness': (0.6, 1.4), 'contrast': (0.6, 1.4), 'saturation': (0.6, 1.4)}
    assert len(view.erase) == 3 and view.erase[2] == {'p': 0.3, 'scale': (0.02, 0.2), 'ratio': (0.05, 8.0)}


def _draw(config, B=64, H=64, W=64, seed=5):
    from datasets.strong_view import StrongView
    return StrongView(config).sample(B, H, W, np.random.default_rng(seed))


def test_probability_zero_is_never_and_one_is_always():
    never = _draw({'color_jitter': {'p': 0}, 'grayscale': {'p': 0}, 'blur': {'p': 0},
                   'erase': [{'p': 0}, {'p': 0}, {'p': 0}]})
    assert never.neutral.all() and not never.erased.any() and np.isnan(never.sigma).all()
    always = _draw({'color_jitter': {'p': 1}, 'grayscale': {'p': 1}, 'blur': {'p': 1},
                    'erase': [{'p': 1}, {'p': 1, 'scale': [0.05, 0.2], 'ratio': [0.3, 3.3]},
                              {'p': 1, 'scale': [0.05, 0.2], 'ratio': [0.3, 3.3]}]})
    assert (always.photo[:, :3] != 1).all() and (always.photo[:, 3] == 1).all() and (always.radius >= 1).all()
    r = always.rects
    assert ((r[:, :, 2] > r[:, :, 0]) & (r[:, :, 3] > r[:, :, 1])).all()          # 64 x 64: every draw fits
    for key in OFF:                                                                # one operation alone
        one = _draw({**OFF, key: {'p': 1} if key != 'erase' else [{'p': 1}]})
        assert (one.photo[:, :3] != 1).all() == (key == 'color_jitter')
        assert (one.photo[:, 3] == 1).all() == (key == 'grayscale') and (one.radius > 0).all() == (key == 'blur')
        assert one.erased.all() == (key == 'erase')
    off = _draw(OFF)
    assert off.neutral.all() and not off.erased.any()


def test_factors_sigmas_and_taps():
    from datasets.strong_view import gaussian_taps
    p = _draw({'color_jitter': {'p': 1, 'brightness': 0.4, 'contrast': 0.2, 'saturation': 0.1}, 'blur': {'p': 1}}, B=200)
    for c, a in enumerate((0.4, 0.2, 0.1)):
        assert (p.photo[:, c] >= F(1 - a)).all() and (p.photo[:, c] <= F(1 + a)).all() and p.photo[:, c].std() > 0.2 * a
    assert (p.sigma >= 0.1).all() and (p.sigma <= 2.0).all()
    assert set(p.radius.tolist()) == {1, 2, 3, 4, 5, 6}
    for b in range(200):
        R = int(p.radius[b])
        assert R == min(6, math.ceil(3 * p.sigma[b]))
        w = p.taps[b]
        assert abs(float(w[:2 * R + 1].astype(np.float64).sum()) - 1.0) < 1e-6 and (w[2 * R + 1:] == 0).all()
        assert np.array_equal(w[:2 * R + 1], w[:2 * R + 1][::-1]) and (w[:2 * R + 1] > 0).all()
        k = np.arange(-R, R + 1, dtype=np.float64)
        e = np.exp(-k * k / (2 * p.sigma[b] ** 2))
        assert np.array_equal(w[:2 * R + 1], (e / e.sum()).astype(F))
    assert gaussian_taps(0.1)[0] == 1 and gaussian_taps(2.0)[0] == 6 and gaussian_taps(5.0)[0] == 6    # capped


def test_rectangles_lie_inside_the_image_with_area_and_ratio_in_their_intervals():
    """h = round(sqrt(area r)) and w = round(sqrt(area / r)) are each within a half of their exact values, so the exact
    area lies in [(h - .5)(w - .5), (h + .5)(w + .5)] and the exact ratio h / w in [(h - .5) / (w + .5), (h + .5) / (w - .5)]:
    both ranges must meet the configured intervals."""
    H, W = 48, 80
    entries = [{'p': 1, 'scale': [0.05, 0.2], 'ratio': [0.3, 3.3]}, {'p': 1, 'scale': [0.02, 0.2], 'ratio': [0.1, 6.0]},
               {'p': 1, 'scale': [0.1, 0.1], 'ratio': [2.0, 2.0]}]
    p = _draw({**OFF, 'erase': entries}, B=300, H=H, W=W)
    seen = 0
    for b in range(300):
        for i, e in enumerate(entries):
            x0, y0, x1, y1 = (int(t) for t in p.rects[b, i])
            w, h = x1 - x0, y1 - y0
            if (x0, y0, x1, y1) == (0, 0, 0, 0):
                continue
            seen += 1
            assert 0 <= x0 and x1 <= W and 0 <= y0 and y1 <= H and 0 <= h < H and 0 <= w < W
            lo, hi = max(h - .5, 0) * max(w - .5, 0), (h + .5) * (w + .5)
            assert lo <= e['scale'][1] * H * W and hi >= e['scale'][0] * H * W, (h, w, e)
            assert max(h - .5, 0) / (w + .5) <= e['ratio'][1] and (h + .5) >= e['ratio'][0] * max(w - .5, 0), (h, w, e)
    assert seen > 800
    fixed = p.rects[:, 2]
    assert {(int(r[2] - r[0]), int(r[3] - r[1])) for r in fixed if r.any()} <= {(14, 28)}    # sqrt(384 / 2), sqrt(384 * 2)
    assert len({tuple(r) for r in p.rects[:, 0].tolist()}) > 250                              # positions vary


def test_tiny_and_flat_images_end_the_ten_try_loop():
    cfg = {**OFF, 'erase': [{'p': 1}, {'p': 1}, {'p': 1}]}
    one = _draw(cfg, B=50, H=1, W=1)
    assert not one.erased.any()                        # h < 1 and w < 1 leave only empty rectangles
    flat = _draw(cfg, B=50, H=2, W=300)
    r = flat.rects
    assert ((r[:, :, 3] - r[:, :, 1]) < 2).all() and (r[:, :, 2] <= 300).all() and (r >= 0).all()


def test_identity_is_neutral():
    from datasets.strong_view import StrongViewParams
    p = StrongViewParams.identity(3)
    assert p.batch == 3 and p.neutral.all() and not p.erased.any() and p.ids.tolist() == [0, 1, 2] and p.seed == 0
    assert p.photo.tolist() == [[1, 1, 1, 0]] * 3 and (p.radius == 0).all() and (p.rects == 0).all()
    x = np.random.default_rng(0).normal(size=(3, 3, 4, 5)).astype(F)
    y = so.strong_view(x, F([.4, .45, .47]), F([.29, .27, .28]), p.photo, p.taps, p.radius, p.rects, p.ids, p.seed)
    assert y.tobytes() == x.tobytes()


# -- refusals -----------------------------------------------------------------------------------------------------------
def test_config_refusals_name_the_offender():
    from datasets.strong_view import StrongView
    for bad, name in (({'hue': {'p': 1}}, 'strong_view.hue'), ({'blur': {'kernel': 3}}, 'blur.kernel'),
                      ({'grayscale': {'p': 1.5}}, 'grayscale.p'), ({'color_jitter': {'p': -0.1}}, 'color_jitter.p'),
                      ({'blur': {'sigma': [2.0, 0.1]}}, 'blur.sigma'), ({'blur': {'sigma': [0.0, 1.0]}}, 'blur.sigma'),
                      ({'blur': {'sigma': -1.0}}, 'blur.sigma'), ({'color_jitter': {'contrast': -0.5}}, 'color_jitter.contrast'),
                      ({'erase': [{'scale': [0.3, 0.1]}]}, r'erase\[0\].scale'),
                      ({'erase': [{}, {'ratio': [3.0, 0.5]}]}, r'erase\[1\].ratio'),
                      ({'erase': [{}, {}, {'p': 2}]}, r'erase\[2\].p'), ({'erase': [{'value': 0}]}, r'erase\[0\].value'),
                      ({'erase': [{}] * 4}, 'erase lists 4')):
        with pytest.raises(ValueError, match=name):
            StrongView(bad)
    StrongView({'erase': []}), StrongView({'blur': {'sigma': 1.0}}), StrongView(OFF)


def test_strong_view_refusals_name_the_argument():
    import torch
    from datasets.strong_view import StrongViewParams, strong_view
    mean, std = (.4, .45, .47), (.29, .27, .28)
    ok, p = torch.zeros(2, 3, 4, 5), StrongViewParams.identity(2)
    for x, params, what in ((torch.zeros(2, 3, 5, 4).transpose(2, 3), p, 'x must be contiguous'),
                            (torch.zeros(2, 4, 4, 5), p, r'x must be a non-empty float32 \[B, 3, H, W\]'),
                            (torch.zeros(3, 4, 5), p, r'x must be a non-empty float32 \[B, 3, H, W\]'),
                            (torch.zeros(2, 3, 4, 5, dtype=torch.float64), p, 'x must be a non-empty float32'),
                            (torch.zeros(2, 3, 4, 5, requires_grad=True), p, 'x requires grad'),
                            (ok, StrongViewParams.identity(3), 'params describe 3 images, the batch x has 2'),
                            (ok, {'photo': 1}, 'params must be a StrongViewParams'),
                            (ok, p, 'x is a cpu tensor')):
        with pytest.raises(RuntimeError, match=what):
            strong_view(x, params, mean, std)
    wide = StrongViewParams.identity(2)
    wide.radius[1] = 7
    with pytest.raises(RuntimeError, match='params.radius'):
        strong_view(ok, wide, mean, std)
    with pytest.raises(RuntimeError, match='mean must have three'):
        strong_view(ok, p, (.4, .5), std)
    with pytest.raises(RuntimeError, match='std=.*zero'):
        strong_view(ok, p, mean, (.2, 0., .2))


# -- the library ----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_refuse_bad_arguments_without_a_device():
    import hip_runtime as hr
    raw = ctypes.CDLL(hr.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    for name in ('cnuda_strong_view', 'cnuda_strong_view_pivot'):
        assert hasattr(raw, name) and hasattr(hr._Sig, name) and ('int %s(' % name) in header
    L = hr.lib()
    assert L.cnuda_abi_version() == 2
    err = lambda: L.cnuda_last_error().decode()
    a, b = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)       # never dereferenced: refused first
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)
    assert L.cnuda_strong_view_pivot(None, None, None, None, None, 1, 4, 4, None) == -1
    assert 'cnuda_strong_view_pivot: null pointer' in err()
    for geom in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert L.cnuda_strong_view_pivot(pa, pa, pa, pa, pa, *geom, None) == -1
        assert 'cnuda_strong_view_pivot: bad sizes' in err()
    tables = [pa] * 5
    assert L.cnuda_strong_view(None, None, *tables[:5], 0, None, None, 0, None, 1, 4, 4, None) == -1
    assert 'cnuda_strong_view: null pointer' in err()
    for geom in ((0, 1, 1), (1, 0, 1), (1, 1, -3)):
        assert L.cnuda_strong_view(pa, pb, *tables, 0, pa, pa, 0, pa, *geom, None) == -1
        assert 'cnuda_strong_view: bad sizes' in err()
    for radius in (-1, 7):
        assert L.cnuda_strong_view(pa, pb, *tables, radius, pa, pa, 0, pa, 1, 1, 1, None) == -1
        assert 'cnuda_strong_view: radius' in err()
    assert L.cnuda_strong_view(pa, pa, *tables, 0, pa, pa, 0, pa, 1, 1, 1, None) == -1
    assert 'cnuda_strong_view: x and y overlap' in err()
    assert L.cnuda_strong_view(pa, pa + 8, *tables, 0, pa, pa, 0, pa, 1, 1, 1, None) == -1 and 'overlap' in err()


# -- the driver's view ----------------------------------------------------------------------------------------------------
def test_the_driver_resolves_weak_strong_teacher_from_the_readme_override():
    import train
    import uda
    from utils.config import load_config
    cls = train.resolve_plugin('WeakStrongTeacher')
    assert cls is uda.WeakStrongTeacher and issubclass(cls, uda.MeanTeacher)
    assert 'WeakStrongTeacher' in dir(uda) and 'WeakStrongTeacher' in uda.__all__
    cfg = load_config(CONFIGS, ['experiment=dla_baseline', OVERRIDE,
                                'datasets.training.params.target_domain_glob=[/data/target/images/*.jpg]'])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is cls and args == {'pseudo_weight': 1.0, 'score_threshold': 0.4, 'burn_in_steps': 2000}
    plugin = got(**args)
    assert (plugin.pseudo_weight, plugin.decay, plugin.score_threshold, plugin.burn_in_steps, plugin.mirror_student,
            plugin.min_size, plugin.evaluate_teacher) == (1.0, 0.999, 0.4, 2000, True, 2.0, False)
    assert plugin.strong_view.blur == {'p': 0.5, 'sigma': (0.1, 2.0)} and len(plugin.strong_view.erase) == 3
    plugin.cfg = cfg
    plugin.init_done()
    assert [float(v) for v in cfg.normalize.mean] == [0.40789654, 0.44719302, 0.47026115] and int(cfg.seed) == 42
    assert OVERRIDE in open(os.path.join(ROOT, 'README.md')).read()
    # the sampler's mapping through the config, a null included; the parent's refusals are the subclass's
    cfg = load_config(CONFIGS, ['experiment=dla_baseline',
                                'model.uda={WeakStrongTeacher: {pseudo_weight: 0.5, strong_view: {grayscale: null, '
                                'blur: {p: 1.0}}, decay: 0.99}}'])
    got, args = train.plugin_from_config(cfg.model.uda)
    plugin = got(**args)
    assert plugin.strong_view.grayscale is None and plugin.strong_view.blur['p'] == 1.0 and plugin.decay == 0.99
    with pytest.raises(ValueError, match='decay'):
        uda.WeakStrongTeacher(1.0, decay=1.0)
    with pytest.raises(ValueError, match='strong_view.hue'):
        uda.WeakStrongTeacher(1.0, strong_view={'hue': 0.1})


def test_signatures():
    import uda
    params = inspect.signature(uda.MeanTeacher.__init__).parameters
    assert list(params)[1:] == ['pseudo_weight', 'decay', 'score_threshold', 'burn_in_steps', 'mirror_student', 'min_size',
                                'evaluate_teacher']
    assert [params[k].default for k in list(params)[2:]] == [0.999, 0.4, 0, True, 2.0, False]
    params = inspect.signature(uda.WeakStrongTeacher.__init__).parameters
    assert list(params)[1:] == ['pseudo_weight', 'strong_view', 'mean_teacher_arguments']
    assert params['strong_view'].default is None and params['mean_teacher_arguments'].kind is inspect.Parameter.VAR_KEYWORD
    assert uda.WeakStrongTeacher.step is uda.MeanTeacher.step          # only the student's view differs
    assert uda.WeakStrongTeacher.student_view is not uda.MeanTeacher.student_view


# -- the oracle, by hand ----------------------------------------------------------------------------------------------
def test_oracle_brightness_contrast_gray_by_hand():
    """mean 0, std 1, so v = clamp(x).  3 x 3 pixels: pure red, green, blue; grays 1.5 (clamped to 1), 1, 0.5; grays 0.5,
    0.5, -0.5 (clamped to 0).
    Pivot: the quantised lumas of red, green and blue are rint(0.299f 65536) = 19595, rint(0.587f 65536) = 38470 and
    rint(0.114f 65536) = 7471, together 65536; a gray v gives 65536 v.  Sum = 65536 (1 + 1 + 1 + 0.5 + 0.5 + 0.5 + 0.5 + 0)
    = 65536 x 4.5 over 65536 x 9: pivot 0.5.
    Brightness 0.75, then contrast 2 about 0.5, then gray:
      red (1, 0, 0) -> (0.75, 0, 0) -> (1, 0, 0) [0.25 x 2 + 0.5; -0.5 x 2 + 0.5 = -0.5 -> 0] -> luma 0.299f; green and
      blue likewise -> 0.587f, 0.114f;  gray 1 -> 0.75 -> 1 -> 1;  gray 0.5 -> 0.375 -> 0.25 -> 0.25;  gray 0 -> 0."""
    x = np.zeros((1, 3, 3, 3), dtype=F)
    x[0, 0, 0, 0] = x[0, 1, 0, 1] = x[0, 2, 0, 2] = 1
    x[0, :, 1] = F([1.5, 1, 0.5])
    x[0, :, 2] = F([0.5, 0.5, -0.5])
    mean, std = F([0, 0, 0]), F([1, 1, 1])
    q = np.rint(so.luma(so.denormalise(x[0], mean, std)) * F(65536))
    assert q.tolist() == [[19595, 38470, 7471], [65536, 65536, 32768], [32768, 32768, 0]]
    assert so.pivot(x, mean, std).tolist() == [0.5]
    taps = np.zeros((1, 13), dtype=F)
    y = so.strong_view(x, mean, std, F([[0.75, 2.0, 1.0, 1.0]]), taps, np.int32([0]), np.zeros((1, 3, 4), np.int32),
                       np.int64([0]), 0)
    want = F([[0.299, 0.587, 0.114], [1, 1, 0.25], [0.25, 0.25, 0]])
    assert y.dtype == F and y.shape == x.shape
    for c in range(3):
        assert y[0, c].tolist() == want.tolist(), c
    # contrast alone about a GIVEN pivot, gray off: (v - 0.25) x 2 + 0.25 on the middle row's channels
    y = so.strong_view(x, mean, std, F([[1.0, 2.0, 1.0, 0.0]]), taps, np.int32([0]), np.zeros((1, 3, 4), np.int32),
                       np.int64([0]), 0, pivots=F([0.25]))
    assert y[0, :, 1].tolist() == [[1, 1, 0.75]] * 3 and y[0, :, 0, 0].tolist() == [1, 0, 0]


def test_oracle_blur_with_replicated_edges_by_hand():
    """One row of five, taps (0.25, 0.5, 0.25), radius 1.  Channel 0 = (0, 1, 0, 0.5, 1) padded to (0 | 0, 1, 0, 0.5, 1 | 1):
    0.25 a + 0.5 b + 0.25 c over every window = (0.25, 0.5, 0.375, 0.5, 0.875).  Channel 1 is constant 1 and stays 1.
    Channel 2 = (0, 0, 0, 0, 1) padded with its edge 1: (0, 0, 0, 0.25, 0.75).  The vertical pass sees three copies of the one
    row: 0.25 v + 0.5 v + 0.25 v = v exactly for these values.  mean 0, std 1."""
    x = F([[[[0, 1, 0, 0.5, 1]], [[1, 1, 1, 1, 1]], [[0, 0, 0, 0, 1]]]])
    taps = np.zeros((1, 13), dtype=F)
    taps[0, :3] = [0.25, 0.5, 0.25]
    y = so.strong_view(x, F([0, 0, 0]), F([1, 1, 1]), F([[1, 1, 1, 0]]), taps, np.int32([1]),
                       np.zeros((1, 3, 4), np.int32), np.int64([0]), 0)
    assert y[0, :, 0].tolist() == [[0.25, 0.5, 0.375, 0.5, 0.875], [1, 1, 1, 1, 1], [0, 0, 0, 0.25, 0.75]]
    # a column of five through the same taps: the vertical pass replicates the top and the bottom row
    yt = so.strong_view(np.ascontiguousarray(x.transpose(0, 1, 3, 2)), F([0, 0, 0]), F([1, 1, 1]), F([[1, 1, 1, 0]]), taps,
                        np.int32([1]), np.zeros((1, 3, 4), np.int32), np.int64([0]), 0)
    assert yt[0, :, :, 0].tolist() == y[0, :, 0].tolist()


def test_oracle_fill_is_philox_by_the_published_vector_and_depends_on_seed_id_and_pixel_alone():
    """Philox4x32-10's known-answer test (Random123 kat_vectors): counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8."""
    z = np.zeros(1, dtype=np.uint64)
    got = [int(w[0]) for w in so.philox4x32_10((z, z, z, z), (0, 0))]
    assert got == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    got = [int(w[0]) for w in so.philox4x32_10((ones, ones, ones, ones), (0xFFFFFFFF, 0xFFFFFFFF))]
    assert got == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    a = so.fill(4, 6, 7, 3)
    assert a.shape == (3, 4, 6) and a.dtype == F and np.abs(a).max() < 1.7320508 and len(np.unique(a)) == 72
    assert np.array_equal(so.fill(2, 6, 7, 3), a[:, :2])            # pixel index y W + x: the first rows of a taller image
    assert not np.array_equal(so.fill(4, 6, 8, 3), a) and not np.array_equal(so.fill(4, 6, 7, 4), a)
    # word 0 of pixel 0 under (seed 0, id 0) is the vector above: u = ((0x6627e8d5 >> 9) + 0.5) / 2^23
    u = F(F((0x6627e8d5 >> 9)) + F(0.5)) * F(1 / 8388608)
    assert so.fill(1, 1, 0, 0)[0, 0, 0] == F(F(u * F(2) - F(1)) * F(1.7320508))
    # rectangles: half-open, empty ones ignored, overlap needs no order
    mask = so.rect_mask(np.int32([[1, 0, 3, 2], [2, 1, 2, 4], [2, 1, 6, 3]]), 4, 6)
    assert mask.astype(int).tolist() == [[0, 1, 1, 0, 0, 0], [0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]]
