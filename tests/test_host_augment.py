"""No GPU: the numpy oracle of the augmentation kernels is pinned by answers that do not come from it (exact
identities, PIL's bilinear resize and affine transform, colorsys), and datasets.augment's host side -- matrix
composition, motion-blur taps, the configured draws -- is checked against the definitions of DESIGN.md."""
import colorsys
import json
import math
import os

import numpy as np
import pytest
from PIL import Image

import augment_oracle as ao

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
IDENT = [1, 0, 0, 0, 1, 0]


def _default_list():
    with open(os.path.join(GOLDEN, 'augmentation_defaults.json')) as fh:
        return json.load(fh)


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's pins: warp
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_and_flip_are_exact():
    src = _img(13, 17, 0)
    assert np.array_equal(ao.warp(src, IDENT, 13, 17), src)
    assert np.array_equal(ao.warp(src, [-1, 0, 17, 0, 1, 0], 13, 17), src[:, ::-1])
    assert np.array_equal(ao.warp(src, [1, 0, 0, 0, -1, 13], 13, 17), src[::-1])


def test_two_to_one_reduction_is_the_rounded_box_mean():
    src = _img(12, 16, 1)
    mean = src.reshape(6, 2, 8, 2, 3).astype(np.float32).mean((1, 3))
    assert np.array_equal(ao.warp(src, [2, 0, 0, 0, 2, 0], 6, 8), np.rint(mean).astype(np.uint8))


@pytest.mark.parametrize('out', [(26, 34), (40, 29), (39, 51)])
def test_enlarging_is_within_one_level_of_pil_bilinear(out):
    src = _img(13, 17, 0)
    ho, wo = out
    got = ao.warp(src, [17 / wo, 0, 0, 0, 13 / ho, 0], ho, wo)
    want = np.asarray(Image.fromarray(src).resize((wo, ho), Image.BILINEAR))
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1          # PIL works in fixed point


def test_rotation_is_within_one_level_of_pil_affine_in_the_interior():
    src = _img(40, 48, 2)
    t, sc = math.radians(20), 1 / 1.15
    a = [sc * math.cos(t), -sc * math.sin(t), 5.3, sc * math.sin(t), sc * math.cos(t), -2.1]
    got = ao.warp(src, a, 40, 48)
    want = np.asarray(Image.fromarray(src).transform((48, 40), Image.AFFINE, a, resample=Image.BILINEAR))
    j, i = np.meshgrid(np.arange(48) + .5, np.arange(40) + .5)
    u, v = a[0] * j + a[1] * i + a[2], a[3] * j + a[4] * i + a[5]
    interior = (u >= 1.5) & (u <= 48 - 1.5) & (v >= 1.5) & (v <= 40 - 1.5)
    assert interior.sum() > 500
    assert np.abs(got.astype(int) - want.astype(int))[interior].max() <= 1
    # and outside pixels occur and are zero
    outside = (u < 0) | (u > 48) | (v < 0) | (v > 40)
    assert outside.any() and not got[outside].any()


def test_three_horizontal_taps_are_the_three_pixel_mean():
    src = _img(13, 17, 0)
    got = ao.warp(src, IDENT, 13, 17, taps=[(-1, 0, 1 / 3), (0, 0, 1 / 3), (1, 0, 1 / 3)])
    s = src.astype(np.float32)
    want = np.rint((s[:, :-2] + s[:, 1:-1] + s[:, 2:]) / 3)
    assert np.array_equal(got[:, 1:-1], want.astype(np.uint8))


def test_valid_size_inside_a_padded_buffer():
    src = _img(13, 20, 3)
    got = ao.warp(src, [20 / 11, 0, 0, 0, 9 / 9, 0], 9, 11, size=(9, 20))
    assert np.array_equal(got, ao.warp(src[:9], [20 / 11, 0, 0, 0, 1, 0], 9, 11))
    # nothing beyond the valid 9 x 17 corner is read: edge replication stops at the valid size
    a, b = src.copy(), src.copy()
    b[9:], b[:, 17:] = 0, 255
    inv = [17 / 11, 0, 0, 0, 1, 0]
    assert np.array_equal(ao.warp(a, inv, 9, 11, size=(9, 17)), ao.warp(b, inv, 9, 11, size=(9, 17)))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's pins: colour
# ---------------------------------------------------------------------------------------------------------------------
def test_neutral_colour_is_exact_and_120_degrees_rolls_the_channels():
    img = _img(64, 64, 1)
    assert np.array_equal(ao.color(img, 0, 0, 0), img)
    assert np.array_equal(ao.color(img, 0, 120, 0), img[..., [2, 0, 1]])
    assert np.array_equal(ao.color(img, 0, 360, 0), img)


def test_grey_levels_survive_any_hue_shift():
    grey = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1).reshape(16, 16, 3)
    for hue in (77, -101, 180, 37.5):
        assert np.array_equal(ao.color(grey, 0, hue, 0), grey)


@pytest.mark.parametrize('hue,add', [(37.5, 0), (-101, 40), (180, -60), (0, 100)])
def test_colour_is_within_one_level_of_colorsys(hue, add):
    img = _img(32, 32, 1)
    want = np.zeros_like(img)
    for i in range(32):
        for j in range(32):
            h, s, v = colorsys.rgb_to_hsv(*(img[i, j] / 255.))
            v = min(max(v + add / 255., 0), 1)
            want[i, j] = np.rint(np.array(colorsys.hsv_to_rgb((h + hue / 360.) % 1.0, s, v)) * 255)
    assert np.abs(ao.color(img, 0, hue, add).astype(int) - want.astype(int)).max() <= 1


def test_full_grayscale_is_the_rounded_luma_on_every_channel():
    img = _img(16, 16, 4)
    x = img.astype(np.float64)
    luma = 0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]
    got = ao.color(img, 1, 0, 0)
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    near_half = np.abs(luma - np.floor(luma) - 0.5) < 1e-3          # float32 may round these the other way
    assert np.array_equal(got[..., 0][~near_half], np.rint(luma).astype(np.uint8)[~near_half])


# ---------------------------------------------------------------------------------------------------------------------
# matrix composition
# ---------------------------------------------------------------------------------------------------------------------
def _full(six):
    return np.vstack([np.asarray(six, dtype=np.float64).reshape(2, 3), [0, 0, 1]])


def test_forward_times_inverse_is_the_identity():
    from datasets.augment import Augmentation
    sizes = np.array([[480, 640], [333, 517], [64, 48]] * 20)
    p = Augmentation(_default_list()).sample(sizes, (512, 384), np.random.default_rng(5))
    assert p.forward.dtype == np.float64 and p.inverse.dtype == np.float32 and p.inverse.shape == (60, 6)
    from datasets.augment import AugmentParams
    mats = np.stack([_full(m) for m in p.forward])
    inv64 = np.linalg.inv(mats)
    for b in range(60):
        assert np.abs(mats[b] @ inv64[b] - np.eye(3)).max() <= 1e-12
        assert np.array_equal(p.inverse[b], inv64[b][:2].reshape(6).astype(np.float32))
    q = AugmentParams.from_matrices(sizes, (512, 384), mats)
    assert np.array_equal(q.forward, p.forward) and np.array_equal(q.inverse, p.inverse)


def test_the_centre_maps_to_the_centre_without_translation():
    from datasets.augment import Augmentation
    aug = Augmentation([{'Affine': {'scale': [0.5, 2.0], 'rotate': [-180, 180]}}, {'Fliplr': {'p': 0.5}},
                        {'Flipud': {'p': 0.5}}])
    sizes = np.array([[480, 640], [37, 91]] * 10)
    p = aug.sample(sizes, (512, 256), np.random.default_rng(2))
    for b in range(20):
        h, w = sizes[b]
        got = _full(p.forward[b]) @ [w / 2, h / 2, 1]
        assert np.abs(got[:2] - [256, 128]).max() <= 1e-9


def test_affine_conventions():
    from datasets.augment import affine_matrix
    h, w = 40, 60
    # positive rotation is clockwise on the y-down image: the point right of the centre goes DOWN
    m = affine_matrix(h, w, rotate=90)
    assert np.allclose(m @ [w / 2 + 10, h / 2, 1], [w / 2, h / 2 + 10, 1], atol=1e-12)
    m = affine_matrix(h, w, scale=(2, 3))
    assert np.allclose(m @ [w / 2 + 1, h / 2 + 1, 1], [w / 2 + 2, h / 2 + 3, 1], atol=1e-12)
    m = affine_matrix(h, w, translate_percent=(0.1, -0.25))
    assert np.allclose(m @ [0, 0, 1], [6, -10, 1], atol=1e-12)


def test_a_quarter_crop_on_both_sides_doubles_horizontal_distances():
    from datasets.augment import crop_matrix
    m = crop_matrix(40, 60, 0.0, 0.25, 0.0, 0.25)
    a, b = m @ [20, 7, 1], m @ [31, 9, 1]
    assert np.allclose(b - a, [22, 2, 0], atol=1e-12)
    assert np.allclose(m @ [15, 0, 1], [0, 0, 1], atol=1e-12) and np.allclose(m @ [45, 40, 1], [60, 40, 1], atol=1e-12)
    with pytest.raises(ValueError, match='leave nothing'):
        crop_matrix(40, 60, 0.5, 0, 0.5, 0)


def test_flip_and_resize_commute():
    from datasets.augment import fliplr_matrix, flipud_matrix, resize_matrix
    h, w, size = 37, 91, (512, 384)
    r = resize_matrix(h, w, size)
    assert np.allclose(fliplr_matrix(size[0]) @ r, r @ fliplr_matrix(w), atol=1e-12)
    assert np.allclose(flipud_matrix(size[1]) @ r, r @ flipud_matrix(h), atol=1e-12)
    assert np.allclose(r @ [w, h, 1], [512, 384, 1], atol=1e-12)


def test_motion_blur_taps():
    from datasets.augment import motion_blur_taps
    t = motion_blur_taps(3, 90, 0.0)
    assert np.allclose(t, [[-1, 0, 1 / 3], [0, 0, 1 / 3], [1, 0, 1 / 3]], atol=1e-15)
    t = motion_blur_taps(4, 0, 0.7)
    assert np.allclose(t[:, 0], 0, atol=1e-15) and np.allclose(t[:, 1], [1.5, 0.5, -0.5, -1.5])
    assert np.allclose(t[:, 2], [(1 + 0.7 * r) / 4 for r in (-1, -1 / 3, 1 / 3, 1)])
    for k in range(1, 11):
        assert abs(motion_blur_taps(k, 33, -0.4)[:, 2].sum() - 1) < 1e-12
    assert np.array_equal(motion_blur_taps(1, 12, 0.9), [[0, 0, 1]])
    with pytest.raises(ValueError, match='k must be'):
        motion_blur_taps(11, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
def test_the_default_list_draws_inside_its_intervals():
    from datasets.augment import Augmentation
    n = 2000
    sizes = np.tile([[480, 640]], (n, 1))
    p = Augmentation(_default_list()).sample(sizes, (512, 512), np.random.default_rng(11))
    d = p.draws
    took = p.applied['Sometimes']

    def within(key, lo, hi):
        v = d[key]
        assert v.shape[0] == n
        drawn = ~np.isnan(v).reshape(n, -1)[:, 0]
        assert np.array_equal(drawn, took), key            # drawn exactly when the branch was taken
        assert (v[drawn] >= lo).all() and (v[drawn] <= hi).all(), key
        return v[drawn]

    within('AddToHue.value', -128, 128)
    within('AddToBrightness.add', -100, 100)
    k = within('MotionBlur.k', 3, 10)
    assert np.array_equal(k, np.rint(k)) and set(k) == set(range(3, 11))
    within('MotionBlur.angle', -90, 90)
    direction = within('MotionBlur.direction', -1, 1)
    assert direction.min() < -0.9 and direction.max() > 0.9
    scale = within('Affine.scale', 0.8, 1.3)
    assert np.array_equal(scale[:, 0], scale[:, 1])                     # one draw for both axes
    shift = within('Affine.translate_percent', -0.2, 0.2)
    assert not np.array_equal(shift[:, 0], shift[:, 1])                 # independent per axis
    assert np.isnan(d['Affine.rotate']).sum() == n - took.sum() and not np.nansum(np.abs(d['Affine.rotate']))
    within('Crop.percent', 0.0, 0.3)
    within('AdditiveGaussianNoise.scale', 0, 8)
    # the record holds what was drawn
    assert np.array_equal(p.ntaps, np.where(took, np.nan_to_num(d['MotionBlur.k'], nan=1), 1).astype(np.int32))
    assert np.allclose(p.color[:, 1], np.nan_to_num(d['AddToHue.value']) / 255 * 360, rtol=1e-6)
    assert np.array_equal(p.color[:, 2], np.nan_to_num(d['AddToBrightness.add']).astype(np.float32))
    assert np.array_equal(p.noise, np.nan_to_num(d['AdditiveGaussianNoise.scale']).astype(np.float32))
    assert not p.color[:, 0].any()
    assert np.allclose(p.taps[:, :, 2].sum(1), 1, atol=1e-6)
    # shares: five binomial standard deviations
    for flags, prob in ((took, 0.8), (p.applied['Fliplr'], 0.5), (p.applied['Flipud'], 0.5)):
        assert abs(flags.mean() - prob) <= 5 * math.sqrt(prob * (1 - prob) / n)
    assert 0 <= p.seed < 2 ** 64 and np.array_equal(p.image_ids, np.arange(n))


def test_the_same_seed_gives_the_same_record():
    from datasets.augment import Augmentation
    aug = Augmentation(_default_list())
    sizes = np.array([[480, 640], [100, 37], [333, 517]])
    a = aug.sample(sizes, (512, 512), np.random.default_rng(7))
    b = aug.sample(sizes, (512, 512), np.random.default_rng(7))
    c = aug.sample(sizes, (512, 512), np.random.default_rng(8))
    for name in ('sizes', 'color', 'taps', 'ntaps', 'forward', 'inverse', 'noise', 'image_ids'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.seed == b.seed and a.input_size == b.input_size == (512, 512)
    assert a.seed != c.seed and not np.array_equal(a.forward, c.forward)
    t = a.take([2, 0])
    assert np.array_equal(t.forward, a.forward[[2, 0]]) and np.array_equal(t.image_ids, [2, 0]) and t.seed == a.seed


def test_identity_is_resize_only():
    from datasets.augment import AugmentParams
    p = AugmentParams.identity([[480, 640], [100, 37]], (512, 256))
    assert np.array_equal(p.ntaps, [1, 1]) and np.array_equal(p.taps[:, 0], [[0, 0, 1]] * 2) and not p.taps[:, 1:].any()
    assert not p.noise.any() and not p.color.any()
    assert np.allclose(p.forward, [[512 / 640, 0, 0, 0, 256 / 480, 0], [512 / 37, 0, 0, 0, 256 / 100, 0]], rtol=1e-15)
    assert p.sizes.dtype == np.int32 and p.color.dtype == p.taps.dtype == p.noise.dtype == np.float32
    assert p.forward.dtype == np.float64 and p.inverse.dtype == np.float32 and p.image_ids.dtype == np.int64


def test_scalars_intervals_and_xy_dicts():
    from datasets.augment import Augmentation
    aug = Augmentation([{'Grayscale': {'alpha': 0.3}}, {'AddToHue': {'value': 85}},
                        {'MotionBlur': {'k': 5, 'angle': 90, 'direction': 0.0}},
                        {'Affine': {'scale': {'x': 2.0, 'y': [0.5, 0.6]}, 'translate_percent': {'x': 0.1}, 'rotate': 0}},
                        {'Fliplr': {}}])
    p = aug.sample([[40, 60]] * 4, (60, 40), np.random.default_rng(0))
    assert np.allclose(p.color, [[0.3, 120, 0]] * 4) and np.array_equal(p.ntaps, [5] * 4)
    assert np.allclose(p.taps[0, :5, 0], [-2, -1, 0, 1, 2]) and np.allclose(p.taps[0, :5, 2], 0.2)
    assert p.applied['Fliplr'].all()
    assert np.array_equal(p.draws['Affine.scale'][:, 0], [2.0] * 4)
    assert ((p.draws['Affine.scale'][:, 1] >= 0.5) & (p.draws['Affine.scale'][:, 1] <= 0.6)).all()
    assert np.array_equal(p.draws['Affine.translate_percent'], [[0.1, 0.0]] * 4)
    # x: scaled by 2 about 30, shifted by 6, flipped: u -> 60 - (2 (u - 30) + 30 + 6)
    assert np.allclose(p.forward[:, :3], [[-2, 0, 84]] * 4)


@pytest.mark.parametrize('config,name', [
    ([{'GaussianBlur': {'sigma': 1.0}}], 'GaussianBlur'),
    ([{'Sometimes': {'p': 0.5, 'then_list': [{'PerspectiveTransform': {}}]}}], 'PerspectiveTransform'),
    ([{'Affine': {'shear': [-8, 8]}}], 'shear'),
    ([{'Crop': {'px': 3}}], 'px'),
    ([{'Sometimes': {'then_list': [{'Sometimes': {'then_list': []}}]}}], 'Sometimes inside Sometimes'),
    ([{'AddToHue': {'value': 3}}, {'AddToHue': {'value': 4}}], 'AddToHue'),
])
def test_what_is_not_built_raises_and_names_it(config, name):
    from datasets.augment import Augmentation
    with pytest.raises(NotImplementedError, match=name):
        Augmentation(config)


def test_refusals_need_no_gpu():
    import torch
    from datasets import augment_images, transform_boxes, transform_points
    from datasets.augment import AugmentParams
    p = AugmentParams.identity([[4, 4]], (4, 4))
    with pytest.raises(RuntimeError, match='MI355X only'):
        augment_images(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), p)
    with pytest.raises(RuntimeError, match='MI355X only'):
        transform_points(torch.zeros(1, 2, 2, dtype=torch.float64), p)
    with pytest.raises(RuntimeError, match='MI355X only'):
        transform_boxes(torch.zeros(1, 2, 4, dtype=torch.float64), p)


def test_entry_points_reject_bad_arguments_before_touching_the_device():
    import hip_runtime as hr
    L = hr.lib()
    assert L.cnuda_augment_color(None, None, None, 1, 4, 4, None) == -1
    assert b'cnuda_augment_color' in L.cnuda_last_error()
    assert L.cnuda_augment_warp(None, None, None, None, None, None, None, None, 0, 1, 4, 4, 4, 4, None) == -1
    assert b'cnuda_augment_warp' in L.cnuda_last_error()
    assert L.cnuda_augment_points(None, None, None, 0, None, None, 0, 1, None) == -1
    assert b'cnuda_augment_points' in L.cnuda_last_error()
