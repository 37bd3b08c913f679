"""MI355X: datasets.augment against tests/augment_oracle.py (itself pinned in tests/test_host_augment.py).  Warp and
colour are compared byte for byte, points and boxes bit for bit with the float64 expression; the noise is checked by its
statistics; build_batch against the hand-made chain of its four stages."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import augment_oracle as ao

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bytes(shape, seed):
    """every byte value as far as the size allows, permuted"""
    n = int(np.prod(shape))
    return np.random.RandomState(seed).permutation(np.arange(n, dtype=np.int64) % 256).astype(np.uint8).reshape(shape)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------
# (buffer [B, H_max, W_max], valid sizes, output (h, w)): an odd output width with a scalar tail and per-image sizes
# inside a padded buffer; a width of whole dword runs; more than one workgroup; a single pixel
SHAPES = {
    'padded-to-9x11': ((2, 13, 20), [[13, 17], [9, 20]], (9, 11)),
    'padded-to-16x16': ((2, 13, 20), [[13, 17], [9, 20]], (16, 16)),
    'wide-4x4100': ((1, 4, 4100), [[4, 4100]], (4, 4100)),
    'pixel-to-3x3': ((1, 1, 1), [[1, 1]], (3, 3)),
}
# (k, direction): one tap, then 3, 4 and 10 taps, flat and ramped
TAPS = [(1, 0.0), (3, 0.0), (3, 0.7), (4, 0.0), (4, 0.7), (10, 0.0), (10, 0.7)]


def _geometry(kind, h, w):
    from datasets.augment import affine_matrix, crop_matrix, fliplr_matrix, flipud_matrix
    if kind == 'resize':
        return np.eye(3)
    if kind == 'fliplr':
        return fliplr_matrix(w)
    if kind == 'flipud':
        return flipud_matrix(h)
    if kind == 'rotate':                       # shrunk, turned and shifted: corners of the output fall outside
        return affine_matrix(h, w, scale=(0.8, 0.8), translate_percent=(0.11, -0.07), rotate=33)
    return crop_matrix(h, w, 0.05, 0.2, 0.15, 0.1)


def _warp_params(shape, kind, k, direction):
    from datasets.augment import AugmentParams, motion_blur_taps, resize_matrix
    _, sizes, (ho, wo) = SHAPES[shape]
    mats = [resize_matrix(h, w, (wo, ho)) @ _geometry(kind, h, w) for h, w in sizes]
    taps = [motion_blur_taps(k, 25.0 + 70.0 * b, direction) for b in range(len(sizes))]
    return AugmentParams.from_matrices(sizes, (wo, ho), np.stack(mats), taps=taps)


@pytest.mark.parametrize('kind', ['resize', 'fliplr', 'flipud', 'rotate', 'crop'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_warp_equals_the_oracle_byte_for_byte(shape, kind):
    import hip_runtime as hr
    from datasets import augment_images
    buf, sizes, (ho, wo) = SHAPES[shape]
    img = _bytes(buf + (3,), seed=buf[2])
    d_img = _gpu(img)
    outside = 0
    for k, direction in TAPS:
        p = _warp_params(shape, kind, k, direction)
        assert list(p.ntaps) == [k] * buf[0]
        with hr.launch_log() as log:
            got = augment_images(d_img, p)
        assert any('augment_warp_kernel' in n for n in log.names), log.names
        assert not any('augment_color_kernel' in n for n in log.names), log.names      # nothing drew a colour change
        assert got.shape == (buf[0], ho, wo, 3) and got.dtype == torch.uint8 and got.is_contiguous()
        want = ao.warp_batch(img, p)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='k=%d direction=%g' % (k, direction))
        outside += int((want.reshape(-1, 3).max(1) == 0).sum())
    if kind == 'rotate':
        assert outside > 0                      # the outside rule was exercised


def test_warp_reads_nothing_beyond_the_valid_size():
    from datasets import augment_images
    from datasets.augment import AugmentParams
    img = _bytes((2, 13, 20, 3), seed=5)
    other = img.copy()
    other[0, :, 17:], other[1, 9:] = 255, 0
    p = AugmentParams.identity([[13, 17], [9, 20]], (31, 27))
    a, b = augment_images(_gpu(img), p), augment_images(_gpu(other), p)
    assert torch.equal(a, b)
    # `sizes` overrides the record's
    q = AugmentParams.identity([[13, 20], [13, 20]], (31, 27))
    q = dataclasses.replace(q, inverse=p.inverse)
    assert torch.equal(augment_images(_gpu(img), q, sizes=[[13, 17], [9, 20]]), a)


# ---------------------------------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------------------------------
COLOURS = [(0, 0, 0), (0, 120, 0), (0, 37.5, 0), (0, -101, 40), (1, 0, 0), (0.3, 180, -60)]


def _all_bytes_image():
    rs = np.random.RandomState(9)
    return np.stack([rs.permutation(256) for _ in range(3)], -1).astype(np.uint8).reshape(16, 16, 3)


@pytest.mark.parametrize('colour', COLOURS, ids=lambda c: 'a%g-h%g-v%g' % c)
def test_colour_equals_the_oracle_byte_for_byte(colour):
    import hip_runtime as hr
    from datasets import augment_images
    from datasets.augment import AugmentParams
    img = _all_bytes_image()
    for c in range(3):
        assert len(np.unique(img[..., c])) == 256
    p = AugmentParams.from_matrices([[16, 16]], (16, 16), np.eye(3)[None], color=[colour])
    with hr.launch_log() as log:
        got = augment_images(_gpu(img[None]), p).cpu().numpy()[0]
    assert any('augment_color_kernel' in n for n in log.names) == any(colour), log.names
    np.testing.assert_array_equal(got, ao.color(img, *colour))      # the identity warp returns its input exactly
    if not any(colour):
        np.testing.assert_array_equal(got, img)


# 5 x 3 = 15 pixels per image: a group of four straddles the two images and two pixels are left for the scalar tail;
# 16 x 16: whole groups
@pytest.mark.parametrize('hw', [(5, 3), (16, 16)])
def test_only_the_image_that_drew_a_colour_changes(hw):
    from datasets import augment_images
    from datasets.augment import AugmentParams
    h, w = hw
    img = _bytes((2, h, w, 3), seed=h)
    for changed in (0, 1):
        colour = [(0, 0, 0), (0, 0, 0)]
        colour[changed] = (0.3, 180, -60)
        p = AugmentParams.from_matrices([[h, w]] * 2, (w, h), np.stack([np.eye(3)] * 2), color=colour)
        got = augment_images(_gpu(img), p).cpu().numpy()
        np.testing.assert_array_equal(got[1 - changed], img[1 - changed])
        np.testing.assert_array_equal(got[changed], ao.color(img[changed], 0.3, 180, -60))
        assert not np.array_equal(got[changed], img[changed])


# ---------------------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------------------
def _noise_params(seed, scales=(0, 8), ids=None):
    from datasets.augment import AugmentParams
    return AugmentParams.from_matrices([[64, 64]] * 2, (64, 64), np.stack([np.eye(3)] * 2), noise=scales, seed=seed,
                                       image_ids=ids)


def test_noise_is_white_gaussian_and_shared_by_the_channels():
    from datasets import augment_images
    img = _gpu(np.full((2, 64, 64, 3), 128, np.uint8))
    got = augment_images(img, _noise_params(2024)).cpu().numpy()
    assert (got[0] == 128).all()
    assert np.array_equal(got[1][..., 0], got[1][..., 1]) and np.array_equal(got[1][..., 0], got[1][..., 2])
    d = got[1][..., 0].astype(np.float64) - 128
    n, sr = 4096, math.sqrt(64 + 1 / 12)                      # a rounded N(0, 8^2): variance 64 + 1/12
    lag_x = np.corrcoef(d[:, :-1].ravel(), d[:, 1:].ravel())[0, 1]
    lag_y = np.corrcoef(d[:-1].ravel(), d[1:].ravel())[0, 1]
    share, p = (np.abs(d) > 16).mean(), 0.0455
    print('mean %.4f std %.4f (%.4f) lag-1 %.4f %.4f share %.4f' % (d.mean(), d.std(), sr, lag_x, lag_y, share))
    assert abs(d.mean()) <= 5 * sr / math.sqrt(n)
    assert abs(d.std() - sr) <= 5 * sr / math.sqrt(2 * n)
    assert abs(lag_x) <= 5 / math.sqrt(n) and abs(lag_y) <= 5 / math.sqrt(n)
    assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / n)


def test_noise_depends_on_seed_and_image_id_alone():
    from datasets import augment_images
    img = _gpu(np.full((2, 64, 64, 3), 128, np.uint8))
    p = _noise_params(77, scales=(5, 8))
    a = augment_images(img, p)
    assert torch.equal(a, augment_images(img, p))
    assert not torch.equal(a, augment_images(img, _noise_params(78, scales=(5, 8))))
    same_scale = augment_images(img, _noise_params(77, scales=(8, 8)))
    assert not torch.equal(same_scale[0], same_scale[1])                  # the two images draw different deviates
    # swapping the images' positions in the batch swaps the results and nothing else
    swapped = augment_images(img.flip(0), p.take([1, 0]))
    assert torch.equal(swapped, a.flip(0))
    # an image alone, under its own id, gets the noise it had in the batch: no dependence on launch geometry
    one = p.take([1])
    assert torch.equal(augment_images(img[1:], one), a[1:])
    # and under another id, other noise
    assert not torch.equal(augment_images(img, _noise_params(77, scales=(5, 8), ids=[0, 5]))[1], a[1])


# ---------------------------------------------------------------------------------------------------------------------
# points and boxes
# ---------------------------------------------------------------------------------------------------------------------
def _rotation_params():
    from datasets.augment import AugmentParams, affine_matrix, fliplr_matrix, resize_matrix
    sizes = [[24, 32], [17, 29]]
    mats = [resize_matrix(24, 32, (40, 36)) @ affine_matrix(24, 32, (1.1, 0.9), (0.05, -0.1), 33.0),
            resize_matrix(17, 29, (40, 36)) @ fliplr_matrix(29) @ affine_matrix(17, 29, (0.7, 0.7), (0, 0), -71.0)]
    return AugmentParams.from_matrices(sizes, (40, 36), np.stack(mats))


@pytest.mark.parametrize('down_ratio', [1, 4])
def test_points_and_boxes_equal_the_float64_expression(down_ratio):
    import hip_runtime as hr
    from datasets import transform_boxes, transform_points
    p = _rotation_params()
    rs = np.random.RandomState(3)
    pts = rs.uniform(-5, 40, (2, 7, 2))
    bxs = np.sort(rs.uniform(0, 30, (2, 7, 2, 2)), 2).reshape(2, 7, 4)           # x1 <= x2, y1 <= y2
    bxs[0, 3, 2] = bxs[0, 3, 0]                                                     # degenerate: x1 == x2
    bxs[1, 6] = bxs[1, 6, [2, 3, 0, 1]]                                             # and one given corner-swapped
    with hr.launch_log() as log:
        got_p = transform_points(_gpu(pts), p, down_ratio)
        got_b = transform_boxes(_gpu(bxs), p, down_ratio)
    assert any('augment_points_kernel' in n for n in log.names), log.names
    assert got_p.dtype == got_b.dtype == torch.float64 and got_p.shape == (2, 7, 2) and got_b.shape == (2, 7, 4)
    fwd = p.forward / float(down_ratio)
    np.testing.assert_array_equal(got_p.cpu().numpy(), np.stack([ao.points(fwd[b], pts[b]) for b in range(2)]))
    want_b = np.stack([ao.boxes(fwd[b], bxs[b]) for b in range(2)])
    np.testing.assert_array_equal(got_b.cpu().numpy(), want_b)
    assert (want_b[..., 2] >= want_b[..., 0]).all() and (want_b[..., 3] >= want_b[..., 1]).all()
    assert want_b[0, 3, 2] > want_b[0, 3, 0]             # a rotated zero-width box has a bounding box with extent
    # float32 points are taken as they are
    got32 = transform_points(_gpu(pts.astype(np.float32)), p, down_ratio).cpu().numpy()
    np.testing.assert_array_equal(got32, np.stack([ao.points(fwd[b], pts[b].astype(np.float32).astype(np.float64))
                                                   for b in range(2)]))


# ---------------------------------------------------------------------------------------------------------------------
# build_batch
# ---------------------------------------------------------------------------------------------------------------------
B, M, J, C = 2, 3, 2, 3
# every scaled box lies inside the 8 x 8 map, so the loop's clip to [0, 7] moves nothing under the identity
SIZE, DOWN = (32, 32), 4
BOXES = np.array([[[3.0, 2.0, 20.5, 15.25], [10.0, 8.0, 27.0, 20.0], [1.5, 12.0, 9.0, 20.5]],
                  [[5.0, 5.0, 27.0, 19.0], [14.0, 1.0, 22.0, 9.5], [0.0, 0.0, 0.0, 0.0]]])
CLASSES = np.array([[0, 2, 1], [1, 1, 0]], np.int32)
COUNTS = np.array([3, 2], np.int32)
SCHEMA = {'input': (torch.float32, (B, 3, 32, 32)), 'hm': (torch.float32, (B, C, 8, 8)),
          'reg_mask': (torch.uint8, (B, M)), 'ind': (torch.int64, (B, M)), 'wh': (torch.float32, (B, M, 2)),
          'reg': (torch.float32, (B, M, 2)), 'gt_dets': (torch.float32, (B, M, 6)),
          'gt_areas': (torch.float32, (B, M))}
KP_SCHEMA = {'kps': (torch.float32, (B, M, 2 * J)), 'gt_kps': (torch.float32, (B, M, J, 2)),
             'kp_reg_mask': (torch.uint8, (B, M, 2 * J))}


def _sources():
    return _bytes((B, 24, 32, 3), seed=24)


def _drawn_params(seed):
    import json
    import os
    from datasets.augment import Augmentation
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augmentation_defaults.json')) as fh:
        aug = Augmentation(json.load(fh))
    for s in range(seed, seed + 50):            # a draw in which both images took the augmenting branch
        p = aug.sample([[24, 32]] * B, SIZE, np.random.default_rng(s))
        if p.applied['Sometimes'].all():
            return p
    raise AssertionError('no draw took the branch twice')


def _keypoints():
    rs = np.random.RandomState(1)
    centres = np.stack([(BOXES[..., 0] + BOXES[..., 2]) / 2, (BOXES[..., 1] + BOXES[..., 3]) / 2], -1)
    kp = centres[:, :, None, :] + rs.uniform(-3, 3, (B, M, J, 2))
    vis = np.array([[[2, 2], [2, 1], [0, 2]], [[2, 2], [2, 2], [2, 2]]], np.int32)
    return kp, vis


def _corners():
    """each box turned about its centre, as utils.box.rotate_bbox lays its vertices out"""
    out = np.zeros((B, M, 4, 2))
    for b in range(B):
        for k in range(M):
            x1, y1, x2, y2 = BOXES[b, k]
            t = math.radians(20.0 + 25 * k + 40 * b)
            rot = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
            c = np.array([(x1 + x2) / 2, (y1 + y2) / 2])
            pts = np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])
            out[b, k] = (pts - c) @ rot.T + c
    return out


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key].view(torch.uint8), want[key].view(torch.uint8)), key      # bit by bit


def _assert_schema(batch, schema):
    assert sorted(batch) == sorted(schema)
    for key, (dtype, shape) in schema.items():
        assert batch[key].dtype == dtype and tuple(batch[key].shape) == shape, key


def test_build_batch_with_keypoints_is_the_chain_of_its_stages():
    from datasets import (augment_images, build_batch, encode_targets, prepare_input, transform_boxes,
                          transform_points)
    p = _drawn_params(100)
    assert p.color.any() and (p.ntaps > 1).all() and (p.noise > 0).all()
    img, (kp, vis) = _gpu(_sources()), _keypoints()
    areas = np.array([[100.0, np.nan, 31.5], [7.0, 8.0, 9.0]], np.float32)
    got = build_batch(img, _gpu(BOXES), _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=SIZE, num_classes=C,
                      down_ratio=DOWN, keypoints=_gpu(kp), visibility=_gpu(vis), areas=_gpu(areas))
    want = {'input': prepare_input(augment_images(img, p))}
    want.update(encode_targets(transform_boxes(_gpu(BOXES), p, DOWN), _gpu(CLASSES), _gpu(COUNTS), C, 8, 8,
                               keypoints=transform_points(_gpu(kp.reshape(B, M * J, 2)), p, DOWN).reshape(B, M, J, 2),
                               visibility=_gpu(vis), areas=_gpu(areas)))
    _assert_same(got, want)
    _assert_schema(got, {**SCHEMA, **KP_SCHEMA})
    assert got['reg_mask'].sum() > 0
    # areas pass through unscaled
    mask = got['reg_mask'].cpu().numpy().astype(bool) & ~np.isnan(areas)
    np.testing.assert_array_equal(got['gt_areas'].cpu().numpy()[mask], areas[mask])


def test_build_batch_with_corners_is_the_chain_of_its_stages():
    from datasets import augment_images, build_batch, encode_targets, prepare_input, transform_points
    p = _drawn_params(200)
    img, corners = _gpu(_sources()), _corners()
    got = build_batch(img, None, _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=SIZE, num_classes=C,
                      down_ratio=DOWN, corners=_gpu(corners))
    moved = transform_points(_gpu(corners.reshape(B, M * 4, 2)), p, DOWN).reshape(B, M, 4, 2)
    want = {'input': prepare_input(augment_images(img, p))}
    want.update(encode_targets(None, _gpu(CLASSES), _gpu(COUNTS), C, 8, 8, corners=moved))
    _assert_same(got, want)
    schema = dict(SCHEMA, wh=(torch.float32, (B, M, 3)), gt_dets=(torch.float32, (B, M, 7)))
    _assert_schema(got, schema)


def test_identity_parameters_put_each_centre_on_the_scaled_box_centre():
    from datasets import build_batch
    from datasets.augment import AugmentParams
    p = AugmentParams.identity([[24, 32]] * B, SIZE)
    got = build_batch(_gpu(_sources()), _gpu(BOXES), _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=SIZE,
                      num_classes=C, down_ratio=DOWN)
    _assert_schema(got, SCHEMA)
    sx, sy = 32 / 32 / DOWN, 32 / 24 / DOWN
    ind, mask = got['ind'].cpu().numpy(), got['reg_mask'].cpu().numpy()
    assert mask.tolist() == [[1, 1, 1], [1, 1, 0]]
    for b in range(B):
        for k in range(COUNTS[b]):
            x1, y1, x2, y2 = BOXES[b, k]
            cx, cy = np.float32((x1 * sx + x2 * sx) / 2), np.float32((y1 * sy + y2 * sy) / 2)
            assert ind[b, k] == int(cy) * 8 + int(cx), (b, k)
    # and the input is the resized image, normalised
    from datasets import prepare_input
    want = prepare_input(_gpu(ao.warp_batch(_sources(), p)))
    assert torch.equal(got['input'], want)


def test_target_images_add_target_domain_input_and_calls_repeat_bit_for_bit():
    from datasets import augment_images, build_batch, prepare_input
    from datasets.augment import AugmentParams
    p = _drawn_params(300)
    img, tgt = _gpu(_sources()), _gpu(_bytes((B, 20, 28, 3), seed=20))
    tsizes = [[20, 28], [15, 19]]

    def call(**kw):
        return build_batch(img, _gpu(BOXES), _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=SIZE, num_classes=C,
                           down_ratio=DOWN, target_images=tgt, **kw)
    a, b = call(target_sizes=tsizes), call(target_sizes=tsizes)
    _assert_same(a, b)
    _assert_schema(a, dict(SCHEMA, target_domain_input=(torch.float32, (B, 3, 32, 32))))
    resized = augment_images(tgt, AugmentParams.identity(tsizes, SIZE))
    assert torch.equal(a['target_domain_input'], prepare_input(resized))
    np.testing.assert_array_equal(resized.cpu().numpy(),
                                  ao.warp_batch(tgt.cpu().numpy(), AugmentParams.identity(tsizes, SIZE)))
    # without sizes the whole buffer is the image; with target_params the target domain is augmented too
    full = call()
    assert torch.equal(full['target_domain_input'],
                       prepare_input(augment_images(tgt, AugmentParams.identity([[20, 28]] * B, SIZE))))
    tp = dataclasses.replace(_drawn_params(400), sizes=np.array([[20, 28]] * B, np.int32))
    aug = call(target_params=tp)
    assert torch.equal(aug['target_domain_input'], prepare_input(augment_images(tgt, tp)))
    assert not torch.equal(aug['target_domain_input'], full['target_domain_input'])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_wrong_inputs_are_refused():
    from datasets import augment_images, build_batch, transform_boxes, transform_points
    from datasets.augment import AugmentParams
    img = _bytes((2, 6, 8, 3), seed=1)
    t = _gpu(img)
    p = AugmentParams.identity([[6, 8]] * 2, (8, 6))
    with pytest.raises(RuntimeError, match='MI355X only'):
        augment_images(torch.from_numpy(img), p)
    with pytest.raises(RuntimeError, match='uint8'):
        augment_images(t.float(), p)
    with pytest.raises(RuntimeError, match=r'\[B, H, W, 3\]'):
        augment_images(t[0], p)
    with pytest.raises(RuntimeError, match=r'\[B, H, W, 3\]'):
        augment_images(t.permute(0, 3, 1, 2).contiguous(), p)
    with pytest.raises(RuntimeError, match='1 to 10 taps'):
        augment_images(t, dataclasses.replace(p, ntaps=np.array([1, 11], np.int32)))
    with pytest.raises(RuntimeError, match='describe 2 images'):
        augment_images(t[:1], p)
    with pytest.raises(RuntimeError, match='do not fit'):
        augment_images(t, p, sizes=[[6, 8], [7, 8]])
    with pytest.raises(RuntimeError, match=r'\[B, N, 2\]'):
        transform_points(torch.zeros(2, 7, 3, dtype=torch.float64, device=DEV), p)
    with pytest.raises(RuntimeError, match=r'\[B, M, 4\]'):
        transform_boxes(torch.zeros(2, 4, dtype=torch.float64, device=DEV), p)
    with pytest.raises(RuntimeError, match='MI355X only'):
        transform_boxes(torch.zeros(2, 3, 4, dtype=torch.float64), p)
    with pytest.raises(RuntimeError, match='input_size'):
        build_batch(t, _gpu(BOXES), _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=(16, 16), num_classes=C)
    with pytest.raises(RuntimeError, match='either boxes or corners'):
        build_batch(t, None, _gpu(CLASSES), _gpu(COUNTS), params=p, input_size=(8, 6), num_classes=C)
    # a view that starts at an odd byte is copied first, a strided one made contiguous
    flat = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = t.reshape(-1)
    odd = flat[1:].view(2, 6, 8, 3)
    assert odd.data_ptr() % 4
    tint = dataclasses.replace(p, color=np.array([[0, 90, 10]] * 2, np.float32))
    want = np.stack([ao.color(img[b], 0, 90, 10) for b in range(2)])
    np.testing.assert_array_equal(augment_images(odd, tint).cpu().numpy(), want)
