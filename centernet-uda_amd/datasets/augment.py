"""Augmentation and resizing of training images on the GPU, annotations included ("Augmentation on the
device").

The reference runs an imgaug chain per image on the host (datasets/coco.py:60-67,140-158 with the `augmentation:` list
of configs/defaults.yaml:38-60).  Here the random draws and the matrix algebra stay on the host, in numpy, and three
HIP kernels apply them to a whole batch:

    aug = Augmentation(config)                        # the reference's list of one-key dicts
    params = aug.sample(sizes, input_size, rng)       # AugmentParams: numpy arrays, no GPU needed
    batch = build_batch(images, boxes, classes, counts, params=params, input_size=input_size, num_classes=C)

`build_batch` returns the reference's batch dict except `id`: `input` (and `target_domain_input`) through
`augment_images` and `prepare_input`, every target key through `transform_points` / `transform_boxes` and
`encode_targets`.  `AugmentParams.identity` is the resize-only record for validation data.

The augmenters are defined geometrically (imgaug and cv2 are no dependency and nothing was compared with them):
Affine, Crop, Fliplr, Flipud and the final Resize compose into ONE forward matrix per image, in float64, and the image
is resampled once; MotionBlur is a line of at most ten taps in source space; Grayscale, AddToHue and AddToBrightness
are one pointwise pass over the source; AdditiveGaussianNoise is white at input resolution, from Philox4x32-10 keyed by
the record's seed and countered by image id and pixel.  The stages run in this fixed order (colour, blur, warp, noise),
whatever their position in the list.
"""
import dataclasses
import math

import numpy as np
import torch

from hip_runtime import check, lib, ptr, require_gpu, stream

from .prepare import MEAN, STD, prepare_input
from .targets import encode_targets

MAX_TAPS = 10

_KEYS = {
    'Grayscale': ('alpha',),
    'AddToHue': ('value',),
    'AddToBrightness': ('add',),
    'MotionBlur': ('k', 'angle', 'direction'),
    'Affine': ('scale', 'translate_percent', 'rotate'),
    'Crop': ('percent',),
    'AdditiveGaussianNoise': ('scale',),
    'Fliplr': ('p',),
    'Flipud': ('p',),
}
_ONCE = ('Grayscale', 'AddToHue', 'AddToBrightness', 'MotionBlur', 'AdditiveGaussianNoise')


# ---------------------------------------------------------------------------------------------------------------------
# matrices: 3 x 3 float64, source coordinates -> destination coordinates, points as columns (u, v, 1)
# ---------------------------------------------------------------------------------------------------------------------
def affine_matrix(h, w, scale=(1.0, 1.0), translate_percent=(0.0, 0.0), rotate=0.0):
    """Scale, then rotate (degrees, positive = clockwise on the y-down image), about the image centre (w/2, h/2);
    then translate by a fraction of the width / height."""
    sx, sy = scale
    t = math.radians(rotate)
    c, s = math.cos(t), math.sin(t)
    lin = np.array([[c, -s], [s, c]]) @ np.diag([float(sx), float(sy)])
    centre = np.array([w / 2.0, h / 2.0])
    m = np.eye(3)
    m[:2, :2] = lin
    m[:2, 2] = centre - lin @ centre + np.array([translate_percent[0] * w, translate_percent[1] * h])
    return m


def crop_matrix(h, w, top, right, bottom, left):
    """Cut the four fractions off the sides and map what remains back onto the full frame."""
    kw, kh = 1.0 - left - right, 1.0 - top - bottom
    if not (kw > 0 and kh > 0):
        raise ValueError("Crop: the fractions (%g, %g, %g, %g) leave nothing of the image" % (top, right, bottom, left))
    return np.array([[1.0 / kw, 0.0, -left * w / kw], [0.0, 1.0 / kh, -top * h / kh], [0.0, 0.0, 1.0]])


def fliplr_matrix(w):
    return np.array([[-1.0, 0.0, float(w)], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def flipud_matrix(h):
    return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, float(h)], [0.0, 0.0, 1.0]])


def resize_matrix(h, w, input_size):
    """(h, w) source -> input_size = (width, height)."""
    return np.diag([input_size[0] / float(w), input_size[1] / float(h), 1.0])


def motion_blur_taps(k, angle, direction):
    """-> [k, 3] float64 (offset x, offset y, weight): k taps on a line through the sample point, tap m at
    (m - (k-1)/2) (sin a, -cos a) with weight (1 + direction (2m/(k-1) - 1)) / k."""
    k = int(k)
    if not 1 <= k <= MAX_TAPS:
        raise ValueError("MotionBlur: k must be in [1, %d], got %d" % (MAX_TAPS, k))
    a = math.radians(angle)
    m = np.arange(k, dtype=np.float64)
    pos = m - (k - 1) / 2.0
    ramp = 2.0 * m / (k - 1) - 1.0 if k > 1 else np.zeros(1)
    return np.stack([pos * math.sin(a), -pos * math.cos(a), (1.0 + direction * ramp) / k], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the parameter record
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class AugmentParams:
    """What one batch drew, as numpy arrays (B images):
    sizes [B, 2] int32 (h, w) of the sources; input_size (width, height) of the result;
    color [B, 3] float32 (grayscale alpha, hue rotation in degrees, brightness add);
    taps [B, 10, 3] float32 (offset x, offset y, weight) and ntaps [B] int32;
    forward [B, 6] float64, source -> input coordinates (row-major 2 x 3); inverse [B, 6] float32, its inverse;
    noise [B] float32 standard deviations; seed: the noise generator's 64-bit key; image_ids [B] int64: the images'
    noise counters (the position in the batch unless the loader names them, e.g. by dataset index);
    draws: {augmenter.key: [B] float64, NaN where the image did not draw it}; applied: {augmenter: [B] bool}."""
    sizes: np.ndarray
    input_size: tuple
    color: np.ndarray
    taps: np.ndarray
    ntaps: np.ndarray
    forward: np.ndarray
    inverse: np.ndarray
    noise: np.ndarray
    seed: int
    image_ids: np.ndarray
    draws: dict = dataclasses.field(default_factory=dict)
    applied: dict = dataclasses.field(default_factory=dict)

    @property
    def batch(self):
        return self.sizes.shape[0]

    @classmethod
    def from_matrices(cls, sizes, input_size, matrices, color=None, taps=None, noise=None, seed=0, image_ids=None):
        """Record from explicit forward matrices [B, 3, 3] (or [B, 2, 3]); taps: per image a [k, 3] array or None."""
        sizes = _sizes(sizes)
        B = sizes.shape[0]
        matrices = np.asarray(matrices, dtype=np.float64)
        if matrices.shape[0] != B or matrices.shape[1:] not in ((3, 3), (2, 3)):
            raise ValueError("from_matrices: matrices must be [%d, 3, 3], got %s" % (B, matrices.shape))
        full = np.tile(np.eye(3), (B, 1, 1))
        full[:, :2] = matrices[:, :2]
        tap_table = np.zeros((B, MAX_TAPS, 3), dtype=np.float32)
        ntaps = np.ones(B, dtype=np.int32)
        tap_table[:, 0, 2] = 1.0
        for b in range(B):
            t = None if taps is None else taps[b]
            if t is not None:
                t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
                if not 1 <= t.shape[0] <= MAX_TAPS:
                    raise ValueError("from_matrices: 1 to %d taps per image, got %d" % (MAX_TAPS, t.shape[0]))
                ntaps[b] = t.shape[0]
                tap_table[b] = 0
                tap_table[b, :t.shape[0]] = t
        return cls(sizes=sizes, input_size=(int(input_size[0]), int(input_size[1])),
                   color=np.zeros((B, 3), np.float32) if color is None
                   else np.asarray(color, dtype=np.float32).reshape(B, 3).copy(),
                   taps=tap_table, ntaps=ntaps,
                   forward=full[:, :2].reshape(B, 6).copy(),
                   inverse=np.linalg.inv(full)[:, :2].reshape(B, 6).astype(np.float32),
                   noise=np.zeros(B, np.float32) if noise is None
                   else np.asarray(noise, dtype=np.float32).reshape(B).copy(),
                   seed=int(seed) & (2 ** 64 - 1),
                   image_ids=np.arange(B, dtype=np.int64) if image_ids is None
                   else np.asarray(image_ids, dtype=np.int64).reshape(B).copy())

    @classmethod
    def identity(cls, sizes, input_size):
        """Resize only: one tap, no noise, neutral colour."""
        sizes = _sizes(sizes)
        return cls.from_matrices(sizes, input_size, np.stack([resize_matrix(h, w, input_size) for h, w in sizes]))

    def take(self, index):
        """The record of the images `index` (a permutation or a subset), each with its own draws and noise counter."""
        index = np.asarray(index, dtype=np.int64)
        return dataclasses.replace(
            self, sizes=self.sizes[index], color=self.color[index], taps=self.taps[index], ntaps=self.ntaps[index],
            forward=self.forward[index], inverse=self.inverse[index], noise=self.noise[index],
            image_ids=self.image_ids[index], draws={k: v[index] for k, v in self.draws.items()},
            applied={k: v[index] for k, v in self.applied.items()})


def _sizes(sizes):
    if isinstance(sizes, torch.Tensor):
        sizes = sizes.cpu().numpy()
    sizes = np.asarray(sizes)
    if sizes.ndim != 2 or sizes.shape[1] != 2 or sizes.shape[0] < 1 or (sizes < 1).any():
        raise ValueError("sizes must be [B, 2] positive (h, w), got shape %s" % (sizes.shape,))
    return sizes.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the configured chain
# ---------------------------------------------------------------------------------------------------------------------
def _interval(v, what):
    """scalar -> (v, v); [a, b] -> (a, b)"""
    if hasattr(v, '__len__') and not isinstance(v, str) and not hasattr(v, 'keys'):
        v = list(v)                                   # a config library's list type
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return float(v), float(v)
    if isinstance(v, (list, tuple)) and len(v) == 2 and all(isinstance(x, (int, float)) for x in v):
        a, b = float(v[0]), float(v[1])
        if a > b:
            raise ValueError("%s: interval [%g, %g] is empty" % (what, a, b))
        return a, b
    raise NotImplementedError("%s: a number or a two-element interval is supported, got %r" % (what, v))


def _xy(v, what):
    """{x, y} dict -> (interval or None, interval or None)"""
    unknown = sorted(set(v) - {'x', 'y'})
    if unknown:
        raise NotImplementedError("%s: unsupported key %r" % (what, unknown[0]))
    return tuple(_interval(v[a], '%s.%s' % (what, a)) if a in v else None for a in 'xy')


class Augmentation:
    """The reference's `augmentation:` list (utils/helper.py:53-71 hands it to imgaug): one-key dicts, `Sometimes:
    {p, then_list}` one level deep.  Anything this build does not restate raises NotImplementedError by name."""

    def __init__(self, config):
        self.steps = self._parse(config, nested=False)
        names = [s[0] for s in self._flat(self.steps)]
        for n in _ONCE:
            if names.count(n) > 1:
                raise NotImplementedError("%s appears %d times: it is applied in one fixed stage and may be listed once"
                                          % (n, names.count(n)))

    @staticmethod
    def _flat(steps):
        for name, spec in steps:
            if name == 'Sometimes':
                yield from spec[1]
            else:
                yield name, spec

    def _parse(self, config, nested):
        if config is None:
            return []
        steps = []
        for n_item, item in enumerate(config):
            item = dict(item)
            if len(item) != 1:
                raise ValueError("augmentation entry %d must be a one-key dict, got %r" % (n_item, sorted(item)))
            name, params = next(iter(item.items()))
            params = dict(params or {})
            if name == 'Sometimes':
                if nested:
                    raise NotImplementedError("Sometimes inside Sometimes is not supported")
                unknown = sorted(set(params) - {'p', 'then_list'})
                if unknown:
                    raise NotImplementedError("Sometimes: unsupported key %r" % unknown[0])
                steps.append((name, (self._p(params.get('p', 0.5), name), self._parse(params.get('then_list'), True))))
                continue
            if name not in _KEYS:
                raise NotImplementedError("augmenter %r is not supported (supported: Sometimes, %s)"
                                          % (name, ', '.join(_KEYS)))
            unknown = sorted(set(params) - set(_KEYS[name]))
            if unknown:
                raise NotImplementedError("%s: unsupported key %r (supported: %s)"
                                          % (name, unknown[0], ', '.join(_KEYS[name])))
            steps.append((name, getattr(self, '_parse_' + name)(params)))
        return steps

    @staticmethod
    def _p(p, name):
        if not isinstance(p, (int, float)) or not 0 <= p <= 1:
            raise ValueError("%s: p must be a probability, got %r" % (name, p))
        return float(p)

    def _parse_Grayscale(self, q):
        a = _interval(q.get('alpha', 1.0), 'Grayscale.alpha')
        if a[0] < 0 or a[1] > 1:
            raise ValueError("Grayscale.alpha must lie in [0, 1], got %r" % (a,))
        return {'alpha': a}

    def _parse_AddToHue(self, q):
        return {'value': _interval(q.get('value', (-255, 255)), 'AddToHue.value')}

    def _parse_AddToBrightness(self, q):
        return {'add': _interval(q.get('add', (-30, 30)), 'AddToBrightness.add')}

    def _parse_MotionBlur(self, q):
        k = _interval(q.get('k', (3, 7)), 'MotionBlur.k')
        if k[0] != int(k[0]) or k[1] != int(k[1]) or k[0] < 1 or k[1] > MAX_TAPS:
            raise ValueError("MotionBlur.k must be integers in [1, %d], got %r" % (MAX_TAPS, k))
        d = _interval(q['direction'], 'MotionBlur.direction') if 'direction' in q else None
        if d is not None and (d[0] < -1 or d[1] > 1):
            raise ValueError("MotionBlur.direction must lie in [-1, 1], got %r" % (d,))
        return {'k': (int(k[0]), int(k[1])), 'angle': _interval(q.get('angle', (0, 360)), 'MotionBlur.angle'),
                'direction': d}

    def _parse_Affine(self, q):
        out = {}
        for key in ('scale', 'translate_percent'):
            v = q.get(key)
            if v is None:
                out[key] = None
            elif isinstance(v, dict) or hasattr(v, 'keys'):
                out[key] = ('xy', _xy(dict(v), 'Affine.' + key))
            else:
                out[key] = ('one', _interval(v, 'Affine.' + key))
        if out['scale'] is not None:
            lows = [iv[0] for iv in (out['scale'][1] if out['scale'][0] == 'xy' else [out['scale'][1]]) if iv]
            if any(lo <= 0 for lo in lows):
                raise ValueError("Affine.scale must be positive")
        out['rotate'] = _interval(q['rotate'], 'Affine.rotate') if 'rotate' in q else None
        return out

    def _parse_Crop(self, q):
        a = _interval(q.get('percent', 0.0), 'Crop.percent')
        if a[0] < 0 or a[1] >= 0.5:
            raise ValueError("Crop.percent must lie in [0, 0.5), got %r" % (a,))
        return {'percent': a}

    def _parse_AdditiveGaussianNoise(self, q):
        a = _interval(q.get('scale', 0.0), 'AdditiveGaussianNoise.scale')
        if a[0] < 0:
            raise ValueError("AdditiveGaussianNoise.scale must not be negative, got %r" % (a,))
        return {'scale': a}

    def _parse_Fliplr(self, q):
        return {'p': self._p(q.get('p', 1.0), 'Fliplr')}

    def _parse_Flipud(self, q):
        return {'p': self._p(q.get('p', 1.0), 'Flipud')}

    # -----------------------------------------------------------------------------------------------------------------
    def sample(self, sizes, input_size, rng):
        """Draw one record for images of `sizes` [B, 2] (h, w), resized to `input_size` (width, height)."""
        sizes = _sizes(sizes)
        B = sizes.shape[0]
        color = np.zeros((B, 3), np.float64)
        noise = np.zeros(B, np.float64)
        taps = [None] * B
        matrices = np.empty((B, 3, 3))
        draws, applied = {}, {}

        def note(key, b, value):
            draws.setdefault(key, np.full((B,) + np.shape(value), np.nan))[b] = value

        def flag(key, b, value):
            applied.setdefault(key, np.zeros(B, dtype=bool))[b] = value

        def draw(iv):
            return iv[0] if iv[0] == iv[1] else float(rng.uniform(iv[0], iv[1]))

        def pair(spec, default, shared):
            """(x, y) from one interval -- one draw for both axes when `shared`, one each otherwise -- or from {x, y}"""
            if spec is None:
                return default, default
            if spec[0] == 'one':
                return (draw(spec[1]),) * 2 if shared else (draw(spec[1]), draw(spec[1]))
            return tuple(default if iv is None else draw(iv) for iv in spec[1])

        def run(steps, b, m, n_sometimes=0):
            h, w = int(sizes[b, 0]), int(sizes[b, 1])
            for name, q in steps:
                if name == 'Sometimes':
                    took = bool(rng.random() < q[0])
                    flag('Sometimes' if n_sometimes == 0 else 'Sometimes.%d' % n_sometimes, b, took)
                    n_sometimes += 1
                    if took:
                        m = run(q[1], b, m)
                elif name == 'Grayscale':
                    color[b, 0] = draw(q['alpha'])
                    note('Grayscale.alpha', b, color[b, 0])
                elif name == 'AddToHue':
                    value = draw(q['value'])
                    note('AddToHue.value', b, value)
                    color[b, 1] = value / 255.0 * 360.0
                elif name == 'AddToBrightness':
                    color[b, 2] = draw(q['add'])
                    note('AddToBrightness.add', b, color[b, 2])
                elif name == 'MotionBlur':
                    k = int(rng.integers(q['k'][0], q['k'][1] + 1))
                    angle = draw(q['angle'])
                    direction = float(rng.uniform(-1.0, 1.0)) if q['direction'] is None else draw(q['direction'])
                    note('MotionBlur.k', b, k), note('MotionBlur.angle', b, angle)
                    note('MotionBlur.direction', b, direction)
                    taps[b] = motion_blur_taps(k, angle, direction)
                elif name == 'Affine':
                    scale = pair(q['scale'], 1.0, shared=True)
                    shift = pair(q['translate_percent'], 0.0, shared=False)
                    rotate = 0.0 if q['rotate'] is None else draw(q['rotate'])
                    note('Affine.scale', b, scale), note('Affine.translate_percent', b, shift)
                    note('Affine.rotate', b, rotate)
                    m = affine_matrix(h, w, scale, shift, rotate) @ m
                elif name == 'Crop':
                    sides = [draw(q['percent']) for _ in range(4)]           # top, right, bottom, left
                    note('Crop.percent', b, sides)
                    m = crop_matrix(h, w, *sides) @ m
                elif name == 'AdditiveGaussianNoise':
                    noise[b] = draw(q['scale'])
                    note('AdditiveGaussianNoise.scale', b, noise[b])
                elif name in ('Fliplr', 'Flipud'):
                    took = bool(rng.random() < q['p'])
                    flag(name, b, took)
                    if took:
                        m = (fliplr_matrix(w) if name == 'Fliplr' else flipud_matrix(h)) @ m
            return m

        for b in range(B):
            m = run(self.steps, b, np.eye(3))
            matrices[b] = resize_matrix(int(sizes[b, 0]), int(sizes[b, 1]), input_size) @ m
        seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        out = AugmentParams.from_matrices(sizes, input_size, matrices, color=color, taps=taps, noise=noise, seed=seed)
        out.draws, out.applied = draws, applied
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _upload(device, *arrays):
    """Several small host arrays -> device tensors with ONE copy: packed into one 8-byte aligned byte buffer."""
    offsets, total = [], 0
    for a in arrays:
        offsets.append(total)
        total += (a.nbytes + 7) // 8 * 8
    host = np.zeros(total, dtype=np.uint8)
    for a, o in zip(arrays, offsets):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    dev = torch.from_numpy(host).to(device)
    return [dev[o:o + a.nbytes].view(getattr(torch, a.dtype.name)).view(a.shape) for a, o in zip(arrays, offsets)]


def _check_params(params, B, what):
    if not isinstance(params, AugmentParams):
        raise RuntimeError("%s: params must be an AugmentParams record, got %s" % (what, type(params).__name__))
    if params.batch != B:
        raise RuntimeError("%s: params describe %d images, the batch has %d" % (what, params.batch, B))


def augment_images(images, params, sizes=None):
    """images [B, H_max, W_max, 3] uint8 on the GPU (image b valid in its top-left sizes[b] = (h, w) corner; `sizes`
    defaults to params.sizes) -> [B, H_in, W_in, 3] uint8: colour, motion blur, the one warp and the noise of
    `params`."""
    require_gpu(images)
    if images.dtype != torch.uint8:
        raise RuntimeError("augment_images: images must be uint8, got %s" % images.dtype)
    if images.dim() != 4 or images.shape[3] != 3 or images.numel() == 0:
        raise RuntimeError("augment_images: images must be a non-empty [B, H, W, 3], got %s" % (tuple(images.shape),))
    B, Hmax, Wmax, _ = images.shape
    _check_params(params, B, 'augment_images')
    sizes = params.sizes if sizes is None else _sizes(sizes)
    if sizes.shape[0] != B or (sizes[:, 0] > Hmax).any() or (sizes[:, 1] > Wmax).any():
        raise RuntimeError("augment_images: sizes %s do not fit %d images of [%d, %d]"
                           % (sizes.tolist(), B, Hmax, Wmax))
    ntaps = np.asarray(params.ntaps, dtype=np.int32)
    if tuple(params.taps.shape) != (B, MAX_TAPS, 3) or ntaps.shape != (B,) or (ntaps < 1).any() \
            or (ntaps > MAX_TAPS).any():
        raise RuntimeError("augment_images: taps must be [B, %d, 3] with 1 to %d taps per image, got %s with counts %s"
                           % (MAX_TAPS, MAX_TAPS, tuple(params.taps.shape), ntaps.tolist()))
    images = images.contiguous()
    if images.data_ptr() % 4:
        images = images.clone()                       # a byte-offset view: the colour kernel loads dwords
    color = np.asarray(params.color, dtype=np.float32).reshape(B, 3)
    d_color, d_sizes, d_inv, d_taps, d_ntaps, d_noise, d_ids = _upload(
        images.device, color, sizes.astype(np.int32), np.asarray(params.inverse, dtype=np.float32).reshape(B, 6),
        np.asarray(params.taps, dtype=np.float32), ntaps, np.asarray(params.noise, dtype=np.float32).reshape(B),
        np.asarray(params.image_ids, dtype=np.int64).reshape(B))
    if color.any():                                   # not launched when no image drew a colour change
        tinted = torch.empty_like(images)
        check(lib().cnuda_augment_color(ptr(images), ptr(tinted), ptr(d_color), B, Hmax, Wmax, stream()),
              'augment_color')
        images = tinted
    W_in, H_in = params.input_size
    out = torch.empty((B, H_in, W_in, 3), dtype=torch.uint8, device=images.device)
    check(lib().cnuda_augment_warp(ptr(images), ptr(out), ptr(d_sizes), ptr(d_inv), ptr(d_taps), ptr(d_ntaps),
                                   ptr(d_noise), ptr(d_ids), int(params.seed), B, Hmax, Wmax, H_in, W_in, stream()),
          'augment_warp')
    return out


def _transform(points, boxes, params, down_ratio, what):
    require_gpu(points, boxes)
    B = (points if points is not None else boxes).shape[0]
    _check_params(params, B, what)
    forward, = _upload((points if points is not None else boxes).device,
                       np.asarray(params.forward, dtype=np.float64).reshape(B, 6) / float(down_ratio))
    N = M = 0
    p_out = b_out = None
    if points is not None:
        points = points.to(torch.float64).contiguous()
        N, p_out = points.shape[1], torch.empty_like(points)
    if boxes is not None:
        boxes = boxes.to(torch.float64).contiguous()
        M, b_out = boxes.shape[1], torch.empty_like(boxes)
    if N + M:
        check(lib().cnuda_augment_points(ptr(forward), ptr(points), ptr(p_out), N, ptr(boxes), ptr(b_out), M, B,
                                         stream()), what)
    return p_out, b_out


def _need(t, tail, what, layout):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tail or t.shape[0] < 1 \
            or not (t.dtype.is_floating_point or t.dtype in (torch.int32, torch.int64)):
        raise RuntimeError("%s must be a numeric %s, got %s" % (what, layout, tuple(getattr(t, 'shape', ())) or type(t)))


def transform_points(points, params, down_ratio=1):
    """points [B, N, 2] (u, v) in source pixels -> float64 [B, N, 2] in input pixels divided by `down_ratio`."""
    _need(points, (2,), 'transform_points: points', '[B, N, 2]')
    return _transform(points, None, params, down_ratio, 'transform_points')[0]


def transform_boxes(boxes, params, down_ratio=1):
    """boxes [B, M, 4] (x1, y1, x2, y2) in source pixels -> float64 [B, M, 4]: the bounding box of the four mapped
    corners, in input pixels divided by `down_ratio`."""
    _need(boxes, (4,), 'transform_boxes: boxes', '[B, M, 4]')
    return _transform(None, boxes, params, down_ratio, 'transform_boxes')[1]


def build_batch(images, boxes, classes, counts, *, params, input_size, num_classes, down_ratio=4, sizes=None,
                corners=None, keypoints=None, visibility=None, areas=None, mean=MEAN, std=STD, target_images=None,
                target_sizes=None, target_params=None):
    """The reference's batch dict except `id` (datasets/coco.py:242-259, 384-401, 98-111) from decoded uint8 images and
    annotations in source pixels: boxes [B, M, 4] x1, y1, x2, y2 (or `corners` [B, M, 4, 2], the `rotate_bbox`
    vertices, with boxes=None), keypoints [B, M, J, 2] with visibility [B, M, J], areas [B, M] (passed through
    unscaled).  input_size = (width, height).  `target_images` add `target_domain_input`, resized only unless
    `target_params` is given (the reference's `augment_target_domain`)."""
    if tuple(params.input_size) != (int(input_size[0]), int(input_size[1])):
        raise RuntimeError("build_batch: params were drawn for input_size %s, not %s"
                           % (tuple(params.input_size), tuple(input_size)))
    if (boxes is None) == (corners is None):
        raise RuntimeError("build_batch: give either boxes or corners (with boxes=None), not %s"
                           % ("both" if boxes is not None else "neither"))
    if (keypoints is None) != (visibility is None):
        raise RuntimeError("build_batch: keypoints and visibility must be given together")
    out = {'input': prepare_input(augment_images(images, params, sizes), mean, std)}
    output_w, output_h = int(input_size[0]) // down_ratio, int(input_size[1]) // down_ratio
    B = images.shape[0]
    clouds = []
    if corners is not None:
        _need(corners, (4, 2), 'build_batch: corners', '[B, M, 4, 2]')
        clouds.append(corners.to(torch.float64).reshape(B, -1, 2))
    if keypoints is not None:
        if keypoints.dim() != 4 or keypoints.shape[3] != 2:
            raise RuntimeError("build_batch: keypoints must be [B, M, J, 2], got %s" % (tuple(keypoints.shape),))
        clouds.append(keypoints.to(torch.float64).reshape(B, -1, 2))
    if boxes is not None:
        _need(boxes, (4,), 'build_batch: boxes', '[B, M, 4]')
    points = None if not clouds else clouds[0] if len(clouds) == 1 else torch.cat(clouds, 1)
    points, boxes = _transform(points, boxes, params, down_ratio, 'build_batch')
    if corners is not None:
        n = corners.shape[1] * 4
        corners, points = points[:, :n].reshape(corners.shape), points[:, n:]
    if keypoints is not None:
        keypoints = points.reshape(keypoints.shape)
    out.update(encode_targets(boxes, classes, counts, num_classes, output_h, output_w, corners=corners,
                              keypoints=keypoints, visibility=visibility, areas=areas))
    if target_images is not None:
        require_gpu(target_images)
        if target_params is None:
            if target_images.dim() != 4:
                raise RuntimeError("build_batch: target_images must be [B, H, W, 3], got %s"
                                   % (tuple(target_images.shape),))
            full = [[target_images.shape[1], target_images.shape[2]]] * target_images.shape[0]
            target_params = AugmentParams.identity(full if target_sizes is None else target_sizes, input_size)
        out['target_domain_input'] = prepare_input(augment_images(target_images, target_params, target_sizes), mean, std)
    return out
