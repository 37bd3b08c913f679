"""The student's strong view for weak/strong self-training ("Strong view"; uda.WeakStrongTeacher): colour
jitter, grayscale, gaussian blur and random erasing of a NORMALISED float32 batch [B, 3, H, W] as it sits on the device.
All four are photometric or occluding, so the boxes a teacher found on the un-augmented image stay valid.

    view = StrongView(config)                      # None: the defaults below
    params = view.sample(B, H, W, rng)             # StrongViewParams: numpy arrays, no GPU needed
    y = strong_view(x, params, mean, std)          # csrc/strongview.hip, on the current stream

The loader's augmentation (datasets/augment.py) works on uint8 images before normalisation and cannot give this view.
The operations are defined in include/centernet_uda_hip.h and follow torchvision's ColorJitter / RandomGrayscale /
GaussianBlur / RandomErasing with these departures: a fixed operation order (brightness, contrast, saturation, gray,
blur, erase), the contrast pivot is the mean luma BEFORE brightness, no hue, rectangles are filled with a unit-variance
uniform instead of a normal, the blur replicates the edges instead of reflecting them, and its radius is capped at 6."""
import collections.abc
import dataclasses
import math

import numpy as np
import torch

from hip_runtime import check, lib, ptr, stream

MAX_RADIUS = 6
TAPS = 2 * MAX_RADIUS + 1
MAX_RECTS = 3
ERASE_TRIES = 10

DEFAULTS = {
    'color_jitter': {'p': 0.8, 'brightness': 0.4, 'contrast': 0.4, 'saturation': 0.4},
    'grayscale': {'p': 0.2},
    'blur': {'p': 0.5, 'sigma': [0.1, 2.0]},
    'erase': [{'p': 0.7, 'scale': [0.05, 0.2], 'ratio': [0.3, 3.3]},
              {'p': 0.5, 'scale': [0.02, 0.2], 'ratio': [0.1, 6.0]},
              {'p': 0.3, 'scale': [0.02, 0.2], 'ratio': [0.05, 8.0]}],
}


# ---------------------------------------------------------------------------------------------------------------------
# the parameter record
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class StrongViewParams:
    """What one batch drew, as numpy arrays (B images) -- the tables of cnuda_strong_view:
    photo [B, 4] float32 (brightness, contrast, saturation factors; gray flag 0 / 1);
    taps [B, 13] float32, of which image b uses the first 2 radius[b] + 1; radius [B] int32 in 0..6;
    rects [B, 3, 4] int32 (x0, y0, x1, y1) half-open, empty when x1 <= x0 or y1 <= y0;
    ids [B] int64 the images' fill counters; seed: the fill generator's 64-bit key;
    sigma [B] float64, NaN where the image drew no blur."""
    photo: np.ndarray
    taps: np.ndarray
    radius: np.ndarray
    rects: np.ndarray
    ids: np.ndarray
    seed: int
    sigma: np.ndarray = None

    @property
    def batch(self):
        return self.photo.shape[0]

    @property
    def neutral(self):
        """[B] bool: photometrically neutral (factors 1, no gray, no blur) -- outside rectangles the image keeps its bits"""
        return (self.photo[:, :3] == 1).all(1) & (self.photo[:, 3] == 0) & (self.radius == 0)

    @property
    def erased(self):
        """[B] bool: has a non-empty rectangle"""
        r = self.rects
        return ((r[:, :, 2] > r[:, :, 0]) & (r[:, :, 3] > r[:, :, 1])).any(1)

    @classmethod
    def identity(cls, B, first_id=0):
        photo = np.tile(np.float32([1, 1, 1, 0]), (int(B), 1))
        taps = np.zeros((int(B), TAPS), dtype=np.float32)
        taps[:, 0] = 1
        return cls(photo=photo, taps=taps, radius=np.zeros(int(B), dtype=np.int32),
                   rects=np.zeros((int(B), MAX_RECTS, 4), dtype=np.int32),
                   ids=int(first_id) + np.arange(int(B), dtype=np.int64), seed=0, sigma=np.full(int(B), np.nan))


def gaussian_taps(sigma):
    """-> (radius, [13] float32): R = min(6, ceil(3 sigma)), weights exp(-k^2 / 2 sigma^2) for k = -R..R normalised in
    float64, then cast."""
    R = min(MAX_RADIUS, int(math.ceil(3.0 * float(sigma))))
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    out = np.zeros(TAPS, dtype=np.float32)
    out[:2 * R + 1] = (w / w.sum()).astype(np.float32)
    return R, out


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, collections.abc.Mapping):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, collections.abc.Sequence) and not isinstance(v, str):
        return [_plain(x) for x in v]
    return v


def _merged(given, default, where):
    """`given` over `default`, key by key; an unknown key is an error that names it."""
    if not isinstance(given, dict):
        raise ValueError("StrongView: %s must be a mapping or null, got %r" % (where, given))
    unknown = sorted(set(given) - set(default))
    if unknown:
        raise ValueError("StrongView: unknown key %s.%s (known: %s)" % (where, unknown[0], ', '.join(sorted(default))))
    return {**default, **given}


def _probability(op, where):
    p = op['p']
    if not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("StrongView: %s.p=%r outside [0, 1]" % (where, p))
    return float(p)


def _interval(v, where, positive=False):
    try:
        lo, hi = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError("StrongView: %s=%r must be an interval [lo, hi]" % (where, v)) from None
    if not lo <= hi:
        raise ValueError("StrongView: %s=%r has lo > hi" % (where, list(v)))
    if lo < 0 or (positive and lo <= 0):
        raise ValueError("StrongView: %s=%r must be %s" % (where, list(v), 'positive' if positive else 'non-negative'))
    return lo, hi


class StrongView:
    """Parses the `strong_view:` mapping (None: DEFAULTS; a key set to null turns its operation off; a given mapping is
    merged over the defaults key by key, an `erase` list entry over the default entry at its position) and draws
    batches of parameters."""

    def __init__(self, config=None):
        cfg = _merged(_plain(config) if config is not None else {}, DEFAULTS, 'strong_view')
        self.color_jitter = self.grayscale = self.blur = None
        self.erase = []
        if cfg['color_jitter'] is not None:
            op = _merged(cfg['color_jitter'], DEFAULTS['color_jitter'], 'color_jitter')
            amounts = {}
            for k in ('brightness', 'contrast', 'saturation'):
                a = op[k]
                if not isinstance(a, (int, float)) or not float(a) >= 0.0:
                    raise ValueError("StrongView: color_jitter.%s=%r is negative" % (k, a))
                amounts[k] = (max(0.0, 1.0 - float(a)), 1.0 + float(a))         # factors uniform in [1 - a, 1 + a]
            self.color_jitter = dict(p=_probability(op, 'color_jitter'), **amounts)
        if cfg['grayscale'] is not None:
            op = _merged(cfg['grayscale'], DEFAULTS['grayscale'], 'grayscale')
            self.grayscale = dict(p=_probability(op, 'grayscale'))
        if cfg['blur'] is not None:
            op = _merged(cfg['blur'], DEFAULTS['blur'], 'blur')
            if isinstance(op['sigma'], (int, float)) and not float(op['sigma']) > 0.0:
                raise ValueError("StrongView: blur.sigma=%r must be positive" % (op['sigma'],))
            sigma = [op['sigma']] * 2 if isinstance(op['sigma'], (int, float)) else op['sigma']
            self.blur = dict(p=_probability(op, 'blur'), sigma=_interval(sigma, 'blur.sigma', positive=True))
        if cfg['erase'] is not None:
            if not isinstance(cfg['erase'], list):
                raise ValueError("StrongView: erase must be a list or null, got %r" % (cfg['erase'],))
            if len(cfg['erase']) > MAX_RECTS:
                raise ValueError("StrongView: erase lists %d entries, at most %d" % (len(cfg['erase']), MAX_RECTS))
            for i, entry in enumerate(cfg['erase']):
                where = 'erase[%d]' % i
                op = _merged(entry, DEFAULTS['erase'][i], where)
                self.erase.append(dict(p=_probability(op, where), scale=_interval(op['scale'], where + '.scale'),
                                       ratio=_interval(op['ratio'], where + '.ratio', positive=True)))

    @staticmethod
    def _rectangle(H, W, scale, ratio, rng):
        """torchvision's RandomErasing.get_params: up to ten tries for a rectangle that is smaller than the image in both
        directions -> (x0, y0, x1, y1), or the empty rectangle."""
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        for _ in range(ERASE_TRIES):
            area = H * W * rng.uniform(scale[0], scale[1])
            r = math.exp(rng.uniform(log_ratio[0], log_ratio[1]))
            h, w = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if not (h < H and w < W):
                continue
            i, j = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            return j, i, j + w, i + h
        return 0, 0, 0, 0

    def sample(self, B, H, W, rng, first_id=0):
        """One batch's parameters, a function of (config, B, H, W, the state of `rng`, first_id) alone."""
        B, H, W = int(B), int(H), int(W)
        if B < 1 or H < 1 or W < 1:
            raise ValueError("StrongView.sample: B, H, W must be positive, got (%d, %d, %d)" % (B, H, W))
        out = StrongViewParams.identity(B, first_id)
        for b in range(B):
            if self.color_jitter is not None and rng.random() < self.color_jitter['p']:
                for c, k in enumerate(('brightness', 'contrast', 'saturation')):
                    out.photo[b, c] = rng.uniform(*self.color_jitter[k])
            if self.grayscale is not None and rng.random() < self.grayscale['p']:
                out.photo[b, 3] = 1
            if self.blur is not None and rng.random() < self.blur['p']:
                out.sigma[b] = rng.uniform(*self.blur['sigma'])
                out.radius[b], out.taps[b] = gaussian_taps(out.sigma[b])
            for i, op in enumerate(self.erase):
                if rng.random() < op['p']:
                    out.rects[b, i] = self._rectangle(H, W, op['scale'], op['ratio'], rng)
        out.seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _three(v, what):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size != 3:
        raise RuntimeError("strong_view: %s must have three values, got %d" % (what, a.size))
    return a


def _check_x(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or x.numel() == 0:
        raise RuntimeError("%s: x must be a non-empty float32 [B, 3, H, W], got %s %s"
                           % (what, getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))
    if not x.is_contiguous():
        raise RuntimeError("%s: x must be contiguous, got strides %s for shape %s"
                           % (what, tuple(x.stride()), tuple(x.shape)))
    if x.requires_grad:
        raise RuntimeError("%s: x requires grad; the view is not differentiable (detach it)" % what)


def _check_normalisation(mean, std):
    mean, std = _three(mean, 'mean'), _three(std, 'std')
    if not (std != 0).all():
        raise RuntimeError("strong_view: std=%s has a zero" % std.tolist())
    return mean, std


def _require_gpu(x, what):
    if not x.is_cuda:
        raise RuntimeError("%s: x is a %s tensor; centernet-uda_amd ops run on MI355X only (there is no CPU fallback)"
                           % (what, x.device))


def _pivot(x, d_mean, d_std):
    B, _, H, W = x.shape
    pivot = torch.empty(B, dtype=torch.float32, device=x.device)
    work = torch.empty(2 * B, dtype=torch.int64, device=x.device)
    check(lib().cnuda_strong_view_pivot(ptr(x), ptr(d_mean), ptr(d_std), ptr(pivot), ptr(work), B, H, W, stream()),
          'strong_view_pivot')
    return pivot


def strong_view_pivot(x, mean, std):
    """x [B, 3, H, W] float32 on the GPU -> [B] float32: every image's contrast pivot, the mean luma of the de-normalised
    image from an exact integer sum (cnuda_strong_view_pivot)."""
    from .augment import _upload
    _check_x(x, 'strong_view_pivot')
    mean, std = _check_normalisation(mean, std)
    _require_gpu(x, 'strong_view_pivot')
    return _pivot(x, *_upload(x.device, mean, std))


def strong_view(x, params, mean, std, out=None):
    """x [B, 3, H, W] float32 on the GPU, contiguous, normalised with (mean, std) -> the strong view of `params`, a new
    tensor (or `out`: a contiguous float32 tensor of x's shape that does not overlap it); x is not written.  When no
    image of the batch draws anything and no `out` is given, nothing is launched and x itself comes back."""
    from .augment import _upload
    _check_x(x, 'strong_view')
    B, _, H, W = x.shape
    if not isinstance(params, StrongViewParams):
        raise RuntimeError("strong_view: params must be a StrongViewParams record, got %s" % type(params).__name__)
    if params.batch != B:
        raise RuntimeError("strong_view: params describe %d images, the batch x has %d" % (params.batch, B))
    radius = np.asarray(params.radius, dtype=np.int32).reshape(-1)
    if tuple(params.taps.shape) != (B, TAPS) or radius.shape != (B,) or (radius < 0).any() or (radius > MAX_RADIUS).any():
        raise RuntimeError("strong_view: params.taps must be [B, %d] with params.radius in 0..%d, got %s with radii %s"
                           % (TAPS, MAX_RADIUS, tuple(params.taps.shape), radius.tolist()))
    mean, std = _check_normalisation(mean, std)
    if out is not None and (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != x.device):
        raise RuntimeError("strong_view: out must be a contiguous float32 %s on %s" % (tuple(x.shape), x.device))
    _require_gpu(x, 'strong_view')
    if out is None and params.neutral.all() and not params.erased.any():
        return x
    photo = np.asarray(params.photo, dtype=np.float32).reshape(B, 4)
    tables = _upload(x.device, mean, std, photo, np.asarray(params.taps, dtype=np.float32), radius,
                     np.asarray(params.rects, dtype=np.int32).reshape(B, MAX_RECTS, 4),
                     np.asarray(params.ids, dtype=np.int64).reshape(B))
    return _launch(x, torch.empty_like(x) if out is None else out, tables, int(radius.max()), params.seed,
                   bool((photo[:, 1] != 1).any()))


def _launch(x, y, tables, max_radius, seed, contrast):
    """The launches behind strong_view, on uploaded tables (mean, std, photo, taps, radius, rects, ids).  contrast: some
    image has a contrast factor -- only then is the pivot launched; otherwise its table stays unwritten and unread."""
    B, _, H, W = x.shape
    d_mean, d_std = tables[:2]
    pivot = _pivot(x, d_mean, d_std) if contrast else torch.empty(B, dtype=torch.float32, device=x.device)
    d_photo, d_taps, d_radius, d_rects, d_ids = tables[2:]
    check(lib().cnuda_strong_view(ptr(x), ptr(y), ptr(d_mean), ptr(d_std), ptr(d_photo), ptr(d_taps), ptr(d_radius),
                                  int(max_radius), ptr(d_rects), ptr(d_ids), int(seed) & (2 ** 64 - 1), ptr(pivot),
                                  B, H, W, stream()), 'strong_view')
    return y
