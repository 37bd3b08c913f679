"""The student's geometric view for self-training ("Geometric view"; uda.GeometricTeacher): a rotation, an
isotropic change of scale and a shift of a NORMALISED float32 batch [B, C, H, W] as it sits on the device, about the
image centre -- a similarity transform, under which a rotated rectangle stays a rectangle.

    view = GeometricView(config)                   # None: the defaults below
    params = view.sample(B, H, W, rng)             # GeometricViewParams: numpy arrays, no GPU needed
    y = warp_batch(x, params.inverse)              # csrc/geomview.hip, on the current stream
    labels = hip_runtime.ops.transform_labels(labels, params.forward_map(down_ratio), map_h, map_w, ...)

Coordinates are those of datasets/augment.py: pixel (row i, column j) has its centre at (j + 0.5, i + 0.5), matrices are
3 x 3 float64 acting on columns (x, y, 1), `forward` maps source pixel coordinates to view coordinates and a mirror is
fliplr_matrix(W).  The loader's warp (csrc/augment.hip) works on uint8 source images before normalisation and cannot give
this view.

Labels.  A rotated-box model takes ANY angle without loss (`rotate: [-180, 180]`): the four corners are mapped point by
point.  An axis-aligned model gets the bounding box of the four mapped corners, the loader's `transform_boxes` rule; that
box grows with the angle (by a factor of up to 2 in area for a square at 45 degrees), so the default interval is small."""
import dataclasses
import math

import numpy as np
import torch

from hip_runtime import check, lib, ptr, stream

from .augment import fliplr_matrix
from .strong_view import _plain, _require_gpu

DEFAULTS = {'p': 1.0, 'rotate': [-15, 15], 'scale': [0.8, 1.25], 'translate_percent': [-0.1, 0.1]}


def similarity_matrices(h, w, rotate=0.0, scale=1.0, translate_percent=(0.0, 0.0)):
    """-> (forward, inverse), 3 x 3 float64: scale (isotropic), then rotate (degrees, positive = clockwise on the y-down
    image, as datasets.augment.affine_matrix) about the image centre (w/2, h/2), then shift by a fraction of the width /
    height.  At a multiple of 90 degrees the cosine and the sine are exactly 0 or +-1, so that a quarter turn resamples
    without interpolation.  The inverse is built from the same numbers, not by elimination."""
    quarter = float(rotate) / 90.0
    if quarter == math.floor(quarter):
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
    else:
        t = math.radians(float(rotate))
        c, s = math.cos(t), math.sin(t)
    k = float(scale)
    if not k > 0.0:
        raise ValueError("similarity_matrices: scale=%r must be positive" % (scale,))
    # (plain floats: sixteen images a step are drawn on the host, and small-array numpy would cost more than the warp)
    a, b = c * k, s * k
    ai, bi = c / k, s / k
    cx, cy = w / 2.0, h / 2.0
    sx, sy = float(translate_percent[0]) * w, float(translate_percent[1]) * h
    px, py = cx + sx, cy + sy
    forward = np.array([[a, -b, (cx - (a * cx - b * cy)) + sx], [b, a, (cy - (b * cx + a * cy)) + sy], [0.0, 0.0, 1.0]])
    inverse = np.array([[ai, bi, cx - (ai * px + bi * py)], [-bi, ai, cy - (ai * py - bi * px)], [0.0, 0.0, 1.0]])
    return forward + 0.0, inverse + 0.0                           # (+ 0.0: no negative zero among the entries)


# ---------------------------------------------------------------------------------------------------------------------
# the parameter record
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class GeometricViewParams:
    """What one batch drew, as numpy arrays (B images): forward [B, 3, 3] float64 (source pixel coordinates -> view
    coordinates), inverse [B, 3, 3] float64, drawn [B] bool; and what was drawn, for the record: rotate [B] (degrees),
    scale [B], translate_percent [B, 2] (0, 1 and (0, 0) where nothing was)."""
    forward: np.ndarray
    inverse: np.ndarray
    drawn: np.ndarray
    rotate: np.ndarray = None
    scale: np.ndarray = None
    translate_percent: np.ndarray = None

    @property
    def batch(self):
        return self.forward.shape[0]

    @property
    def neutral(self):
        """[B] bool: the image's matrix is exactly the identity -- the warp copies it, the labels keep every row"""
        eye = np.eye(3)
        return (self.forward == eye).all((1, 2)) & (self.inverse == eye).all((1, 2))

    @classmethod
    def identity(cls, B):
        B = int(B)
        return cls(forward=np.tile(np.eye(3), (B, 1, 1)), inverse=np.tile(np.eye(3), (B, 1, 1)),
                   drawn=np.zeros(B, dtype=bool), rotate=np.zeros(B), scale=np.ones(B), translate_percent=np.zeros((B, 2)))

    def mirrored(self, W):
        """-> (forward . F, F . inverse) with F = fliplr_matrix(W), its own inverse: the view of the MIRRORED image, for a
        student that sees the mirror of what the teacher labelled.  The mirror costs no launch of its own; with a neutral
        image the result is F exactly, whose weights are 0."""
        F = fliplr_matrix(W)
        return self.forward @ F + 0.0, F @ self.inverse + 0.0

    def forward_map(self, down_ratio):
        """[B, 6] float64: `forward` at output-map resolution -- the same linear part, the translation divided by
        `down_ratio` (the coordinate convention has no half-pixel term, so this is exact)."""
        m = np.array(self.forward[:, :2, :], dtype=np.float64)
        m[:, :, 2] /= float(down_ratio)
        return m.reshape(-1, 6)


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _interval(v, where, positive=False):
    try:
        lo, hi = (float(t) for t in v)
    except (TypeError, ValueError):
        raise ValueError("GeometricView: %s=%r must be an interval [lo, hi]" % (where, v)) from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("GeometricView: %s=%r is not finite" % (where, list(v)))
    if not lo <= hi:
        raise ValueError("GeometricView: %s=%r has lo > hi" % (where, list(v)))
    if positive and lo <= 0:
        raise ValueError("GeometricView: %s=%r must be positive" % (where, list(v)))
    return lo, hi


class GeometricView:
    """Parses the `geometric_view:` mapping (None: DEFAULTS; a component -- rotate, scale, translate_percent -- set to null
    is off; a given mapping is merged over the defaults) and draws batches of parameters.  Per image, in this order: one
    uniform against `p`, then for every component that is on one uniform in its interval (two for translate_percent, x
    then y).  `scale` is isotropic, one draw per image.  With every component off nothing is drawn at all."""

    def __init__(self, config=None):
        given = _plain(config) if config is not None else {}
        if not isinstance(given, dict):
            raise ValueError("GeometricView: geometric_view must be a mapping or null, got %r" % (given,))
        unknown = sorted(set(given) - set(DEFAULTS))
        if unknown:
            raise ValueError("GeometricView: unknown key geometric_view.%s (known: %s)"
                             % (unknown[0], ', '.join(sorted(DEFAULTS))))
        cfg = {**DEFAULTS, **given}
        p = 1.0 if cfg['p'] is None else cfg['p']
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
            raise ValueError("GeometricView: p=%r outside [0, 1]" % (p,))
        self.p = float(p)
        self.rotate = None if cfg['rotate'] is None else _interval(cfg['rotate'], 'rotate')
        self.scale = None if cfg['scale'] is None else _interval(cfg['scale'], 'scale', positive=True)
        self.translate_percent = (None if cfg['translate_percent'] is None
                                  else _interval(cfg['translate_percent'], 'translate_percent'))

    @property
    def off(self):
        return self.rotate is None and self.scale is None and self.translate_percent is None

    def sample(self, B, H, W, rng):
        """One batch's parameters, a function of (config, B, H, W, the state of `rng`) alone."""
        B, H, W = int(B), int(H), int(W)
        if B < 1 or H < 1 or W < 1:
            raise ValueError("GeometricView.sample: B, H, W must be positive, got (%d, %d, %d)" % (B, H, W))
        out = GeometricViewParams.identity(B)
        if self.off:
            return out
        for b in range(B):
            if not rng.random() < self.p:
                continue
            out.drawn[b] = True
            if self.rotate is not None:
                out.rotate[b] = rng.uniform(*self.rotate)
            if self.scale is not None:
                out.scale[b] = rng.uniform(*self.scale)
            if self.translate_percent is not None:
                out.translate_percent[b] = (rng.uniform(*self.translate_percent), rng.uniform(*self.translate_percent))
            out.forward[b], out.inverse[b] = similarity_matrices(H, W, out.rotate[b], out.scale[b],
                                                                 out.translate_percent[b])
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _check_x(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] < 1 or x.dtype != torch.float32 or x.numel() == 0:
        raise RuntimeError("%s: x must be a non-empty float32 [B, C, H, W], got %s %s"
                           % (what, getattr(x, 'dtype', type(x).__name__), tuple(getattr(x, 'shape', ()))))
    if not x.is_contiguous():
        raise RuntimeError("%s: x must be contiguous, got strides %s for shape %s"
                           % (what, tuple(x.stride()), tuple(x.shape)))
    if x.requires_grad:
        raise RuntimeError("%s: x requires grad; the view is not differentiable (detach it)" % what)


def warp_batch(x, inverse, fill=0.0, out=None):
    """x [B, C, H, W] float32 on the GPU, contiguous -> its bilinear resampling under inverse [B, 3, 3] (or [B, 2, 3], or
    [B, 6]) float64, which maps output pixel centres to source positions (cnuda_warp_bilinear; the arithmetic is written
    out in include/centernet_uda_hip.h).  A tap outside the image has the value `fill` (0: the mean colour of a
    normalised batch).  -> a new tensor (or `out`: a contiguous float32 tensor of x's shape that does not overlap it); x
    is not written.  An image whose matrix is exactly the identity is copied; when every image's is and no `out` is given,
    nothing is launched and x itself comes back."""
    from .augment import _upload
    _check_x(x, 'warp_batch')
    B = x.shape[0]
    m = np.asarray(inverse, dtype=np.float64)
    if m.shape == (B, 3, 3):
        if not (m[:, 2] == (0.0, 0.0, 1.0)).all():
            raise RuntimeError("warp_batch: inverse must be affine (last row 0, 0, 1)")
        m = m[:, :2]
    if m.size != 6 * B or m.shape[0] != B:
        raise RuntimeError("warp_batch: inverse must be [%d, 3, 3], [%d, 2, 3] or [%d, 6], got %s"
                           % (B, B, B, tuple(np.shape(inverse))))
    m = np.ascontiguousarray(m.reshape(B, 6))
    if not np.isfinite(m).all() or not math.isfinite(float(fill)):
        raise RuntimeError("warp_batch: inverse and fill must be finite")
    if out is not None and (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != x.device):
        raise RuntimeError("warp_batch: out must be a contiguous float32 %s on %s" % (tuple(x.shape), x.device))
    _require_gpu(x, 'warp_batch')
    if out is None and (m == np.float64([1, 0, 0, 0, 1, 0])).all():
        return x
    d_inverse, = _upload(x.device, m)
    y = torch.empty_like(x) if out is None else out
    _, C, H, W = x.shape
    check(lib().cnuda_warp_bilinear(ptr(x), ptr(y), ptr(d_inverse), float(fill), B, C, H, W, stream()), 'warp_bilinear')
    return y
