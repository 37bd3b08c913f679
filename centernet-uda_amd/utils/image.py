"""`entropy_map` (utils/image.py:121-124): per-pixel, per-class normalised
entropy contribution -p*log2(p+1e-30)/log2(C) of softmax(hm), the
discriminator's input in the ADVENT plugin.

`FDA_source_to_target` (utils/image.py:137-230): Fourier domain adaptation, the source image with the amplitude of
the target's low (square mode) or all but the lowest (circular mode) frequencies, one batched HIP transform
(csrc/fda.hip).  `fda_low_freq_mask` builds, on the host, which bins take the target's amplitude.

The image-augmentation helpers of the reference's file and its numpy FDA variants are dataset-side code and not part
of this build."""
import numpy as np

from hip_runtime import ops


def entropy_map(hm):
    return ops.entropy_map(hm)


# ---------------------------------------------------------------------------
# FDA
# ---------------------------------------------------------------------------
_XY_SHIFT = 16
_XY_ONE = 1 << _XY_SHIFT


def _tdiv(a, b):
    """C integer division (truncates toward zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _clip_line(w, h, p1, p2):
    """cv::clipLine on the image scaled to fixed point; -> (visible, p1, p2)"""
    right, bottom = w - 1, h - 1
    (x1, y1), (x2, y2) = p1, p2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def _put(img, x, y):
    if 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
        img[y, x] = True


def _line8(img, p1, p2):
    """cv::Line2: an 8-connected segment between two fixed-point (XY_SHIFT) points"""
    h, w = img.shape
    ok, (x1, y1), (x2, y2) = _clip_line(w << _XY_SHIFT, h << _XY_SHIFT, p1, p2)
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    if abs(dx) > abs(dy):
        if dx < 0:
            (x1, y1), (x2, y2) = (x2, y2), (x1, y1)
            dy = -dy
        y_step = _tdiv(dy << _XY_SHIFT, abs(dx) | 1)
        ecount = (x2 - x1) >> _XY_SHIFT
    else:
        if dy < 0:
            (x1, y1), (x2, y2) = (x2, y2), (x1, y1)
            dx = -dx
        x_step = _tdiv(dx << _XY_SHIFT, abs(dy) | 1)
        ecount = (y2 - y1) >> _XY_SHIFT
    x1 += _XY_ONE >> 1
    y1 += _XY_ONE >> 1
    _put(img, (x2 + (_XY_ONE >> 1)) >> _XY_SHIFT, (y2 + (_XY_ONE >> 1)) >> _XY_SHIFT)
    if abs(dx) > abs(dy):
        x1 >>= _XY_SHIFT
        while ecount >= 0:
            _put(img, x1, y1 >> _XY_SHIFT)
            x1 += 1
            y1 += y_step
            ecount -= 1
    else:
        y1 >>= _XY_SHIFT
        while ecount >= 0:
            _put(img, x1 >> _XY_SHIFT, y1)
            x1 += x_step
            y1 += 1
            ecount -= 1


def _fill_convex_poly(img, v):
    """cv::FillConvexPoly with LINE_8 on fixed-point (XY_SHIFT) vertices: the outline, then the scanlines"""
    h, w = img.shape
    npts, delta = len(v), _XY_ONE >> 1
    p0 = v[-1]
    xmin = xmax = v[0][0]
    ymin = ymax = v[0][1]
    imin = 0
    for i, p in enumerate(v):
        if p[1] < ymin:
            ymin, imin = p[1], i
        ymax, xmax, xmin = max(ymax, p[1]), max(xmax, p[0]), min(xmin, p[0])
        _line8(img, p0, p)
        p0 = p
    xmin, xmax = (xmin + delta) >> _XY_SHIFT, (xmax + delta) >> _XY_SHIFT
    ymin, ymax = (ymin + delta) >> _XY_SHIFT, (ymax + delta) >> _XY_SHIFT
    if npts < 3 or xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    edges = npts
    edge = [dict(idx=imin, di=1, x=-_XY_ONE, dx=0, ye=ymin), dict(idx=imin, di=npts - 1, x=-_XY_ONE, dx=0, ye=ymin)]
    y = ymin
    while True:
        for e in edge:
            if y >= e['ye']:
                idx0, di = e['idx'], e['di']
                idx = idx0 + di
                if idx >= npts:
                    idx -= npts
                while edges > 0:
                    edges -= 1
                    ty = (v[idx][1] + delta) >> _XY_SHIFT
                    if ty > y:
                        xs, xe = v[idx0][0], v[idx][0]
                        e['ye'] = ty
                        e['dx'] = _tdiv((xe - xs) * 2 + (ty - y), 2 * (ty - y))
                        e['x'] = xs
                        e['idx'] = idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= npts:
                        idx -= npts
                else:
                    edges -= 1          # the C loop's `edges-- > 0` also counts the failing test
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]['x'] > edge[1]['x'] else (0, 1)
            xx1 = (edge[left]['x'] + delta) >> _XY_SHIFT
            xx2 = (edge[right]['x'] + delta) >> _XY_SHIFT
            if xx2 >= 0 and xx1 < w:
                img[y, max(xx1, 0):min(xx2, w - 1) + 1] = True
        edge[0]['x'] += edge[0]['dx']
        edge[1]['x'] += edge[1]['dx']
        y += 1
        if y > ymax:
            break


def _sin_table(deg):
    # OpenCV's SinTable: sin of whole degrees as 7-decimal float literals
    return float(np.float32(round(np.sin(np.deg2rad(deg)), 7)))


def filled_ellipse_at_origin(h, w, axes):
    """cv2.ellipse(zeros(h, w), center=(0, 0), axes, 0, 0, 360, 255, thickness=-1) > 0 as a bool [h, w] array:
    axes = (semi-axis along x = columns, semi-axis along y = rows).

    A restatement of OpenCV's rasteriser for this call (EllipseEx -> ellipse2Poly -> FillConvexPoly, LINE_8): polygon
    vertices every 90 / 30 / 18 / 5 degrees for a larger semi-axis below 3 / 10 / 15 / otherwise, rounded to 16-bit
    fixed point, duplicate neighbours dropped; then the 8-connected outline and the scanline fill, clipped to the
    image.  Written from the algorithm, not from OpenCV's code, and not compared with cv2 itself (cv2 is not a
    dependency of this build): a boundary bin may differ."""
    ax, ay = abs(int(axes[0])), abs(int(axes[1]))
    img = np.zeros((h, w), dtype=bool)
    if h <= 0 or w <= 0:
        return img
    m = max(ax, ay)
    step = 90 if m < 3 else 30 if m < 10 else 18 if m < 15 else 5
    pts = []
    for a in range(0, 360 + step, step):
        a = min(a, 360)
        x = (ax << _XY_SHIFT) * _sin_table(450 - a)
        y = (ay << _XY_SHIFT) * _sin_table(a)
        p = (int(round(x)), int(round(y)))
        if not pts or p != pts[-1]:
            pts.append(p)
    if len(pts) == 1:
        pts = [(0, 0), (0, 0)]
    _fill_convex_poly(img, pts)
    return img


def fda_low_freq_mask(h, w, L, use_circular):
    """bool [h, w]: True where FDA_source_to_target puts the TARGET's amplitude (utils/image.py:137-154).
    Square mode: b = floor(min(h, w) * L) (float64, as numpy), the four b x b corners of the spectrum.
    Circular mode: every bin OUTSIDE the quarter ellipse cv2.ellipse draws at the DC corner with axes
    (int(h L), int(w L)) -- cv2's first axis runs along x (filled_ellipse_at_origin) -- the source keeps its amplitude
    inside.  With cv2 importable, the reference's own call draws the ellipse."""
    if use_circular:
        axes = (int(h * L), int(w * L))
        try:
            import cv2
        except ImportError:
            inside = filled_ellipse_at_origin(h, w, axes)
        else:
            inside = cv2.ellipse(np.zeros((h, w, 3), np.uint8), (0, 0), axes, 0, 0, 360, (255, 255, 255), -1)[..., 0] > 0
        return ~inside
    b = int(np.floor(np.amin((h, w)) * L))
    rows = np.zeros(h, dtype=bool)
    cols = np.zeros(w, dtype=bool)
    if b > 0:
        rows[:b] = rows[h - b:] = True
        cols[:b] = cols[w - b:] = True
    return rows[:, None] & cols[None, :]


_MASKS = {}


def _device_mask(h, w, L, use_circular, device):
    key = (h, w, float(L), bool(use_circular), str(device))
    m = _MASKS.get(key)
    if m is None:
        import torch
        half = np.ascontiguousarray(fda_low_freq_mask(h, w, L, use_circular)[:, :w // 2 + 1])
        m = torch.from_numpy(half.astype(np.uint8)).to(device)
        _MASKS[key] = m
    return m


def FDA_source_to_target(src_img, trg_img, L=0.1, use_circular=False):
    """src_img with the amplitude spectrum of trg_img where fda_low_freq_mask says so, per image and channel:
    S = fft2(src), T = fft2(trg), Z = |T| S / |S| on the target bins ((|T|, 0) where |S| = 0), S elsewhere, and the
    result the reference's torch.irfft(Z, 2, onesided=False, signal_sizes=(H, W)) -- which only reads the columns
    kx <= W/2 and the real part of the DC and Nyquist columns (= torch.fft.irfft2(Z[..., :W//2+1], s=(H, W))).
    src_img, trg_img: [B, C, H, W] fp32 on the GPU, same shape, neither requiring grad (the transform is not
    differentiable here; the reference never back-propagates through it)."""
    if src_img.requires_grad or trg_img.requires_grad:
        raise RuntimeError("FDA_source_to_target is not differentiable: pass inputs that do not require grad")
    if src_img.shape != trg_img.shape or src_img.dim() != 4:
        raise ValueError("FDA_source_to_target: src_img and trg_img must be [B, C, H, W] of one shape, got %s and %s"
                         % (tuple(src_img.shape), tuple(trg_img.shape)))
    if not 0.0 <= L <= 1.0:
        raise ValueError("FDA_source_to_target: L must lie in [0, 1], got %r" % (L,))
    h, w = src_img.shape[-2:]
    return ops.fda_source_to_target(src_img, trg_img, _device_mask(h, w, L, use_circular, src_img.device))
