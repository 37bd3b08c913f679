"""Detection previews on the GPU: `Visualizer` with the reference's constructor and `visualize_detections`
(utils/visualize.py:10-49), rendered by one kernel launch instead of one imgaug / cv2 / PIL call per object.

The reference copies the normalised float batch to the host (utils/tensorboard.py:25) and paints each image twice,
predictions left and ground truth right.  Here the host only turns the detections into a flat list of integer
primitives (`build_primitives`: pure numpy); `cnuda_render_detections` (csrc/render.hip, the pixel rules are in
include/centernet_uda_hip.h and DESIGN.md section 23) denormalises the resident `input`, blends the primitives over it
in list order and leaves the finished [n, 3, H, 2W] uint8 pictures on the device, so that only bytes cross the bus.

Deliberate departures from the reference: rotated outlines are hard-edged (cv2.LINE_AA there), the text is PIL's
built-in default font (imgaug ships DejaVu), the denormalisation is float32 and clamps to [0, 255] (float64 and a
wrapping `astype(uint8)` there), and no torch / imgaug / cv2 call is made per object.
"""
import colorsys
import struct
import warnings

import numpy as np
import torch

from hip_runtime import check, lib, ptr, require_gpu, stream
from utils.box import rotate_bboxes

RECORD = 16                  # int32 words per primitive (CNUDA_RENDER_RECORD)
CHUNK = 256                  # primitives a workgroup tests and compacts per pass (CNUDA_RENDER_CHUNK)
RING, FILL, QUAD, GLYPH = 0, 1, 2, 3
PRED, GT = 0, 1              # panels
COORD_MIN, COORD_MAX = -32768, 32767
KEYPOINT_COLOR = (0, 255, 255)
BOX_THICKNESS = 2
FIRST_CHAR, LAST_CHAR = 32, 126     # the atlas holds printable ASCII, glyph index = ord(ch) - 32


def alpha_bits(alpha):
    """the record's alpha word: the bits of float32(alpha clipped to [0, 1])"""
    return struct.unpack('<i', struct.pack('<f', min(max(float(alpha), 0.0), 1.0)))[0]


def _records(rows):
    """int rows [N, RECORD] -> int32 records, the coordinates clamped to [COORD_MIN, COORD_MAX]"""
    a = np.array(rows, dtype=np.int64).reshape(-1, RECORD)
    a[:, 5:13] = np.clip(a[:, 5:13], COORD_MIN, COORD_MAX)
    return a.astype(np.int32)


def record(kind, panel, color, alpha, t, geometry):
    """-> one primitive record, int32 [RECORD]; coordinates are clamped to [COORD_MIN, COORD_MAX]"""
    row = [kind, panel, int(color[0]) | int(color[1]) << 8 | int(color[2]) << 16, alpha_bits(alpha), t]
    row += [int(v) for v in geometry]
    return _records([row + [0] * (RECORD - len(row))])[0]


def _numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _three(v, what):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size != 3:
        raise RuntimeError("Visualizer: %s must have three values, got %d" % (what, a.size))
    return [float(x) for x in a]


def render(input, index, first, prims, mean, std, atlas=None):
    """One launch of cnuda_render_detections on the current stream.  input [B, 3, H, W] float32 on the GPU; index [n],
    first [n + 1] and prims [N, RECORD] are host int32 arrays and cross in one copy; atlas is a [G, gh, gw] uint8
    tensor on the GPU or None.  -> [n, 3, H, 2W] uint8 on input's device."""
    require_gpu(input, atlas)
    if input.dtype != torch.float32 or input.dim() != 4 or input.shape[1] != 3 or input.numel() == 0:
        raise RuntimeError("render: input must be a non-empty float32 [B, 3, H, W], got %s %s"
                           % (input.dtype, tuple(input.shape)))
    input = input.contiguous()
    B, _, H, W = input.shape
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
    first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    prims = np.ascontiguousarray(prims, dtype=np.int32).reshape(-1, RECORD)
    n, N = index.size, prims.shape[0]
    if n == 0 or first.size != n + 1:
        raise RuntimeError("render: need at least one image and n + 1 range bounds, got n = %d, %d bounds" % (n, first.size))
    if index.min() < 0 or index.max() >= B:
        raise RuntimeError("render: index names an image outside the batch of %d" % B)
    if first[0] < 0 or first[-1] > N or np.any(np.diff(first) < 0):
        raise RuntimeError("render: first must rise from >= 0 to <= %d" % N)
    head = -(-(2 * n + 1) // 4) * 4                              # the records start 16-byte aligned
    host = np.zeros(head + N * RECORD, np.int32)
    host[:n], host[n:2 * n + 1], host[head:] = index, first, prims.reshape(-1)
    return launch(input, torch.from_numpy(host).to(input.device), n, N, mean, std, atlas)


def launch(input, table, n, N, mean, std, atlas=None):
    """render's device half: table is the int32 tensor [index n | first n + 1 | padding to a multiple of four words |
    prims N * RECORD] on input's device"""
    B, _, H, W = input.shape
    head = -(-(2 * n + 1) // 4) * 4
    require_gpu(table)
    if table.dtype != torch.int32 or not table.is_contiguous() or table.numel() < head + N * RECORD:
        raise RuntimeError("render: the table must be a contiguous int32 tensor of at least %d words" % (head + N * RECORD))
    if atlas is not None and atlas.numel():
        if atlas.dtype != torch.uint8 or atlas.dim() != 3:
            raise RuntimeError("render: atlas must be uint8 [G, gh, gw], got %s %s" % (atlas.dtype, tuple(atlas.shape)))
        atlas = atlas.contiguous()
        G, gh, gw = atlas.shape
    else:
        atlas, G, gh, gw = None, 0, 0, 0
    out = torch.empty((n, 3, H, 2 * W), dtype=torch.uint8, device=input.device)
    base = table.data_ptr()
    check(lib().cnuda_render_detections(ptr(input), base, base + 4 * head if N else None, base + 4 * n, ptr(atlas),
                                        ptr(out), B, n, H, W, N, G, gh, gw, *_three(mean, 'mean'), *_three(std, 'std'),
                                        stream()), 'render_detections')
    return out


def default_palette(n):
    """[n, 3] bytes: matplotlib's gist_rainbow sampled as the reference samples it (utils/visualize.py:19-21) when
    matplotlib imports, an HSV hue wheel of the same length otherwise"""
    try:
        import matplotlib
        cm = matplotlib.colormaps['gist_rainbow'] if hasattr(matplotlib, 'colormaps') else None
        if cm is None:
            from matplotlib.cm import get_cmap
            cm = get_cmap('gist_rainbow')
        rows = [[int(y * 255.0) for y in cm(1.0 * x / n)[:3]] for x in range(n)]
    except ImportError:
        rows = [[int(y * 255.0) for y in colorsys.hsv_to_rgb(1.0 * x / n, 1.0, 1.0)] for x in range(n)]
    return np.asarray(rows, dtype=np.uint8).reshape(n, 3)


_warned_no_pil = False


def default_atlas(font_size):
    """-> (coverage uint8 [95, gh, gw], advances int32 [95]): printable ASCII in PIL's built-in default font, the
    sized one where PIL offers it and the legacy bitmap font otherwise; ([0, 0, 0], [0]) with one warning without PIL"""
    global _warned_no_pil
    try:
        from PIL import Image, ImageDraw, ImageFont
    except ImportError:
        if not _warned_no_pil:
            warnings.warn("Visualizer: PIL is not importable, labels are drawn as bars without text")
            _warned_no_pil = True
        return np.zeros((0, 0, 0), np.uint8), np.zeros(0, np.int32)
    try:
        font = ImageFont.load_default(size=font_size)
    except (TypeError, OSError):
        font = ImageFont.load_default()
    chars = [chr(c) for c in range(FIRST_CHAR, LAST_CHAR + 1)]
    boxes = [font.getbbox(ch) for ch in chars]
    advances = np.asarray([max(1, int(np.ceil(font.getlength(ch)))) for ch in chars], dtype=np.int32)
    gw = int(max(max(b[2] for b in boxes), advances.max()))
    gh = int(max(b[3] for b in boxes))
    coverage = np.zeros((len(chars), gh, gw), np.uint8)
    for k, ch in enumerate(chars):
        cell = Image.new('L', (gw, gh), 0)
        ImageDraw.Draw(cell).text((0, 0), ch, fill=255, font=font)
        coverage[k] = np.asarray(cell, dtype=np.uint8)
    return coverage, advances


class Visualizer:
    def __init__(self, classes, score_threshold, mean, std, font_size=14, alpha=0.5, *, colors=None):
        self.classes = classes
        self.score_threshold = score_threshold
        self.font_size = font_size
        self.mean = mean
        self.std = std
        self.alpha = alpha
        if colors is None:
            self.cmap = default_palette(len(classes))
        else:
            self.cmap = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
        self.set_atlas(*default_atlas(font_size))

    def set_atlas(self, coverage, advances):
        """replace the glyph atlas: coverage uint8 [G, gh, gw] for the characters chr(32) .. chr(32 + G - 1), advances
        [G] in pixels"""
        coverage = np.ascontiguousarray(coverage, dtype=np.uint8)
        advances = np.asarray(advances, dtype=np.int32).reshape(-1)
        if coverage.ndim != 3 or advances.size != coverage.shape[0]:
            raise ValueError("set_atlas: coverage must be [G, gh, gw] with one advance per glyph")
        self.atlas, self.advances = coverage, advances
        self._device_atlas = {}

    def _atlas_on(self, device):
        if self.atlas.size == 0:
            return None
        key = (device.type, device.index)
        if key not in self._device_atlas:
            self._device_atlas[key] = torch.from_numpy(self.atlas).to(device)
        return self._device_atlas[key]

    # -- detections -> primitives (host, numpy; whole arrays at a time: a validation batch has thousands of glyphs) --
    def _name(self, cid):
        """the label of a class id; an id the dataset does not know ('' in the reference's Dataset.classes) is itself"""
        try:
            entry = self.classes[cid]
        except (KeyError, IndexError):
            entry = ''
        name = entry['name'] if hasattr(entry, '__getitem__') and not isinstance(entry, str) else cid
        return str(name).replace('\x00', '?')

    def _glyphs(self, texts, x1, x2):
        """-> (keep [n, L] bool, glyph [n, L], x [n, L]): the characters of every label that are drawn, their glyphs and
        cell origins.  Cells advance from x1 + 2; the first cell that would pass x2 ends its label."""
        n, G = len(texts), self.atlas.shape[0]
        L = max(len(t) for t in texts) if G else 0
        if L == 0:
            empty = np.zeros((n, 0), np.int64)
            return empty.astype(bool), empty, empty
        codes = np.frombuffer(''.join(t.ljust(L, '\x00') for t in texts).encode('latin-1', 'replace'), np.uint8)
        codes = codes.reshape(n, L).astype(np.int64)
        valid = codes != 0
        glyph = codes - FIRST_CHAR
        fallback = ord('?') - FIRST_CHAR
        glyph[(glyph < 0) | (glyph >= G)] = fallback if fallback < G else 0
        advance = np.where(valid, self.advances.astype(np.int64)[glyph], 0)
        x = (x1 + 2)[:, None] + np.cumsum(advance, 1) - advance
        fits = x + self.atlas.shape[2] - 1 <= x2[:, None]
        return valid & np.logical_and.accumulate(fits, 1), glyph, x

    def _objects(self, panel, boxes, classes, scores, rotated):
        """-> int64 [N, RECORD]: per object in array order its box, its label bar and the label's glyphs"""
        boxes = boxes.reshape(-1, boxes.shape[-1])
        classes = np.asarray(classes).reshape(-1).astype(np.int64)
        if scores is not None:
            scores = np.asarray(scores).reshape(-1)
            shown = ~(scores < self.score_threshold)              # the reference's `if score < threshold: continue`
            boxes, classes, scores = boxes[shown], classes[shown], scores[shown]
        n = boxes.shape[0]
        if n == 0:
            return np.zeros((0, RECORD), np.int64)
        if classes.min() < 0 or classes.max() >= len(self.cmap):
            bad = classes[(classes < 0) | (classes >= len(self.cmap))][0]
            raise ValueError("Visualizer: class id %d is outside the palette of %d colours" % (bad, len(self.cmap)))
        rgb = self.cmap[classes].astype(np.int64)
        color = rgb[:, 0] | rgb[:, 1] << 8 | rgb[:, 2] << 16
        names = {int(c): self._name(int(c)) for c in np.unique(classes)}
        if scores is None:
            texts = [names[c] for c in classes.tolist()]
        else:
            texts = ["%s: %.2f" % (names[c], s) for c, s in zip(classes.tolist(), scores.tolist())]
        geometry = np.zeros((n, 8), np.int64)
        with np.errstate(invalid='ignore'):
            if rotated:
                pts = np.rint(rotate_bboxes(boxes[:, :5]).astype(np.float64)).astype(np.int64)       # [n, 4, 2]
                geometry[:] = pts.reshape(n, 8)
                x1, y1, x2 = pts[:, :, 0].min(1), pts[:, :, 1].min(1), pts[:, :, 0].max(1)
                kind, alpha = QUAD, 1.0                           # the reference draws these opaque
            else:
                b = np.rint(boxes[:, :4].astype(np.float64)).astype(np.int64)
                x1, x2 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
                y1, y2 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
                geometry[:, 0], geometry[:, 1], geometry[:, 2], geometry[:, 3] = x1, y1, x2, y2
                kind, alpha = RING, self.alpha
        height = self.font_size + 4
        keep, glyph, gx = self._glyphs(texts, x1, x2)
        count = keep.sum(1)
        start = np.cumsum(2 + count) - (2 + count)                # the object's first record
        rows = np.zeros((int((2 + count).sum()), RECORD), np.int64)
        rows[:, 1] = panel
        rows[start, 0], rows[start, 2], rows[start, 3], rows[start, 4] = kind, color, alpha_bits(alpha), BOX_THICKNESS
        rows[start, 5:13] = geometry
        bar = start + 1
        rows[bar, 0], rows[bar, 2], rows[bar, 3] = FILL, color, alpha_bits(self.alpha)
        rows[bar, 5], rows[bar, 6], rows[bar, 7], rows[bar, 8] = x1, y1 - height, x2, y1 - 1
        obj, pos = np.nonzero(keep)                               # row-major: by object, then along the label
        dark = 0.299 * rgb[:, 0] + 0.587 * rgb[:, 1] + 0.114 * rgb[:, 2] < 128
        at = start[obj] + 2 + pos                                 # the kept characters of a label are its first ones
        rows[at, 0], rows[at, 2], rows[at, 3] = GLYPH, np.where(dark, 0xFFFFFF, 0)[obj], alpha_bits(1.0)
        rows[at, 4], rows[at, 5], rows[at, 6] = glyph[obj, pos], gx[obj, pos], (y1 - height + 2)[obj]
        return rows

    def _keypoints(self, panel, kps, scores):
        """-> int64 [N, RECORD]: a 3 x 3 FILL around every keypoint of the objects that are shown"""
        kps = np.asarray(kps)
        if scores is not None:
            kps = kps[~(np.asarray(scores).reshape(-1)[:kps.shape[0]] < self.score_threshold)]
        with np.errstate(invalid='ignore'):
            pts = np.rint(kps[..., :2].astype(np.float64)).astype(np.int64).reshape(-1, 2)
        rows = np.zeros((pts.shape[0], RECORD), np.int64)
        rows[:, 0], rows[:, 1], rows[:, 3] = FILL, panel, alpha_bits(self.alpha)
        rows[:, 2] = KEYPOINT_COLOR[0] | KEYPOINT_COLOR[1] << 8 | KEYPOINT_COLOR[2] << 16
        rows[:, 5], rows[:, 6], rows[:, 7], rows[:, 8] = pts[:, 0] - 1, pts[:, 1] - 1, pts[:, 0] + 1, pts[:, 1] + 1
        return rows

    def build_primitives(self, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_kps=None, pred_kps=None):
        """-> int32 [N, RECORD]: the prediction panel's objects in array order (predictions below the score threshold
        skipped; per object the box, its label bar and the label's glyphs), then that panel's keypoints, then the
        same for the ground-truth panel.  Pure numpy."""
        pred_boxes, gt_boxes = _numpy(pred_boxes), _numpy(gt_boxes)
        pred_classes, pred_scores, gt_classes = _numpy(pred_classes), _numpy(pred_scores), _numpy(gt_classes)
        rotated = gt_boxes.shape[-1] == 5                         # the reference's mode switch (utils/visualize.py:35)
        parts = [self._objects(PRED, pred_boxes, pred_classes, pred_scores, rotated)]
        if pred_kps is not None:
            parts.append(self._keypoints(PRED, _numpy(pred_kps), pred_scores))
        parts.append(self._objects(GT, gt_boxes, gt_classes, None, rotated))
        if pred_kps is not None and gt_kps is not None:
            parts.append(self._keypoints(GT, _numpy(gt_kps), None))
        return _records(np.concatenate(parts))

    # -- rendering -----------------------------------------------------------------------------------------------------
    def visualize_batch(self, input, detections, indices=None):
        """input [B, 3, H, W] float32 on the GPU, detections as uda.Model.get_detections returns them, indices the
        images to render (default: all) -> [n, 3, H, 2W] uint8 on input's device; one launch on the current stream"""
        require_gpu(input)
        indices = list(range(input.shape[0])) if indices is None else [int(i) for i in indices]
        lists = []
        for i in indices:
            lists.append(self.build_primitives(
                detections['pred_boxes'][i], detections['pred_classes'][i], detections['pred_scores'][i],
                detections['gt_boxes'][i], detections['gt_classes'][i],
                detections['gt_kps'][i] if 'gt_kps' in detections else None,
                detections['pred_kps'][i] if 'pred_kps' in detections else None))
        first = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
        prims = np.concatenate(lists) if lists else np.zeros((0, RECORD), np.int32)
        return render(input, indices, first, prims, self.mean, self.std, self._atlas_on(input.device))

    def visualize_detections(self, image, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_kps=None,
                             pred_kps=None):
        """the reference's call for one image: image [H, W, 3] float32 on the GPU -> [3, H, 2W] uint8 on the GPU"""
        require_gpu(image)
        if image.dim() != 3 or image.shape[2] != 3:
            raise RuntimeError("visualize_detections: image must be [H, W, 3], got %s" % (tuple(image.shape),))
        detections = {'pred_boxes': [pred_boxes], 'pred_classes': [pred_classes], 'pred_scores': [pred_scores],
                      'gt_boxes': [gt_boxes], 'gt_classes': [gt_classes]}
        if pred_kps is not None:
            detections['pred_kps'] = [pred_kps]
            if gt_kps is not None:
                detections['gt_kps'] = [gt_kps]
        return self.visualize_batch(image.permute(2, 0, 1).unsqueeze(0), detections)[0]
