"""Run a trained model over images: detections in source-image pixels, with mirror and multi-scale test-time
augmentation ("Prediction").

    python predict.py RUN_DIR IMAGE_OR_DIR_OR_GLOB... [--out results.json] [--best] [--teacher]
        [--flip] [--scales 0.75,1,1.25] [--soft-nms] [--polygon-nms] [--score-threshold T]
        [--batch-size N] [--num-workers N] [--gpu I] [--annotation-file F]
        [--flip-pairs 1-2,3-4]

RUN_DIR is a run directory of train.py: its `.hydra/config.yaml` names the backend, `input_size`, `normalize`,
`max_detections`, `score_threshold`, `rotated_boxes` and the default batch size and worker count; `model_last.pth` (or
`model_best.pth` with --best) holds the weights.  The result is a COCO results file.

As a library:

    predictor = Predictor(backend, input_size, flip=True, scales=(0.75, 1, 1.25))
    out = predictor(images, sizes)          # padded uint8 [B, Hmax, Wmax, 3] on the GPU, sizes [B, 2] (h, w) on the host
    for record in predict_files(predictor, files, batch_size=16, num_workers=16, device=device): ...

Per scale the images are stretched to the network size by `augment_images(AugmentParams.identity(...))` and
`prepare_input` (the validation loader's resize: no aspect-preserving padding), the mirrors -- with `flip` -- ride in
the same 2B forward and `cnuda_tta_merge` folds the two halves of the head maps, `decode_detection` picks the K best and
`cnuda_project_detections` maps them through the float64 inverse of the resize matrix into source pixels.  Several
scales (or `soft_nms=True`) end in `cnuda_soft_nms_merge`; a rotated model takes `soft_nms='polygon'` instead, alone or
with several scales, and ends in `cnuda_soft_nms_merge_rotated` (the same merge on the projected vertices, with the
exact polygon IoU).  The call reads nothing back; apart from the kernels named here no torch compute kernel runs
between the uint8 batch and the result.
"""
import argparse
import glob as globlib
import json
import logging
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

PKG = os.path.dirname(os.path.abspath(__file__))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import hip_runtime as hr   # noqa: E402
from datasets.prepare import MEAN, STD   # noqa: E402

log = logging.getLogger("predict")

IMAGE_EXTENSIONS = ('.bmp', '.jpeg', '.jpg', '.png', '.tif', '.tiff', '.webp')
MAX_CANDIDATES = 2048            # CNUDA_SOFT_NMS_MAX_CANDIDATES (include/centernet_uda_hip.h)


# ---------------------------------------------------------------------------------------------------------------------
# host-side rules (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def scale_size(side, scale):
    """The network's side for `scale`: the nearest multiple of 32 (halves up) of scale * side, at least 64."""
    return max(64, 32 * int(math.floor(float(scale) * side / 32.0 + 0.5)))


def flip_permutation(flip_pairs, J):
    """-> int32 [J]: the joint that takes joint j's place in a mirrored image (identity without pairs).  ValueError
    unless `flip_pairs` are disjoint pairs of distinct joints below J."""
    perm = np.arange(J, dtype=np.int32)
    seen = set()
    for pair in (flip_pairs or ()):
        pair = tuple(pair)
        if len(pair) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in pair):
            raise ValueError("flip_pairs: %r is not a pair of joint indices" % (pair,))
        a, b = int(pair[0]), int(pair[1])
        if not (0 <= a < J and 0 <= b < J):
            raise ValueError("flip_pairs: (%d, %d) names a joint outside [0, %d)" % (a, b, J))
        if a == b or a in seen or b in seen:
            raise ValueError("flip_pairs: (%d, %d) repeats a joint; the pairs must be disjoint" % (a, b))
        seen.update((a, b))
        perm[a], perm[b] = b, a
    return perm


def inverse_matrices(params):
    """AugmentParams -> float64 [B, 6]: input pixels -> source pixels, the float64 inverse of `params.forward`."""
    B = params.batch
    full = np.tile(np.eye(3), (B, 1, 1))
    full[:, :2] = np.asarray(params.forward, dtype=np.float64).reshape(B, 2, 3)
    return np.ascontiguousarray(np.linalg.inv(full)[:, :2].reshape(B, 6))


def expand_files(paths):
    """Files, directories (their image files, not recursive) and glob patterns -> one sorted list without repeats."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    out = set()
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            found = [os.path.join(p, f) for f in os.listdir(p) if f.lower().endswith(IMAGE_EXTENSIONS)]
            found = [f for f in found if os.path.isfile(f)]
        elif os.path.isfile(p):
            found = [p]
        else:
            found = [f for f in globlib.glob(p) if os.path.isfile(f)]
            if not found:
                raise FileNotFoundError("%s is no file, no directory and matches nothing" % p)
        out.update(found)
    return sorted(out)


def image_ids_from_annotations(annotation_file):
    """A COCO annotation file's `file_name -> id` table."""
    with open(annotation_file) as f:
        return {im['file_name']: im['id'] for im in json.load(f).get('images', [])}


def coco_results(records, image_ids=None):
    """Records of predict_files -> the COCO results list.  category_id = label + 1 (datasets.coco's mapping); bbox
    [x, y, w, h]; rotated models (boxes [n, 4, 2]) add `segmentation` and take the polygon's bounds as bbox; keypoints
    as [x, y, 1, ...].  image_id: `image_ids[file name]` (base name, then the path as given) or, without a table, the
    1-based position of the record."""
    out = []
    for n, r in enumerate(records):
        if image_ids is None:
            image_id = int(r.get('index', n)) + 1
        else:
            name = os.path.basename(r['file'])
            if name not in image_ids and r['file'] not in image_ids:
                raise KeyError("%s is not an image of the annotation file" % r['file'])
            image_id = image_ids[name] if name in image_ids else image_ids[r['file']]
        boxes = np.asarray(r['boxes'], dtype=np.float64)
        kps = r.get('kps')
        for i in range(boxes.shape[0]):
            det = {'image_id': image_id, 'category_id': int(r['classes'][i]) + 1}
            if boxes.ndim == 3:
                poly = boxes[i]
                x1, y1, x2, y2 = poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()
                det['segmentation'] = [[float(v) for v in poly.reshape(-1)]]
            else:
                x1, y1, x2, y2 = boxes[i]
            det['bbox'] = [float(x1), float(y1), float(x2 - x1), float(y2 - y1)]
            det['score'] = float(r['scores'][i])
            if kps is not None:
                det['keypoints'] = [float(v) for p in np.asarray(kps[i], dtype=np.float64) for v in (p[0], p[1], 1.0)]
            out.append(det)
    return out


def write_coco_results(records, path, *, image_ids=None):
    results = coco_results(records, image_ids)
    with open(path, 'w') as f:
        json.dump(results, f)
    return results


# ---------------------------------------------------------------------------------------------------------------------
# the three device steps (csrc/predict.hip)
# ---------------------------------------------------------------------------------------------------------------------
def mirror_input(x, out=None):
    """[..., H, W] float32 -> its exact left-right mirror."""
    hr.require_gpu(x, out)
    x = hr.f32c(x)
    if x.dim() < 2 or x.numel() == 0:
        raise RuntimeError("mirror_input: expected a non-empty [..., H, W] tensor, got %s" % (tuple(x.shape),))
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("mirror_input: out must be a contiguous float32 %s" % (tuple(x.shape),))
    H, W = x.shape[-2:]
    hr.check(hr.lib().cnuda_mirror_input(hr.ptr(x), hr.ptr(out), x.numel() // (H * W), H, W, hr.stream()), 'mirror_input')
    return out


def tta_merge(heads, perm=None):
    """heads: the raw output dict of a 2B batch (images, then their mirrors) -> the merged dict of B images; 'hm' comes
    back as clamped probabilities, ready for decode_detection.  perm: int32 [J] device tensor (flip_permutation)."""
    hm, wh = hr.f32c(heads['hm']), hr.f32c(heads['wh'])
    reg = hr.f32c(heads['reg']) if heads.get('reg') is not None else None
    kps = hr.f32c(heads['kps']) if heads.get('kps') is not None else None
    hr.require_gpu(hm, wh, reg, kps, perm)
    B2, C, H, W = hm.shape
    if B2 % 2:
        raise RuntimeError("tta_merge: the batch holds images and their mirrors, got %d maps" % B2)
    B, J = B2 // 2, 0 if kps is None else kps.shape[1] // 2
    for name, t in (('wh', wh), ('reg', reg), ('kps', kps)):
        if t is not None and (t.dim() != 4 or t.shape[0] != B2 or tuple(t.shape[2:]) != (H, W)):
            raise RuntimeError("tta_merge: %s %s does not match hm %s" % (name, tuple(t.shape), tuple(hm.shape)))
    if kps is not None and (kps.shape[1] % 2 or J == 0):
        raise RuntimeError("tta_merge: kps must have 2J channels, got %d" % kps.shape[1])
    if perm is not None and (kps is None or perm.dtype != torch.int32 or tuple(perm.shape) != (J,)
                             or not perm.is_contiguous()):
        raise RuntimeError("tta_merge: perm must be an int32 [J] tensor beside a kps head")
    new = lambda t: None if t is None else torch.empty((B,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    out = {'hm': new(hm), 'wh': new(wh), 'reg': new(reg), 'kps': new(kps)}
    hr.check(hr.lib().cnuda_tta_merge(hr.ptr(hm), hr.ptr(wh), hr.ptr(reg), hr.ptr(kps), hr.ptr(perm), hr.ptr(out['hm']),
                                      hr.ptr(out['wh']), hr.ptr(out['reg']), hr.ptr(out['kps']), B, C, wh.shape[1], J, H,
                                      W, hr.stream()), 'tta_merge')
    return {k: v for k, v in out.items() if v is not None}


def _result_buffers(B, K, J, rotated, device):
    """One float32 allocation behind every output (all are 4-byte types): a result crosses to the host in one copy."""
    nbox = 8 if rotated else 4
    parts = [('boxes', B * K * nbox), ('scores', B * K), ('classes', B * K), ('counts', B), ('kps', B * K * J * 2)]
    packed = torch.empty(sum((n + 3) // 4 * 4 for _, n in parts), dtype=torch.float32, device=device)
    views, at = {}, 0
    for name, n in parts:
        views[name] = packed[at:at + n]
        at += (n + 3) // 4 * 4                        # 16-byte aligned parts
    out = {'boxes': views['boxes'].view((B, K, 4, 2) if rotated else (B, K, 4)), 'scores': views['scores'].view(B, K),
           'classes': views['classes'].view(torch.int32).view(B, K), 'counts': views['counts'].view(torch.int32),
           'packed': packed}
    if J:
        out['kps'] = views['kps'].view(B, K, J, 2)
    return out


def unpack_result(packed, B, K, J, rotated):
    """The host copy of a result's `packed` buffer (numpy float32) -> the dict of numpy arrays."""
    nbox, at, out = 8 if rotated else 4, 0, {}
    for name, n, dtype, shape in (('boxes', B * K * nbox, np.float32, (B, K, 4, 2) if rotated else (B, K, 4)),
                                  ('scores', B * K, np.float32, (B, K)), ('classes', B * K, np.int32, (B, K)),
                                  ('counts', B, np.int32, (B,)), ('kps', B * K * J * 2, np.float32, (B, K, J, 2))):
        if n:
            out[name] = packed[at:at + n].view(dtype).reshape(shape)
        at += (n + 3) // 4 * 4
    return out


def project_detections(dets, kps, matrix, sizes, threshold, rotated=False, scale=1.0, out=None, first=0):
    """dets [B, K, 6|7] and kps [B, K, J, 2] (or None) as decode_detection leaves them, times `scale` -> source pixels
    through matrix [B, 6] float64 (device), clipped to sizes [B, 2] int32 (device) when axis-aligned.  -> dict of boxes,
    scores, classes, counts (kps).  `out`: a dict of such tensors with at least first + K rows per image to write rows
    first .. first + K - 1 of (one candidate table for several scales)."""
    hr.require_gpu(dets, kps, matrix, sizes)
    dets = hr.f32c(dets)
    kps = None if kps is None else hr.f32c(kps)
    ncol = 7 if rotated else 6
    if dets.dim() != 3 or dets.shape[2] != ncol or dets.numel() == 0:
        raise RuntimeError("project_detections: dets must be a non-empty [B, K, %d], got %s" % (ncol, tuple(dets.shape)))
    B, K, _ = dets.shape
    J = 0 if kps is None else kps.shape[2]
    if kps is not None and (kps.dim() != 4 or tuple(kps.shape[:2]) != (B, K) or kps.shape[3] != 2 or J == 0):
        raise RuntimeError("project_detections: kps must be [B, K, J, 2], got %s" % (tuple(kps.shape),))
    if matrix.dtype != torch.float64 or tuple(matrix.shape) != (B, 6) or not matrix.is_contiguous():
        raise RuntimeError("project_detections: matrix must be a contiguous float64 [B, 6]")
    if sizes.dtype != torch.int32 or tuple(sizes.shape) != (B, 2) or not sizes.is_contiguous():
        raise RuntimeError("project_detections: sizes must be a contiguous int32 [B, 2]")
    if out is None:
        out = _result_buffers(B, K, J, rotated, dets.device)
    rows = out['scores'].shape[1]
    want = (B, rows, 4, 2) if rotated else (B, rows, 4)
    if tuple(out['boxes'].shape) != want or tuple(out['classes'].shape) != (B, rows) or first < 0 or first + K > rows \
            or (J and tuple(out['kps'].shape) != (B, rows, J, 2)):
        raise RuntimeError("project_detections: out does not hold rows %d..%d of %d images" % (first, first + K, B))
    hr.check(hr.lib().cnuda_project_detections(
        hr.ptr(dets), hr.ptr(kps), hr.ptr(matrix), hr.ptr(sizes), hr.ptr(out['boxes']), hr.ptr(out['scores']),
        hr.ptr(out['classes']), hr.ptr(out['kps']) if J else None, hr.ptr(out['counts']), B, K, J, 1 if rotated else 0,
        float(scale), float(np.float32(threshold)), rows, int(first), hr.stream()), 'project_detections')
    return out


def _soft_nms_merge(who, rotated, boxes, scores, classes, kps, num_classes, max_detections, threshold, ncand, out):
    """the checks and the call of both merges; a box is [4] or, rotated, [4, 2]"""
    hr.require_gpu(boxes, scores, classes, kps, ncand)
    boxes, scores = hr.f32c(boxes), hr.f32c(scores)
    kps = None if kps is None else hr.f32c(kps)
    box = (4, 2) if rotated else (4,)
    if boxes.dim() != 2 + len(box) or tuple(boxes.shape[2:]) != box or boxes.shape[0] < 1:
        raise RuntimeError("%s: boxes must be [B, N, %s], got %s" % (who, ', '.join(map(str, box)), tuple(boxes.shape)))
    B, N = boxes.shape[:2]
    if N > MAX_CANDIDATES:
        raise RuntimeError("%s: %d candidates per image exceed the supported %d" % (who, N, MAX_CANDIDATES))
    if tuple(scores.shape) != (B, N) or tuple(classes.shape) != (B, N) or classes.dtype != torch.int32:
        raise RuntimeError("%s: scores must be float32 [B, N] and classes int32 [B, N]" % who)
    classes = classes.contiguous()
    J = 0 if kps is None else kps.shape[2]
    if kps is not None and (kps.dim() != 4 or tuple(kps.shape[:2]) != (B, N) or kps.shape[3] != 2 or J == 0):
        raise RuntimeError("%s: kps must be [B, N, J, 2], got %s" % (who, tuple(kps.shape)))
    if ncand is not None and (ncand.dtype != torch.int32 or tuple(ncand.shape) != (B,) or not ncand.is_contiguous()):
        raise RuntimeError("%s: ncand must be a contiguous int32 [B]" % who)
    K = int(max_detections)
    if out is None:
        out = _result_buffers(B, K, J, rotated, boxes.device)
    if tuple(out['boxes'].shape) != (B, K) + box or (J and tuple(out['kps'].shape) != (B, K, J, 2)):
        raise RuntimeError("%s: out does not hold %d rows of %d images" % (who, K, B))
    L = hr.lib()
    ws = hr.workspace(L.cnuda_predict_workspace_bytes(B, N), boxes.device)
    merge = L.cnuda_soft_nms_merge_rotated if rotated else L.cnuda_soft_nms_merge
    hr.check(merge(
        hr.ptr(boxes) if N else None, hr.ptr(scores) if N else None, hr.ptr(classes) if N else None,
        hr.ptr(kps) if J and N else None, hr.ptr(ncand), hr.ptr(out['boxes']), hr.ptr(out['scores']),
        hr.ptr(out['classes']), hr.ptr(out['kps']) if J else None, hr.ptr(out['counts']), B, N, int(num_classes), J, K,
        float(np.float32(threshold)), hr.ptr(ws), ws.numel(), hr.stream()), who)
    return out


def soft_nms_merge(boxes, scores, classes, kps, num_classes, max_detections, threshold, ncand=None, out=None):
    """Gaussian soft-NMS over boxes [B, N, 4], scores [B, N], classes [B, N] int32 (kps [B, N, J, 2] or None) per
    (image, class), then the per-image order (include/centernet_uda_hip.h).  ncand: int32 [B] device tensor, the
    candidates in use per image (None: all N).  -> dict of boxes [B, max_detections, 4], scores, classes, counts (kps)."""
    return _soft_nms_merge('soft_nms_merge', False, boxes, scores, classes, kps, num_classes, max_detections, threshold,
                           ncand, out)


def soft_nms_merge_rotated(boxes, scores, classes, kps, num_classes, max_detections, threshold, ncand=None, out=None):
    """`soft_nms_merge` over rotated boxes: boxes [B, N, 4, 2] vertices (x, y) as `project_detections(rotated=True)`
    writes them, overlap = the exact polygon IoU of the round's winner and the candidate (hip_runtime.ops.rotated_iou).
    -> dict of boxes [B, max_detections, 4, 2], scores, classes, counts (kps)."""
    return _soft_nms_merge('soft_nms_merge_rotated', True, boxes, scores, classes, kps, num_classes, max_detections,
                           threshold, ncand, out)


# ---------------------------------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------------------------------
class Predictor:
    """backend: a CenterNet backend of backends/ (on the GPU, or moved there by the caller); input_size = (width,
    height) of scale 1.  soft_nms=None: only with more than one scale (the published behaviour); True: always;
    'polygon': always, on the vertices of a rotated model with the exact polygon IoU -- the one form a rotated model
    takes, and what opens several scales to it."""

    def __init__(self, backend, input_size, *, max_detections=150, score_threshold=0.1, rotated=False, mean=MEAN,
                 std=STD, flip=False, scales=(1.0,), soft_nms=None, flip_pairs=None, nms=3):
        input_size = tuple(int(v) for v in input_size)
        if len(input_size) != 2 or min(input_size) < 1:
            raise ValueError("input_size must be (width, height), got %r" % (input_size,))
        try:
            scales = tuple(float(s) for s in scales)
        except TypeError:
            raise ValueError("scales must be a sequence of positive numbers, got %r" % (scales,)) from None
        if not scales or not all(s > 0 and math.isfinite(s) for s in scales):
            raise ValueError("scales must be a non-empty sequence of positive numbers, got %r" % (scales,))
        polygon = isinstance(soft_nms, str)
        if polygon and soft_nms != 'polygon':
            raise ValueError("soft_nms must be None, a bool or 'polygon', got %r" % (soft_nms,))
        if polygon and not rotated:
            raise ValueError("soft_nms='polygon' merges the vertices of a rotated model; this one is axis-aligned "
                             "(soft_nms=True is its soft-NMS)")
        use_soft = len(scales) > 1 if soft_nms is None else bool(soft_nms)
        if rotated and len(scales) > 1 and not polygon:
            raise ValueError("scales: a rotated model is predicted at one scale (there is no rotated soft-NMS), got %r"
                             % (scales,))
        if rotated and use_soft and not polygon:
            raise ValueError("soft_nms is not available for rotated models")
        if len(scales) > 1 and not use_soft:
            raise ValueError("soft_nms=False cannot merge %d scales" % len(scales))
        heads = dict(getattr(backend, 'heads', {}) or {})
        self.num_classes = int(heads.get('hm', 0))
        self.num_keypoints = int(heads.get('kps', 0)) // 2
        self.perm = flip_permutation(flip_pairs, self.num_keypoints)
        self.down_ratio = int(getattr(backend, 'down_ratio', 4))
        self.max_detections = int(max_detections)
        self.sizes = [(scale_size(input_size[0], s), scale_size(input_size[1], s)) for s in scales]
        cells = min((w // self.down_ratio) * (h // self.down_ratio) for w, h in self.sizes)
        if self.max_detections < 1 or self.max_detections > cells:
            raise ValueError("max_detections=%d does not fit the smallest scale's map of %d cells"
                             % (self.max_detections, cells))
        if use_soft and len(scales) * self.max_detections > MAX_CANDIDATES:
            raise ValueError("scales: %d scales of max_detections=%d give more than the %d candidates soft-NMS takes"
                             % (len(scales), self.max_detections, MAX_CANDIDATES))
        from export import CenterNet
        self.model = CenterNet(backend, self.max_detections, bool(rotated), int(nms)).eval()
        self.backend, self.input_size, self.scales = backend, input_size, scales
        self.rotated, self.flip, self.soft_nms, self.nms = bool(rotated), bool(flip), use_soft, int(nms)
        self.score_threshold = float(score_threshold)
        self.mean, self.std = tuple(mean), tuple(std)
        self._perm_dev = None

    def _scale(self, images, params, B):
        """One scale: uint8 batch -> (dets [B, K, 6|7], kps [B, K, J, 2] or None) in map cells."""
        from backends.decode import decode_detection
        from datasets.augment import augment_images
        from datasets.prepare import prepare_input
        from hip_runtime import ops
        resized = augment_images(images, params)
        if self.flip:
            _, H, W, _ = resized.shape
            x = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=images.device)
            prepare_input(resized, self.mean, self.std, out=x[:B])
            mirror_input(x[:B], out=x[B:])
            heads = tta_merge(self.model.heads(x), self._perm_dev)
            hm = heads['hm']
        else:
            heads = self.model.heads(prepare_input(resized, self.mean, self.std))
            hm = ops.sigmoid_clamp_(heads['hm'])
        got = decode_detection(hm, heads['wh'], heads.get('reg'), kps=heads.get('kps'), K=self.max_detections,
                               rotated=self.rotated, nms_size=self.nms)
        return got if isinstance(got, tuple) else (got, None)

    @torch.no_grad()
    def __call__(self, images, sizes):
        """images: padded uint8 [B, Hmax, Wmax, 3] on the GPU (image b in its top-left sizes[b] corner); sizes [B, 2]
        (h, w), a host array.  -> {'boxes', 'scores', 'classes', 'counts'[, 'kps'], 'packed'} on the device, in source
        pixels; rows at and past counts[b] score below the threshold."""
        from datasets.augment import AugmentParams
        hr.require_gpu(images)
        B, K, J, S = images.shape[0], self.max_detections, self.num_keypoints, len(self.scales)
        params = [AugmentParams.identity(sizes, size) for size in self.sizes]
        host = torch.empty(S * B * 6 * 2 + B * 2, dtype=torch.int32).pin_memory()
        host[:S * B * 12].view(torch.float64).view(S, B, 6).copy_(
            torch.from_numpy(np.stack([inverse_matrices(p) for p in params])))
        host[S * B * 12:].view(B, 2).copy_(torch.from_numpy(params[0].sizes))
        dev = host.to(images.device, non_blocking=True)
        matrices, d_sizes = dev[:S * B * 12].view(torch.float64).view(S, B, 6), dev[S * B * 12:].view(B, 2)
        if self.flip and J and self._perm_dev is None:
            self._perm_dev = torch.from_numpy(self.perm).pin_memory().to(images.device, non_blocking=True)
        out = _result_buffers(B, K, J, self.rotated, images.device)
        cand = _result_buffers(B, S * K, J, self.rotated, images.device) if self.soft_nms else out
        for s in range(S):
            dets, kps = self._scale(images, params[s], B)
            project_detections(dets, kps, matrices[s], d_sizes, self.score_threshold, self.rotated,
                               scale=self.down_ratio, out=cand, first=s * K)
        if self.soft_nms:
            merge = soft_nms_merge_rotated if self.rotated else soft_nms_merge
            merge(cand['boxes'], cand['scores'], cand['classes'], cand.get('kps'), self.num_classes, K,
                  self.score_threshold, out=out)
        return out


# ---------------------------------------------------------------------------------------------------------------------
# files in, records out
# ---------------------------------------------------------------------------------------------------------------------
def predict_files(predictor, files, *, batch_size=16, num_workers=16, device=None):
    """Generator of one record per file, in order: {'file', 'index', 'size' (h, w), 'boxes', 'scores', 'classes',
    'kps' (None without the head)} -- numpy arrays cut to the image's count.  Images are decoded by
    datasets.coco.load_rgb in min(num_workers, 16) threads (0: inline) into pinned buffers; batch k + 1 is decoded and
    uploaded (on a side stream) while batch k runs, and a batch's result comes back in one device-to-host copy."""
    from datasets.coco import load_rgb
    files = [os.fspath(f) for f in files]
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    batch_size = max(1, int(batch_size))
    threads = min(max(int(num_workers), 0), 16)
    pool = ThreadPoolExecutor(threads) if threads else None
    side = torch.cuda.Stream(device)
    staging = [None, None]                            # two pinned upload buffers, used in turn
    K, J, rotated = predictor.max_detections, predictor.num_keypoints, predictor.rotated

    def load(k):
        chunk = files[k * batch_size:(k + 1) * batch_size]
        decoded = list(pool.map(load_rgb, chunk)) if pool else [load_rgb(f) for f in chunk]
        sizes = np.array([im.shape[:2] for im in decoded], dtype=np.int32)
        shape = (len(chunk), int(sizes[:, 0].max()), int(sizes[:, 1].max()), 3)
        need = int(np.prod(shape))
        if staging[k % 2] is None or staging[k % 2].numel() < need:
            staging[k % 2] = torch.empty(need, dtype=torch.uint8).pin_memory()
        host = staging[k % 2][:need].view(shape)
        view = host.numpy()
        for b, im in enumerate(decoded):
            view[b, :im.shape[0], :im.shape[1]] = im          # (what lies outside an image's corner is never sampled)
        with torch.cuda.stream(side):
            images = host.to(device, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(side)
        return chunk, sizes, images, ready

    batches = (len(files) + batch_size - 1) // batch_size
    try:
        with torch.cuda.device(device):
            nxt = load(0) if batches else None
            for k in range(batches):
                chunk, sizes, images, ready = nxt
                main = torch.cuda.current_stream(device)
                main.wait_event(ready)
                images.record_stream(main)
                out = predictor(images, sizes)
                back = torch.empty(out['packed'].shape, dtype=torch.float32).pin_memory()
                back.copy_(out['packed'], non_blocking=True)         # the batch's one device-to-host copy
                done = torch.cuda.Event()
                done.record(main)
                nxt = load(k + 1) if k + 1 < batches else None       # decoded and uploaded while batch k runs
                done.synchronize()
                got = unpack_result(back.numpy(), len(chunk), K, J, rotated)
                for b, f in enumerate(chunk):
                    n = int(got['counts'][b])
                    yield {'file': f, 'index': k * batch_size + b, 'size': (int(sizes[b, 0]), int(sizes[b, 1])),
                           'boxes': got['boxes'][b, :n].copy(), 'scores': got['scores'][b, :n].copy(),
                           'classes': got['classes'][b, :n].copy(),
                           'kps': got['kps'][b, :n].copy() if J else None}
    finally:
        if pool:
            pool.shutdown(wait=True)


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def _scales(text):
    try:
        return tuple(float(v) for v in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError("--scales takes comma-separated numbers, got %r" % text) from None


def _pairs(text):
    try:
        return tuple(tuple(int(v) for v in pair.split('-')) for pair in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError("--flip-pairs takes pairs like 1-2,3-4, got %r" % text) from None


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('run_dir', help="a run directory of train.py (.hydra/config.yaml, model_last.pth)")
    ap.add_argument('inputs', nargs='+', help="image files, directories or glob patterns")
    ap.add_argument('--out', default='results.json', help="the COCO results file (default: %(default)s)")
    ap.add_argument('--best', action='store_true', help="load model_best.pth instead of model_last.pth")
    ap.add_argument('--teacher', action='store_true',
                    help="load the mean teacher (teacher_state_dict) of a uda.MeanTeacher run instead of the student")
    ap.add_argument('--flip', action='store_true', help="average with the left-right mirror")
    ap.add_argument('--scales', type=_scales, default=(1.0,), help="comma-separated test scales (default: 1)")
    ap.add_argument('--soft-nms', action='store_true', help="soft-NMS for a single scale too")
    ap.add_argument('--polygon-nms', action='store_true',
                    help="rotated models: soft-NMS on the vertices with the exact polygon IoU (allows several scales)")
    ap.add_argument('--score-threshold', type=float, default=None, help="default: the run's score_threshold")
    ap.add_argument('--batch-size', type=int, default=None, help="default: the run's batch_size")
    ap.add_argument('--num-workers', type=int, default=None, help="decoding threads, at most 16 (default: the run's)")
    ap.add_argument('--gpu', type=int, default=None, help="device index (default: the run's gpu)")
    ap.add_argument('--annotation-file', default=None, help="COCO file whose file_name -> id table names the images")
    ap.add_argument('--flip-pairs', type=_pairs, default=None, help="mirrored joint pairs of a keypoint model: 1-2,3-4")
    return ap.parse_args(argv)


def _soft_nms_setting(args):
    """Predictor's `soft_nms` of the command line: --polygon-nms wins over --soft-nms"""
    if getattr(args, 'polygon_nms', False):
        return 'polygon'
    return True if args.soft_nms else None


def settings_from_run(args):
    """The run's `.hydra/config.yaml` and the command line -> {'backend' (the {'name', 'params'} spec), 'predictor'
    (Predictor's keyword arguments, `input_size` included), 'batch_size', 'num_workers', 'gpu', 'use_last'}."""
    from utils.config import load_config, to_plain
    path = os.path.join(args.run_dir, '.hydra', 'config.yaml')
    if not os.path.isfile(path):
        raise FileNotFoundError("%s not found: RUN_DIR must be a run directory of train.py" % path)
    cfg = load_config(path, [])
    spec = {'name': cfg.model.backend.name, 'params': dict(to_plain(cfg.model.backend.params))}
    splits = cfg.get('datasets') or {}
    input_size = None
    for split in ('validation', 'training', 'test'):
        got = ((splits.get(split) or {}).get('params') or {}).get('input_size')
        if got is not None:
            input_size = tuple(int(v) for v in got)
            break
    if input_size is None:
        raise ValueError("%s names no datasets.*.params.input_size" % path)
    normalize = cfg.get('normalize') or {}
    gpu = cfg.get('gpu', 0) if args.gpu is None else args.gpu
    if isinstance(gpu, (list, tuple)):
        gpu = gpu[0]
    predictor = {
        'input_size': input_size,
        'max_detections': int(cfg.get('max_detections', 150)),
        'score_threshold': float(cfg.get('score_threshold', 0.1) if args.score_threshold is None
                                 else args.score_threshold),
        'rotated': bool(spec['params'].get('rotated_boxes', False)),
        'mean': tuple(normalize.get('mean', MEAN)), 'std': tuple(normalize.get('std', STD)),
        'flip': bool(args.flip), 'scales': tuple(args.scales), 'soft_nms': _soft_nms_setting(args),
        'flip_pairs': args.flip_pairs,
    }
    return {'backend': spec, 'predictor': predictor, 'use_last': not args.best, 'gpu': int(gpu or 0),
            'state_key': 'teacher_state_dict' if getattr(args, 'teacher', False) else 'state_dict',
            'batch_size': int(cfg.get('batch_size', 16) if args.batch_size is None else args.batch_size),
            'num_workers': int(cfg.get('num_workers', 16) if args.num_workers is None else args.num_workers)}


def main(argv=None):
    """-> {'out', 'images', 'detections', 'seconds', 'images_per_second', 'records'}"""
    import export
    args = parse_args(argv)
    settings = settings_from_run(args)
    files = expand_files(args.inputs)
    image_ids = image_ids_from_annotations(args.annotation_file) if args.annotation_file else None
    torch.cuda.set_device(settings['gpu'])
    device = torch.device('cuda', settings['gpu'])
    kwargs = dict(settings['predictor'])
    model = export.build_model(args.run_dir, settings['backend'], False, kwargs['max_detections'],
                               use_last=settings['use_last'], state_key=settings['state_key'])
    predictor = Predictor(model.backend.to(device).eval(), kwargs.pop('input_size'), **kwargs)
    began = time.perf_counter()
    records = list(predict_files(predictor, files, batch_size=settings['batch_size'],
                                 num_workers=settings['num_workers'], device=device))
    seconds = time.perf_counter() - began
    results = write_coco_results(records, args.out, image_ids=image_ids)
    rate = len(files) / seconds if seconds > 0 else 0.0
    log.info("%d images, %d detections in %.3f s: %.1f images/s -> %s", len(files), len(results), seconds, rate, args.out)
    return {'out': args.out, 'images': len(files), 'detections': len(results), 'seconds': seconds,
            'images_per_second': rate, 'records': records}


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format='[%(asctime)s][%(name)s][%(levelname)s] - %(message)s')
    main()
