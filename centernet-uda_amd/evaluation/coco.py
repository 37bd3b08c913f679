"""`Evaluator` (evaluation/coco.py): MS COCO detection metrics of the dictionaries `uda.base.Model.get_detections`
returns, driven as train.py drives the reference's: `add_batch(**detections)` per validation batch, `evaluate()` per
epoch -> TensorBoard-named scalars (`MSCOCO_Precision/mAP`, ... and per class `MSCOCO_Class_<name or id>/...`).

The reference hands the annotations to pycocotools (and, for rotated boxes, cv2.fillPoly + RLE masks in a process
pool); this build depends on neither.  What pycocotools' computeIoU / evaluateImg do per image and category runs on
the GPU (csrc/evalcoco.hip: box masks as row spans, pair IoU in float64, greedy matching for 10 IoU thresholds x 4 area
ranges); grouping, sorting and COCOeval's accumulate / the reference's summary are numpy on the host.

`add_batch` uploads one batch, queues its kernels on the current stream and returns; results stay on the device until
`evaluate()`, which synchronises once and reads them back.

Differences from the reference, all documented in README.md:
  * the mask of a rotated box is the project's own convex fill (utils/image.py::_fill_convex_poly on the
    `rotate_bbox` vertices), not cv2.fillPoly; the two have not been compared;
  * `rotated_iou = 'polygon'` (an attribute, default 'mask': the path above) measures rotated boxes without masks: the
    exact float64 IoU of the two polygons on the untruncated vertices (`utils.box.rotate_bboxes_float`,
    `cnuda_eval_iou_quads`), the polygon areas for COCO's area ranges, one launch, no workspace and no limit on the
    image size;
  * an image id repeated within one evaluation raises ValueError (the reference merges the two images' annotations);
  * per-class values stay float64 (the reference rounds them to float32 before the mean over classes);
  * `num_workers` is accepted and unused (no pool); keypoints are ignored here, as in the reference (their metrics are
    evaluation/coco_keypoints.py); no crowd regions."""
import ctypes

import numpy as np
import torch

import hip_runtime as hr
from utils.box import rotate_bboxes, rotate_bboxes_float

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
MAX_DETECTIONS = (1, 10, 100)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)
ROTATED_IOU_MODES = ('mask', 'polygon')
_VERTEX_LIMIT = 1 << 24          # vertices are clamped to +-2^24 pixels: the kernels' fixed-point arithmetic stays in 64 bits

# (mean name, per-class name, precision?, IoU threshold index or None, area range, detection limit): the reference's
# twelve summaries under the names its TensorBoard conversion gives them
SUMMARIES = (
    ('MSCOCO_Precision/mAP', 'MSCOCO_Class_{}/Precision/AP', True, None, 0, 100),
    ('MSCOCO_Precision/mAP.50IOU', 'MSCOCO_Class_{}/Precision/AP.50IOU', True, 0, 0, 100),
    ('MSCOCO_Precision/mAP.75IOU', 'MSCOCO_Class_{}/Precision/AP.75IOU', True, 5, 0, 100),
    ('MSCOCO_Recall/mAR1', 'MSCOCO_Class_{}/Recall/AR1', False, None, 0, 1),
    ('MSCOCO_Recall/mAR10', 'MSCOCO_Class_{}/Recall/AR10', False, None, 0, 10),
    ('MSCOCO_Recall/mAR100', 'MSCOCO_Class_{}/Recall/AR100', False, None, 0, 100),
    ('MSCOCO_Precision/mAP_small', 'MSCOCO_Class_{}/Precision/mAP_small', True, None, 1, 100),
    ('MSCOCO_Precision/mAP_medium', 'MSCOCO_Class_{}/Precision/mAP_medium', True, None, 2, 100),
    ('MSCOCO_Precision/mAP_large', 'MSCOCO_Class_{}/Precision/mAP_large', True, None, 3, 100),
    ('MSCOCO_Recall/mAR100_small', 'MSCOCO_Class_{}/Recall/AR100_small', False, None, 1, 100),
    ('MSCOCO_Recall/mAR100_medium', 'MSCOCO_Class_{}/Recall/AR100_medium', False, None, 2, 100),
    ('MSCOCO_Recall/mAR100_large', 'MSCOCO_Class_{}/Recall/AR100_large', False, None, 3, 100),
)


def group_batch(pred_classes, pred_scores, gt_classes, score_threshold, max_det=MAX_DETECTIONS[-1]):
    """Index bookkeeping of one batch.  Per image: predictions with score < threshold dropped, the rest and the ground
    truths grouped by category (ascending), a group's detections in descending score order (stable) and cut to `max_det`.
    -> (det_src [ND, 2] (image in batch, prediction index), gt_src [NGT, 2], groups [G, 5] int32 as csrc/evalcoco.hip
    reads them, group_key [G, 2] (image in batch, category), labels seen (before the cut))"""
    det_src, gt_src, groups, keys, labels = [], [], [], [], set()
    nd = ngt = npairs = 0
    thr = np.float32(score_threshold)
    for i in range(len(gt_classes)):
        pc, ps = np.asarray(pred_classes[i]).astype(np.int64), np.asarray(pred_scores[i], dtype=np.float32)
        gc = np.asarray(gt_classes[i]).astype(np.int64)
        kept = np.flatnonzero(~(ps < thr))
        cats = np.union1d(pc[kept], gc)
        labels.update(int(c) for c in cats)
        for c in cats:
            d = kept[pc[kept] == c]
            d = d[np.argsort(-ps[d], kind='mergesort')][:max_det]
            g = np.flatnonzero(gc == c)
            det_src.append(np.stack([np.full(len(d), i), d], 1))
            gt_src.append(np.stack([np.full(len(g), i), g], 1))
            groups.append((nd, len(d), ngt, len(g), npairs))
            keys.append((i, int(c)))
            nd, ngt, npairs = nd + len(d), ngt + len(g), npairs + len(d) * len(g)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros((0, 2), np.int64)
    return (cat(det_src), cat(gt_src), np.asarray(groups, dtype=np.int32).reshape(-1, 5),
            np.asarray(keys, dtype=np.int64).reshape(-1, 2), labels)


def accumulate(cats, det, gt, max_dets=MAX_DETECTIONS):
    """COCOeval.accumulate.  det: dict(image, cat, rank (position in its group), score float32, bits uint32 [ND, 4]);
    gt: dict(cat, ignore bool [NGT, 4]); max_dets: the detection limits M.  -> precision [T, R, K, A, M],
    recall [T, K, A, M], -1 where undefined."""
    T, R, K, A, M = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), len(cats), len(AREA_RANGES), len(max_dets)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    shifts = np.arange(T, dtype=np.uint32)[:, None]
    for k, c in enumerate(cats):
        of_cat = np.flatnonzero(det['cat'] == c)
        of_cat = of_cat[np.lexsort((det['rank'][of_cat], det['image'][of_cat]))]       # images ascending, score order inside
        gt_of_cat = gt['cat'] == c
        if not len(of_cat) and not gt_of_cat.any():
            continue
        for a in range(A):
            npig = int(np.count_nonzero(~gt['ignore'][gt_of_cat, a]))
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sel = of_cat[det['rank'][of_cat] < max_det]
                sel = sel[np.argsort(-det['score'][sel], kind='mergesort')]
                bits = det['bits'][sel, a][None, :]
                matched, ignored = (bits >> shifts) & 1 == 1, (bits >> (shifts + 16)) & 1 == 1
                tp_sum = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                nd = len(sel)
                if nd == 0:
                    recall[:, k, a, m] = 0
                    precision[:, :, k, a, m] = 0
                    continue
                rc = tp_sum / npig
                pr = tp_sum / (fp_sum + tp_sum + np.spacing(1))
                recall[:, k, a, m] = rc[:, -1]
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]          # non-increasing from the right
                for t in range(T):
                    at = np.searchsorted(rc[t], RECALL_THRESHOLDS, side='left')
                    inside = at < nd
                    q = np.zeros(R)
                    q[inside] = pr[t, at[inside]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall, is_precision, iou_index, area_index, max_det, max_dets=MAX_DETECTIONS):
    """The reference's summary of one metric: -1 -> NaN, per class the mean over thresholds (and recall points) that
    have a value, then the mean over the classes that have one.  -> (per class [K], mean)"""
    m = tuple(max_dets).index(max_det)
    v = precision[:, :, :, area_index, m] if is_precision else recall[:, :, area_index, m]
    if iou_index is not None:
        v = v[iou_index:iou_index + 1]
    v = np.where(v == -1, np.nan, v).reshape(-1, v.shape[-1])
    valid = ~np.isnan(v)
    count = valid.sum(0)
    per_class = np.full(v.shape[1], np.nan)
    has = count > 0
    per_class[has] = np.where(valid, v, 0.0).sum(0)[has] / count[has]
    return per_class, (per_class[has].mean() if has.any() else np.nan)


def to_tensorboard(summaries, existent_labels, per_class, classes, table=SUMMARIES):
    """summaries: [(per-label array, mean)] in the order of `table` -> {scalar name: value}.  With per_class False the
    per-label arrays are returned whole under the unformatted per-class names, as the reference does."""
    out = {}
    for (mean_name, class_name, *_), (per_label, mean) in zip(table, summaries):
        if per_class:
            for c in existent_labels:
                label = classes[c]['name'] if classes is not None and c in classes else c
                out[class_name.format(str(label))] = per_label[c]
        else:
            out[class_name] = per_label
        out[mean_name] = mean
    return out


def _gather(per_image, src, ncol):
    """rows `src` = (image in batch, row) of the per-image arrays, first `ncol` columns, float32"""
    out = np.zeros((len(src), ncol), dtype=np.float32)
    for i in np.unique(src[:, 0]):
        a = np.asarray(per_image[i], dtype=np.float32)
        pick = src[:, 0] == i
        out[pick] = a.reshape(len(a), -1)[src[pick, 1], :ncol]
    return out


class Evaluator:
    _known_ids = []          # process-wide: ground-truth id -> 1-based image id, in order of first appearance
    summaries, max_detections = SUMMARIES, MAX_DETECTIONS          # evaluation/coco_keypoints.py has its own

    def __init__(self, per_class=True, score_threshold=0.1):
        hr.lib()             # RuntimeError when the HIP library has not been built
        if not torch.cuda.is_available():
            raise RuntimeError("centernet-uda_amd ops run on MI355X only: the COCO evaluator found no GPU "
                               "(there is no CPU fallback; a numpy oracle lives in tests/ for tests)")
        self.per_class = per_class
        self.classes = None
        self.score_threshold = score_threshold
        self.use_rotated_boxes = False
        self.rotated_iou = 'mask'            # how rotated boxes overlap: 'mask' (rasterised row spans) or 'polygon' (exact)
        self.num_workers = None
        self.existent_labels = {}
        self.ids = []
        self._batches = []
        self._keep_intermediates = False

    def reset(self):
        self.ids.clear()
        self._batches.clear()

    # -- one batch -------------------------------------------------------------------------------------------------
    def _group(self, pred_classes, pred_scores, gt_classes, gt_ids):
        """the batch's image ids (new to this evaluation, else ValueError) and its `group_batch`"""
        image_ids = []
        for gid in gt_ids:
            gid = int(gid)
            if gid not in Evaluator._known_ids:
                Evaluator._known_ids.append(gid)
            image_id = Evaluator._known_ids.index(gid) + 1
            if image_id in self.ids or image_id in image_ids:
                raise ValueError("Evaluator.add_batch: image id %r was already added to this evaluation" % gid)
            image_ids.append(image_id)
        det_src, gt_src, groups, keys, labels = group_batch(pred_classes, pred_scores, gt_classes, self.score_threshold,
                                                            self.max_detections[-1])
        self.ids.extend(image_ids)
        for lb in labels:
            self.existent_labels[lb] = True
        return image_ids, det_src, gt_src, groups, keys

    def _match(self, image_ids, det_src, groups, d_groups, keys, pred_scores, iou, det_area, gt_area, gt_flags=None):
        """queues the matching of one batch (`d_groups`, the pair similarities `iou`, the areas and, for keypoints, the
        flags of the ground truths to ignore: all on the device) and keeps its record for `evaluate()`"""
        nd, ngt = len(det_src), int(groups[:, 3].sum())
        npairs = int((groups[:, 1].astype(np.int64) * groups[:, 3]).sum())
        dev = iou.device
        L, st = hr.lib(), hr.stream()
        det_bits = torch.zeros((max(nd, 1), 4), dtype=torch.int32, device=dev)
        gt_ignore = torch.zeros((max(ngt, 1), 4), dtype=torch.uint8, device=dev)
        thr = (ctypes.c_double * len(IOU_THRESHOLDS))(*IOU_THRESHOLDS)
        rng = (ctypes.c_double * AREA_RANGES.size)(*AREA_RANGES.reshape(-1))
        if gt_flags is None:
            hr.check(L.cnuda_eval_match(hr.ptr(iou), hr.ptr(d_groups), len(groups), hr.ptr(det_area), hr.ptr(gt_area), nd,
                                        ngt, npairs, thr, len(IOU_THRESHOLDS), rng, hr.ptr(det_bits), hr.ptr(gt_ignore),
                                        st), 'eval_match')
        else:
            hr.check(L.cnuda_eval_match_flagged(hr.ptr(iou), hr.ptr(d_groups), len(groups), hr.ptr(det_area),
                                                hr.ptr(gt_area), hr.ptr(gt_flags), nd, ngt, npairs, thr,
                                                len(IOU_THRESHOLDS), rng, hr.ptr(det_bits), hr.ptr(gt_ignore), st),
                     'eval_match_flagged')
        ids = np.asarray(image_ids, dtype=np.int64)
        rank = np.concatenate([np.arange(n) for n in groups[:, 1]]) if len(groups) else np.zeros(0, np.int64)
        scores = _gather(pred_scores, det_src, 1)[:, 0]
        record = {
            'det_image': np.repeat(ids[keys[:, 0]], groups[:, 1]) if len(groups) else np.zeros(0, np.int64),
            'det_cat': np.repeat(keys[:, 1], groups[:, 1]) if len(groups) else np.zeros(0, np.int64),
            'det_rank': rank.astype(np.int64), 'det_score': scores,
            'gt_cat': np.repeat(keys[:, 1], groups[:, 3]) if len(groups) else np.zeros(0, np.int64),
            'nd': nd, 'ngt': ngt, 'det_bits': det_bits, 'gt_ignore': gt_ignore, 'groups': groups, 'keys': keys}
        if self._keep_intermediates:          # the tests compare these with the oracle's; an epoch does not hold them
            record.update({'iou': iou, 'det_area': det_area, 'gt_area': gt_area})
            if gt_flags is not None:
                record['gt_flags'] = gt_flags
        self._batches.append(record)

    def add_batch(self, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_ids, gt_areas, image_shape,
                  pred_kps=None, gt_kps=None):
        if self.rotated_iou not in ROTATED_IOU_MODES:
            raise ValueError("Evaluator.rotated_iou must be one of %s, got %r" % (ROTATED_IOU_MODES, self.rotated_iou))
        B = len(gt_ids)
        H, W = int(image_shape[1]), int(image_shape[2])
        image_ids, det_src, gt_src, groups, keys = self._group(pred_classes, pred_scores, gt_classes, gt_ids)
        ncol = 5 if self.use_rotated_boxes else 4
        det_boxes, gt_boxes_ = _gather(pred_boxes, det_src, ncol), _gather(gt_boxes, gt_src, ncol)
        nd, ngt, npairs = len(det_src), len(gt_src), int((groups[:, 1].astype(np.int64) * groups[:, 3]).sum())
        dev = torch.device('cuda', torch.cuda.current_device())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        L, st = hr.lib(), hr.stream()
        d_groups = up(groups)
        iou = torch.empty(max(npairs, 1), dtype=torch.float64, device=dev)
        if self.use_rotated_boxes and self.rotated_iou == 'polygon':
            d_quads = up(rotate_bboxes_float(np.concatenate([det_boxes, gt_boxes_])))
            area = torch.empty(max(nd + ngt, 1), dtype=torch.float64, device=dev)
            hr.check(L.cnuda_eval_iou_quads(hr.ptr(d_quads), hr.ptr(d_groups), len(groups), nd, ngt, npairs, hr.ptr(iou),
                                            hr.ptr(area), st), 'eval_iou_quads')
            det_area, gt_area = area[:nd], area[nd:nd + ngt]
        elif self.use_rotated_boxes:
            verts = np.clip(rotate_bboxes(np.concatenate([det_boxes, gt_boxes_])), -_VERTEX_LIMIT, _VERTEX_LIMIT)
            d_verts = up(verts.astype(np.int32))
            rows = torch.empty((max(nd + ngt, 1), 2), dtype=torch.int32, device=dev)
            area = torch.empty(max(nd + ngt, 1), dtype=torch.float64, device=dev)
            nbytes = L.cnuda_eval_workspace_bytes(nd + ngt, H)
            ws = hr.workspace(nbytes, dev)
            hr.check(L.cnuda_eval_box_spans(hr.ptr(d_verts), nd + ngt, H, W, hr.ptr(rows), hr.ptr(area), hr.ptr(ws),
                                            ws.numel(), st), 'eval_box_spans')
            hr.check(L.cnuda_eval_iou_rotated(hr.ptr(d_groups), len(groups), nd, ngt, npairs, hr.ptr(rows), hr.ptr(area),
                                              H, hr.ptr(iou), hr.ptr(ws), ws.numel(), st), 'eval_iou_rotated')
            det_area, gt_area = area[:nd], area[nd:nd + ngt]
        else:
            def xywh(b):
                return np.stack([np.round(b[:, 0], 2), np.round(b[:, 1], 2), np.round(b[:, 2] - b[:, 0], 2),
                                 np.round(b[:, 3] - b[:, 1], 2)], 1).astype(np.float32)
            given = (np.concatenate([np.asarray(gt_areas[i], dtype=np.float64).reshape(-1) for i in range(B)])
                     if B else np.zeros(0))
            first = np.cumsum([0] + [len(np.asarray(gt_classes[i])) for i in range(B)])
            gt_area_host = given[first[gt_src[:, 0]] + gt_src[:, 1]] if ngt else np.zeros(0)
            det_area_host = ((det_boxes[:, 3] - det_boxes[:, 1]) * (det_boxes[:, 2] - det_boxes[:, 0])).astype(np.float64)
            d_det, d_gt = up(xywh(det_boxes)), up(xywh(gt_boxes_))
            det_area, gt_area = up(det_area_host), up(gt_area_host)
            hr.check(L.cnuda_eval_iou_axis(hr.ptr(d_det), hr.ptr(d_gt), hr.ptr(d_groups), len(groups), nd, ngt, npairs,
                                           hr.ptr(iou), st), 'eval_iou_axis')
        self._match(image_ids, det_src, groups, d_groups, keys, pred_scores, iou, det_area, gt_area)

    # -- the epoch's result ----------------------------------------------------------------------------------------
    def _read_back(self):
        """the one synchronisation: every batch's detection bits and ground-truth ignore flags in one copy"""
        parts = []
        for b in self._batches:
            parts += [b['det_bits'][:b['nd']].reshape(-1).view(torch.uint8), b['gt_ignore'][:b['ngt']].reshape(-1)]
        flat = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.uint8)
        bits, ignore, at = [], [], 0
        for b in self._batches:
            n = b['nd'] * 16
            bits.append(flat[at:at + n].view(np.uint32).reshape(-1, 4))
            at += n
            n = b['ngt'] * 4
            ignore.append(flat[at:at + n].reshape(-1, 4) != 0)
            at += n
        return bits, ignore

    def evaluate(self):
        existent_labels = sorted(self.existent_labels)
        if not existent_labels:
            raise ValueError("Evaluator.evaluate: no prediction above the score threshold and no ground truth was added")
        bits, ignore = self._read_back()
        join = lambda key, dtype: (np.concatenate([b[key] for b in self._batches]).astype(dtype)
                                   if self._batches else np.zeros(0, dtype))
        det = {'image': join('det_image', np.int64), 'cat': join('det_cat', np.int64), 'rank': join('det_rank', np.int64),
               'score': join('det_score', np.float32),
               'bits': np.concatenate(bits) if bits else np.zeros((0, 4), np.uint32)}
        gt = {'cat': join('gt_cat', np.int64), 'ignore': np.concatenate(ignore) if ignore else np.zeros((0, 4), bool)}
        precision, recall = accumulate(existent_labels, det, gt, self.max_detections)
        summaries = []
        for _, _, is_precision, iou_index, area_index, max_det in self.summaries:
            per_class, mean = summarize(precision, recall, is_precision, iou_index, area_index, max_det,
                                        self.max_detections)
            per_label = np.full(max(existent_labels) + 1, np.nan)
            per_label[existent_labels] = per_class
            summaries.append((per_label, mean))
        results = to_tensorboard(summaries, existent_labels, self.per_class, self.classes, self.summaries)
        self.reset()
        return results
