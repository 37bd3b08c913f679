"""`Evaluator` (evaluation/coco_keypoints.py): MS COCO keypoint metrics -- COCOeval with iouType='keypoints', written
from the published protocol -- of the dictionaries `uda.base.Model.get_detections` returns for a model with a `kps`
head.  The driver loads it like the box evaluator (`evaluation: {coco_keypoints: {...}}`) and feeds both the same
batches; the scalars are `MSCOCO_Keypoints_Precision/mAP`, ... and per class `MSCOCO_Keypoints_Class_<name or id>/...`.

What differs from evaluation/coco.py, whose grouping, matching, accumulation and summary this module reuses:
  * the similarity of a (detection, ground truth) pair is the object keypoint similarity (csrc/evalcoco.hip,
    cnuda_eval_oks: float64, COCOeval.computeOks' order of operations, the sum over joints in ascending order);
  * a ground truth without a labelled joint is ignored in every area range (cnuda_eval_match_flagged), and its
    similarity is measured against its box doubled about its centre;
  * a detection's area is the bounds of its predicted joints (COCO's loadRes); a ground truth's is `gt_areas` as given,
    for rotated models too (the box evaluator counts mask pixels there);
  * at most 20 detections per image and category; `all`, `medium` and `large` areas are summarised (COCOeval has no
    `small` keypoint summary).

`gt_kps[i]` is [n, J, 2] (every joint labelled) or [n, J, 3] with COCO's `v` in the third column (datasets.loader's
`keypoint_visibility=True`).  No CPU fallback, no crowd regions; pycocotools is not a dependency and the two have not
been compared (tests/test_host_cocoeval_kps.py does it where the package is installed)."""
import numpy as np
import torch

import hip_runtime as hr
from evaluation import coco
from utils.box import rotate_bboxes

# COCO's person constants (cocoeval.py, Params.setKpParams: these divided by 10 are the per-joint sigmas)
COCO_PERSON_SIGMAS = (0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087,
                      0.087, 0.089, 0.089)
MAX_DETECTIONS = (20,)
MAX_JOINTS = 64

# (mean name, per-class name, precision?, IoU threshold index or None, area range, detection limit): COCOeval's ten
# keypoint summaries, named after the box evaluator's
SUMMARIES = (
    ('MSCOCO_Keypoints_Precision/mAP', 'MSCOCO_Keypoints_Class_{}/Precision/AP', True, None, 0, 20),
    ('MSCOCO_Keypoints_Precision/mAP.50IOU', 'MSCOCO_Keypoints_Class_{}/Precision/AP.50IOU', True, 0, 0, 20),
    ('MSCOCO_Keypoints_Precision/mAP.75IOU', 'MSCOCO_Keypoints_Class_{}/Precision/AP.75IOU', True, 5, 0, 20),
    ('MSCOCO_Keypoints_Precision/mAP_medium', 'MSCOCO_Keypoints_Class_{}/Precision/mAP_medium', True, None, 2, 20),
    ('MSCOCO_Keypoints_Precision/mAP_large', 'MSCOCO_Keypoints_Class_{}/Precision/mAP_large', True, None, 3, 20),
    ('MSCOCO_Keypoints_Recall/mAR20', 'MSCOCO_Keypoints_Class_{}/Recall/AR20', False, None, 0, 20),
    ('MSCOCO_Keypoints_Recall/mAR20.50IOU', 'MSCOCO_Keypoints_Class_{}/Recall/AR20.50IOU', False, 0, 0, 20),
    ('MSCOCO_Keypoints_Recall/mAR20.75IOU', 'MSCOCO_Keypoints_Class_{}/Recall/AR20.75IOU', False, 5, 0, 20),
    ('MSCOCO_Keypoints_Recall/mAR20_medium', 'MSCOCO_Keypoints_Class_{}/Recall/AR20_medium', False, None, 2, 20),
    ('MSCOCO_Keypoints_Recall/mAR20_large', 'MSCOCO_Keypoints_Class_{}/Recall/AR20_large', False, None, 3, 20),
)


def split_gt_keypoints(gt_kps):
    """per image [n, J, 2] or [n, J, 3] -> ([n, J, 2] float32, [n, J] uint8 COCO `v`: 2 for the two-column form)"""
    points, vis = [], []
    for k in gt_kps:
        k = np.asarray(k)
        if k.ndim != 3 or k.shape[2] not in (2, 3):
            raise ValueError("Evaluator.add_batch: gt_kps rows must be [n, J, 2] or [n, J, 3] (x, y, v), got %s"
                             % (k.shape,))
        points.append(k[:, :, :2].astype(np.float32))
        vis.append(np.full(k.shape[:2], 2, np.uint8) if k.shape[2] == 2
                   else np.clip(np.nan_to_num(k[:, :, 2]), 0, 255).astype(np.uint8))
    return points, vis


def _rows(per_image, src, dtype, tail):
    """rows `src` = (image in batch, row) of the per-image arrays, as one [len(src), *tail] array of `dtype`"""
    out = np.zeros((len(src),) + tuple(tail), dtype=dtype)
    for i in np.unique(src[:, 0]):
        pick = src[:, 0] == i
        out[pick] = np.asarray(per_image[i]).reshape((-1,) + tuple(tail))[src[pick, 1]]
    return out


class Evaluator(coco.Evaluator):
    summaries, max_detections = SUMMARIES, MAX_DETECTIONS

    def __init__(self, per_class=True, score_threshold=0.1, sigmas=None):
        if sigmas is not None:
            sigmas = np.asarray(sigmas, dtype=np.float64).reshape(-1)
            if not (1 <= len(sigmas) <= MAX_JOINTS) or not (sigmas > 0).all():
                raise ValueError("coco_keypoints.Evaluator: sigmas must be between 1 and %d positive numbers, one per "
                                 "joint, got %r" % (MAX_JOINTS, sigmas.tolist()))
        super().__init__(per_class=per_class, score_threshold=score_threshold)
        self.sigmas = sigmas
        self._d_sigmas = None

    def _sigmas_for(self, J, dev):
        if self.sigmas is None:
            if J != len(COCO_PERSON_SIGMAS):
                raise ValueError("coco_keypoints.Evaluator: no sigmas were given and the model has J = %d joints; the "
                                 "defaults are COCO's %d person constants: pass `sigmas`, one positive number per "
                                 "joint" % (J, len(COCO_PERSON_SIGMAS)))
            sigmas = np.asarray(COCO_PERSON_SIGMAS, dtype=np.float64)
        else:
            sigmas = self.sigmas
            if len(sigmas) != J:
                raise ValueError("coco_keypoints.Evaluator: %d sigmas for J = %d joints" % (len(sigmas), J))
        if self._d_sigmas is None or self._d_sigmas.device != dev or self._d_sigmas.numel() != J:
            self._d_sigmas = torch.from_numpy(sigmas.copy()).to(dev)
        return self._d_sigmas

    def add_batch(self, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_ids, gt_areas, image_shape,
                  pred_kps=None, gt_kps=None):
        if pred_kps is None or gt_kps is None:
            raise ValueError("coco_keypoints.Evaluator.add_batch: pred_kps and gt_kps are required (a model without a "
                             "`kps` head has no keypoint metrics: take coco_keypoints out of `evaluation`)")
        pred_kps = np.asarray(pred_kps)
        if pred_kps.ndim != 4 or pred_kps.shape[3] != 2:
            raise ValueError("coco_keypoints.Evaluator.add_batch: pred_kps must be [B, K, J, 2], got %s"
                             % (pred_kps.shape,))
        J = int(pred_kps.shape[2])
        gt_points, gt_vis = split_gt_keypoints(gt_kps)
        for i, k in enumerate(gt_points):
            if k.shape[1] != J or k.shape[0] != len(np.asarray(gt_classes[i])):
                raise ValueError("coco_keypoints.Evaluator.add_batch: gt_kps[%d] is %s for %d ground truths of J = %d "
                                 "joints" % (i, k.shape, len(np.asarray(gt_classes[i])), J))
        dev = torch.device('cuda', torch.cuda.current_device())
        d_sigmas = self._sigmas_for(J, dev)
        image_ids, det_src, gt_src, groups, keys = self._group(pred_classes, pred_scores, gt_classes, gt_ids)
        nd, ngt, npairs = len(det_src), len(gt_src), int((groups[:, 1].astype(np.int64) * groups[:, 3]).sum())
        ncol = 5 if self.use_rotated_boxes else 4
        box = coco._gather(gt_boxes, gt_src, ncol)
        if self.use_rotated_boxes:                # the bounds of the vertices the box evaluator rasterises
            v = rotate_bboxes(box).reshape(ngt, 4, 2)
            box = np.concatenate([v.min(1), v.max(1) - v.min(1)], 1) if ngt else np.zeros((0, 4))
        else:
            box = np.stack([box[:, 0], box[:, 1], box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        d_groups = up(groups)
        d_det = up(_rows(pred_kps, det_src, np.float32, (J, 2)))
        d_gt, d_vis = up(_rows(gt_points, gt_src, np.float32, (J, 2))), up(_rows(gt_vis, gt_src, np.uint8, (J,)))
        gt_area, d_box = up(_rows(gt_areas, gt_src, np.float64, ())), up(box.astype(np.float32))
        oks = torch.empty(max(npairs, 1), dtype=torch.float64, device=dev)
        det_area = torch.empty(max(nd, 1), dtype=torch.float64, device=dev)
        gt_flags = torch.zeros(max(ngt, 1), dtype=torch.uint8, device=dev)
        hr.check(hr.lib().cnuda_eval_oks(hr.ptr(d_det), hr.ptr(d_gt), hr.ptr(d_vis), hr.ptr(gt_area), hr.ptr(d_box),
                                         hr.ptr(d_sigmas), J, hr.ptr(d_groups), len(groups), nd, ngt, npairs, hr.ptr(oks),
                                         hr.ptr(det_area), hr.ptr(gt_flags), hr.stream()), 'eval_oks')
        self._match(image_ids, det_src, groups, d_groups, keys, pred_scores, oks, det_area, gt_area, gt_flags)
