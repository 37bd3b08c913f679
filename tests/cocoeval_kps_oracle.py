"""Independent oracle of evaluation/coco_keypoints.py: a numpy restatement of COCOeval's keypoint protocol
(iouType='keypoints') on top of tests/cocoeval_oracle.py's `evaluate_img` and accumulation, with the detection limits
(20,).  `oks` follows computeOks' order of operations in float64; the one deliberate difference is the sum over the
joints, taken in ascending order by a loop (np.sum adds pairwise: the two differ in the last bits).  Shares no code
with evaluation/coco_keypoints.py; utils.box.rotate_bbox gives the vertices of a rotated ground-truth box."""
import contextlib

import numpy as np

import cocoeval_oracle as co
from utils.box import rotate_bbox

MAX_DETS = [20]
COCO_PERSON_SIGMAS = np.array([0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107,
                               0.087, 0.087, 0.089, 0.089])


def oks(d_kps, g_kps, g_vis, g_area, g_box, sigmas):
    """computeOks for one pair.  d_kps, g_kps [J, 2] float32; g_vis [J] COCO's v; g_box (x, y, w, h) float32."""
    var = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    xd, yd = np.asarray(d_kps)[:, 0].astype(np.float64), np.asarray(d_kps)[:, 1].astype(np.float64)
    xg, yg = np.asarray(g_kps)[:, 0].astype(np.float64), np.asarray(g_kps)[:, 1].astype(np.float64)
    vg = np.asarray(g_vis)
    k1 = np.count_nonzero(vg > 0)
    if k1 > 0:
        dx, dy = xd - xg, yd - yg
    else:
        bx, by, bw, bh = (np.float64(v) for v in g_box)
        x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
        z = np.zeros(len(xd))
        dx = np.maximum(z, x0 - xd) + np.maximum(z, xd - x1)
        dy = np.maximum(z, y0 - yd) + np.maximum(z, yd - y1)
    e = (dx ** 2 + dy ** 2) / var / (np.float64(g_area) + np.spacing(1)) / 2
    if k1 > 0:
        e = e[vg > 0]
    total = 0.0
    for v in np.exp(-e):                     # ascending j
        total = total + float(v)
    return total / e.shape[0]


def result_area(d_kps):
    """the area COCO.loadRes gives a keypoint result: the bounds of its joints"""
    x, y = np.asarray(d_kps)[:, 0].astype(np.float64), np.asarray(d_kps)[:, 1].astype(np.float64)
    return float((x.max() - x.min()) * (y.max() - y.min()))


def evaluate_img(dt, gt, ious, area_range):
    """COCOeval.evaluateImg with _prepare's keypoint rule: a ground truth without a labelled joint is ignored whatever
    its area.  co.evaluate_img ignores by area alone, so such a ground truth goes in with an area below every range."""
    return co.evaluate_img(dt, [{'area': -1.0} if g['ignore'] else g for g in gt], ious, area_range)


@contextlib.contextmanager
def _limits():
    """tests/cocoeval_oracle.py reads its detection limits from its module: (20,) while this oracle accumulates"""
    saved, co.MAX_DETS = co.MAX_DETS, MAX_DETS
    try:
        yield
    finally:
        co.MAX_DETS = saved


_NAMES = [('ap', None, 'all', 'Precision/{m}AP'), ('ap', 0.5, 'all', 'Precision/{m}AP.50IOU'),
          ('ap', 0.75, 'all', 'Precision/{m}AP.75IOU'), ('ap', None, 'medium', 'Precision/mAP_medium'),
          ('ap', None, 'large', 'Precision/mAP_large'), ('ar', None, 'all', 'Recall/{m}AR20'),
          ('ar', 0.5, 'all', 'Recall/{m}AR20.50IOU'), ('ar', 0.75, 'all', 'Recall/{m}AR20.75IOU'),
          ('ar', None, 'medium', 'Recall/{m}AR20_medium'), ('ar', None, 'large', 'Recall/{m}AR20_large')]


class OracleKeypointEvaluator(co.OracleEvaluator):
    def __init__(self, per_class=True, score_threshold=0.1, sigmas=None):
        super().__init__(per_class, score_threshold)
        self.sigmas = sigmas

    def _box(self, box):
        if self.use_rotated_boxes:
            v = np.array(rotate_bbox(*box))
            lo, hi = v.min(0), v.max(0)
            return np.float32([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])
        x_min, y_min, x_max, y_max = np.asarray(box, dtype=np.float32)[:4]
        return np.float32([x_min, y_min, x_max - x_min, y_max - y_min])

    def add_batch(self, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_ids, gt_areas, image_shape,
                  pred_kps=None, gt_kps=None):
        J = np.asarray(pred_kps).shape[2]
        if self.sigmas is None:
            assert J == 17
        for i, gid in enumerate(gt_ids):
            gid = int(gid)
            if gid not in co.OracleEvaluator._known_ids:
                co.OracleEvaluator._known_ids.append(gid)
            image_id = co.OracleEvaluator._known_ids.index(gid) + 1
            if image_id in self.images:
                raise ValueError('image id %r was already added to this evaluation' % gid)
            self.images.append(image_id)
            for kp, lb, sc in zip(pred_kps[i], pred_classes[i], pred_scores[i]):
                if np.float32(sc) < np.float32(self.score_threshold):
                    continue
                kp = np.asarray(kp, dtype=np.float32)
                self.dts.setdefault((image_id, int(lb)), []).append(
                    {'image_id': image_id, 'category_id': int(lb), 'score': sc, 'kps': kp, 'area': result_area(kp)})
                self.existent_labels[int(lb)] = True
            for kp, bb, lb, ar in zip(gt_kps[i], gt_boxes[i], gt_classes[i], gt_areas[i]):
                kp = np.asarray(kp)
                vis = kp[:, 2].astype(np.int64) if kp.shape[1] == 3 else np.full(len(kp), 2)
                self.gts.setdefault((image_id, int(lb)), []).append(
                    {'image_id': image_id, 'category_id': int(lb), 'kps': kp[:, :2].astype(np.float32), 'vis': vis,
                     'area': float(ar), 'bbox': self._box(bb), 'ignore': bool((vis > 0).sum() == 0)})
                self.existent_labels[int(lb)] = True

    def per_image(self):
        sigmas = COCO_PERSON_SIGMAS if self.sigmas is None else self.sigmas
        out = {}
        for key in sorted(set(self.dts) | set(self.gts)):
            dt, gt = self.dts.get(key, []), self.gts.get(key, [])
            order = np.argsort([-d['score'] for d in dt], kind='mergesort')
            dt = [dt[i] for i in order][:MAX_DETS[-1]]
            ious = [[oks(d['kps'], g['kps'], g['vis'], g['area'], g['bbox'], sigmas) for g in gt] for d in dt]
            out[key] = {'dt': dt, 'gt': gt, 'ious': ious,
                        'ranges': [evaluate_img(dt, gt, ious, rng) for rng in co.AREA_RANGES]}
        return out

    def evaluate(self):
        cats = sorted(self.existent_labels)
        per_image = self.per_image()
        out = {}
        with _limits():
            precision, recall = self.accumulate(per_image, cats)
            for kind, thr, area, name in _NAMES:
                per_class, mean = self.summarize(precision, recall, kind == 'ap', thr, area, MAX_DETS[-1])
                full = np.full(max(cats) + 1, np.nan)
                full[cats] = per_class
                out['MSCOCO_Keypoints_' + name.replace('{m}', 'm')] = mean
                cls_name = 'MSCOCO_Keypoints_Class_{}/' + name.replace('{m}', '')
                if self.per_class:
                    for c in cats:
                        label = self.classes[c]['name'] if self.classes is not None and c in self.classes else c
                        out[cls_name.format(str(label))] = full[c]
                else:
                    out[cls_name] = full
        self.reset()
        self.detail = {'per_image': per_image, 'precision': precision, 'recall': recall}
        return out
