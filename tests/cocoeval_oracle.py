"""Independent oracle of evaluation/coco.py: COCO detection metrics by plain loops over dictionaries, following
COCOeval's per-image and per-category procedure literally (sequential matching scan with its early exit, accumulation
per category / area range / detection limit).  Masks of rotated boxes are full boolean images filled by
utils.image._fill_convex_poly -- the project's mask rule -- and their intersections np.logical_and(...).sum().
Shares no code with evaluation/coco.py beyond that fill routine and utils.box.rotate_bbox."""
import numpy as np

from utils.box import rotate_bbox
from utils.image import _fill_convex_poly

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = [1, 10, 100]
AREA_RANGES = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_LABELS = ['all', 'small', 'medium', 'large']


def quad_mask(verts, H, W):
    """bool [H, W]: the mask rule on four integer (x, y) vertices"""
    img = np.zeros((H, W), dtype=bool)
    _fill_convex_poly(img, [(int(x) << 16, int(y) << 16) for x, y in verts])
    return img


def sweep_boxes(n=4000, seed=0, size=128):
    """The row-hole sweep's boxes [n, 5] float32 (cx, cy, w, h, angle) for a size x size image."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-10, size + 10, (n, 2))
    w = rng.choice([0.3, 1, 2, 3, 5, 17, 40, 90], n) * rng.uniform(0.5, 1.5, n)
    h = w + rng.uniform(0, 60, n)
    ang = rng.uniform(-90, 90, n)
    ang[::5] = rng.choice([-90, -45, 0, 45, 89.99], len(ang[::5]))
    return np.concatenate([c, w[:, None], h[:, None], ang[:, None]], 1).astype(np.float32)


def mask_rows(mask):
    """-> (left [H], right [H], holes): first / last set column per row (0, -1 for an empty row), rows with a gap"""
    H = mask.shape[0]
    left, right, holes = np.zeros(H, np.int64), -np.ones(H, np.int64), 0
    for r in range(H):
        cols = np.flatnonzero(mask[r])
        if len(cols):
            left[r], right[r] = cols[0], cols[-1]
            holes += int(cols[-1] - cols[0] + 1 != len(cols))
    return left, right, holes


def box_iou(d, g):
    """pycocotools' bbIou for two non-crowd [x, y, w, h] boxes, in Python floats (IEEE double, no fused multiply-add)"""
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    return i / (dw * dh + gw * gh - i)


def mask_iou(d, g):
    i = int(np.logical_and(d['mask'], g['mask']).sum())
    u = d['area'] + g['area'] - i
    return i / u if u > 0 else 0.0


def evaluate_img(dt, gt, ious, area_range, thrs=IOU_THRS):
    """COCOeval.evaluateImg for non-crowd annotations.  dt: detections in score order (already cut), gt: ground truths,
    ious[d][g] in these orders.  -> dict(matched [T][D] bool, dt_ignore [T][D] bool, gt_ignore [G] bool, match [T][D])"""
    lo, hi = area_range
    ig = [bool(float(g['area']) < lo or float(g['area']) > hi) for g in gt]
    order = sorted(range(len(gt)), key=lambda i: ig[i])          # non-ignored first, stable
    T, D, G = len(thrs), len(dt), len(gt)
    gtm = [[False] * G for _ in range(T)]                        # by position in `order`
    dtm = [[-1] * D for _ in range(T)]
    dtig = [[False] * D for _ in range(T)]
    for t, thr in enumerate(thrs):
        for d in range(D):
            best, m = min(float(thr), 1 - 1e-10), -1
            for pos, gi in enumerate(order):
                if gtm[t][pos]:
                    continue
                if m > -1 and not ig[order[m]] and ig[gi]:
                    break
                if ious[d][gi] < best:
                    continue
                best, m = ious[d][gi], pos
            if m == -1:
                continue
            dtig[t][d] = ig[order[m]]
            dtm[t][d] = order[m]
            gtm[t][m] = True
    for d in range(D):
        outside = bool(float(dt[d]['area']) < lo or float(dt[d]['area']) > hi)
        for t in range(T):
            dtig[t][d] = dtig[t][d] or (dtm[t][d] == -1 and outside)
    return {'matched': [[m > -1 for m in row] for row in dtm], 'dt_ignore': dtig, 'gt_ignore': ig, 'match': dtm,
            'scores': [d['score'] for d in dt]}


_NAMES = [('ap', None, 'all', 100, 'Precision/{m}AP'), ('ap', 0.5, 'all', 100, 'Precision/{m}AP.50IOU'),
          ('ap', 0.75, 'all', 100, 'Precision/{m}AP.75IOU'), ('ar', None, 'all', 1, 'Recall/{m}AR1'),
          ('ar', None, 'all', 10, 'Recall/{m}AR10'), ('ar', None, 'all', 100, 'Recall/{m}AR100'),
          ('ap', None, 'small', 100, 'Precision/mAP_small'), ('ap', None, 'medium', 100, 'Precision/mAP_medium'),
          ('ap', None, 'large', 100, 'Precision/mAP_large'), ('ar', None, 'small', 100, 'Recall/{m}AR100_small'),
          ('ar', None, 'medium', 100, 'Recall/{m}AR100_medium'), ('ar', None, 'large', 100, 'Recall/{m}AR100_large')]


class OracleEvaluator:
    _known_ids = []

    def __init__(self, per_class=True, score_threshold=0.1):
        self.per_class, self.score_threshold = per_class, score_threshold
        self.classes, self.num_workers, self.use_rotated_boxes = None, None, False
        self.existent_labels = {}
        self.reset()

    def reset(self):
        self.images, self.dts, self.gts = [], {}, {}
        self.detail = {}

    def _anno(self, box, label, image_id, score, area, shape):
        a = {'image_id': image_id, 'category_id': int(label)}
        if self.use_rotated_boxes:
            a['mask'] = quad_mask(rotate_bbox(*box), shape[1], shape[2])
            a['area'] = int(a['mask'].sum())
        else:
            x_min, y_min, x_max, y_max = box[:4]
            height, width = y_max - y_min, x_max - x_min
            a['bbox'] = [np.round(x_min, 2), np.round(y_min, 2), np.round(width, 2), np.round(height, 2)]
            a['area'] = height * width if area is None else area
        if score is not None:
            a['score'] = score
        return a

    def add_batch(self, pred_boxes, pred_classes, pred_scores, gt_boxes, gt_classes, gt_ids, gt_areas, image_shape,
                  pred_kps=None, gt_kps=None):
        for i, gid in enumerate(gt_ids):
            gid = int(gid)
            if gid not in OracleEvaluator._known_ids:
                OracleEvaluator._known_ids.append(gid)
            image_id = OracleEvaluator._known_ids.index(gid) + 1
            if image_id in self.images:
                raise ValueError('image id %r was already added to this evaluation' % gid)
            self.images.append(image_id)
            for bb, lb, sc in zip(pred_boxes[i], pred_classes[i], pred_scores[i]):
                if np.float32(sc) < np.float32(self.score_threshold):
                    continue
                self.dts.setdefault((image_id, int(lb)), []).append(self._anno(bb, lb, image_id, sc, None, image_shape))
                self.existent_labels[int(lb)] = True
            for bb, lb, ar in zip(gt_boxes[i], gt_classes[i], gt_areas[i]):
                self.gts.setdefault((image_id, int(lb)), []).append(self._anno(bb, lb, image_id, None, ar, image_shape))
                self.existent_labels[int(lb)] = True

    def per_image(self):
        """-> {(image id, category): dict(dt, gt, ious, ranges: [evaluate_img result per area range])}"""
        out = {}
        for key in sorted(set(self.dts) | set(self.gts)):
            dt, gt = self.dts.get(key, []), self.gts.get(key, [])
            order = np.argsort([-d['score'] for d in dt], kind='mergesort')
            dt = [dt[i] for i in order][:MAX_DETS[-1]]
            if self.use_rotated_boxes:
                ious = [[mask_iou(d, g) for g in gt] for d in dt]
            else:
                ious = [[box_iou(d['bbox'], g['bbox']) for g in gt] for d in dt]
            out[key] = {'dt': dt, 'gt': gt, 'ious': ious,
                        'ranges': [evaluate_img(dt, gt, ious, rng) for rng in AREA_RANGES]}
        return out

    def accumulate(self, per_image, cats):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cats), len(AREA_RANGES), len(MAX_DETS)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        for k, cat in enumerate(cats):
            for a in range(A):
                for m, max_det in enumerate(MAX_DETS):
                    E = [per_image[(img, cat)]['ranges'][a] for img in sorted(self.images) if (img, cat) in per_image]
                    if not E:
                        continue
                    scores = np.concatenate([np.asarray(e['scores'][:max_det], dtype=np.float32) for e in E])
                    inds = np.argsort(-scores, kind='mergesort')
                    dtm = np.concatenate([np.asarray(e['matched'], dtype=bool).reshape(T, -1)[:, :max_det] for e in E], 1)[:, inds]
                    dtig = np.concatenate([np.asarray(e['dt_ignore'], dtype=bool).reshape(T, -1)[:, :max_det] for e in E], 1)[:, inds]
                    gtig = np.concatenate([np.asarray(e['gt_ignore'], dtype=bool) for e in E])
                    npig = np.count_nonzero(~gtig)
                    if npig == 0:
                        continue
                    tps, fps = np.logical_and(dtm, ~dtig), np.logical_and(~dtm, ~dtig)
                    tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(float), np.cumsum(fps, axis=1).astype(float)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        q = np.zeros(R)
                        for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                            if pi < nd:
                                q[ri] = pr[pi]
                        precision[t, :, k, a, m] = q
        return precision, recall

    @staticmethod
    def summarize(precision, recall, ap, iou_thr, area, max_det):
        a, m = AREA_LABELS.index(area), MAX_DETS.index(max_det)
        v = (precision if ap else recall).copy()
        if iou_thr is not None:
            v = v[iou_thr == IOU_THRS]
        v = v[:, :, :, a, m] if ap else v[:, :, a, m]
        v[v == -1] = np.nan
        v = v.reshape(-1, v.shape[-1])
        per_class = np.full(v.shape[1], np.nan)
        for k in range(v.shape[1]):
            col = v[:, k][~np.isnan(v[:, k])]
            if len(col):
                per_class[k] = col.mean()
        have = per_class[~np.isnan(per_class)]
        return per_class, (have.mean() if len(have) else np.nan)

    def evaluate(self):
        cats = sorted(self.existent_labels)
        per_image = self.per_image()
        precision, recall = self.accumulate(per_image, cats)
        out = {}
        for kind, thr, area, max_det, name in _NAMES:
            per_class, mean = self.summarize(precision, recall, kind == 'ap', thr, area, max_det)
            full = np.full(max(cats) + 1, np.nan)
            full[cats] = per_class
            out['MSCOCO_' + name.replace('{m}', 'm')] = mean
            cls_name = 'MSCOCO_Class_{}/' + name.replace('{m}', '')
            if self.per_class:
                for c in cats:
                    label = self.classes[c]['name'] if self.classes is not None and c in self.classes else c
                    out[cls_name.format(str(label))] = full[c]
            else:
                out[cls_name] = full
        self.reset()
        self.detail = {'per_image': per_image, 'precision': precision, 'recall': recall}      # for the tests
        return out
