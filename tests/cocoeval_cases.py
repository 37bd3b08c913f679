"""Seeded inputs of the COCO-evaluation tests (tests/test_host_cocoeval.py, tests/test_gpu_cocoeval.py): every case is
a list of `add_batch` keyword dictionaries plus the box mode.  Shapes are the smallest that reach every index: images
of 64 x 96 (H != W), three classes, more ground truths of one class than a wave has lanes, more detections of one class
than the cut to 100, areas on both sides of 32^2 and 96^2, a class with detections only and one with ground truths
only."""
import numpy as np

H, W = 64, 96
SHAPE = (3, H, W)


def _scores(rng, n):
    s = rng.uniform(0.02, 1.0, n).astype(np.float32)
    s[::7] = np.float32(0.5)               # equal scores: the stable sorts decide
    s[3::11] = np.float32(0.1)             # exactly the threshold: kept
    return s


def _rotated_image(rng, K, G, classes):
    gt = np.stack([rng.uniform(-5, W + 5, G), rng.uniform(-5, H + 5, G), rng.uniform(2, 30, G), rng.uniform(2, 40, G),
                   rng.uniform(-90, 90, G)], 1)
    gt[::9, 4] = rng.choice([-90, 0, 45, 89.99], len(gt[::9]))
    gc = rng.randint(0, classes, G)
    src = rng.randint(0, G, K)
    det = gt[src] + np.stack([rng.normal(0, 1.5, K), rng.normal(0, 1.5, K), rng.normal(0, 1.5, K), rng.normal(0, 1.5, K),
                              rng.normal(0, 4, K)], 1)
    det[::4] = gt[src[::4]]                # exact copies: IoU 1, above min(t, 1 - 1e-10)
    det[:, 2:4] = np.abs(det[:, 2:4]) + 0.3
    dc = np.where(rng.uniform(size=K) < 0.85, gc[src], rng.randint(0, classes, K))
    return det.astype(np.float32), dc.astype(np.int32), gt.astype(np.float32), gc.astype(np.int32)


def _axis_image(rng, K, G, classes, sides=(8, 16, 24, 32, 40), grid=8, span=(0, 88)):
    """boxes on a grid: many pairs touch along an edge (zero width of the intersection) or do not overlap at all; every
    third one is moved off the grid by hundredths, so the rounding to two decimals matters"""
    def boxes(n):
        x0 = rng.randint(span[0] // grid, span[1] // grid, n) * float(grid)
        y0 = rng.randint(span[0] // grid, span[1] // grid, n) * float(grid)
        b = np.stack([x0, y0, x0 + rng.choice(sides, n), y0 + rng.choice(sides, n)], 1)
        b[::3] += rng.uniform(-3, 3, (len(b[::3]), 4)).round(3)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 0.5)
        return b
    gt = boxes(G)
    gc = rng.randint(0, classes, G)
    src = rng.randint(0, G, K)
    det = np.where(rng.uniform(size=(K, 1)) < 0.6, gt[src], boxes(K))
    det[1::4] += rng.uniform(-2, 2, (len(det[1::4]), 4))
    det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 0.5)
    dc = np.where(rng.uniform(size=K) < 0.85, gc[src], rng.randint(0, classes, K))
    return det.astype(np.float32), dc.astype(np.int32), gt.astype(np.float32), gc.astype(np.int32)


def _batch(rng, maker, B, K, first_id, shape=SHAPE, **kw):
    imgs = [maker(rng, K, **kw) for _ in range(B)]
    gts = [g for _, _, g, _ in imgs]
    if gts[0].shape[1] == 5:
        areas = [(g[:, 2] * g[:, 3]).astype(np.float32) for g in gts]         # rotated mode ignores them
    else:
        areas = [((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])).astype(np.float32) for g in gts]
    return {'pred_boxes': np.stack([d for d, _, _, _ in imgs]), 'pred_classes': np.stack([c for _, c, _, _ in imgs]),
            'pred_scores': np.stack([_scores(rng, K) for _ in imgs]), 'gt_boxes': gts,
            'gt_classes': [c for _, _, _, c in imgs], 'gt_ids': [np.int64(first_id + i) for i in range(B)],
            'gt_areas': areas, 'image_shape': shape}


def case(name):
    """-> (rotated, [add_batch kwargs, add_batch kwargs])"""
    rng = np.random.RandomState({'rotated': 1, 'axis': 2, 'many_dets': 3, 'many_gts': 4, 'areas': 5, 'lonely': 6}[name])
    if name == 'rotated':          # 3 images, 40 detections x 70 ground truths over 3 classes, twice
        return True, [_batch(rng, _rotated_image, 3, 40, 100 + 3 * b, G=70, classes=3) for b in range(2)]
    if name == 'axis':
        return False, [_batch(rng, _axis_image, 3, 40, 200 + 3 * b, G=70, classes=3) for b in range(2)]
    if name == 'many_dets':        # 130 detections of one class in one image: the cut to 100 per (image, category)
        return False, [_batch(rng, _axis_image, 1, 130, 300 + b, G=20, classes=1) for b in range(2)]
    if name == 'many_gts':         # 70 ground truths of one class: a lane owns more than one
        return True, [_batch(rng, _rotated_image, 1, 50, 400 + b, G=70, classes=1) for b in range(2)]
    if name == 'areas':            # sides around 32 and 96: areas on both sides of, and exactly at, 32^2 and 96^2
        kw = dict(G=30, classes=2, sides=(20, 31, 32, 33, 60, 95, 96, 97, 120), grid=16, span=(0, 256))
        return False, [_batch(rng, _axis_image, 2, 40, 500 + 2 * b, shape=(3, 384, 384), **kw) for b in range(2)]
    if name == 'lonely':           # class 0: detections only, class 1: ground truths only, class 2: both
        out = []
        for b in range(2):
            kw = _batch(rng, _axis_image, 2, 30, 600 + 2 * b, G=20, classes=2)
            kw['pred_classes'] = np.where(kw['pred_classes'] == 0, 0, 2).astype(np.int32)
            kw['gt_classes'] = [np.where(c == 0, 1, 2).astype(np.int32) for c in kw['gt_classes']]
            out.append(kw)
        return False, out
    raise KeyError(name)


CASES = ('rotated', 'axis', 'many_dets', 'many_gts', 'areas', 'lonely')


def hand_worked():
    """One image, one class, two 40 x 40 ground truths; detections: 0.9 on the first exactly, 0.8 on nothing, 0.7 on the
    second exactly.  AP at every threshold = (51 + 100 / 3) / 101, AR@1 = 0.5, AR@10 = AR@100 = 1; areas 1600 are
    'medium': small and large have no ground truth."""
    gt = np.array([[10, 10, 50, 50], [100, 100, 140, 140]], dtype=np.float32)
    det = np.array([[10, 10, 50, 50], [200, 200, 240, 240], [100, 100, 140, 140]], dtype=np.float32)
    return {'pred_boxes': det[None], 'pred_classes': np.zeros((1, 3), np.int32),
            'pred_scores': np.array([[0.9, 0.8, 0.7]], np.float32), 'gt_boxes': [gt], 'gt_classes': [np.zeros(2, np.int32)],
            'gt_ids': [np.int64(7000)], 'gt_areas': [np.array([1600, 1600], np.float32)], 'image_shape': (3, 256, 256)}


HAND_AP = (51 + 100 / 3) / 101
