#!/usr/bin/env python
"""Times the COCO evaluator at the validation shape: `add_batch` x 8, then `evaluate()`, for batches of 16 images of
512 x 512 with K = 150 predictions each over 6 classes, axis-aligned and rotated boxes, seeded random boxes (half of the
predictions are jittered copies of ground truths).  One warm-up evaluation, then the median of 5 repetitions, printed
beside the time of this project's numpy / Python oracle (tests/cocoeval_oracle.py) for the same batches on the same
machine -- NOT pycocotools, which this build does not depend on.  One JSON line per mode.

    python profiles/eval_timing.py [--batches 8] [--reps 5] [--oracle-batches 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'centernet-uda_amd')):
    sys.path.insert(0, p)

B, K, CLASSES, SIZE = 16, 150, 6, 512


def make_batch(rng, rotated, first_id):
    boxes, classes, scores, gt_boxes, gt_classes, gt_areas = [], [], [], [], [], []
    for _ in range(B):
        G = int(rng.randint(10, 80))
        c = rng.uniform(0, SIZE, (G, 2))
        wh = rng.choice([12, 24, 48, 96, 160], (G, 2)) * rng.uniform(0.6, 1.4, (G, 2))
        gt = np.concatenate([c, wh, rng.uniform(-90, 90, (G, 1))], 1)
        gc = rng.randint(0, CLASSES, G)
        src = rng.randint(0, G, K)
        det = gt[src] + rng.normal(0, 1, (K, 5)) * [3, 3, 3, 3, 5]
        fresh = rng.uniform(size=K) < 0.5
        det[fresh, :2] = rng.uniform(0, SIZE, (int(fresh.sum()), 2))
        det[:, 2:4] = np.abs(det[:, 2:4]) + 1
        dc = np.where(fresh, rng.randint(0, CLASSES, K), gc[src])
        if not rotated:                      # (cx, cy, w, h) -> corners
            gt = np.concatenate([gt[:, :2] - gt[:, 2:4] / 2, gt[:, :2] + gt[:, 2:4] / 2], 1)
            det = np.concatenate([det[:, :2] - det[:, 2:4] / 2, det[:, :2] + det[:, 2:4] / 2], 1)
            area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        else:
            area = gt[:, 2] * gt[:, 3]
        boxes.append(det.astype(np.float32))
        classes.append(dc.astype(np.int32))
        scores.append(rng.uniform(0, 1, K).astype(np.float32))
        gt_boxes.append(gt.astype(np.float32))
        gt_classes.append(gc.astype(np.int32))
        gt_areas.append(area.astype(np.float32))
    return {'pred_boxes': np.stack(boxes), 'pred_classes': np.stack(classes), 'pred_scores': np.stack(scores),
            'gt_boxes': gt_boxes, 'gt_classes': gt_classes, 'gt_ids': [np.int64(first_id + i) for i in range(B)],
            'gt_areas': gt_areas, 'image_shape': (3, SIZE, SIZE)}


def run(evaluator, batches, sync):
    t0 = time.perf_counter()
    for b in batches:
        evaluator.add_batch(**b)
    sync()
    t1 = time.perf_counter()
    out = evaluator.evaluate()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--oracle-batches', type=int, default=8, help='0 skips the oracle')
    args = ap.parse_args()
    import torch
    import cocoeval_oracle as co
    from evaluation.coco import Evaluator
    for rotated in (False, True):
        rng = np.random.RandomState(7)
        batches = [make_batch(rng, rotated, 1 + B * i) for i in range(args.batches)]
        ev = Evaluator()
        ev.use_rotated_boxes = rotated
        run(ev, batches, torch.cuda.synchronize)                         # warm-up
        add, evaluate, host_add = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for b in batches:
                ev.add_batch(**b)
            host_add.append(time.perf_counter() - t0)                    # add_batch returns before its kernels end
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            got = ev.evaluate()
            add.append(t1 - t0)
            evaluate.append(time.perf_counter() - t1)
        line = {'mode': 'rotated' if rotated else 'axis', 'batches': args.batches, 'images': B * args.batches,
                'add_batch_total_ms': round(1e3 * float(np.median(add)), 2),
                'add_batch_host_ms': round(1e3 * float(np.median(host_add)), 2),
                'evaluate_ms': round(1e3 * float(np.median(evaluate)), 2),
                'mAP': round(float(got['MSCOCO_Precision/mAP']), 6)}
        if args.oracle_batches:
            o = co.OracleEvaluator()
            o.use_rotated_boxes = rotated
            t_add, t_eval, want = run(o, batches[:args.oracle_batches], lambda: None)
            line.update({'oracle_batches': args.oracle_batches, 'oracle_add_batch_ms': round(1e3 * t_add, 1),
                         'oracle_evaluate_ms': round(1e3 * t_eval, 1)})
            if args.oracle_batches == args.batches:
                line['max_abs_difference'] = max(abs(got[k] - want[k]) for k in want if not np.isnan(want[k]))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
