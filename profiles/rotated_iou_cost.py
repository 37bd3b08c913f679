#!/usr/bin/env python
"""Times the COCO evaluator's two ways of measuring rotated boxes at the shape of the rotated benchmark configuration
(BASELINE.json configs[4]: 640 x 640, 16 images; 150 detections and 150 ground truths per image over 6 classes, seeded
random boxes, half of the detections jittered copies of ground truths): `rotated_iou = 'mask'` (row spans of rasterised
masks) and `'polygon'` (exact polygon IoU), in one process.  One warm-up evaluation per mode, then the median of
`--reps` repetitions of `add_batch` + `evaluate()` on a host clock, with the library's launch counts of one repetition.
One JSON line per mode, appended to profiles/rotated_iou_cost.jsonl.  Recorded, asserted nowhere.

    python profiles/rotated_iou_cost.py [--reps 7] [--out profiles/rotated_iou_cost.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'centernet-uda_amd'))

B, K, GT, CLASSES, SIZE = 16, 150, 150, 6, 640


def make_batch(rng):
    boxes, classes, scores, gt_boxes, gt_classes, gt_areas = [], [], [], [], [], []
    for _ in range(B):
        c = rng.uniform(0, SIZE, (GT, 2))
        wh = rng.choice([12, 24, 48, 96, 160], (GT, 2)) * rng.uniform(0.6, 1.4, (GT, 2))
        gt = np.concatenate([c, wh, rng.uniform(-90, 90, (GT, 1))], 1)
        gc = rng.randint(0, CLASSES, GT)
        src = rng.randint(0, GT, K)
        det = gt[src] + rng.normal(0, 1, (K, 5)) * [3, 3, 3, 3, 5]
        fresh = rng.uniform(size=K) < 0.5
        det[fresh, :2] = rng.uniform(0, SIZE, (int(fresh.sum()), 2))
        det[:, 2:4] = np.abs(det[:, 2:4]) + 1
        boxes.append(det.astype(np.float32))
        classes.append(np.where(fresh, rng.randint(0, CLASSES, K), gc[src]).astype(np.int32))
        scores.append(rng.uniform(0.1, 1, K).astype(np.float32))
        gt_boxes.append(gt.astype(np.float32))
        gt_classes.append(gc.astype(np.int32))
        gt_areas.append((gt[:, 2] * gt[:, 3]).astype(np.float32))
    return {'pred_boxes': np.stack(boxes), 'pred_classes': np.stack(classes), 'pred_scores': np.stack(scores),
            'gt_boxes': gt_boxes, 'gt_classes': gt_classes, 'gt_ids': [np.int64(1 + i) for i in range(B)],
            'gt_areas': gt_areas, 'image_shape': (3, SIZE, SIZE)}


def kernel_name(symbol):
    """demangled symbol -> the kernel's own name"""
    return symbol.replace('void ', '').replace('cnuda::(anonymous namespace)::', '').replace('cnuda::', '').split('(')[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rotated_iou_cost.jsonl'))
    args = ap.parse_args()
    import torch
    import hip_runtime as hr
    from evaluation.coco import Evaluator
    batch = make_batch(np.random.RandomState(7))
    lines = []
    for mode in ('mask', 'polygon'):
        ev = Evaluator()
        ev.use_rotated_boxes, ev.rotated_iou = True, mode
        ev.add_batch(**batch)
        ev.evaluate()                                                    # warm-up
        torch.cuda.synchronize()
        total, host_add, device = [], [], []
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            start.record()
            ev.add_batch(**batch)
            stop.record()
            host_add.append(time.perf_counter() - t0)                    # add_batch returns before its kernels end
            got = ev.evaluate()                                          # synchronises once
            total.append(time.perf_counter() - t0)
            device.append(start.elapsed_time(stop))                      # uploads and kernels of add_batch on the stream
        with hr.launch_log() as log:
            ev.add_batch(**batch)
            ev.evaluate()
        lines.append({'rotated_iou': mode, 'images': B, 'detections_per_image': K, 'ground_truths_per_image': GT,
                      'image_size': SIZE, 'reps': args.reps,
                      'add_batch_plus_evaluate_ms': round(1e3 * float(np.median(total)), 3),
                      'add_batch_host_ms': round(1e3 * float(np.median(host_add)), 3),
                      'add_batch_stream_ms': round(float(np.median(device)), 3),
                      'launches': int(sum(log.counts.values())),
                      'kernels': {kernel_name(k): v for k, v in sorted(log.counts.items())},
                      'mAP': round(float(got['MSCOCO_Precision/mAP']), 6),
                      'mAP.50IOU': round(float(got['MSCOCO_Precision/mAP.50IOU']), 6),
                      'device': torch.cuda.get_device_name(0)})
    with open(args.out, 'a') as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
