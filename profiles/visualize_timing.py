"""Times the detection previews on one MI355X: `Visualizer.visualize_batch` for 16 images of
512 x 512 with 150 predicted and 150 ground-truth boxes each, labels on; its parts (the host's build_primitives, the
upload plus the one launch, the copy of the finished uint8 pictures back); and, as the yardstick, the one step of the
reference's way that no host drawing code can avoid: `batch['input'].cpu()` for the same float batch
(utils/tensorboard.py:25).  Stream events around the device work, a host clock around calls that end in a synchronise;
warm-up first, then the median of `--repeats` runs.  Prints one JSON line.

    python profiles/visualize_timing.py [--repeats 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'centernet-uda_amd'))


def _events(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def _wall(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--boxes', type=int, default=150)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('visualize_timing: needs the GPU; nothing is timed without it')
    from utils.visualize import RECORD, Visualizer, launch, render
    dev = torch.device('cuda:0')
    B, S, K = args.batch, args.size, args.boxes
    rng = np.random.RandomState(0)
    classes = {i: {'name': n} for i, n in enumerate(['person', 'car', 'bicycle', 'traffic light', 'dog', 'truck'])}
    vis = Visualizer(classes, 0.3, (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835))

    def boxes(n):
        x1, y1 = rng.uniform(0, S - 40, n), rng.uniform(20, S - 40, n)
        return np.stack([x1, y1, x1 + rng.uniform(20, 200, n), y1 + rng.uniform(20, 200, n)], 1).astype(np.float32)

    dets = {'pred_boxes': np.stack([boxes(K) for _ in range(B)]),
            'pred_classes': rng.randint(0, len(classes), (B, K)).astype(np.int32),
            'pred_scores': rng.uniform(0.3, 1.0, (B, K)).astype(np.float32) + np.float32(1e-3),
            'gt_boxes': [boxes(K) for _ in range(B)],
            'gt_classes': [rng.randint(0, len(classes), K).astype(np.int32) for _ in range(B)]}
    x = torch.from_numpy(rng.uniform(-1.5, 2.0, (B, 3, S, S)).astype(np.float32)).to(dev)

    lists = [vis.build_primitives(dets['pred_boxes'][i], dets['pred_classes'][i], dets['pred_scores'][i],
                                  dets['gt_boxes'][i], dets['gt_classes'][i]) for i in range(B)]
    first = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
    prims = np.concatenate(lists)
    atlas = vis._atlas_on(dev)
    out = vis.visualize_batch(x, dets)
    assert torch.equal(out, render(x, list(range(B)), first, prims, vis.mean, vis.std, atlas))

    head = -(-(2 * B + 1) // 4) * 4
    host = np.zeros(head + len(prims) * RECORD, np.int32)
    host[:B], host[B:2 * B + 1], host[head:] = np.arange(B), first, prims.reshape(-1)
    table = torch.from_numpy(host).to(dev)
    assert torch.equal(out, launch(x, table, B, len(prims), vis.mean, vis.std, atlas))

    t0 = time.perf_counter()
    for _ in range(3):
        for i in range(B):
            vis.build_primitives(dets['pred_boxes'][i], dets['pred_classes'][i], dets['pred_scores'][i],
                                 dets['gt_boxes'][i], dets['gt_classes'][i])
    host_ms = (time.perf_counter() - t0) * 1e3 / 3

    result = {
        'shape': [B, 3, S, S], 'boxes_per_panel': K, 'primitives': int(len(prims)), 'repeats': args.repeats,
        'glyph_cell': list(vis.atlas.shape[1:]),
        'visualize_batch_ms': _wall(lambda: vis.visualize_batch(x, dets), args.repeats),
        'build_primitives_host_ms': host_ms,
        'upload_and_launch_ms': _events(lambda: render(x, list(range(B)), first, prims, vis.mean, vis.std, atlas),
                                        args.repeats),
        'launch_alone_ms': _events(lambda: launch(x, table, B, len(prims), vis.mean, vis.std, atlas), args.repeats),
        'uint8_copy_back_ms': _events(lambda: out.cpu(), args.repeats),
        'float_batch_cpu_ms': _events(lambda: x.cpu(), args.repeats),
        'note': 'triples are (median, min, max) in milliseconds',
    }
    print(json.dumps(result))


if __name__ == '__main__':
    main()
