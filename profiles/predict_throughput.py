"""Time predict.predict_files on generated PNGs (profiles/make_driver_dataset.py's pictures, 640 x 480): the headline
model (DLA-34, 6 classes, 512 x 512, random weights), batch 16, 16 decoding threads, in three modes -- plain, --flip,
and --flip --scales 0.75,1,1.25 -- and append one line per mode to profiles/predict_throughput.jsonl:

    images per second: a host clock around a whole pass over the files (decoding, upload, network, merge, read-back),
        ended by the generator's last device-to-host copy; the median of the timed passes, every pass listed;
    launch share: of the library's kernel launches in one more pass (hip_runtime.launch_log), the part that are the
        prediction kernels of csrc/predict.hip -- a count of launches, not of time.

    yardstick: a fourth line, the same backend through export.CenterNet (eval forward + decode) on a batch that is
        resident in HBM, timed with device events as bench.py --full's `inference` leg does -- what the network
        alone allows, without files, upload, resize or projection.

    python profiles/predict_throughput.py [--images 384] [--passes 5] [--out profiles/predict_throughput.jsonl]

Needs the GPU; there is no fallback.  Recorded, not asserted anywhere.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, 'centernet-uda_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_driver_dataset   # noqa: E402

MODES = (('plain', {}),
         ('flip', {'flip': True}),
         ('flip_scales_0.75_1_1.25', {'flip': True, 'scales': (0.75, 1.0, 1.25)}))
NEW_KERNELS = ('mirror_input_kernel', 'tta_merge_kernel', 'project_detections_kernel', 'soft_nms_class_kernel',
               'soft_nms_order_kernel')


def one_pass(predict, predictor, files, batch, device):
    torch.cuda.synchronize(device)
    began = time.perf_counter()
    detections = sum(len(r['scores']) for r in predict.predict_files(predictor, files, batch_size=batch, num_workers=16,
                                                                     device=device))
    torch.cuda.synchronize(device)
    return time.perf_counter() - began, detections


def resident_inference(backend, size, batch, device, calls=20):
    from export import CenterNet
    model = CenterNet(backend, 150).eval()
    x = torch.randn(batch, 3, size, size, device=device)
    for _ in range(3):
        model(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    e0.record()
    for _ in range(calls):
        model(x)
    e1.record()
    torch.cuda.synchronize(device)
    ms = e0.elapsed_time(e1) / calls
    return {'what': 'export.CenterNet on a resident batch (eval forward + decode)', 'batch': batch, 'calls': calls,
            'ms_per_batch': ms, 'images_per_second': batch / (ms * 1e-3), 'device': torch.cuda.get_device_name(device)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=384)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(HERE, 'predict_throughput.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predict_throughput.py measures on the GPU; none is visible")
    import hip_runtime as hr
    import predict
    from backends import dla
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    backend = dla.build(num_classes=6).to(device).eval()
    with tempfile.TemporaryDirectory() as tmp:
        folder, _ = make_driver_dataset.split(tmp, 'val', args.images, np.random.default_rng(0), 6, 1)
        files = predict.expand_files([folder])
        lines = []
        for name, options in MODES:
            predictor = predict.Predictor(backend, (512, 512), max_detections=150, score_threshold=0.1, **options)
            one_pass(predict, predictor, files[:2 * args.batch], args.batch, device)          # every shape once
            timed = [one_pass(predict, predictor, files, args.batch, device) for _ in range(args.passes)]
            with hr.launch_log() as log:
                one_pass(predict, predictor, files, args.batch, device)
            launches = sum(log.counts.values())
            new = {k: sum(v for name_, v in log.counts.items() if k in name_) for k in NEW_KERNELS}
            seconds = [t for t, _ in timed]
            lines.append({'what': 'predict_files', 'mode': name, 'model': 'dla34, 6 classes, 512x512, random weights',
                          'images': len(files), 'image_size': [make_driver_dataset.H, make_driver_dataset.W],
                          'batch': args.batch, 'num_workers': 16,
                          'images_per_second': len(files) / statistics.median(seconds),
                          'pass_seconds': seconds, 'detections_per_pass': timed[0][1],
                          'kernel_launches_per_pass': launches, 'new_kernel_launches': new,
                          'new_kernel_launch_share': sum(new.values()) / max(launches, 1),
                          'device': torch.cuda.get_device_name(device)})
            print(json.dumps(lines[-1]), flush=True)
    lines.append(resident_inference(backend, 512, args.batch, device))
    print(json.dumps(lines[-1]), flush=True)
    with open(args.out, 'a') as f:
        for line in lines:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
