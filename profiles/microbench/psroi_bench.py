"""Deformable PSROI pooling (csrc/psroi.hip) on one MI355X: the workload for a kernel trace, and the table made of it.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/microbench/psroi_bench.py --shape large
    python profiles/microbench/psroi_bench.py --shape large --stats DIR/*/*kernel_stats.csv [--out FILE]

The second form prints one JSON line per kernel: average microseconds, the kernel's algorithmic bytes (SURVEY 8d:
tensors in, tensors out, each once) and the fraction of the 8 TB/s HBM peak that makes."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'centernet-uda_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12
#            B  OD  G  H   W   N    P  S  scale
SHAPES = {'example_dpooling': (2, 32, 1, 64, 64, 20, 7, 4, 0.25),          # testcuda.py:183-223
          'large': (4, 10, 7, 40, 64, 300, 7, 4, 0.23)}


def algorithmic_bytes(shape):
    B, OD, G, H, W, N, P, S, _ = SHAPES[shape]
    x = 4 * B * OD * G * G * H * W
    bins = 4 * N * OD * P * P
    trans, rois = 4 * N * 2 * P * P, 4 * N * 5
    return {'psroi_bins_kernel<false>': x + rois + trans + 2 * bins,                 # input -> output, count
            'psroi_bins_kernel<true>': x + rois + trans + 2 * bins + 2 * bins,       # input, grad, count -> 2 partial sums
            'psroi_offset_reduce_kernel': 2 * bins + trans,
            'psroi_roi_lists_kernel': rois + 4 * (B + B * N),
            'psroi_grad_input_kernel': 2 * bins + rois + trans + 4 * (B + B * N) + x}


def run(shape, iters):
    import torch
    import _ext
    B, OD, G, H, W, N, P, S, scale = SHAPES[shape]
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, OD * G * G, H, W, generator=g).to(dev)
    x1, y1 = torch.rand(N, generator=g) * W / scale * 0.8, torch.rand(N, generator=g) * H / scale * 0.8
    w, h = torch.rand(N, generator=g) * W / scale * 0.5, torch.rand(N, generator=g) * H / scale * 0.5
    rois = torch.stack((torch.randint(B, (N,), generator=g).float(), x1, y1, x1 + w, y1 + h), dim=1).to(dev)
    off = torch.randn(N, 2, P, P, generator=g).to(dev)
    go = torch.randn(N, OD, P, P, generator=g).to(dev)
    args = (0, scale, OD, G, P, P, S, 0.1)
    for _ in range(iters):
        out, count = _ext.dcn_v2_psroi_pooling_forward(x, rois, off, *args)
        _ext.dcn_v2_psroi_pooling_backward(go, x, rois, off, count, *args)
    torch.cuda.synchronize()


def table(shape, stats_csv, out):
    want = algorithmic_bytes(shape)
    lines = []
    for r in csv.DictReader(open(stats_csv)):
        name = r['Name'].replace('void ', '').replace('cnuda::(anonymous namespace)::', '').split('(')[0].strip()
        if name not in want:
            continue
        us = float(r['AverageNs']) / 1e3
        lines.append({'shape': shape, 'dims': dict(zip('B OD G H W N P S scale'.split(), SHAPES[shape])), 'kernel': name,
                      'calls': int(r['Calls']), 'avg_us': round(us, 2), 'algorithmic_MB': round(want[name] / 1e6, 3),
                      'GB_per_s': round(want[name] / us / 1e3, 1),
                      'fraction_of_8TBps': round(want[name] / (us * 1e-6) / HBM_PEAK, 4)})
    for rec in lines:
        print(json.dumps(rec))
    if out:
        with open(out, 'a') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=list(SHAPES), required=True)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--stats', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.stats:
        table(a.shape, a.stats, a.out)
    else:
        run(a.shape, a.iters)
