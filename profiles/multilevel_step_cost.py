"""What a uda.MultiLevelMaxSquaresMinimization(0.3, aux_weight=0.1) step costs beside the benched
uda.MaxSquaresMinimization(0.3) step: one process, the BASELINE.json configs[3] shape (DLA-34 + DCNv2, 512 x 512, 16
source + 16 target images, Adam, bench.py's builder and synthetic batch).  Both plugins are built and warmed up first; then
the two are timed in alternating rounds of `--steps` steps, one synchronisation at either end of a round, so that
whatever else the machine does falls on both.  Appends one JSON line per plugin to profiles/multilevel_step_cost.jsonl:
the median, lowest and highest ms per step over the rounds, and the launches of one steady step (all kernels of the
library, and the guidance's own).

    python profiles/multilevel_step_cost.py [--steps 10] [--rounds 7] [--warmup 5] [--size 512] [--batch 16]

A measurement, not a check: nothing is asserted on the figures."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'centernet-uda_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

LOSS_KERNELS = ('guidance_fwd_kernel', 'guidance_grad_kernel', 'GuidanceEpilogue', 'focal_fwd_kernel', 'focal_bwd_kernel',
                'softmax_reduce_kernel', 'softmax_grad_kernel', 'ScaleEpilogue')   # *Epilogue: finalize_kernel's instances


def main():
    import torch
    import bench
    import hip_runtime as hr
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--aux-weight', type=float, default=0.1)
    ap.add_argument('--threshold', type=float, default=0.95)
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    # bench.py's table of workloads, with the multi-level form beside configs[3]'s entry (same backend, loss, optimizer)
    bench.UDA_WORKLOADS['ml_maxsq'] = ('none', lambda uda: uda.MultiLevelMaxSquaresMinimization(
        0.3, aux_weight=args.aux_weight, threshold=args.threshold), False, False, 1e-4)
    names = ('maxsq', 'ml_maxsq')
    batch = bench.synthetic_batch(args.batch, args.size, 42, device)
    plugins = {}
    for name in names:
        plugins[name] = bench.build_plugin(device, parallel=False, uda_name=name, backend_name='dla34')
        plugins[name].host_stats = False
        for _ in range(args.warmup):
            plugins[name].step(batch)
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            began = time.perf_counter()
            for _ in range(args.steps):
                plugins[name].step(batch)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - began) / args.steps)
    rows = []
    for name in names:
        with hr.launch_log() as log:
            out = plugins[name].step(batch)
            torch.cuda.synchronize()
        rows.append({'plugin': type(plugins[name]).__name__, 'size': args.size, 'batch': args.batch, 'steps': args.steps,
                     'rounds': args.rounds, 'warmup': args.warmup,
                     'ms_per_step_median': round(statistics.median(ms[name]), 3),
                     'ms_per_step_min': round(min(ms[name]), 3), 'ms_per_step_max': round(max(ms[name]), 3),
                     'launches_per_step': sum(log.counts.values()),
                     'loss_launches': {k: sum(v for n, v in log.counts.items() if k in n) for k in LOSS_KERNELS
                                       if any(k in n for n in log.counts)},
                     'stats': {k: float(v) for k, v in out['stats'].items()}})
    rows[1]['threshold'], rows[1]['aux_weight'] = args.threshold, args.aux_weight
    rows[1]['extra_ms_over_max_squares'] = round(rows[1]['ms_per_step_median'] - rows[0]['ms_per_step_median'], 3)
    rows[1]['extra_launches_over_max_squares'] = rows[1]['launches_per_step'] - rows[0]['launches_per_step']
    with open(os.path.join(ROOT, 'profiles', 'multilevel_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
