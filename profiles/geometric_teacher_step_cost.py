"""What a uda.GeometricTeacher step costs beside a uda.WeakStrongTeacher step, and what the warp alone costs beside a
copy: one process, the headline shape (DLA-34 + DCNv2, 512 x 512, 16 source + 16 target images, Adam, bench.py's builder
and synthetic batch).  Both plugins are built and warmed up first; then the two are timed in alternating rounds of
`--steps` steps, one synchronisation at either end of a round, so that whatever else the machine does falls on both.
Appends to profiles/geometric_teacher_step_cost.jsonl one JSON line per plugin (the median, lowest and highest ms per step
over the rounds, the launches of one steady step) and one line for the kernel: the time of `warp_batch`'s launch alone on
[batch, 3, size, size] under a 30 degree / 0.9 / 5 % similarity, beside `torch`'s device-to-device copy of the same tensor
-- the floor of one read plus one write -- in alternating rounds as well.

    python profiles/geometric_teacher_step_cost.py [--steps 10] [--rounds 7] [--warmup 5] [--size 512] [--batch 16]

A measurement, not a check: nothing is asserted on the figures.  The model is untrained, so its pseudo-labels mean
nothing and `pseudo_boxes` may be 0: the figures say what the view costs, not what it is worth."""
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

VIEW_KERNELS = ('warp_bilinear_kernel', 'labels_transform_kernel', 'labels_totals_kernel', 'strong_view_kernel',
                'strong_view_pivot_kernel', 'mirror_input_kernel', 'ema_update_kernel', 'pseudo_labels_kernel')


def kernel_alone(args, device):
    """ms per warp (the launch on an uploaded matrix table) beside ms per copy, medians over rounds"""
    import numpy as np
    import torch
    from datasets.augment import _upload
    from datasets.geometric_view import similarity_matrices
    from hip_runtime import check, lib, ptr, stream
    B, S = args.batch, args.size
    x = torch.randn(B, 3, S, S, device=device)
    y = torch.empty_like(x)
    inverse = np.tile(similarity_matrices(S, S, 30.0, 0.9, (0.05, 0.05))[1][:2].reshape(1, 6), (B, 1))
    table, = _upload(device, np.ascontiguousarray(inverse))         # uploaded once: the timed call is one launch, as the copy is
    calls = {'warp': lambda: check(lib().cnuda_warp_bilinear(ptr(x), ptr(y), ptr(table), 0.0, B, 3, S, S, stream()), 'warp'),
             'copy': lambda: y.copy_(x)}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            began = time.perf_counter()
            for _ in range(10 * args.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - began) / (10 * args.steps))
    warp, copy = statistics.median(ms['warp']), statistics.median(ms['copy'])
    moved = 2 * x.numel() * 4                                       # one read and one write of the tensor
    return {'kernel': 'warp_bilinear', 'shape': [B, 3, S, S], 'transform': {'rotate': 30.0, 'scale': 0.9, 'translate_percent': 0.05},
            'calls_per_round': 10 * args.steps, 'rounds': args.rounds, 'warp_ms_median': round(warp, 4),
            'warp_ms_min': round(min(ms['warp']), 4), 'warp_ms_max': round(max(ms['warp']), 4),
            'copy_ms_median': round(copy, 4), 'copy_ms_min': round(min(ms['copy']), 4), 'copy_ms_max': round(max(ms['copy']), 4),
            'ratio_to_copy': round(warp / copy, 2), 'algorithmic_bytes': moved,
            'warp_GBps_of_algorithmic_bytes': round(moved / warp / 1e6, 1),
            'copy_GBps_of_algorithmic_bytes': round(moved / copy / 1e6, 1)}


def main():
    import torch
    import bench
    import hip_runtime as hr
    from datasets.prepare import MEAN, STD
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--score-threshold', type=float, default=0.1,
                    help="an untrained heat map sits near sigmoid(-2.19) = 0.1: low enough for some pseudo-labels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometric_teacher_step_cost: no GPU; the figures are measured on the MI355X or not at all")
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    # bench.py's table of workloads, with the two teachers beside the headline's entry (same backend, loss, optimizer)
    bench.UDA_WORKLOADS['weak_strong'] = ('none', lambda uda: uda.WeakStrongTeacher(
        1.0, score_threshold=args.score_threshold), False, False, 1e-4)
    bench.UDA_WORKLOADS['geometric'] = ('none', lambda uda: uda.GeometricTeacher(
        1.0, score_threshold=args.score_threshold), False, False, 1e-4)
    names = ('weak_strong', 'geometric')
    batch = bench.synthetic_batch(args.batch, args.size, 42, device)
    plugins = {}
    for name in names:
        plugins[name] = bench.build_plugin(device, parallel=False, uda_name=name, backend_name='dla34')
        plugins[name].host_stats = False
        plugins[name].cfg['seed'] = 42
        plugins[name].cfg['normalize'] = bench._Cfg(mean=list(MEAN), std=list(STD))
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
                     'view_launches': {k: sum(v for n, v in log.counts.items() if k + '(' in n or n.endswith(k))
                                       for k in VIEW_KERNELS if any(k in n for n in log.counts)},
                     'stats': {k: float(v) for k, v in out['stats'].items()}})
    rows[1]['extra_ms_over_weak_strong'] = round(rows[1]['ms_per_step_median'] - rows[0]['ms_per_step_median'], 3)
    rows[1]['extra_launches_over_weak_strong'] = rows[1]['launches_per_step'] - rows[0]['launches_per_step']
    del plugins, batch, out
    torch.cuda.empty_cache()
    rows.append(kernel_alone(args, device))
    with open(os.path.join(ROOT, 'profiles', 'geometric_teacher_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
