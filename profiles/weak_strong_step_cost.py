"""What a uda.WeakStrongTeacher step costs beside a uda.MeanTeacher step, and what the strong view alone costs beside
a copy: one process, the headline shape (DLA-34 + DCNv2, 512 x 512, 16 source + 16 target images, Adam, bench.py's
builder and synthetic batch).  Both plugins are built and warmed up first; then the two are timed in alternating rounds
of `--steps` steps, one synchronisation at either end of a round, so that whatever else the machine does falls on both.
Appends to profiles/weak_strong_step_cost.jsonl one JSON line per plugin (the median, lowest and highest ms per step over
the rounds, the launches of one steady step) and one line for the kernel: the time of `strong_view` alone on
[batch, 3, size, size] under one record drawn from the default sampler, beside `torch`'s device-to-device copy of the
same tensor -- the floor of one read plus one write -- in alternating rounds as well.

    python profiles/weak_strong_step_cost.py [--steps 10] [--rounds 7] [--warmup 5] [--size 512] [--batch 16]

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

VIEW_KERNELS = ('strong_view_kernel', 'strong_view_pivot_kernel', 'mirror_input_kernel', 'ema_update_kernel',
                'pseudo_labels_kernel')


def kernel_alone(args, device):
    """ms per strong view (the pivot launch and the view launch on uploaded tables) beside ms per copy, medians over rounds"""
    import numpy as np
    import torch
    from datasets.prepare import MEAN, STD
    from datasets import strong_view as sv
    from datasets.augment import _upload
    x = torch.randn(args.batch, 3, args.size, args.size, device=device)
    y = torch.empty_like(x)
    params = sv.StrongView().sample(args.batch, args.size, args.size, np.random.default_rng([42, 0x57534B, 0]))
    # the tables are uploaded once: the timed call is the pivot launch plus the view launch, as the copy is one launch
    tables = _upload(device, np.float32(MEAN), np.float32(STD), params.photo, params.taps, params.radius, params.rects,
                     params.ids)
    contrast = bool((params.photo[:, 1] != 1).any())
    calls = {'strong_view': lambda: sv._launch(x, y, tables, int(params.radius.max()), params.seed, contrast),
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
    view, copy = statistics.median(ms['strong_view']), statistics.median(ms['copy'])
    return {'kernel': 'strong_view', 'shape': [args.batch, 3, args.size, args.size], 'calls_per_round': 10 * args.steps,
            'rounds': args.rounds, 'strong_view_ms_median': round(view, 4), 'strong_view_ms_min': round(min(ms['strong_view']), 4),
            'copy_ms_median': round(copy, 4), 'copy_ms_min': round(min(ms['copy']), 4), 'ratio_to_copy': round(view / copy, 2),
            'images_with_blur': int((params.radius > 0).sum()), 'images_with_contrast': int((params.photo[:, 1] != 1).sum()),
            'images_neutral': int(params.neutral.sum()), 'images_erased': int(params.erased.sum())}


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
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    # bench.py's table of workloads, with the two teachers beside the headline's entry (same backend, loss, optimizer)
    bench.UDA_WORKLOADS['mean_teacher'] = ('none', lambda uda: uda.MeanTeacher(1.0, score_threshold=args.score_threshold),
                                           False, False, 1e-4)
    bench.UDA_WORKLOADS['weak_strong'] = ('none', lambda uda: uda.WeakStrongTeacher(
        1.0, score_threshold=args.score_threshold), False, False, 1e-4)
    names = ('mean_teacher', 'weak_strong')
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
    rows[1]['extra_ms_over_mean_teacher'] = round(rows[1]['ms_per_step_median'] - rows[0]['ms_per_step_median'], 3)
    rows[1]['extra_launches_over_mean_teacher'] = rows[1]['launches_per_step'] - rows[0]['launches_per_step']
    del plugins, batch, out
    torch.cuda.empty_cache()
    rows.append(kernel_alone(args, device))
    with open(os.path.join(ROOT, 'profiles', 'weak_strong_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
