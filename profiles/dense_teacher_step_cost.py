"""What a uda.DenseTeacher step costs beside a uda.WeakStrongTeacher step: one process, the headline shape (DLA-34 +
DCNv2, 512 x 512, 16 source + 16 target images, Adam, bench.py's builder and synthetic batch).  Both plugins are built
and warmed up first; then the two are timed in alternating rounds of `--steps` steps, one synchronisation at either end of
a round, so that whatever else the machine does falls on both.  Appends to profiles/dense_teacher_step_cost.jsonl one
JSON line per plugin: the median, lowest and highest ms per step over the rounds, the launches of one steady step, and
the launches of the kernels that make the target term (decode, filter and target encoding on one side; select, loss and
gradient on the other).

    python profiles/dense_teacher_step_cost.py [--steps 10] [--rounds 7] [--warmup 5] [--size 512] [--batch 16]

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

# the shared pieces (view, EMA) and each side's own target-term kernels, by the start of their names
TERM_KERNELS = ('strong_view', 'mirror_input', 'ema_update', 'pseudo_labels', 'decode', 'nms', 'topk', 'encode',
                'sigmoid_clamp', 'focal', 'regl1', 'dense_')


def short(name):
    return name.replace('void ', '').replace('cnuda::(anonymous namespace)::', '').split('(')[0].split('<')[0].strip()


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
    ap.add_argument('--ratio', type=float, default=0.01)
    ap.add_argument('--score-threshold', type=float, default=0.1,
                    help="an untrained heat map sits near sigmoid(-2.19) = 0.1: low enough for some pseudo-labels")
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    # bench.py's table of workloads, with the two teachers beside the headline's entry (same backend, loss, optimizer)
    bench.UDA_WORKLOADS['weak_strong'] = ('none', lambda uda: uda.WeakStrongTeacher(
        1.0, score_threshold=args.score_threshold), False, False, 1e-4)
    bench.UDA_WORKLOADS['dense'] = ('none', lambda uda: uda.DenseTeacher(1.0, ratio=args.ratio), False, False, 1e-4)
    names = ('weak_strong', 'dense')
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
        term = {}
        for kernel, n in log.counts.items():
            k = short(kernel)
            if k.startswith(TERM_KERNELS):
                term[k] = term.get(k, 0) + n
        rows.append({'plugin': type(plugins[name]).__name__, 'size': args.size, 'batch': args.batch, 'steps': args.steps,
                     'rounds': args.rounds, 'warmup': args.warmup,
                     'ms_per_step_median': round(statistics.median(ms[name]), 3),
                     'ms_per_step_min': round(min(ms[name]), 3), 'ms_per_step_max': round(max(ms[name]), 3),
                     'launches_per_step': sum(log.counts.values()), 'term_launches': dict(sorted(term.items())),
                     'stats': {k: float(v) for k, v in out['stats'].items()}})
    rows[1]['ms_over_weak_strong'] = round(rows[1]['ms_per_step_median'] - rows[0]['ms_per_step_median'], 3)
    rows[1]['launches_over_weak_strong'] = rows[1]['launches_per_step'] - rows[0]['launches_per_step']
    with open(os.path.join(ROOT, 'profiles', 'dense_teacher_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
