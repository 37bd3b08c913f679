"""What a uda.MeanTeacher step costs beside the headline EntropyMinimization step: one process, the headline shape
(DLA-34 + DCNv2, 512 x 512, 16 source + 16 target images, Adam, bench.py's builder and synthetic batch), each plugin
warmed up and then timed over the same number of steps with one synchronisation at either end.  Appends one JSON line per
plugin to profiles/mean_teacher_step_cost.jsonl: ms per step, the launches of one steady step (all kernels, the pack
kernels, the two kernels of csrc/teacher.hip) and, for the teacher, the pseudo-labels per image.

    python profiles/mean_teacher_step_cost.py [--steps 20] [--warmup 5] [--size 512] [--batch 16]

A measurement, not a check: nothing is asserted on the figures."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'centernet-uda_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def measure(name, device, args):
    import torch
    import bench
    import hip_runtime as hr
    plugin = bench.build_plugin(device, parallel=False, uda_name=name, backend_name='dla34')
    plugin.host_stats = False
    batch = bench.synthetic_batch(args.batch, args.size, 42, device)
    for _ in range(args.warmup):
        plugin.step(batch)
    torch.cuda.synchronize()
    began = time.perf_counter()
    for _ in range(args.steps):
        out = plugin.step(batch)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - began) / args.steps
    with hr.launch_log() as log:
        out = plugin.step(batch)
        torch.cuda.synchronize()
    named = lambda frag: sum(v for k, v in log.counts.items() if frag in k)
    row = {'plugin': type(plugin).__name__, 'size': args.size, 'batch': args.batch, 'steps': args.steps,
           'warmup': args.warmup, 'ms_per_step': round(ms, 3), 'launches_per_step': sum(log.counts.values()),
           'pack_launches': named('pack_kernel') + named('pack_taps_kernel'), 'pack_refresh_launches': named('pack_multi_kernel'),
           'ema_update_launches': named('ema_update_kernel'), 'pseudo_labels_launches': named('pseudo_labels_kernel'),
           'stats': {k: float(v) for k, v in out['stats'].items()}}
    del plugin, batch, out
    torch.cuda.empty_cache()
    return row


def main():
    import torch
    import bench
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--score-threshold', type=float, default=0.1,
                    help="an untrained heat map sits near sigmoid(-2.19) = 0.1: low enough for some pseudo-labels")
    args = ap.parse_args()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    # bench.py's table of workloads, with the teacher beside the headline's entry (same backend, loss and optimizer)
    bench.UDA_WORKLOADS['mean_teacher'] = ('none', lambda uda: uda.MeanTeacher(1.0, score_threshold=args.score_threshold),
                                           False, False, 1e-4)
    rows = [measure(name, device, args) for name in ('entropy', 'mean_teacher')]
    rows[1]['extra_ms_over_entropy'] = round(rows[1]['ms_per_step'] - rows[0]['ms_per_step'], 3)
    with open(os.path.join(ROOT, 'profiles', 'mean_teacher_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
