"""One launch of every optimizer rule (csrc/optim.hip) and of adam_kernel over an arena of DLA-34's size: microseconds
and GB/s per rule, bytes per element as in DESIGN.md section 19.

    python profiles/microbench/optim_rules.py [out.jsonl]

Each timed launch works on another of SETS copies of the operands, so that the footprint between two visits of one
buffer (SETS x bytes per element x N >= 0.9 GB) exceeds the 256 MB Infinity Cache, as it does inside a training step.
The rules are timed in turn, ROUNDS times over; per rule the median over the rounds of (event time of REPS launches
/ REPS) is reported, with the minimum and maximum beside it."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'centernet-uda_amd'))
import torch
from backends import dla
from hip_runtime import ops
from hip_runtime.arena import ParamArena

SETS, REPS, ROUNDS = 4, 40, 5
dev = torch.device('cuda', 0)
N = sum((p.numel() + ParamArena.ALIGN - 1) // ParamArena.ALIGN * ParamArena.ALIGN
        for p in dla.build(num_classes=6).parameters() if p.requires_grad)
g = torch.Generator(device=dev).manual_seed(0)
sets = [{'p': torch.randn(N, device=dev, generator=g), 'g': torch.randn(N, device=dev, generator=g) * 1e-3,
         'a': torch.randn(N, device=dev, generator=g) * 1e-3, 'b': torch.rand(N, device=dev, generator=g) + 0.5,
         'c': torch.rand(N, device=dev, generator=g) + 0.5} for _ in range(SETS)]

# name -> (bytes per element, launch on one operand set); lr = 0 keeps the parameters where they are
RULES = {
    'adam_kernel': (28, lambda s: ops.adam_step_(s['p'], s['g'], s['a'], s['b'], 0.0, 0.9, 0.999, 1e-8, 1e-4, 7)),
    'sgd': (12, lambda s: ops.sgd_step_(s['p'], s['g'], None, 0.0, 0, 0, 1e-4, False, False, False)),
    'sgd_momentum': (20, lambda s: ops.sgd_step_(s['p'], s['g'], s['a'], 0.0, 0.9, 0, 1e-4, False, False, False)),
    'adamw': (28, lambda s: ops.adamw_step_(s['p'], s['g'], s['a'], s['b'], None, 0.0, 0.9, 0.999, 1e-8, 1e-2, True, False, 7)),
    'adamw_amsgrad': (36, lambda s: ops.adamw_step_(s['p'], s['g'], s['a'], s['b'], s['c'], 0.0, 0.9, 0.999, 1e-8, 1e-2, True, False, 7)),
    'rmsprop': (20, lambda s: ops.rmsprop_step_(s['p'], s['g'], s['b'], None, None, 0.0, 0.99, 1e-8, 0.0, 0.0, False)),
    'rmsprop_centered': (28, lambda s: ops.rmsprop_step_(s['p'], s['g'], s['b'], s['a'], None, 0.0, 0.99, 1e-8, 0.0, 0.0, False)),
    'rmsprop_centered_momentum': (36, lambda s: ops.rmsprop_step_(s['p'], s['g'], s['b'], s['a'], s['c'], 0.0, 0.99, 1e-8, 0.0, 0.5, False)),
}


def timed(launch):
    for i in range(SETS):
        launch(sets[i])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(REPS):
        launch(sets[i % SETS])
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / REPS          # microseconds per launch


samples = {k: [] for k in RULES}
for _ in range(ROUNDS):
    for k, (_, launch) in RULES.items():
        samples[k].append(timed(launch))
lines = []
for k, (bpe, _) in RULES.items():
    us = statistics.median(samples[k])
    lines.append({'rule': k, 'elements': N, 'bytes_per_element': bpe, 'us': round(us, 1),
                  'us_min': round(min(samples[k]), 1), 'us_max': round(max(samples[k]), 1),
                  'gb_per_s': round(bpe * N / us / 1e3, 1), 'sets': SETS, 'reps': REPS, 'rounds': ROUNDS})
    print(json.dumps(lines[-1]), flush=True)
assert all(torch.isfinite(s[k]).all() for s in sets for k in s)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        f.write(''.join(json.dumps(l) + '\n' for l in lines))
