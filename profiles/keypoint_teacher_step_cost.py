"""What a uda.KeypointTeacher step costs beside a uda.GeometricTeacher step: one process, the headline shape (DLA-34 +
DCNv2, 512 x 512, 16 source + 16 target images, Adam, bench.py's builder and synthetic batch).  The two models are NOT
the same: the keypoint teacher needs a keypoint model, so it runs DLA-34 with J = 17 joints (the `kps` head, its loss term
on both halves, the keypoint decode) beside DLA-34 with J = 0 under GeometricTeacher.  The difference therefore includes
the extra head and its loss, not only the two keypoint kernels.  Both plugins are built and warmed up first; then the two
are timed in alternating rounds of `--steps` steps, one synchronisation at either end of a round, so that whatever else
the machine does falls on both.  Appends to profiles/keypoint_teacher_step_cost.jsonl one JSON line per plugin: the median,
lowest and highest ms per step over the rounds, the launches of one steady step and those of the teacher-side kernels.

    python profiles/keypoint_teacher_step_cost.py [--steps 10] [--rounds 7] [--warmup 5] [--size 512] [--batch 16]

A measurement, not a check: nothing is asserted on the figures.  The models are untrained, so their pseudo-labels mean
nothing and `pseudo_boxes` may be 0 (the label kernels then run on empty tables): the figures say what the path costs, not
what it is worth."""
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

JOINTS = 17
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
TEACHER_KERNELS = ('warp_bilinear_kernel', 'labels_transform_kernel', 'labels_totals_kernel', 'labels_transform_kps_kernel',
                   'labels_totals_kps_kernel', 'pseudo_labels_kernel', 'pseudo_labels_kps_kernel', 'decode_kps_kernel',
                   'strong_view_kernel', 'strong_view_pivot_kernel', 'ema_update_kernel')


def keypoint_plugin(bench, device, score_threshold):
    """bench.build_plugin's recipe for DLA-34 with JOINTS joints under uda.KeypointTeacher (bench.py builds no keypoint
    model): the same seed, DCN offset initialisation, loss weights and optimizer, plus `kp_weight` 1."""
    import warnings
    import torch
    import uda
    from backends import dla
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        backend = dla.build(num_classes=bench.NUM_CLASSES, num_keypoints=JOINTS)
    with torch.no_grad():
        for n, p in backend.named_parameters():
            if 'conv_offset_mask.weight' in n:
                p.normal_(0, 0.5 / (p.shape[1] * 9) ** 0.5)
    plugin = uda.KeypointTeacher(1.0, flip_pairs=FLIP_PAIRS, score_threshold=score_threshold)
    plugin.cfg = bench._Cfg(max_detections=bench.MAX_OBJS, model=bench._Cfg(backend=bench._Cfg(params=bench._Cfg(
        rotated_boxes=False, num_classes=bench.NUM_CLASSES, num_keypoints=JOINTS))))
    plugin.backend, plugin.device = backend, device
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, kp_weight=1.0)
    plugin.optimizer = optim.Adam([p for p in backend.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
    plugin.init_done()
    plugin.to(device, False)
    plugin.set_phase(True)
    return plugin


def main():
    import numpy as np
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
        raise SystemExit("keypoint_teacher_step_cost: no GPU; the figures are measured on the MI355X or not at all")
    device = torch.device('cuda', 0)
    torch.cuda.set_device(device)
    bench.UDA_WORKLOADS['geometric'] = ('none', lambda uda: uda.GeometricTeacher(
        1.0, score_threshold=args.score_threshold), False, False, 1e-4)
    batch = bench.synthetic_batch(args.batch, args.size, 42, device)
    # the keypoint model's source batch: the same, plus joint offsets for the rows that hold an object
    rs = np.random.RandomState(43)
    kp_batch = dict(batch)
    kp_batch['kps'] = torch.from_numpy(
        rs.uniform(-8, 8, (args.batch, bench.MAX_OBJS, 2 * JOINTS)).astype(np.float32)).to(device)
    kp_batch['kp_reg_mask'] = batch['reg_mask'].to(torch.uint8)[..., None].repeat(1, 1, 2 * JOINTS).contiguous()
    plugins = {'geometric': bench.build_plugin(device, parallel=False, uda_name='geometric', backend_name='dla34'),
               'keypoint': keypoint_plugin(bench, device, args.score_threshold)}
    batches = {'geometric': batch, 'keypoint': kp_batch}
    names = tuple(plugins)
    for name in names:
        plugins[name].host_stats = False
        plugins[name].cfg['seed'] = 42
        plugins[name].cfg['normalize'] = bench._Cfg(mean=list(MEAN), std=list(STD))
        for _ in range(args.warmup):
            plugins[name].step(batches[name])
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            began = time.perf_counter()
            for _ in range(args.steps):
                plugins[name].step(batches[name])
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - began) / args.steps)
    rows = []
    for name in names:
        with hr.launch_log() as log:
            out = plugins[name].step(batches[name])
            torch.cuda.synchronize()
        rows.append({'plugin': type(plugins[name]).__name__, 'backend': 'dla34', 'num_keypoints': JOINTS if name == 'keypoint' else 0,
                     'size': args.size, 'batch': args.batch, 'steps': args.steps, 'rounds': args.rounds, 'warmup': args.warmup,
                     'ms_per_step_median': round(statistics.median(ms[name]), 3),
                     'ms_per_step_min': round(min(ms[name]), 3), 'ms_per_step_max': round(max(ms[name]), 3),
                     'launches_per_step': sum(log.counts.values()),
                     'teacher_launches': {k: sum(v for n, v in log.counts.items() if k + '(' in n or n.endswith(k))
                                          for k in TEACHER_KERNELS if any(k + '(' in n or n.endswith(k) for n in log.counts)},
                     'stats': {k: float(v) for k, v in out['stats'].items()}})
    rows[1]['extra_ms_over_geometric'] = round(rows[1]['ms_per_step_median'] - rows[0]['ms_per_step_median'], 3)
    rows[1]['extra_launches_over_geometric'] = rows[1]['launches_per_step'] - rows[0]['launches_per_step']
    with open(os.path.join(ROOT, 'profiles', 'keypoint_teacher_step_cost.jsonl'), 'a') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')
            print(json.dumps(row))


if __name__ == '__main__':
    main()
