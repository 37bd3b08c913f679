#!/usr/bin/env python
"""Benchmark of the CenterNet-UDA hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W          (N > 1, one rank per GPU)

Metric (BASELINE.json): source images/sec of one full UDA training step of
CenterNet DLA-34 (+16 DCNv2 layers) at 512x512, per-GPU batch 16 source + 16
target images, `uda=entropy_minimization` (configs[2]): 2 forwards, detection +
entropy loss, 2 backwards, Adam step -- uda/entropy_minimization.py:11-43 of
the reference -- on synthetic COCO-shaped batches already resident in HBM.
Weak scaling: every rank owns its own 16+16 images; gradients are averaged with
bucketed RCCL all-reduces overlapped with backward.

One JSON line is printed by rank 0.  A plain run sets up, warms up, times the
K steps and prints it; `--dump-outputs DIR` also writes the arrays the last
timed step returned (dump_outputs).  Everything else is measured only with
`--full`: `roofline` (dominant kernel, fp32 MFMA bound, timed with hipEvents
recorded inside the library around that kernel's launches during extra, untimed
steps of the same workload), `cpu_baseline` (the CPU oracle's step on a bounded
sample, host cores of this box), decode latency, inference, the one-rank RCCL
leg, the other configs and the DCN offset regimes.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, 'tests', 'golden'), ROOT, os.path.join(ROOT, 'centernet-uda_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: fp32 matrix peak (dense, = vector peak)
PEAK_HBM_GBPS = 8000.0              # MI355X_MICROARCH.md: HBM3E spec (6.29 TB/s measured with a float4 copy)
NUM_CLASSES = 6                     # configs/defaults.yaml:16
MAX_OBJS = 150                      # max_detections


def synthetic_batch(B, S, seed, device, rotated=False):
    """Batch with the schema of datasets/coco.py:168-174,242-251 (rotated: :303-312,384-393) -- SURVEY 8d."""
    import inputs as gin
    H = W = S // 4
    rs = np.random.RandomState(seed)
    n_obj = tuple(int(rs.randint(1, 21)) for _ in range(B))
    b = gin.detection_batch(B, NUM_CLASSES, H, W, MAX_OBJS, n_obj, 3 if rotated else 2, seed)
    data = {k: torch.from_numpy(v) for k, v in b.items()}
    g = torch.Generator().manual_seed(seed)
    data['input'] = torch.randn(B, 3, S, S, generator=g)
    data['target_domain_input'] = torch.randn(B, 3, S, S, generator=g)
    return {k: v.to(device) for k, v in data.items()}


class _Cfg(dict):
    __getattr__ = dict.__getitem__


UDA_WORKLOADS = {
    # --uda      BASELINE.json config, plugin factory, rotated boxes, periodic angle loss, Adam weight decay
    'none': ('configs[1]', lambda uda: uda.base.Model(), False, False, 0.0),
    'entropy': ('configs[2]', lambda uda: uda.EntropyMinimization(1e-4), False, False, 1e-4),
    'maxsq': ('configs[3]', lambda uda: uda.MaxSquaresMinimization(0.3), False, False, 1e-4),
    'advent': ('configs[4]', lambda uda: uda.AdversarialEntropyMinimization(
        1e-3, optimizer=_Cfg(name='Adam', params=_Cfg(lr=1e-4, weight_decay=0.0))), True, True, 1e-4),
}


def build_plugin(device, parallel, uda_name='entropy', backend_name='dla34'):
    import warnings
    import uda
    import uda.base
    from backends import dla, resnet
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    _, factory, rotated, periodic, wd = UDA_WORKLOADS[uda_name]
    torch.manual_seed(42)                                   # defaults.yaml: seed 42
    if backend_name == 'resnet18':                          # configs[0]: configs/defaults.yaml with backend=resnet
        backend = resnet.build(18, num_classes=NUM_CLASSES, pretrained=False, rotated_boxes=rotated)
    else:
        with warnings.catch_warnings():                     # random-init weights are the stated bench condition
            warnings.simplefilter('ignore', RuntimeWarning)
            backend = dla.build(num_classes=NUM_CLASSES, rotated_boxes=rotated)
    # give the DCN offset/mask convs non-zero weights so that deformable sampling is exercised (Q7)
    with torch.no_grad():
        for n, p in backend.named_parameters():
            if 'conv_offset_mask.weight' in n:
                p.normal_(0, 0.5 / (p.shape[1] * 9) ** 0.5)
    plugin = factory(uda)
    plugin.cfg = _Cfg(max_detections=MAX_OBJS,
                      model=_Cfg(backend=_Cfg(params=_Cfg(rotated_boxes=rotated, num_classes=NUM_CLASSES))))
    plugin.backend = backend
    plugin.device = device
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, angle_weight=1.0,
                                          periodic=periodic)
    # the optimizer is created before init_done()/to(): train.py:88-90,119-134
    plugin.optimizer = optim.Adam([p for p in backend.parameters() if p.requires_grad], lr=5e-5, weight_decay=wd)
    plugin.init_done()
    plugin.to(device, parallel)
    plugin.set_phase(True)
    return plugin


def fresh(batch):
    # the loss masks batch['wh'/'reg'] in place (Q2).  That is idempotent for every workload benched here (two-channel
    # `wh`, and the periodic angle loss of --uda advent); only the NON-periodic rotated loss also replaces the angle
    # target by its sigmoid on every call (losses/centernet.py:117) -- not a bench workload -- so the same resident
    # batch is reused
    return batch


def rewind_point(plugin):
    """--dump-outputs: remembers the parameters of every optimizer of `plugin` as they are before the first step; the
    returned function puts them back and zeroes the Adam moments and step counts.  A step's forward pass is bit-
    reproducible from run to run, its backward pass is not (atomic accumulation order), and Adam turns that last-bit
    noise into differences of 1e-4 after two steps and 0.2 after five (measured on the headline step).  The timed step
    whose outputs are dumped therefore starts from this state: its inputs, and so its outputs, are the same in every
    run, and two builds compare output for output.  (Train-mode BatchNorm does not read its running statistics.)"""
    import hip_runtime as hr
    from hip_runtime.arena import arena_for
    opts = [o for o in (plugin.optimizer, getattr(plugin, 'discriminator_optimizer', None)) if o is not None]
    params = [p for o in opts for g in o.param_groups for p in g['params']]
    saved = [p.detach().clone() for p in params]

    def rewind():
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.copy_(s)
            for o in opts:
                for st in o.state.values():
                    for t in st.values():
                        t.zero_()                   # exp_avg, exp_avg_sq (views of the fused kernel's moments), step
                o._step = 0                         # (the count the fused kernel's bias correction uses)
                # parameters written behind the library's back: the packed weights follow, as after optimizer.step()
                hr.bump_param_epoch(arena_for(o.param_groups[0]['params']).flat_param)
    return rewind


DUMP_LIMIT_BYTES = 60 * 1000 * 1000      # array data: under 64 MB in all with the .npy headers, in either unit


def dump_outputs(out, dirname, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: every tensor of `out` (what plugin.step returned: both domains' head maps, the loss stats) as
    DIR/<key path joined by '.'>.npy, float64 kept, everything else as float32.  Above `limit` bytes in all, each
    array is cut to the same fraction of its elements (at least one), a fixed seeded sample (flattened, in index order)."""
    arrays = {}

    def walk(name, v):
        if isinstance(v, dict):
            for k in sorted(v):
                walk('%s.%s' % (name, k) if name else str(k), v[k])
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk('%s.%d' % (name, i), x)
        elif torch.is_tensor(v):
            a = v.detach().cpu().numpy()
            arrays[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    walk('', out)
    total = sum(a.nbytes for a in arrays.values())
    os.makedirs(dirname, exist_ok=True)
    for name, a in sorted(arrays.items()):
        if total > limit:
            k = max(1, a.size * limit // total)
            a = a.reshape(-1)[np.sort(np.random.RandomState(0).permutation(a.size)[:k])]
        np.save(os.path.join(dirname, name + '.npy'), a)
    return sorted(arrays)


def _cpu_step_fn():
    """-> step(size, seed) -> seconds: one EntropyMinimization step of the CPU oracle (torch CPU ops + scalar C DCN
    loops, the reference's CPU sequence: uda/entropy_minimization.py:11-43) on 1 source + 1 target image."""
    import warnings
    from oracle import dla as odla
    from oracle import losses as ol
    from backends import dla
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        model = dla.build(num_classes=NUM_CLASSES)
    state = {}
    for k, v in model.state_dict().items():
        t = v.detach().clone()
        if t.is_floating_point() and 'running_' not in k:
            if 'conv_offset_mask.weight' in k:
                t.normal_(0, 0.5 / (t.shape[1] * 9) ** 0.5)
            t.requires_grad_(True)
        state[k] = t
    opt = torch.optim.Adam([v for v in state.values() if v.requires_grad], lr=5e-5, weight_decay=1e-4)

    def step(size, seed, images=1):
        batch = synthetic_batch(images, size, seed, 'cpu')
        t0 = time.perf_counter()
        opt.zero_grad()
        out_s = odla.forward(state, batch['input'], training=True)
        out_t = odla.forward(state, batch['target_domain_input'], training=True)
        c_loss, _, _ = ol.detection_loss(out_s, batch, 1.0, 0.1, 1.0, 1.0, False)
        e_loss = ol.entropy_loss(out_t['hm']) * 1e-4
        c_loss.backward()
        e_loss.backward()
        opt.step()
        return time.perf_counter() - t0
    return step


def cpu_baseline(budget_s=150.0):
    """The reference's CPU path beside the GPU number, on the metric's own 512x512 images:
    one untimed warm-up step at 256x256 (thread pools, allocator, oneDNN primitive caches), then up to three timed
    EntropyMinimization steps at 512x512 as long as the budget allows (always at least one); `value` = 1 / median.
    (Round 2 scaled a 256x256 sample by pixel count: off by up to 2x on a many-core host -- dropped.)"""
    step = _cpu_step_fn()
    t_begin = time.perf_counter()
    step(256, 5)                                            # warm-up
    times = []
    for i in range(3):
        spent = time.perf_counter() - t_begin
        if times and spent + 1.15 * max(times) > budget_s:
            break
        times.append(step(512, 11 + i))
    ts = sorted(times)
    med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
    # B = 2 beside B = 1, and the linear extrapolation to the metric's B = 16 (time per step
    # = a + b * B through the two samples); one step, when the budget still has room for it
    b2 = None
    if time.perf_counter() - t_begin + 2.2 * med <= budget_s:
        t2 = step(512, 17, images=2)
        per_image = max(t2 - med, 1e-9)                     # b of a + b * B
        t16 = med + 15.0 * per_image
        b2 = {'s_per_step': round(t2, 3), 'images_per_s': round(2.0 / t2, 5),
              'extrapolated_b16': {'s_per_step': round(t16, 2), 'images_per_s': round(16.0 / t16, 5),
                                   'how': 't(B) = a + b*B through the B=1 median and this B=2 step'}}
    try:
        affinity = len(os.sched_getaffinity(0))
    except AttributeError:
        affinity = os.cpu_count()
    return {
        'value': round(1.0 / med, 5), 'unit': 'images/sec (512x512 source images)', 'cores': torch.get_num_threads(),
        'nproc': affinity, 'host_cpus': os.cpu_count(), 'b2': b2,
        'kind': 'port',
        's_per_step_512': {'median': round(med, 3), 'min': round(ts[0], 3), 'max': round(ts[-1], 3), 'repeats': len(ts)},
        # the same leg on other boxes of this pool (128-thread hosts): 0.074 (round-3 collection box), 0.089 (round-3
        # driver box), 0.081 and 0.044 (two round-4 boxes: the host side varies 2x with what else the machine runs) --
        # quote the CPU figure as 0.04-0.09 img/s, not to three digits
        'box_to_box_range': [0.044, 0.089],
        'sample': ('EntropyMinimization step of the CPU oracle on 1 source + 1 target 512x512 image: 1 untimed warm-up '
                   'at 256x256, %d timed step(s) (median %.2f s, spread %.2f-%.2f s, budget %.0f s); torch CPU conv/BN '
                   '(%d threads) + single-thread C DCN loops like the reference CPU extension; `value` = 1 / median'
                   % (len(ts), med, ts[0], ts[-1], budget_s, torch.get_num_threads())),
    }


def decode_latency(device, with_cpu=True):
    """BASELINE.json's second metric: `decode_detection` latency at B=16, K=150 on 128x128 maps (cfg2-4) and
    160x160 maps (cfg5, 640x640 input), C=6 (the reference's default) and C=80 (COCO stress) -- SURVEY 8d.  Inputs
    resident in HBM, probabilities as `Model.get_detections` hands them over (Q1).  Algorithmic bytes = one read of
    the heat map + gathered wh/reg + the [B,K,6] result."""
    from backends.decode import decode_detection
    res = {}
    B, K = 16, 150
    for H in (128, 160):
        W = H
        for C in (6, 80):
            g = torch.Generator(device='cpu').manual_seed(7 + C + H)
            heat = torch.sigmoid(torch.randn(B, C, H, W, generator=g) - 2.19).clamp(1e-4, 1 - 1e-4)
            wh, reg = torch.rand(B, 2, H, W, generator=g) * 40, torch.rand(B, 2, H, W, generator=g)
            hd, whd, regd = heat.to(device), wh.to(device), reg.to(device)
            for _ in range(10):
                dets = decode_detection(hd, whd, regd, K=K)
            # median of five groups of 40 back-to-back calls (a host hiccup -- a Python gen-2 collection takes tens of
            # milliseconds -- lands in one group, not in the figure)
            n, groups = 40, []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(n):
                    dets = decode_detection(hd, whd, regd, K=K)
                e1.record()
                torch.cuda.synchronize()
                groups.append(e0.elapsed_time(e1) * 1e3 / n)
            us = sorted(groups)[len(groups) // 2]
            nbytes = B * C * H * W * 4 + B * K * 4 * 4 + B * K * 6 * 4
            entry = {'us': round(us, 1), 'algorithmic_bytes': nbytes, 'gb_per_s': round(nbytes / us / 1e3, 1),
                     'hbm_frac': round(nbytes / (us * 1e-6) / 8e12, 4)}
            if with_cpu and C == 6:
                from oracle import decode as oracle_decode       # checker / baseline leg only
                t0 = time.perf_counter()
                want = oracle_decode.decode_detection(heat.numpy(), wh.numpy(), reg.numpy(), K=K)
                entry['cpu_port_us'] = round((time.perf_counter() - t0) * 1e6, 1)
                got = dets.cpu().numpy()
                entry['matches_oracle'] = bool(np.array_equal(got[..., 4:], want[..., 4:])
                                               and abs(got - want).max() <= 1e-4)
            res['C%d' % C if H == 128 else 'C%d_160' % C] = entry
    res['shape'] = 'B=16, K=150, fp32; C6 / C80: 128x128 maps, C6_160 / C80_160: 160x160 maps (cfg5)'
    return res


def inference_throughput(device, backend, size, batch):
    """the export.CenterNet wrapper (eval forward -> clamped sigmoid -> decode -> x down_ratio) on the
    trained backend of this run; images/s and latency per batch with inputs resident in HBM."""
    from export import CenterNet
    was_training = backend.training
    model = CenterNet(backend, MAX_OBJS).eval()
    x = torch.randn(batch, 3, size, size, device=device)
    for _ in range(3):
        model(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 10
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        model(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    backend.train(was_training)
    # forward only: 65.58 GFLOP per 512x512 image
    tf = 65.58e9 * (size / 512.0) ** 2 * batch / (ms * 1e-3) / 1e12
    return {'images_per_s': round(batch / (ms * 1e-3), 1), 'ms_per_batch': round(ms, 3), 'batch': batch,
            'mfma_fraction': round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
            'what': 'export.CenterNet: eval forward + decode (K=%d), fp32, BatchNorm folded into the conv / DCN '
                    'weights (bias + skip connection + ReLU in the GEMM epilogues), no tape' % MAX_OBJS}


def dp1_rccl_leg(device, args):
    """The headline step through the data-parallel wrapper with a ONE-rank RCCL group -- the N = 1 point of the
    multi-GPU code path: gradient arena flushed per bucket, 4 bucketed all-reduces launched from the gradient-ready
    hooks, finish_gradient_sync, the global-normaliser all-reduces of the detection loss -- timed beside the plain
    step of the same process, so the wrapper's fixed overhead is a number (SCALE runs then start from it)."""
    import socket
    created = False
    # RCCL prints a version banner on STDOUT when its first communicator comes up; the bench line must stay the only
    # thing on stdout, so file descriptor 1 points at stderr for the duration of this leg
    sys.stdout.flush()
    saved_fd = os.dup(1)
    os.dup2(2, 1)
    try:                # everything after the redirect sits inside: whatever raises, `finally` hands stdout back
        if not dist.is_initialized():
            s = socket.socket()
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
            s.close()
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            os.environ['MASTER_PORT'] = str(port)
            dist.init_process_group(backend='nccl', rank=0, world_size=1, device_id=device)
            created = True
        plugin = build_plugin(device, parallel=True, uda_name=args.uda, backend_name=args.backend)
        batch = synthetic_batch(args.batch, args.size, 42, device, rotated=UDA_WORKLOADS[args.uda][2])
        for _ in range(3):
            plugin.step(fresh(batch))
        torch.cuda.synchronize()
        dp = plugin.backend
        dp.reset_exchange_stats(measure=True)
        n = max(5, args.steps)
        t0 = time.perf_counter()
        for _ in range(n):
            plugin.step(fresh(batch))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        xs = dp.exchange_stats()
        dp.reset_exchange_stats(measure=False)
        del plugin, batch
        torch.cuda.empty_cache()
        return {'ms_per_step': round(dt * 1e3, 3), 'value': round(args.batch / dt, 3), 'unit': 'images/sec',
                'steps': n, 'collective': xs,
                'what': 'same workload, uda.Model.to(device, parallel=True): hip_runtime.parallel.DataParallel over a '
                        'one-rank RCCL process group (all-reduce = identity, every launch and wait of the N > 1 path)'}
    finally:
        try:
            if created:
                dist.destroy_process_group()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)


def other_configs(device, skip):
    """BASELINE.json's other configs as short legs of the driver's own run (3 warm-up + 5 timed steps each, fresh
    plugin, batch resident in HBM): the numbers the driver's command would otherwise never time."""
    res = {}
    for idx in sorted(CONFIGS):
        if idx == skip:
            continue
        backend_name, uda_name, size, batch_n = CONFIGS[idx]
        plugin = build_plugin(device, parallel=False, uda_name=uda_name, backend_name=backend_name)
        batch = synthetic_batch(batch_n, size, 42, device, rotated=UDA_WORKLOADS[uda_name][2])
        for _ in range(3):
            plugin.step(fresh(batch))
        torch.cuda.synchronize()
        import gc
        gc.collect()
        gc.freeze()
        t0 = time.perf_counter()
        for _ in range(5):
            out = plugin.step(fresh(batch))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 5
        # the losses of the last timed step (the 8th on this batch): a leg that times a broken step says so here
        losses = {k: round(float(v), 6) for k, v in out['stats'].items()}
        res['configs[%d]' % idx] = {'backend': backend_name, 'uda': uda_name, 'size': size, 'batch': batch_n,
                                    'ms_per_step': round(dt * 1e3, 3), 'images_per_s': round(batch_n / dt, 2),
                                    'steps': 5, 'warmup': 3, 'losses_last_step': losses,
                                    'losses_finite': bool(all(np.isfinite(v) for v in losses.values()))}
        del out
        del plugin, batch
        torch.cuda.empty_cache()
    return res


def _dcn_offset_convs(backend):
    return [(n, m) for n, m in getattr(backend, 'module', backend).named_modules() if n.endswith('conv_offset_mask')]


def measure_dcn_offsets(plugin, batch):
    """-> {layer: std of its sampling offsets in px} on `batch` (one no-grad train-mode forward of both domains' source
    half is enough: the statistic, not the step, is wanted)."""
    got, hooks = {}, []
    for n, m in _dcn_offset_convs(plugin.backend):
        hooks.append(m.register_forward_hook(
            lambda mod, inp, out, n=n: got.__setitem__(n, float(out[:, :18].detach().std()))))
    with torch.no_grad():
        plugin.backend(batch['input'])
    for h in hooks:
        h.remove()
    return got


def set_dcn_offset_std(plugin, batch, std_px, passes=3):
    """Re-initialise every `conv_offset_mask` (libs/DCNv2/dcn_v2.py:104-116; zero in the reference, Q7) so that each of
    the 16 DCN layers samples with offsets of standard deviation `std_px` pixels ON THIS BATCH: the 18 offset channels'
    kernels are rescaled layer by layer against the measured statistic (a few passes: a layer's input depends on the
    layers before it).  A trained CenterNet has offsets of pixels; the default initialisation leaves a fraction."""
    for _ in range(passes):
        cur = measure_dcn_offsets(plugin, batch)
        with torch.no_grad():
            for n, m in _dcn_offset_convs(plugin.backend):
                m.weight[:18].mul_(std_px / max(cur[n], 1e-12))
                m.bias[:18].zero_()
    import hip_runtime as hr
    hr.bump_param_epoch()               # (parameters written behind the library's back: cached packed weights follow)
    for m in getattr(plugin.backend, 'module', plugin.backend).modules():
        if hasattr(m, '_census_calls'):
            m._census_calls = 0         # the layers re-measure their offset regime at their next training forward
    return measure_dcn_offsets(plugin, batch)


def dcn_offsets_leg(device, sigmas=(1.0, 2.0)):
    """The headline step with the DCN layers in the offset regime of a TRAINED model: same workload,
    every conv_offset_mask re-initialised for offsets of sigma = 1 px and 2 px.  Beside the headline, never as it: the
    default initialisation (SURVEY 8d's workload) leaves offsets of a fraction of a pixel, the cheapest regime for
    any kernel that keeps an input window on chip."""
    res = {}
    base = build_plugin(device, parallel=False, uda_name='entropy')
    batch = synthetic_batch(16, 512, 42, device)
    st0 = measure_dcn_offsets(base, batch)
    res['default_init'] = {'offset_std_px': {'mean': round(float(np.mean(list(st0.values()))), 4),
                                             'min': round(min(st0.values()), 4), 'max': round(max(st0.values()), 4)}}
    del base
    for sg in sigmas:
        plugin = build_plugin(device, parallel=False, uda_name='entropy')
        st = set_dcn_offset_std(plugin, batch, sg)
        for _ in range(3):
            plugin.step(fresh(batch))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            out = plugin.step(fresh(batch))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 5
        after = measure_dcn_offsets(plugin, batch)
        res['sigma_%g_px' % sg] = {
            'ms_per_step': round(dt * 1e3, 3), 'images_per_s': round(16 / dt, 2), 'steps': 5, 'warmup': 3,
            'offset_std_px_set': {'mean': round(float(np.mean(list(st.values()))), 3), 'min': round(min(st.values()), 3),
                                  'max': round(max(st.values()), 3)},
            'offset_std_px_after_8_steps': round(float(np.mean(list(after.values()))), 3),
            'losses_finite': bool(all(np.isfinite(float(v)) for v in out['stats'].values()))}
        del plugin, out
        torch.cuda.empty_cache()
    return res


def code_fingerprint():
    """sha256 (16 hex digits) over the gfx950 code objects inside libcenternet_uda_hip.so (profiles/fingerprint.py):
    says whether a committed counter profile was collected from the kernels this run EXECUTES.  Comment or
    whitespace edits of the sources do not change it (round 3 hashed the source text and a comment-only commit
    disowned the profile)."""
    sys.path.insert(0, os.path.join(ROOT, 'profiles'))
    try:
        import fingerprint
        return fingerprint.code_fingerprint()
    finally:
        sys.path.pop(0)


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` from the newest committed rocprofv3 counter profile (separate
    `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this same command, profiles/collect_pmc_traffic.sh).  PMC
    passes cannot run inside the timed process, so the note says whether that profile was collected from the
    kernel code this run executes (code_fingerprint)."""
    import glob
    import re
    files = glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json'))
    if not files:
        return None, None
    # newest = highest ROUND NUMBER (r10 after r2), not the lexicographic maximum
    path = max(files, key=lambda f: int(re.match(r'r(\d+)', os.path.basename(f)).group(1)))
    data = json.load(open(path))
    meta = data.get('_meta', {})
    import re
    # (profiler names carry the template defaults the library's own kernel names leave out)
    # (... and the QUADS flag of the DCN data-gradient kernels, which the library's scope names do not carry: the benched
    # layers all take the quad-interleaved column gradient, `<true>`)
    norm = lambda k: re.sub(r'<(true|false)>$', '', re.sub(r'(,(true|false))?(,16)?>$', '>', k.replace(' ', '')))
    t = {norm(k): v for k, v in data.items() if k != '_meta'}.get(norm(kernel_name.split(' (')[0].split(' [')[0]))
    if not t:
        return None, '%s has no entry for this kernel' % os.path.basename(path)
    mine = code_fingerprint()
    same = meta.get('code_sha16') == mine
    fetch = t['fetch_kb_per_launch'] * (2.0 if meta.get('fetch_doubled_for_wide_reads') else 1.0)
    note = ('bytes/launch = FETCH_SIZE + WRITE_SIZE from profiles/%s, %s'
            % (os.path.basename(path),
               'collected from the kernel code this run executes (code object %s)' % mine if same else
               'COLLECTED FROM DIFFERENT KERNEL CODE (profile %s, this run %s): indicative only'
               % (meta.get('code_sha16', 'unknown: pre-round-4 profile'), mine)))
    return round((fetch + t['write_kb_per_launch']) * 1024), note


def pmc_step_bytes():
    """HBM bytes of one step from the newest committed counter profile: `_meta.hbm_bytes_per_step`, the sum over EVERY kernel
    of the two `--pmc` passes (profiles/collect_pmc_traffic.sh) -- or None for a profile of an older round."""
    import glob
    import re
    files = glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json'))
    if not files:
        return None, None
    path = max(files, key=lambda f: int(re.match(r'r(\d+)', os.path.basename(f)).group(1)))
    meta = json.load(open(path)).get('_meta', {})
    if 'hbm_bytes_per_step' not in meta:
        return None, '%s carries no per-step total' % os.path.basename(path)
    same = meta.get('code_sha16') == code_fingerprint()
    return int(meta['hbm_bytes_per_step']), ('profiles/%s, %s' % (os.path.basename(path), 'same kernel code' if same else
                                                                'COLLECTED FROM DIFFERENT KERNEL CODE: indicative only'))


def spawn_ranks(n):
    """`python bench.py --gpus N` -> `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same
    arguments>` as a child process; returns its exit code (non-zero when any rank failed)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault('OMP_NUM_THREADS', '1')
    return subprocess.call(cmd, env=env)


CONFIGS = {
    # --config N: BASELINE.json configs[N] -> (backend, uda, size, batch)
    0: ('resnet18', 'none', 256, 2),
    1: ('dla34', 'none', 512, 16),
    2: ('dla34', 'entropy', 512, 16),
    3: ('dla34', 'maxsq', 512, 16),
    4: ('dla34', 'advent', 640, 16),
}


def apply_config(args):
    if args.config is not None:
        args.backend, args.uda, args.size, args.batch = CONFIGS[args.config]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=16, help='per-GPU source batch (and target batch)')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--uda', default='entropy', choices=sorted(UDA_WORKLOADS),
                    help="BASELINE.json configs[1..4]: none / entropy (default, the headline) / maxsq / advent (use --size 640)")
    ap.add_argument('--backend', default='dla34', choices=['dla34', 'resnet18'])
    ap.add_argument('--config', type=int, default=None, choices=sorted(CONFIGS),
                    help='BASELINE.json configs[N]: sets --backend/--uda/--size/--batch (2 = the default headline workload)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the arrays the last timed step returned as DIR/<name>.npy (dump_outputs)')
    ap.add_argument('--full', action='store_true',
                    help='also run every leg beyond the headline: roofline profile steps, cpu_baseline, decode latency, '
                         'inference, the one-rank RCCL leg, other configs, DCN offset regimes (the options below)')
    ap.add_argument('--cpu-baseline-budget', type=float, default=150.0,
                    help='seconds of host time the cpu_baseline leg may spend (the 512x512 sample is skipped beyond it)')
    ap.add_argument('--profile-steps', type=int, default=1, help='with --full: untimed steps of the roofline leg')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the cpu_baseline leg')
    ap.add_argument('--no-extras', action='store_true',
                    help='with --full: skip the decode-latency, inference and other legs (profiling runs)')
    ap.add_argument('--matrix-mode-split', action='store_true',
                    help='with --full: also time the step in matrix mode 1 (split bf16 operands; round-1 kernel set): '
                         '`matrix_mode_split`')
    ap.add_argument('--dcn-offset-std', type=float, default=None,
                    help='profiling runs only: re-initialise every conv_offset_mask for sampling offsets of this standard '
                         'deviation in pixels before the warm-up (set_dcn_offset_std); the metric name then says so')
    args = ap.parse_args()

    apply_config(args)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # started plainly (`python bench.py --gpus N`): spawn the N ranks ourselves.  Decided from the environment
        # alone, BEFORE anything touches the GPU; the ranks are fresh child processes of torch.distributed.run and
        # this process only waits for them (never exec from a process that has initialised HIP).
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus != world:
        raise SystemExit('bench.py --gpus %d was launched with WORLD_SIZE=%d' % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X: the product path has no CPU fallback')
    # test knobs (a one-GPU box cannot host two RCCL ranks): CNUDA_BENCH_ONE_DEVICE=1 puts every rank on cuda:0,
    # CNUDA_BENCH_BACKEND=gloo swaps the collective backend; the driver's runs use neither
    one_device = os.environ.get('CNUDA_BENCH_ONE_DEVICE') == '1'
    backend = os.environ.get('CNUDA_BENCH_BACKEND', 'nccl')
    device = torch.device('cuda', 0 if one_device else local_rank)
    torch.cuda.set_device(device)
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group(backend='nccl', device_id=device)      # nccl == RCCL on ROCm
        else:
            dist.init_process_group(backend=backend)

    plugin = build_plugin(device, parallel=world > 1, uda_name=args.uda, backend_name=args.backend)
    batch = synthetic_batch(args.batch, args.size, 42 + rank, device, rotated=UDA_WORKLOADS[args.uda][2])

    if args.dcn_offset_std is not None and args.backend == 'dla34':
        set_dcn_offset_std(plugin, batch, args.dcn_offset_std)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    rewind = rewind_point(plugin) if args.dump_outputs else None
    for _ in range(args.warmup):
        plugin.step(fresh(batch))
    # Python's cyclic collector: a full (generation-2) pass over the ~10^5 long-lived objects of the model, the tape
    # closures and the arena takes ~80 ms and fires every few thousand container allocations (measured: step 13 of the
    # ResNet-18 config, 6.7 -> 84 ms).  The objects alive after the warm-up are moved to the permanent generation, as
    # long-running training loops do; garbage created by the timed steps is still collected.
    import gc
    gc.collect()
    gc.freeze()
    dp = plugin.backend if hasattr(plugin.backend, 'reset_exchange_stats') else None
    if dp is not None:
        dp.reset_exchange_stats(measure=True)
    barrier()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    starts = marks[:-1]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if rewind is not None and i == args.steps - 1:
            # the dumped step starts from the state before the warm-up (rewind_point); neither the clock nor this
            # step's start event counts the rewind
            torch.cuda.synchronize()
            t_rewind = time.perf_counter()
            rewind()
            torch.cuda.synchronize()
            starts[i] = torch.cuda.Event(enable_timing=True)
            starts[i].record()
            t0 += time.perf_counter() - t_rewind
        out = plugin.step(fresh(batch))
        marks[i + 1].record()                 # (an event record does not block: the timed region is unchanged)
    barrier()
    elapsed = time.perf_counter() - t0
    per_step = [starts[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    collective = dp.exchange_stats() if dp is not None else None
    if dp is not None:
        dp.reset_exchange_stats(measure=False)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    stats = {k: float(v) for k, v in out['stats'].items()}
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs)
    # a plain run stops here: the legs below run with --full only
    extras = args.full and world == 1 and not args.no_extras

    roofline = None
    if args.full and args.profile_steps > 0:
        # extra, untimed steps with the in-library kernel timer.  EVERY rank runs them (the gradient all-reduce
        # inside step() is collective); only rank 0 records and reports.
        import hip_runtime as hr
        if rank == 0:
            hr.prof_begin()
        for _ in range(args.profile_steps):
            plugin.step(fresh(batch))
        torch.cuda.synchronize()
        per_kernel = hr.prof_end() if rank == 0 else None
        if per_kernel:
            all_kernels = per_kernel
            hbm_kernels = {k: v for k, v in per_kernel.items() if v['flops'] == 0}
            per_kernel = {k: v for k, v in per_kernel.items() if v['flops'] > 0}
            name, d = max(per_kernel.items(), key=lambda kv: kv[1]['ms'])
            achieved = d['flops'] / (d['ms'] * 1e-3) / 1e12
            traffic, traffic_note = pmc_traffic(name)
            executed_tflop = sum(v['flops'] for v in per_kernel.values()) / args.profile_steps / 1e12
            top_mfma = {
                'bound': 'mfma', 'kernel': name, 'achieved': round(achieved, 3), 'peak': PEAK_FP32_MFMA_TFLOPS,
                'unit': 'TFLOP/s', 'frac': round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), 'traffic': traffic,
                'traffic_note': traffic_note,
                'launches_per_step': d['launches'] // args.profile_steps,
                'avg_launch_ms': round(d['ms'] / d['launches'], 4),
                'algorithmic_gflop_per_launch': round(d['flops'] / d['launches'] / 1e9, 3),
                'kernel_ms_per_step': round(d['ms'] / args.profile_steps, 3),
            }
            # `roofline` proper: the kernel with the most time per step over ALL profiled kernels, against its OWN bound --
            # the fp32 MFMA peak for a GEMM, 8 TB/s of HBM for a streaming kernel (algorithmic bytes / time) -- so that
            # the line names what the top row of the rocprofv3 summary names (a selection over the
            # MFMA kernels alone hid dcn_bwd_data_kernel, the largest row since round 5).  The largest MFMA kernel
            # stays beside it under `top_mfma_kernel`.
            tname, td = max(all_kernels.items(), key=lambda kv: kv[1]['ms'])
            if td['flops'] > 0:
                roofline = dict(top_mfma)
            else:
                gbs = td['bytes'] / (td['ms'] * 1e-3) / 1e9
                ttraffic, tnote = pmc_traffic(tname)
                roofline = {
                    'bound': 'hbm', 'kernel': tname, 'achieved': round(gbs, 1), 'peak': PEAK_HBM_GBPS, 'unit': 'GB/s',
                    'frac': round(gbs / PEAK_HBM_GBPS, 4), 'traffic': ttraffic, 'traffic_note': tnote,
                    'launches_per_step': td['launches'] // args.profile_steps,
                    'avg_launch_ms': round(td['ms'] / td['launches'], 4),
                    'algorithmic_mb_per_launch': round(td['bytes'] / td['launches'] / 1e6, 1),
                    'kernel_ms_per_step': round(td['ms'] / args.profile_steps, 3),
                }
            dcn_family = {k: v for k, v in all_kernels.items()
                          if 'dcn' in k.lower() or k.startswith('igemm_fwd_shortk_kernel')}
            hbm_step, hbm_note = pmc_step_bytes()
            roofline.update({
                'top_mfma_kernel': top_mfma,
                # FLOPs the timed GEMM launches of one step actually execute (sum over all_mfma_kernels)
                'executed_tflop_per_step': round(executed_tflop, 4),
                # every kernel of the deformable convolutions (window / gathering forward, sample + GEMM pairs, the
                # column-gradient GEMM -- the only user of the short-K kernel --, prep, the data-gradient walks, the
                # weight gradient from the saved columns); the 27-channel offset convolutions are plain convolutions
                'dcn_family_ms': round(sum(v['ms'] for v in dcn_family.values()) / args.profile_steps, 3),
                'dcn_family_kernels': sorted(dcn_family),
                # HBM bytes of one step, summed over every kernel of the committed counter profile (FETCH_SIZE as
                # reported + WRITE_SIZE; profiles/collect_pmc_traffic.sh), and the time they take at 6.3 TB/s
                'hbm_bytes_per_step': hbm_step, 'hbm_bytes_note': hbm_note,
                'hbm_ms_at_6p3TBps': round(hbm_step / 6.3e12 * 1e3, 2) if hbm_step else None,
                # continuity with rounds 1-4, whose dominant kernel was igemm_fwd_ws_kernel<128, ConvFwdBufLoader>: since
                # round 5 that kernel exists twice -- with and without the BatchNorm-statistics tail in its epilogue
                # (ConvFwdBufStatsLoader / ConvFwdBufLoader) -- and the two instances together are reported here
                'forward_ws128_family': (lambda fam: {
                    'kernels': sorted(fam), 'ms_per_step': round(sum(v['ms'] for v in fam.values()) / args.profile_steps, 3),
                    'tflops': round(sum(v['flops'] for v in fam.values()) / (sum(v['ms'] for v in fam.values()) * 1e-3) / 1e12, 2),
                    'frac': round(sum(v['flops'] for v in fam.values()) / (sum(v['ms'] for v in fam.values()) * 1e-3) / 1e12
                                  / PEAK_FP32_MFMA_TFLOPS, 4)} if fam else None)(
                    {k: v for k, v in per_kernel.items() if k.startswith('igemm_fwd_ws_kernel<128, ConvFwdBuf')}),
                # (gb_per_s: the launches' activation tensors once each / time -- a kernel at 4-5 TB/s is bound by HBM whatever its
                # TFLOP/s: the 2..6-output head convolutions, the 16-channel layers at 512 x 512)
                'all_mfma_kernels': {k: {'ms_per_step': round(v['ms'] / args.profile_steps, 3),
                                         'tflops': round(v['flops'] / (v['ms'] * 1e-3) / 1e12, 2),
                                         'gb_per_s': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 0),
                                         'launches': v['launches'] // args.profile_steps}
                                     for k, v in sorted(per_kernel.items(), key=lambda kv: -kv[1]['ms'])},
                # the profiled kernels without MFMA work, against the HBM roofline (algorithmic bytes / time)
                'hbm_kernels': {k: {'ms_per_step': round(v['ms'] / args.profile_steps, 3),
                                    'gb_per_s': round(v['bytes'] / (v['ms'] * 1e-3) / 1e9, 1),
                                    'frac_of_8TBps': round(v['bytes'] / (v['ms'] * 1e-3) / 8e12, 4),
                                    'launches': v['launches'] // args.profile_steps}
                                for k, v in sorted(hbm_kernels.items(), key=lambda kv: -kv[1]['ms'])},
            })
    split_leg = None
    if extras and args.matrix_mode_split:
        # (opt-in since round 6, --matrix-mode-split: mode 1 keeps the round-1 kernel set -- no wave-specialised, halo-tile,
        # short-K or window kernels -- so beside the round-6 f32 set it is no longer an A/B of the matrix pipe alone)
        # the same step with the convolution GEMMs on the bf16 matrix pipe (exact three-way operand split, six
        # partial products, f32 accumulation: DESIGN.md section 4a); reported beside the headline, never as it
        import hip_runtime as hr
        mode0 = hr.get_matrix_mode()
        if mode0 == 0:
            hr.set_matrix_mode(1)
            for _ in range(2):
                plugin.step(fresh(batch))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                plugin.step(fresh(batch))
            torch.cuda.synchronize()
            e1 = time.perf_counter() - t1
            hr.set_matrix_mode(mode0)
            split_leg = {'ms_per_step': round(e1 / args.steps * 1e3, 3),
                         'value': round(args.batch * args.steps / e1, 3), 'unit': 'images/sec',
                         'note': 'cnuda_set_matrix_mode(1) for conv forward / input-gradient / DCN column-gradient '
                                 'GEMMs; weight-gradient and DCN forward GEMMs stay on the f32 MFMA'}
    dp1 = None
    if extras:
        try:
            dp1 = dp1_rccl_leg(device, args)
        except Exception as e:                       # (a box without a usable RCCL: report, do not lose the line)
            dp1 = {'error': '%s: %s' % (type(e).__name__, e)}
    if world > 1:
        dist.barrier()

    if rank == 0:
        import hip_runtime as hr
        ms = elapsed / args.steps * 1e3
        value = args.batch * world * args.steps / elapsed
        # whole-step algorithmic work: 195.5 GFLOP per forwarded 512x512 image, 2 forwards per source image
        step_tflop = 195.5e9 * (args.size / 512.0) ** 2 * (1 if args.uda == 'none' else 2) * args.batch / 1e12
        arch = 'DLA-34' if args.backend == 'dla34' else 'ResNet-18'
        line = {
            'metric': 'images/sec CenterNet DLA-34 512x512 UDA step (entropy minimisation)'
            if args.uda == 'entropy' and args.size == 512 and args.backend == 'dla34' and args.dcn_offset_std is None
            else 'images/sec CenterNet %s %dx%d train step (uda=%s%s)'
                 % (arch, args.size, args.size, args.uda,
                    '' if args.dcn_offset_std is None else ', DCN offsets re-initialised to sigma = %g px' % args.dcn_offset_std),
            'value': round(value, 3), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': round(ms, 3), 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f32' if hr.get_matrix_mode() == 0 else 'f32 (bf16 x3 split operands)',
            'data': 'synthetic', 'matrix_mode': hr.get_matrix_mode(),
            'config': {'workload': '%s: %s%s, %dx%d, per-GPU batch %d source%s, uda=%s, '
                                   'Adam(lr 5e-5), random-init weights'
                                   % ('configs[0]' if args.backend == 'resnet18' else UDA_WORKLOADS[args.uda][0],
                                      'DLA-34 + DCNv2' if args.backend == 'dla34' else 'ResNet-18 (torchvision-0.6 trunk restated) + 3 deconv',
                                      ' rotated-box head' if args.uda == 'advent' else '',
                                      args.size, args.size, args.batch,
                                      '' if args.uda == 'none' else ' + %d target' % args.batch,
                                      {'none': 'none', 'entropy': 'entropy_minimization',
                                       'maxsq': 'max_squares_minimization',
                                       'advent': 'adversarial_entropy_minimization'}[args.uda]),
                       'global_batch': args.batch * world, 'input': [3, args.size, args.size],
                       'parallelism': 'dp%d' % world},
            # whole-step algorithmic FLOPs are tabulated for DLA-34 only
            # two accountings of the whole step against the fp32 MFMA peak.  `step_mfma_fraction`: SURVEY 8d's nominal
            # 195.5 GFLOP per forwarded image (3x the forward pass, every head of every forwarded image).
            # `step_mfma_fraction_executed`: the FLOPs of the GEMM launches the step really runs (the target-domain
            # wh / reg head backward, which neither the reference's autograd nor this build executes, is not in it)
            'step_mfma_fraction': round(step_tflop / (ms * 1e-3) / PEAK_FP32_MFMA_TFLOPS, 4)
            if args.backend == 'dla34' else None,
            'step_mfma_fraction_executed': round(roofline['executed_tflop_per_step'] / (ms * 1e-3) / PEAK_FP32_MFMA_TFLOPS, 4)
            if roofline else None,
            'gc_frozen': True,      # gc.freeze() after the warm-up (see above): gen-2 passes over warm-up objects are not in `value`
            'ms_per_step_sd': round(float(np.std(per_step)), 3), 'ms_per_step_min': round(min(per_step), 3),
            'ms_per_step_max': round(max(per_step), 3),
            'collective': collective,
            'losses': {k: round(v, 5) for k, v in stats.items()},
            'roofline': roofline,
            'decode_latency': decode_latency(device, with_cpu=not args.no_cpu_baseline)
            if extras else None,
            'inference': inference_throughput(device, getattr(plugin.backend, 'module', plugin.backend), args.size,
                                              args.batch) if extras else None,
            'matrix_mode_split': split_leg,
            'dp1_rccl': dp1,
            'other_configs': other_configs(device, args.config if args.config is not None else 2)
            if extras and args.config in (None, 2) and args.uda == 'entropy'
            and args.size == 512 and args.batch == 16 else None,
            'dcn_offsets': dcn_offsets_leg(device)
            if extras and args.config in (None, 2) and args.uda == 'entropy'
            and args.size == 512 and args.batch == 16 and args.backend == 'dla34' else None,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            line['cpu_baseline'] = cpu_baseline(args.cpu_baseline_budget)
        else:
            line['cpu_baseline'] = None
        print(json.dumps(line), flush=True)
    # The bench line is the only thing this process may leave on stdout.  RCCL (this build) prints a version banner on
    # STDOUT when the process that initialised it exits -- after the line, from every rank: from here on file
    # descriptor 1 is stderr.
    sys.stdout.flush()
    os.dup2(2, 1)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
