"""`python bench.py --gpus N` started plainly spawns its N ranks itself (fresh children of torch.distributed.run,
decided from the environment before anything touches the GPU) and exits non-zero when a rank fails."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=900):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    env.pop('RANK', None)
    env.pop('LOCAL_RANK', None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_plain_multi_gpu_start_spawns_ranks_and_propagates_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip('covered by the GPU variant below')
    r = _run(['--gpus', '2', '--steps', '1', '--warmup', '0', '--no-cpu-baseline'])
    assert r.returncode != 0
    # the refusal comes from a spawned RANK (no GPU here), not from an argument check in the parent: torchrun prefixes
    # nothing, but it reports the failed child (`rank : N (local_rank: N)`) and ends the survivor as soon as the first
    # rank fails, so the message is guaranteed once, not twice
    assert r.stderr.count('bench.py needs an MI355X') >= 1, r.stderr[-2000:]
    assert 'local_rank' in r.stderr, r.stderr[-2000:]


def test_world_size_mismatch_is_refused():
    r = _run(['--gpus', '2'], {'WORLD_SIZE': '4', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and 'WORLD_SIZE=4' in r.stderr


@pytest.mark.gpu
def test_plain_two_rank_start_prints_one_json_line():
    r = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '2', '--size', '128', '--full',
              '--no-cpu-baseline', '--no-extras'], {'CNUDA_BENCH_ONE_DEVICE': '1', 'CNUDA_BENCH_BACKEND': 'gloo'})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['steps'] == 2 and line['config']['global_batch'] == 4
    assert line['value'] > 0 and line['scaling'] == 'weak'
    assert line['roofline']['kernel'] and line['roofline']['achieved'] > 0
    # the N > 1 line proves what the exchange step did: the process group really had two ranks, every parameter
    # gradient of DLA-34 went through the bucketed all-reduce, and the exposed (non-overlapped) time is reported
    c = line['collective']
    assert c['backend'] == 'gloo' and c['world_size'] == 2 and c['steps'] == 2
    assert c['bytes_per_step'] >= 4 * 18e6 and c['buckets_per_step'] >= 2          # ~18.5 M parameters, 24 MB buckets
    assert c['host_wait_ms_per_step'] >= 0 and 'exposed_allreduce_ms_per_step' in c
    assert line['ms_per_step_sd'] >= 0 and line['ms_per_step_min'] <= line['ms_per_step'] * 1.05


@pytest.mark.gpu
def test_single_gpu_run_with_the_rccl_leg_leaves_exactly_one_line_on_stdout():
    # the one-rank RCCL leg brings a communicator up; this RCCL build prints a version banner on STDOUT when such a
    # process exits -- after the bench line.  The driver reads stdout: nothing but the line may be there.
    r = _run(['--steps', '1', '--warmup', '1', '--batch', '2', '--size', '128', '--full', '--no-cpu-baseline'])
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1 and out[0].startswith('{'), out
    line = json.loads(out[0])
    assert line['n_gpus'] == 1 and line.get('dp1_rccl'), sorted(line)


def test_dump_outputs_names_dtypes_and_seeded_sample(tmp_path):
    """--dump-outputs writes every tensor a step returned under its key path; over the size limit each array keeps
    the same fraction of its elements, the same seeded sample from run to run."""
    import numpy as np
    import torch
    import bench
    out = {'source_domain': {'hm': torch.rand(2, 3, 4, 4), 'wh': torch.rand(2, 2, 4, 4, dtype=torch.float64)},
           'stats': {'total_loss': torch.tensor(1.5), 'n': torch.tensor(3)}}
    names = bench.dump_outputs(out, str(tmp_path / 'all'))
    assert names == ['source_domain.hm', 'source_domain.wh', 'stats.n', 'stats.total_loss']
    hm = np.load(tmp_path / 'all' / 'source_domain.hm.npy')
    assert hm.dtype == np.float32 and np.array_equal(hm, out['source_domain']['hm'].numpy())
    assert np.load(tmp_path / 'all' / 'source_domain.wh.npy').dtype == np.float64
    assert np.load(tmp_path / 'all' / 'stats.n.npy').dtype == np.float32
    assert float(np.load(tmp_path / 'all' / 'stats.total_loss.npy')) == 1.5
    total = 96 * 4 + 64 * 8 + 4 + 4
    for d in ('a', 'b'):
        bench.dump_outputs(out, str(tmp_path / d), limit=total // 2)
    got = {f: np.load(tmp_path / 'a' / f) for f in sorted(os.listdir(tmp_path / 'a'))}
    assert sum(a.nbytes for a in got.values()) <= total // 2 + 8 * len(got)        # (at least one element each)
    assert got['source_domain.hm.npy'].size == 48 and got['source_domain.wh.npy'].size == 32
    assert set(got['source_domain.hm.npy']) <= set(out['source_domain']['hm'].numpy().ravel())
    for f, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / 'b' / f))


def test_rewind_point_restores_the_parameters_and_the_adam_state():
    """The dumped step starts from the state before the warm-up: parameters as they were, Adam moments and step count
    zero (CPU tensors: the arena and the optimizer's bookkeeping, not the fused kernel)."""
    import types
    import torch
    import bench
    from hip_runtime import optim
    torch.manual_seed(0)
    net = torch.nn.Linear(4, 3)
    opt = optim.Adam(net.parameters(), lr=1e-2)
    rewind = bench.rewind_point(types.SimpleNamespace(optimizer=opt))
    opt.zero_grad()                     # the first step's call: the parameters move into the arena, moments appear
    before = [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
        for st in opt.state.values():
            st['exp_avg'].fill_(0.5)
            st['exp_avg_sq'].fill_(0.25)
            st['step'].fill_(7.0)
    opt._step = 7
    rewind()
    assert all(torch.equal(p, b) for p, b in zip(net.parameters(), before))
    assert opt._step == 0 and len(opt.state) == 2
    assert all(not t.any() for st in opt.state.values() for t in st.values())


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_the_last_step(tmp_path):
    r = _run(['--steps', '3', '--warmup', '1', '--batch', '2', '--size', '128', '--dump-outputs', str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(out) == 1 and out[0].startswith('{'), out
    line = json.loads(out[0])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['ms_per_step_min'] <= line['ms_per_step'] * 1.05
    for leg in ('roofline', 'cpu_baseline', 'decode_latency', 'inference', 'matrix_mode_split', 'dp1_rccl',
                'other_configs', 'dcn_offsets'):
        assert line[leg] is None, leg
    import numpy as np
    files = sorted(os.listdir(tmp_path))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64e6
    for domain in ('source_domain', 'target_domain'):
        for head, ch in (('hm', 6), ('wh', 2), ('reg', 2)):
            a = np.load(os.path.join(tmp_path, '%s.%s.npy' % (domain, head)))
            assert a.dtype == np.float32 and a.shape == (2, ch, 32, 32) and np.isfinite(a).all()
    for k, v in line['losses'].items():
        assert abs(float(np.load(os.path.join(tmp_path, 'stats.%s.npy' % k))) - v) <= 1e-5 * max(1.0, abs(v)), k
    # same arguments, same inputs: a second run dumps the same outputs (the dumped step starts from the state before
    # the warm-up, bench.rewind_point -- without it Adam spreads the backward pass's last-bit noise within a few steps)
    again = tmp_path / 'again'
    r = _run(['--steps', '3', '--warmup', '1', '--batch', '2', '--size', '128', '--dump-outputs', str(again)])
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(again)) == files
    for f in files:
        a, b = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(again, f))
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6), (f, float(np.abs(a - b).max()))
