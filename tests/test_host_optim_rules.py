"""The arithmetic of csrc/optim.hip without a GPU: the rule functors are `__host__ __device__`, and a stand-alone
program (tests/optim_rules_host.cpp, built here with the address and undefined-behaviour sanitizers on the host side)
runs them on the CPU.  One update from a mid-training state, every flag of every rule, against torch.optim's functional
single-tensor forms.  Bound: 1e-6 of max(1, |ref|), the bound the GPU tests hold over five steps; eight leading
elements are an alignment gap (all zero) and must stay finite for eps = 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.optim.adam import adam
from torch.optim.rmsprop import rmsprop
from torch.optim.sgd import sgd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, GAP = 4096, 8


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path_factory.mktemp('optim_rules') / 'optim_rules_host')
    subprocess.check_call([hipcc, '-O2', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-Xarch_host',
                           '-fsanitize=address,undefined', '-I', os.path.join(ROOT, 'centernet-uda_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'optim_rules_host.cpp'), '-o', exe])

    def run(rule, h, arrays, amsgrad=0):
        path = exe + '.bin'
        np.concatenate([t.numpy() for t in arrays]).astype(np.float32).tofile(path)
        subprocess.check_call([exe, rule, str(N)] + [repr(float(x)) for x in h] + [path, str(int(amsgrad))])
        return torch.from_numpy(np.fromfile(path, dtype=np.float32)).view(5, N)
    return run


def _arrays(seed):
    g = torch.Generator().manual_seed(seed)
    p, grad = torch.randn(N, generator=g), torch.randn(N, generator=g)
    first = (torch.randn(N, generator=g) * 0.3).clamp(-0.4, 0.4)       # momentum buffer / exp_avg / grad_avg
    second = torch.rand(N, generator=g) + 0.2                           # second moments (> first ** 2)
    third = torch.rand(N, generator=g) + 0.1
    for t in (p, grad, first, second, third):
        t[:GAP] = 0
    return p, grad, first, second, third


def _hold(tag, got, want, eps_zero=False):
    for k, (x, y) in enumerate(zip(got, want)):
        if y is None:
            continue
        assert torch.isfinite(x[:GAP]).all(), (tag, k)
        if eps_zero:
            assert not x[:GAP].any(), (tag, k)
        err = ((x[GAP:] - y[GAP:]).abs() / y[GAP:].abs().clamp_min(1.0)).max().item()
        print('%s operand %d: %.2e' % (tag, k, err))
        assert err <= 1e-6, (tag, k, err)


@pytest.mark.parametrize('mu,damp,wd,nesterov,maximize,first', [
    (0, 0, 0, 0, 0, 0), (0.9, 0, 1e-2, 0, 0, 0), (0.9, 0, 1e-2, 0, 0, 1), (0.9, 0.1, 0, 0, 0, 0), (0.9, 0, 0, 1, 0, 0),
    (0, 0, 0, 0, 1, 0), (0.9, 0, 1e-2, 1, 1, 0)])
def test_sgd_rule(program, mu, damp, wd, nesterov, maximize, first):
    p, g, a, b, c = _arrays(1)
    out = program('sgd', [1e-2, mu, damp, wd, nesterov, maximize, first, 1 if mu else 0], (p, g, a, b, c))
    P, bufs = p.clone(), [None if (first or not mu) else a.clone()]
    sgd([P], [g.clone()], bufs, weight_decay=wd, momentum=mu, lr=1e-2, dampening=damp, nesterov=bool(nesterov),
        maximize=bool(maximize), foreach=False, has_sparse_grad=False)
    _hold('sgd', [out[0], out[2]], [P, bufs[0] if mu else None])


@pytest.mark.parametrize('wd,decoupled,maximize,amsgrad,step,eps,beta1', [
    (1e-2, 1, 0, 0, 1, 1e-8, 0.9), (1e-2, 1, 0, 1, 3, 1e-8, 0.9), (1e-2, 0, 0, 1, 5, 1e-8, 0.9), (1e-2, 0, 1, 0, 2, 1e-8, 0.9),
    (0, 1, 0, 1, 4, 0.0, 0.9), (1e-2, 1, 0, 0, 2, 1e-8, 0.3)])
def test_adam_family_rule(program, wd, decoupled, maximize, amsgrad, step, eps, beta1):
    p, g, m, v, vmax = _arrays(2)
    vmax = torch.maximum(vmax, v * (torch.arange(N) % 2))
    vmax[:GAP] = 0
    out = program('adam', [1e-2, beta1, 0.999, eps, wd, decoupled, maximize, step], (p, g, m, v, vmax), amsgrad)
    lo = GAP if eps == 0 else 0                      # torch's own 0 / 0 in the gap is NaN: the reference skips it
    P, G, M, V, X = (t[lo:].clone() for t in (p, g, m, v, vmax))
    adam([P], [G], [M], [V], [X] if amsgrad else [], [torch.tensor(float(step - 1))], amsgrad=bool(amsgrad), beta1=beta1,
         beta2=0.999, lr=1e-2, weight_decay=wd, eps=eps, maximize=bool(maximize), foreach=False, capturable=False,
         differentiable=False, fused=False, has_complex=False, decoupled_weight_decay=bool(decoupled))
    pad = lambda t: torch.cat([torch.zeros(lo), t])
    _hold('adam', out[[0, 2, 3, 4]], [pad(P), pad(M), pad(V), pad(X) if amsgrad else None], eps == 0 and not wd)


@pytest.mark.parametrize('wd,mu,maximize,centered,eps', [
    (0, 0, 0, 0, 1e-8), (0, 0, 0, 1, 1e-8), (1e-2, 0.5, 0, 1, 1e-8), (0, 0.5, 1, 0, 1e-8), (0, 0, 0, 0, 0.0),
    (0, 0.5, 0, 1, 0.0)])
def test_rmsprop_rule(program, wd, mu, maximize, centered, eps):
    p, g, ga, sq, buf = _arrays(3)
    out = program('rms', [1e-2, 0.99, eps, wd, mu, maximize, centered, 0], (p, g, sq, ga, buf))
    lo = GAP if eps == 0 else 0
    P, G, SQ, GA, BUF = (t[lo:].clone() for t in (p, g, sq, ga, buf))
    rmsprop([P], [G], [SQ], [GA] if centered else [], [BUF] if mu else [], [torch.tensor(0.0)], lr=1e-2, alpha=0.99,
            eps=eps, weight_decay=wd, momentum=mu, centered=bool(centered), maximize=bool(maximize), foreach=False,
            capturable=False, differentiable=False, has_complex=False)
    pad = lambda t: torch.cat([torch.zeros(lo), t])
    _hold('rmsprop', out[[0, 2, 3, 4]], [pad(P), pad(SQ), pad(GA) if centered else None, pad(BUF) if mu else None],
          eps == 0)
