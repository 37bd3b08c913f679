"""MI355X parity of the arena optimizers beyond plain Adam (csrc/optim.hip, hip_runtime/optim.py) against torch.optim on
the CPU with the same gradients: every rule and flag, untouched parameters, a parameter whose first gradient arrives
late, parameter groups under a scheduler, the alignment gaps with eps = 0, packed weights after a step, and ADVENT's
discriminator on a non-Adam optimizer.  Bound: `_close(mine, ref, 1e-6)` of tests/test_gpu_ops.py, the one the Adam
test holds."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import _close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the long tensor: more than one workgroup's share (256 threads x 4 floats) and no multiple of 64 -- its last slot is part gap
SHAPES = [(5, 3), (7,), (2, 2, 3), (11,), (70001,)]
STEPS = 5
NEVER, LATE, LATE_FROM = 2, 3, 2            # tensor 2 never receives a gradient; tensor 3 from the third step on
_G = torch.Generator().manual_seed(8)
START = [torch.randn(s, generator=_G) for s in SHAPES]
GRADS = [[torch.randn(s, generator=_G) for s in SHAPES] for _ in range(STEPS)]
GRADS_DEV = []


def _grads_dev():
    if not GRADS_DEV:
        GRADS_DEV.extend([g.to(DEV) for g in gs] for gs in GRADS)
    return GRADS_DEV


def _pair(name, kw, grouped=None):
    from hip_runtime import optim
    ref = [t.clone().requires_grad_(True) for t in START]
    mine = [t.clone().to(DEV).requires_grad_(True) for t in START]

    def groups(ps):
        return ps if grouped is None else [dict(params=[ps[i] for i in idx], **g) for idx, g in grouped]
    return ref, mine, getattr(torch.optim, name)(groups(ref), **kw), getattr(optim, name)(groups(mine), **kw)


def _run(ref, mine, o_ref, o_mine, scheds=(), late=True, after_step=None):
    gd = _grads_dev()
    for it in range(STEPS):
        o_ref.zero_grad()
        o_mine.zero_grad()
        for i, (r, m) in enumerate(zip(ref, mine)):
            if i == NEVER or (late and i == LATE and it < LATE_FROM):
                continue
            (r * GRADS[it][i]).sum().backward()
            (m * gd[it][i]).sum().backward()
        o_ref.step()
        o_mine.step()
        for s in scheds:
            s.step()
        if after_step is not None:
            after_step(it)


def _compare(ref, mine, o_ref, o_mine):
    for i, (r, m) in enumerate(zip(ref, mine)):
        _close(m, r, 1e-6)
        want = o_ref.state.get(r, {})
        got = o_mine.state[m] if m in o_mine.state else {}
        assert set(got) == set(want), (i, set(got), set(want))          # torch's keys, absent where torch has none
        for k, v in want.items():
            if k == 'step':
                assert float(got[k]) == float(v), (i, float(got[k]), float(v))
            else:
                _close(got[k], v, 1e-6)
    assert torch.equal(mine[NEVER].cpu(), START[NEVER])                 # no gradient: bit-equal to its start
    assert not torch.equal(mine[LATE].cpu(), START[LATE])


CASES = {
    'sgd': ('SGD', dict(lr=1e-2)),
    'sgd_momentum_wd': ('SGD', dict(lr=1e-2, momentum=0.9, weight_decay=1e-2)),
    'sgd_dampening': ('SGD', dict(lr=1e-2, momentum=0.9, dampening=0.1)),
    'sgd_nesterov': ('SGD', dict(lr=1e-2, nesterov=True, momentum=0.9)),
    'sgd_maximize': ('SGD', dict(lr=1e-2, maximize=True)),
    'adamw_wd': ('AdamW', dict(lr=1e-2, weight_decay=1e-2)),
    'adamw_amsgrad': ('AdamW', dict(lr=1e-2, amsgrad=True)),
    'adam_amsgrad': ('Adam', dict(lr=1e-2, amsgrad=True)),
    'rmsprop': ('RMSprop', dict()),
    'rmsprop_centered': ('RMSprop', dict(centered=True)),
    'rmsprop_momentum_centered_wd': ('RMSprop', dict(momentum=0.5, centered=True, weight_decay=1e-2)),
    # the remaining flags that change the arithmetic, once each
    'adam_maximize_wd': ('Adam', dict(lr=1e-2, maximize=True, weight_decay=1e-2)),
    'rmsprop_maximize_momentum': ('RMSprop', dict(maximize=True, momentum=0.5)),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_rule_matches_torch_skips_untouched_and_counts_per_parameter(case):
    name, kw = CASES[case]
    ref, mine, o_ref, o_mine = _pair(name, kw)
    _run(ref, mine, o_ref, o_mine)
    _compare(ref, mine, o_ref, o_mine)
    sd = o_mine.state_dict()
    assert len(sd['param_groups']) == 1 and NEVER not in sd['state']


def test_one_launch_per_group_and_run_and_a_cut_at_the_first_update():
    import hip_runtime as hr
    ref, mine, o_ref, o_mine = _pair('SGD', dict(lr=1e-2, momentum=0.9))
    seen = [0]
    launches = []

    def optim_launches():
        return sum(v for k, v in hr.launch_counts().items() if 'optim_kernel' in k)

    def count(it):
        now = optim_launches()
        launches.append(now - seen[0])
        seen[0] = now
    seen[0] = optim_launches()
    _run(ref, mine, o_ref, o_mine, after_step=count)
    # tensors 0 1 | 2 never | 3 from the third step | 4: runs [0 1] [4]; then [0 1] [3: first update] [4]; then [0 1] [3 4]
    assert launches == [2, 2, 3, 2, 2], launches
    _compare(ref, mine, o_ref, o_mine)


@pytest.mark.parametrize('name,kw', [('SGD', dict(momentum=0.9)), ('AdamW', dict()), ('RMSprop', dict(centered=True)),
                                     ('Adam', dict())], ids=['SGD', 'AdamW', 'RMSprop', 'Adam'])
def test_two_groups_with_their_own_lr_and_weight_decay_under_a_scheduler(name, kw):
    grouped = [((0, 1), dict(lr=1e-2, weight_decay=0.0)), ((2, 3, 4), dict(lr=3e-3, weight_decay=1e-2))]
    ref, mine, o_ref, o_mine = _pair(name, kw, grouped)
    scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[2], gamma=0.1) for o in (o_ref, o_mine)]
    # plain Adam keeps one step counter for the arena: every tensor but the untouched one gets its gradient from the start
    _run(ref, mine, o_ref, o_mine, scheds, late=name != 'Adam')
    assert [g['lr'] for g in o_mine.param_groups] == [g['lr'] for g in o_ref.param_groups]
    assert o_mine.param_groups[0]['lr'] == pytest.approx(1e-3)                  # the milestone fired inside the run
    if name == 'Adam':
        for r, m in zip(ref, mine):
            _close(m, r, 1e-6)
        assert torch.equal(mine[NEVER].cpu(), START[NEVER])
    else:
        _compare(ref, mine, o_ref, o_mine)


@pytest.mark.parametrize('name,kw', [('Adam', dict(amsgrad=True, eps=0)), ('AdamW', dict(eps=0)), ('RMSprop', dict(eps=0)),
                                     ('RMSprop', dict(eps=0, centered=True, momentum=0.5))],
                         ids=['adam_amsgrad', 'adamw', 'rmsprop', 'rmsprop_centered_momentum'])
def test_alignment_gaps_stay_finite_with_eps_zero(name, kw):
    ref, mine, o_ref, o_mine = _pair(name, kw)
    _run(ref, mine, o_ref, o_mine, late=False)
    a = o_mine._arena
    assert torch.isfinite(a.flat_param).all()
    assert o_mine._bufs and all(torch.isfinite(b).all() for b in o_mine._bufs.values())
    gap = a.flat_param[a.offsets[1] + 7:a.offsets[2]]                  # behind the 7-element tensor, inside its slot
    assert gap.numel() == 57 and not gap.any()
    for i, (r, m) in enumerate(zip(ref, mine)):                         # and the guard costs the real elements nothing
        _close(m, r, 1e-6)


def test_packed_weights_follow_the_sgd_step():
    """The check of test_pack_refresh_after_the_fused_adam_step at one small layer: the forward after optim.SGD.step()
    computes with the stepped weights (the step bumps the parameter epoch: the cached packed image is rebuilt)."""
    from hip_runtime import nn as hnn, optim
    g = torch.Generator().manual_seed(21)
    conv = hnn.Conv2d(16, 32, 3, padding=1, bias=True).to(DEV)
    x = torch.randn(2, 16, 9, 11, generator=g).to(DEV)

    def ref():
        return F.conv2d(x.cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu(), 1, 1)
    opt = optim.SGD(conv.parameters(), lr=0.5, momentum=0.9)
    y0 = conv(x)
    _close(y0, ref())
    for _ in range(2):
        opt.zero_grad()
        conv(x).square().mean().backward()
        w0 = conv.weight.detach().clone()
        opt.step()
        assert not torch.equal(conv.weight.detach(), w0)
        y = conv(x)
        _close(y, ref())
    assert (y - y0).abs().max().item() > 1e-3


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def test_advent_discriminator_on_rmsprop():
    """uda/adversarial_entropy_minimization.py:47 resolves `optimizer.name`: with RMSprop the discriminator is
    stepped by optim.RMSprop, and one plugin step moves its parameters like torch.optim.RMSprop on the CPU from the
    pre-step parameters and the gradients the step left in the arena."""
    import numpy as np
    import inputs as gin
    import uda
    from backends import dla
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    torch.manual_seed(0)
    model = dla.build(num_classes=6, rotated_boxes=True)
    plugin = uda.AdversarialEntropyMinimization(1e-2, optimizer=_Cfg(name='RMSprop', params=_Cfg(lr=1e-3)))
    plugin.cfg = _Cfg(max_detections=20, model=_Cfg(backend=_Cfg(params=_Cfg(rotated_boxes=True, num_classes=6))))
    plugin.backend = model
    plugin.device = torch.device(DEV)
    plugin.optimizer = optim.Adam(model.parameters(), lr=5e-5, weight_decay=1e-4)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, angle_weight=1.0, periodic=True)
    plugin.init_done()
    assert type(plugin.discriminator_optimizer) is optim.RMSprop
    plugin.to(DEV)
    plugin.set_phase(True)
    B, S, M = 2, 128, 8
    data = {k: T(v) for k, v in gin.detection_batch(B, 6, S // 4, S // 4, M, (4, 2), 3, 71).items()}
    data['input'] = T(gin.image_batch(B, S, S, 72))
    data['target_domain_input'] = T(gin.image_batch(B, S, S, 73))
    dparams = list(plugin.discriminator.parameters())
    before = [p.detach().cpu().clone() for p in dparams]
    out = plugin.step(data)
    assert all(np.isfinite(float(v)) for v in out['stats'].values())
    a = plugin.discriminator_optimizer._arena
    assert all(a.touched) and len(a.params) == len(dparams)
    cpu = [torch.nn.Parameter(b.clone()) for b in before]
    for c, p in zip(cpu, dparams):
        c.grad = p.grad.detach().cpu().clone()              # a view of the arena's flat gradient
        assert c.grad.abs().max() > 0
    torch.optim.RMSprop(cpu, lr=1e-3).step()
    for c, p, b in zip(cpu, dparams, before):
        _close(p, c, 1e-6)
        assert not torch.equal(p.detach().cpu(), b)
