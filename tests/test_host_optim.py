"""Host-side (no GPU) checks of hip_runtime.optim: the names `resolve` knows, constructor signatures and argument
checks against torch.optim's, parameter groups, and the state-dict interchange with torch.optim in both directions
(CPU tensors: the arena's bookkeeping is device-agnostic, only the kernels need the GPU)."""
import inspect

import pytest
import torch

NAMES = ('Adam', 'AdamW', 'SGD', 'RMSprop')
ABSTRACT = ('foreach', 'fused', 'capturable', 'differentiable')     # which implementation torch picks, not arithmetic


def test_resolve_knows_the_four_and_names_them_otherwise():
    from hip_runtime import optim
    for n in NAMES:
        cls = optim.resolve(n)
        assert inspect.isclass(cls) and cls.__name__ == n and issubclass(cls, torch.optim.Optimizer)
    with pytest.raises(NotImplementedError) as e:
        optim.resolve('Adagrad')
    for n in NAMES:
        assert n in str(e.value)


@pytest.mark.parametrize('name', NAMES)
def test_constructor_has_every_hyper_parameter_and_default_of_torch(name):
    from hip_runtime import optim
    mine = inspect.signature(getattr(optim, name).__init__).parameters
    ref = inspect.signature(getattr(torch.optim, name).__init__).parameters
    for k, p in ref.items():
        assert k in mine, k
        assert mine[k].default == p.default, (k, mine[k].default, p.default)
        assert mine[k].kind == p.kind, k
    w = torch.nn.Parameter(torch.zeros(3))
    for k in ABSTRACT:
        if k in ref:
            getattr(optim, name)([w], **{k: ref[k].default})            # False / None: accepted and ignored
            with pytest.raises(ValueError, match=k):
                getattr(optim, name)([w], **{k: True})
    # the groups carry torch's keys: a state dict of ours is laid out like torch's
    assert set(getattr(optim, name)([w]).param_groups[0]) == set(getattr(torch.optim, name)([w]).param_groups[0])


@pytest.mark.parametrize('name,kw', [
    ('SGD', dict(nesterov=True)), ('SGD', dict(nesterov=True, momentum=0.9, dampening=0.1)), ('SGD', dict(lr=-1.0)),
    ('SGD', dict(momentum=-0.5)), ('SGD', dict(weight_decay=-1.0)),
    ('Adam', dict(lr=-1.0)), ('Adam', dict(betas=(1.0, 0.9))), ('Adam', dict(betas=(0.9, -0.1))), ('Adam', dict(eps=-1.0)),
    ('AdamW', dict(weight_decay=-1.0)), ('AdamW', dict(betas=(0.9, 1.0))),
    ('RMSprop', dict(lr=-1.0)), ('RMSprop', dict(alpha=-0.1)), ('RMSprop', dict(eps=-1.0)), ('RMSprop', dict(momentum=-1.0)),
    ('RMSprop', dict(weight_decay=-1.0))])
def test_invalid_values_raise_where_torch_does(name, kw):
    from hip_runtime import optim
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        getattr(torch.optim, name)([w], **kw)
    with pytest.raises(ValueError):
        getattr(optim, name)([w], **kw)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(5, 3), (7,), (2, 2, 3), (70,)]]


def _stepped_torch(name, kw, two_groups=False):
    """a torch optimizer stepped twice on the CPU; the third tensor never receives a gradient"""
    ps = _params(1)
    groups = [{'params': ps[:2], 'lr': 0.02}, {'params': ps[2:], 'lr': 0.005}] if two_groups else ps
    opt = getattr(torch.optim, name)(groups, **kw)
    g = torch.Generator().manual_seed(2)
    for _ in range(2):
        opt.zero_grad()
        for i, p in enumerate(ps):
            if i != 2:
                (p * torch.randn(p.shape, generator=g)).sum().backward()
        opt.step()
    return opt, ps


CASES = [('SGD', dict(lr=0.01, momentum=0.9)), ('RMSprop', dict(centered=True, momentum=0.5)),
         ('AdamW', dict(amsgrad=True)), ('Adam', dict(amsgrad=True)), ('Adam', dict()), ('SGD', dict(lr=0.01)),
         ('RMSprop', dict())]


@pytest.mark.parametrize('name,kw', CASES, ids=lambda v: v if isinstance(v, str) else ','.join(v) or 'default')
@pytest.mark.parametrize('two_groups', [False, True], ids=['one_group', 'two_groups'])
def test_state_dict_interchanges_with_torch_in_both_directions(name, kw, two_groups):
    from hip_runtime import optim
    ref, ref_ps = _stepped_torch(name, kw, two_groups)
    sd = ref.state_dict()
    ps = _params(3)
    groups = [{'params': ps[:2]}, {'params': ps[2:]}] if two_groups else ps
    mine = getattr(optim, name)(groups, lr=1.0)
    mine.load_state_dict(sd)
    assert [g['lr'] for g in mine.param_groups] == [g['lr'] for g in ref.param_groups]
    plain_adam = name == 'Adam' and not kw                   # one counter, state for every parameter from the start
    for i, (p, rp) in enumerate(zip(ps, ref_ps)):
        want = ref.state.get(rp, {})
        if not want and not plain_adam:
            assert p not in mine.state                       # a key is absent where torch leaves it absent
            continue
        got = mine.state[p]
        assert set(got) == (set(want) or {'step', 'exp_avg', 'exp_avg_sq'})
        for k, v in want.items():
            assert torch.equal(got[k], v), k
            if k != 'step':                                  # a view into the flat state buffer, not a copy
                assert got[k].data_ptr() == mine._bufs[k].data_ptr() + 4 * mine._arena.offsets[i]
    # ours saved -> a fresh torch optimizer: equal tensors, the groups' own learning rates
    out = mine.state_dict()
    assert set(out['state']) == (set(sd['state']) if not plain_adam else set(range(len(ps))))
    fresh_ps = _params(4)
    fresh = getattr(torch.optim, name)([{'params': fresh_ps[:2]}, {'params': fresh_ps[2:]}] if two_groups else fresh_ps,
                                       **kw)
    fresh.load_state_dict(out)
    assert [g['lr'] for g in fresh.param_groups] == [g['lr'] for g in ref.param_groups]
    for fp, rp in zip(fresh_ps, ref_ps):
        for k, v in ref.state.get(rp, {}).items():
            assert torch.equal(fresh.state[fp][k], v), k
    # and torch goes on from there exactly as the original does (the state it read is complete)
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    with torch.no_grad():
        for fp, rp in zip(fresh_ps, ref_ps):
            fp.copy_(rp)
    for o, params, g in ((ref, ref_ps, g1), (fresh, fresh_ps, g2)):
        o.zero_grad()
        for i, p in enumerate(params):
            if i != 2:
                (p * torch.randn(p.shape, generator=g)).sum().backward()
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(fresh_ps, ref_ps))


def test_checkpoint_helpers_carry_the_new_optimizers_unchanged(tmp_path):
    """utils.helper.save_model / load_model (helper.py:83-147) with an optimizer other than Adam and two groups."""
    from hip_runtime import optim
    from utils.helper import load_model, save_model
    ref, ref_ps = _stepped_torch('RMSprop', dict(centered=True, momentum=0.5), two_groups=True)
    sched = torch.optim.lr_scheduler.MultiStepLR(ref, milestones=[1], gamma=0.1)
    ref.step()
    sched.step()
    net = torch.nn.Linear(4, 3)
    path = tmp_path / 'resume.pth'
    torch.save({'epoch': 2, 'state_dict': net.state_dict(), 'optimizer': ref.state_dict(),
                'scheduler': sched.state_dict()}, path)
    ps = _params(5)
    mine = optim.RMSprop([{'params': ps[:2]}, {'params': ps[2:]}], lr=1.0)
    msched = torch.optim.lr_scheduler.MultiStepLR(mine, milestones=[7], gamma=0.5)
    assert load_model(net, mine, msched, path, resume=True) == 3
    assert [g['lr'] for g in mine.param_groups] == pytest.approx([0.002, 0.0005])
    assert torch.equal(mine.state[ps[0]]['grad_avg'], ref.state[ref_ps[0]]['grad_avg'])
    out = tmp_path / 'again.pth'
    save_model(net, out, epoch=3, optimizer=mine, scheduler=msched)
    ck = torch.load(out, weights_only=False)
    fresh_ps = _params(6)
    fresh = torch.optim.RMSprop([{'params': fresh_ps[:2]}, {'params': fresh_ps[2:]}], centered=True, momentum=0.5)
    fresh.load_state_dict(ck['optimizer'])
    assert torch.equal(fresh.state[fresh_ps[3]]['momentum_buffer'], ref.state[ref_ps[3]]['momentum_buffer'])


def test_groups_own_contiguous_ranges_and_a_late_group_is_refused():
    from hip_runtime import optim
    ps = _params(7)
    frozen = torch.nn.Parameter(torch.zeros(9), requires_grad=False)
    opt = optim.SGD([{'params': [ps[0], frozen, ps[1]], 'lr': 0.1}], lr=0.01, momentum=0.9)
    opt.zero_grad()                                         # builds the arena over the first group
    opt.add_param_group({'params': ps[2:], 'weight_decay': 0.5})     # before the first step: the arena is rebuilt
    opt.zero_grad()
    a = opt._arena
    assert [id(p) for p in a.params] == [id(p) for p in ps] and a.valid()
    assert opt._ranges == [(0, 2), (2, 4)]                  # frozen parameters take no slot
    assert opt.param_groups[1]['lr'] == 0.01 and opt.param_groups[1]['momentum'] == 0.9
    assert not any(a.touched)
    # runs: per group, over touched neighbours, cut where the launches differ (first update of a momentum buffer)
    a.touched = [True, True, True, True]
    opt._count = [1, 1, 0, 1]
    assert opt._runs(a, opt.param_groups[0], 0, 2) == [[0, a.offsets[2], False]]
    assert opt._runs(a, opt.param_groups[1], 2, 4) == [[a.offsets[2], a.offsets[3], True], [a.offsets[3], a.numel, False]]
    a.touched = [True, False, True, True]
    opt._count = [1, 1, 1, 1]
    assert opt._runs(a, opt.param_groups[0], 0, 2) == [[0, a.offsets[1], False]]
    assert opt._runs(a, opt.param_groups[1], 2, 4) == [[a.offsets[2], a.numel, False]]
    opt.load_state_dict(opt.state_dict())                   # state exists from here on (as after a step)
    with pytest.raises(RuntimeError, match='arena'):
        opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))]})


def test_new_abi_entries_reject_bad_arguments_without_a_gpu():
    import ctypes
    import hip_runtime as hr
    L = hr.lib()
    assert L.cnuda_sgd_step(None, None, None, 64, 0.1, 0.0, 0.0, 0.0, 0, 0, 0, None) == -1
    assert L.cnuda_adamw_step(None, None, None, None, None, 64, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 1, None) == -1
    assert L.cnuda_rmsprop_step(None, None, None, None, None, 64, 1e-2, 0.99, 1e-8, 0.0, 0.0, 0, None) == -1
    buf = (ctypes.c_float * 80)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) // 16 * 16)             # a 16-byte aligned host address: never dereferenced
    off = ctypes.c_void_p(p.value + 4)
    for n in (0, -4, 6):                                    # n <= 0, not a multiple of four floats
        assert L.cnuda_sgd_step(p, p, None, n, 0.1, 0.0, 0.0, 0.0, 0, 0, 0, None) == -1
        assert L.cnuda_adamw_step(p, p, p, p, None, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 1, None) == -1
        assert L.cnuda_rmsprop_step(p, p, p, None, None, n, 1e-2, 0.99, 1e-8, 0.0, 0.0, 0, None) == -1
    assert L.cnuda_sgd_step(off, p, None, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 0, None) == -1          # misaligned operand
    assert b'aligned' in L.cnuda_last_error()
    assert L.cnuda_sgd_step(p, p, None, 8, 0.1, 0.9, 0.0, 0.0, 0, 0, 0, None) == -1            # momentum without a buffer
    assert L.cnuda_sgd_step(p, p, p, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 0, None) == -1              # a buffer without momentum
    assert L.cnuda_sgd_step(p, p, p, 8, 0.1, 0.9, 0.1, 0.0, 1, 0, 0, None) == -1              # nesterov with dampening
    assert L.cnuda_sgd_step(p, p, None, 8, 0.1, 0.0, 0.0, 0.0, 0, 2, 0, None) == -1           # a flag that is not 0 / 1
    assert L.cnuda_adamw_step(p, p, p, p, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0, None) == -1    # step 0
    assert L.cnuda_rmsprop_step(p, p, p, None, None, 8, 1e-2, 0.99, 1e-8, 0.0, 0.5, 0, None) == -1      # momentum, no buffer


def test_ops_refuse_cpu_tensors():
    from hip_runtime import ops
    z = torch.zeros(64)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.sgd_step_(z, z, None, 0.1, 0, 0, 0, False, False, False)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.adamw_step_(z, z, z, z, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, True, False, 1)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.rmsprop_step_(z, z, z, None, None, 1e-2, 0.99, 1e-8, 0.0, 0.0, False)


def _old_style(sd, keep):
    """the state dict with only the group keys an older writer knew"""
    out = {'state': sd['state'], 'param_groups': [{k: v for k, v in g.items() if k in keep} for g in sd['param_groups']]}
    assert all(set(g) == set(keep) for g in out['param_groups'])
    return out


@pytest.mark.parametrize('keep', [('params', 'lr', 'betas', 'eps', 'weight_decay'),
                                  ('params', 'lr', 'betas', 'eps', 'weight_decay', 'amsgrad')],
                         ids=['this_projects_earlier_adam', 'torch_1x_adam'])
def test_adam_reads_checkpoints_whose_groups_lack_the_newer_keys(keep):
    """Resume checkpoints written before the groups carried amsgrad / maximize / ... (this project's earlier Adam: four
    hyper-parameters; torch 1.x: + amsgrad) load, the missing keys take their defaults, and the one-counter path is kept."""
    from hip_runtime import optim
    ref, ref_ps = _stepped_torch('Adam', dict(lr=5e-5, weight_decay=1e-4))
    ps = _params(3)
    opt = optim.Adam(ps, lr=1.0)
    opt.load_state_dict(_old_style(ref.state_dict(), keep))
    g = opt.param_groups[0]
    assert g['lr'] == 5e-5 and g['weight_decay'] == 1e-4
    assert set(g) == set(optim.Adam(_params(4)).param_groups[0])
    assert g['amsgrad'] is False and g['maximize'] is False and g['decoupled_weight_decay'] is False and g['fused'] is None
    assert opt._global_count and opt._step == 2
    assert torch.equal(opt.state[ps[0]]['exp_avg'], ref.state[ref_ps[0]]['exp_avg'])
    assert opt._runs(opt._arena, g, 0, 4) == []              # (nothing touched; the walk reads the groups' flags)


@pytest.mark.parametrize('name,kw,keep', [
    ('SGD', dict(lr=0.01, momentum=0.9), ('params', 'lr', 'momentum', 'dampening', 'weight_decay', 'nesterov')),
    ('RMSprop', dict(centered=True), ('params', 'lr', 'momentum', 'alpha', 'eps', 'centered', 'weight_decay'))])
def test_sgd_and_rmsprop_read_torch_1x_groups(name, kw, keep):
    from hip_runtime import optim
    ref, _ = _stepped_torch(name, kw)
    opt = getattr(optim, name)(_params(3), lr=1.0)
    opt.load_state_dict(_old_style(ref.state_dict(), keep))
    g = opt.param_groups[0]
    assert set(g) == set(getattr(optim, name)(_params(4)).param_groups[0])
    assert g['maximize'] is False and g['foreach'] is None and g['lr'] == ref.param_groups[0]['lr']


def test_adam_settles_its_step_counting_once():
    """One counter while every group is plain, per-parameter counts otherwise; settled by the first step or a load."""
    from hip_runtime import optim
    ps = _params(5)
    mixed = optim.Adam([{'params': ps[:2]}, {'params': ps[2:], 'amsgrad': True}])
    assert not mixed._global_count
    plain = optim.Adam(_params(6))
    plain.zero_grad()
    assert plain._global_count and len(plain.state) == 4
    ref, _ = _stepped_torch('Adam', dict(amsgrad=True))
    plain.load_state_dict(ref.state_dict())                 # the loaded groups decide: amsgrad -> torch's counts
    assert not plain._global_count and plain._count == [2, 2, 0, 2] and len(plain.state) == 3
    plain.param_groups[0]['amsgrad'] = False                # a later change of flags does not change the counting
    assert not plain._global_count


def test_add_param_group_releases_an_early_arena_and_refuses_a_shared_one():
    from hip_runtime import arena as arena_mod, optim
    ps = _params(8)
    opt = optim.SGD(ps[:2], lr=0.1)
    opt.zero_grad()
    old = opt._arena
    ptrs = [p.data_ptr() for p in ps[:2]]
    opt.add_param_group({'params': ps[2:]})
    assert old._hooks == [] and not any(k in arena_mod._BY_PTR for k in ptrs)      # released, not just dropped
    opt.zero_grad()
    assert len(opt._arena.params) == 4
    shared = optim.SGD(_params(9)[:2], lr=0.1)
    shared.zero_grad()
    shared._arena.on_ready = lambda i: None                 # what the data-parallel wrapper installs
    with pytest.raises(RuntimeError, match='shared'):
        shared.add_param_group({'params': [torch.nn.Parameter(torch.zeros(3))]})
