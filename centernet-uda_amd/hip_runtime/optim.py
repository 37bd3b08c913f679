"""Optimizers on the flat arena: `Adam`, `AdamW`, `SGD` and `RMSprop` with torch.optim's constructors, arithmetic and
state-dict layout (the driver resolves `torch.optim.<name>` from the config, train.py:88-90; this build resolves the
same names through `resolve`).

One arena holds the parameters of all groups in group order, so a group owns one contiguous range of it.  A step is
one kernel launch per (group, run of neighbouring parameters that received a gradient), with that group's
hyper-parameters as they are at that moment (schedulers write `param_groups[i]['lr']`), then one
`bump_param_epoch(flat_param)`: the packed weights follow.  State tensors (`exp_avg`, `momentum_buffer`, ...) are views
into flat buffers laid out like the arena; `state_dict()` / `load_state_dict()` interchange with torch.optim's.

Step counts.  torch creates a parameter's state when it first receives a gradient and counts its steps from there.
`SGD`, `AdamW`, `RMSprop` -- and `Adam` wherever it leaves the plain rule (amsgrad, maximize, decoupled_weight_decay)
-- keep that count per parameter, and a run is cut wherever neighbours need different launches (a different bias
correction; a momentum buffer that is still to be initialised), so a parameter first touched at step 3 gets torch's
result.  Once every parameter has been updated equally often, nothing is cut.  Plain `Adam` keeps ONE counter for the
whole arena, advanced by every step(), and carries state for every parameter from the start: a parameter whose first
gradient arrives late is bias-corrected with the global count there, not with its own as torch does.  An `Adam` that
mixes plain groups with others counts per parameter in all of them; which of the two it is, is settled at the first
step (or by a loaded state dict) and kept.

Under `hip_runtime.parallel.DataParallel` the groups must list the trainable parameters in `module.parameters()`
order: that is what makes the optimizer and the wrapper resolve to the same arena (arena.arena_for)."""
import torch

from . import ops
from .arena import arena_for


def _refuse(cls, **implementations):
    for name, v in implementations.items():
        if v:
            raise ValueError("hip_runtime.optim.%s: %s=%r is not available: the step is one fused arena kernel "
                             "(pass False or None)" % (cls, name, v))


class _ArenaOptimizer(torch.optim.Optimizer):
    """What the four classes share: the arena over the groups, the flat state buffers, the per-parameter update
    counts, the cutting of runs and the state-dict interchange.  A subclass names the state keys a group carries
    (`_state_keys`), what tells two launches apart (`_run_key`) and how to launch (`_launch`)."""
    _has_step = True            # torch keeps a 'step' entry in the state (SGD does not)
    _global_count = False       # plain Adam: `_step` counts for every parameter of the arena

    def __init__(self, params, defaults):
        self._arena = None
        self._bufs = {}             # state key -> flat buffer laid out like the arena
        self._count = []            # per arena parameter: updates so far
        self._ranges = []           # per group: [lo, hi) indices into arena.params
        self._layout_fixed = False  # a step ran or state was loaded
        self._one_count = None      # plain Adam's choice between one counter and per-parameter counts, once made
        self._step = 0              # steps so far; plain Adam's one counter for the whole arena
        super().__init__(params, defaults)

    # -- subclass hooks ------------------------------------------------------------
    def _state_keys(self, group):
        raise NotImplementedError

    def _run_key(self, group, count):
        """what the launch needs to know about a parameter that is updated for the `count`-th time"""
        return None

    def _launch(self, group, sl, key):
        raise NotImplementedError

    # -- layout ----------------------------------------------------------------------
    def add_param_group(self, param_group):
        if self._layout_fixed:
            raise RuntimeError("%s.add_param_group after the first step (or after load_state_dict): the arena is built "
                               "over the groups' parameters in group order, so a new group would move every parameter "
                               "and its state; add all groups before the first step" % type(self).__name__)
        old = self._arena                           # built by an early zero_grad(): rebuilt with the new group
        if old is not None:
            if old.on_ready is not None:
                raise RuntimeError("%s.add_param_group: the arena over the present groups is already shared with a "
                                   "data-parallel wrapper, and a new group would move the parameters out of it; add "
                                   "all groups before wrapping the module" % type(self).__name__)
            for p, t in zip(old.params, old.touched):
                if not t:
                    p.grad = None                   # a zeroed view is not a gradient the new arena should adopt
            old.release()                           # its hooks and address table entries go with it
            self._arena = None
            self.state.clear()                      # nothing has stepped: only bindings of the old layout
        super().add_param_group(param_group)

    def __setstate__(self, state):
        """Group dicts of a checkpoint replace the live ones (Optimizer.load_state_dict): keys a checkpoint of an older
        torch, or of this class before it had them, does not carry take their defaults, as torch.optim's classes do."""
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)

    def _buf(self, key):
        b = self._bufs.get(key)
        if b is None or b.numel() != self._arena.numel or b.device != self._arena.flat_param.device:
            b = self._bufs[key] = torch.zeros_like(self._arena.flat_param)
        return b

    def _bind(self, i, group, count):
        """self.state[parameter i] = views into the flat buffers (+ 'step'); no entry where torch keeps none"""
        a = self._arena
        p, o = a.params[i], a.offsets[i]
        st = {'step': torch.tensor(float(count))} if self._has_step else {}
        for k in self._state_keys(group):
            st[k] = self._buf(k)[o:o + p.numel()].view(p.shape)
        if st:
            self.state[p] = st
        elif p in self.state:
            del self.state[p]

    def _group_of(self):
        return [g for g, (lo, hi) in zip(self.param_groups, self._ranges) for _ in range(lo, hi)]

    def _ensure(self):
        if self._arena is None or not self._arena.valid():
            old = self._bufs
            a = self._arena = arena_for([p for g in self.param_groups for p in g['params']])
            self._ranges, lo = [], 0
            for g in self.param_groups:
                hi = lo + sum(1 for p in g['params'] if p.requires_grad)
                self._ranges.append((lo, hi))
                lo = hi
            self._bufs = {}
            for k, b in old.items():                # parameters re-pointed (module.to()): the state moves along
                if b.numel() == a.numel:
                    self._buf(k).copy_(b)
            if len(self._count) != len(a.params):
                self._count = [0] * len(a.params)
            for i, g in enumerate(self._group_of()):
                if self._global_count:
                    self._bind(i, g, self._step)
                elif self._count[i]:
                    self._bind(i, g, self._count[i])
        return self._arena

    def zero_grad(self, set_to_none=False):
        # gradients are views of the arena: zeroing is one memset, never `None`
        self._ensure().zero_grad()

    # -- step ------------------------------------------------------------------------
    def _runs(self, a, group, lo, hi):
        """[(start, end, key)]: maximal element ranges over neighbouring touched parameters of one group that take the
        same launch.  Ranges begin and end on slot boundaries (the alignment gap after a tensor belongs to its slot)."""
        runs, run, one_count = [], None, self._global_count
        for i in range(lo, hi):
            if not a.touched[i]:
                run = None
                continue
            key = self._run_key(group, self._step if one_count else self._count[i] + 1)
            end = a.offsets[i + 1] if i + 1 < len(a.params) else a.numel
            if run is not None and run[2] == key:
                run[1] = end
            else:
                run = [a.offsets[i], end, key]
                runs.append(run)
        return runs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        a = self._ensure()
        if not self._layout_fixed:
            self._layout_fixed, self._one_count = True, self._global_count
            if not self._one_count:             # bindings an early zero_grad() made while every group was still plain
                for p in [p for p, c in zip(a.params, self._count) if not c and p in self.state]:
                    del self.state[p]
        self._step += 1
        for group, (lo, hi) in zip(self.param_groups, self._ranges):
            for start, end, key in self._runs(a, group, lo, hi):
                self._launch(group, slice(start, end), key)
        if self._global_count:
            self._count = [self._step] * len(a.params)
            for p in a.params:
                self.state[p]['step'].fill_(float(self._step))
        else:
            for i, g in enumerate(self._group_of()):
                if a.touched[i]:
                    self._count[i] += 1
                    if self._count[i] == 1:
                        self._bind(i, g, 1)
                    elif self._has_step:
                        self.state[a.params[i]]['step'].fill_(float(self._count[i]))
        from . import bump_param_epoch
        # the kernel wrote the flat arena: torch's version counters did not move; cached packed weights follow
        bump_param_epoch(a.flat_param)
        return loss

    # -- state dict --------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        a = self._ensure()            # before the base class fills self.state: _ensure() rebinds every entry
        super().load_state_dict(state_dict)
        self._one_count = None
        self._layout_fixed, self._one_count = True, self._global_count      # the loaded groups decide
        loaded = [dict(self.state[p]) if p in self.state else {} for p in a.params]
        if self._global_count:
            steps = [int(st['step']) for st in loaded if 'step' in st]
            self._step = max(steps) if steps else 0
        for i, (g, st) in enumerate(zip(self._group_of(), loaded)):
            p, o = a.params[i], a.offsets[i]
            for k in self._state_keys(g):
                flat = self._buf(k)[o:o + p.numel()]
                if k in st:
                    flat.copy_(st[k].reshape(-1))
                else:
                    flat.zero_()
            if self._global_count:
                self._count[i] = self._step
                self._bind(i, g, self._step)
                continue
            # SGD keeps no 'step': a momentum buffer in the checkpoint says that the first update is behind it
            self._count[i] = int(st['step']) if 'step' in st else int(bool(st))
            if self._count[i]:
                self._bind(i, g, self._count[i])
            elif p in self.state:
                del self.state[p]


def _check_adam(lr, betas, eps, weight_decay):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: %r" % (lr,))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: %r" % (eps,))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: %r" % (betas[0],))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: %r" % (betas[1],))
    if not 0.0 <= weight_decay:
        raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))


class Adam(_ArenaOptimizer):
    """torch.optim.Adam.  A group with the plain rule (amsgrad, maximize and decoupled_weight_decay all false) runs on
    adam_kernel, the others on the Adam-family kernel of csrc/optim.hip.  If EVERY group is plain at the first step
    (or in a loaded state dict) the optimizer keeps ONE step counter for the arena (module docstring); otherwise all
    groups, the plain ones included, count per parameter as torch does.  The choice is made once and kept: flags
    changed later change the kernel a group runs on, not how steps are counted."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _check_adam(lr, betas, eps, weight_decay)
        _refuse(type(self).__name__, foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize, foreach=foreach, capturable=capturable,
                                      differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    @staticmethod
    def _plain(group):
        return not (group['amsgrad'] or group['maximize'] or group['decoupled_weight_decay'])

    @property
    def _global_count(self):
        if self._one_count is None:         # decided at the first step or load, and kept from there
            return all(self._plain(g) for g in self.param_groups)
        return self._one_count

    def _state_keys(self, group):
        return ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq') if group['amsgrad'] else ('exp_avg', 'exp_avg_sq')

    def _run_key(self, group, count):
        return count                    # the bias corrections

    def _launch(self, group, sl, step):
        a = self._arena
        if self._plain(group):
            ops.adam_step_(a.flat_param[sl], a.flat_grad[sl], self._buf('exp_avg')[sl], self._buf('exp_avg_sq')[sl],
                           group['lr'], group['betas'][0], group['betas'][1], group['eps'], group['weight_decay'], step)
        else:
            vmax = self._buf('max_exp_avg_sq')[sl] if group['amsgrad'] else None
            ops.adamw_step_(a.flat_param[sl], a.flat_grad[sl], self._buf('exp_avg')[sl], self._buf('exp_avg_sq')[sl],
                            vmax, group['lr'], group['betas'][0], group['betas'][1], group['eps'],
                            group['weight_decay'], group['decoupled_weight_decay'], group['maximize'], step)


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay (p *= 1 - lr*wd before the moment update)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)


class SGD(_ArenaOptimizer):
    """torch.optim.SGD (momentum, dampening, nesterov, weight decay, maximize)."""
    _has_step = False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        _refuse('SGD', foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize, foreach=foreach,
                                      differentiable=differentiable, fused=fused))

    def _state_keys(self, group):
        return ('momentum_buffer',) if group['momentum'] != 0 else ()

    def _run_key(self, group, count):
        return group['momentum'] != 0 and count == 1         # the first update sets the buffer to the gradient

    def _launch(self, group, sl, first):
        a = self._arena
        buf = self._buf('momentum_buffer')[sl] if group['momentum'] != 0 else None
        ops.sgd_step_(a.flat_param[sl], a.flat_grad[sl], buf, group['lr'], group['momentum'], group['dampening'],
                      group['weight_decay'], group['nesterov'], group['maximize'], first)


class RMSprop(_ArenaOptimizer):
    """torch.optim.RMSprop (centered, momentum, weight decay, maximize).  Its state starts at zero and the step count
    enters no formula, so runs are never cut; the count is kept for the state dict."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False,
                 capturable=False, foreach=None, maximize=False, differentiable=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= momentum:
            raise ValueError("Invalid momentum value: %r" % (momentum,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if not 0.0 <= alpha:
            raise ValueError("Invalid alpha value: %r" % (alpha,))
        _refuse('RMSprop', capturable=capturable, foreach=foreach, differentiable=differentiable)
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered,
                                      weight_decay=weight_decay, capturable=capturable, foreach=foreach,
                                      maximize=maximize, differentiable=differentiable))

    def _state_keys(self, group):
        return (('square_avg',) + (('momentum_buffer',) if group['momentum'] > 0 else ())
                + (('grad_avg',) if group['centered'] else ()))

    def _launch(self, group, sl, _):
        a = self._arena
        ga = self._buf('grad_avg')[sl] if group['centered'] else None
        buf = self._buf('momentum_buffer')[sl] if group['momentum'] > 0 else None
        ops.rmsprop_step_(a.flat_param[sl], a.flat_grad[sl], self._buf('square_avg')[sl], ga, buf, group['lr'],
                          group['alpha'], group['eps'], group['weight_decay'], group['momentum'], group['maximize'])


_BUILT = {'Adam': Adam, 'AdamW': AdamW, 'SGD': SGD, 'RMSprop': RMSprop}


def resolve(name):
    """`optimizer.name` from the config -> class (train.py:88: torch.optim.<name>)."""
    if name in _BUILT:
        return _BUILT[name]
    raise NotImplementedError("optimizer %r: the fused arena kernels cover %s" % (name, ', '.join(sorted(_BUILT))))
