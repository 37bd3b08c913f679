"""The packed-weight cache (csrc/pack.hip, hip_runtime.pack_stamp) through every module that stamps a call.

The cache is the one place where a correct kernel, given correct inputs, can silently compute with OTHER weights: when
the key {token, source pointer, mode, shape, extra} and the version stamp of a slot match, the pack kernel is skipped and
the GEMM reads whatever the slot holds.  One coherence scenario (`_scenario`) is run over every stamping module: after
each event that changes the weights (or should not), forward output and all gradients are compared with an fp64 CPU
reference that shares no code with the library and is recomputed from the module's CURRENT parameters; the whole
scenario is then repeated with the cache off and must give the same bits.

Bounds.  Values against fp64: the project's `1e-4 * max(1, |ref|_max)` per tensor (tests/test_gpu_dcn.py TOL).  For
calibration: the fp32 oracle sits below 5e-7 of that scale on these shapes; computing every deformable group with group
0's weights (the stale image this file was written for) moves the output by 0.4 to 0.5 of it.  Cache on against cache
off: equal bits, except grad_input of the deformable layers (1e-5 of its maximum: the order of col2im's straggler
atomics, as in test_dcn_layer_is_reproducible_at_full_size).  Fill counts: a repeated call with unchanged weights adds no
fill and no arena byte; a call after a weight change adds at least one fill per token whose images are cached.
"""
import copy
import gc

import pytest
import torch
import torch.nn.functional as F

from oracle import dcn as od

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4


def _close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert err <= TOL * scale, '%s: error %.3e at scale %.3e (%.3e of it)' % (what, err, scale, err / scale)


def _names(log):
    from test_zz_kernel_coverage import short
    return sorted(short(n) for n in log.names)


# ---------------------------------------------------------------------------------------------------------------------
# The rows: how to build the module, its inputs at two sizes, how to call it, and the fp64 restatement of what it computes
# ---------------------------------------------------------------------------------------------------------------------
class Row:
    cached_tokens = 1          # tokens of the module whose packed images live in the cache
    loose_grad_input = False   # grad of input 0 carries col2im's atomics (deformable layers)
    sizes = ()                 # [(B, H, W)] x 2

    def make(self):
        raise NotImplementedError

    def inputs(self, g, size):
        raise NotImplementedError

    def run(self, m, xs):
        return m(*xs)

    def ref(self, P, xs):
        raise NotImplementedError

    def tokens(self, m):
        return [int(m._pack_token)]

    def context(self):
        import contextlib
        return contextlib.nullcontext()

    def check_kernels(self, names):
        pass


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


class DCNv2Row(Row):
    loose_grad_input = True

    def __init__(self, case):
        from test_gpu_dcn import CASES
        c = CASES[case]
        self.C, self.Co, self.dg = c['C'], c['Co'], c.get('dg', 1)
        self.off_scale = c.get('off_scale', 2.0)
        B, H, W = c['B'], c['H'], c['W']
        self.sizes = [(B, H, W), (B, H // 2 + 3, W // 2 + 2)]
        self.window = case in ('dla_64', 'dg2_64ch')
        # deformable_groups > 1: the per-group inner calls are not cached (csrc/dcn.hip: every group's weights pass
        # through one workspace buffer, so one key would name dg different images)
        self.cached_tokens = 1 if self.dg == 1 else 0

    def make(self):
        from libs.DCNv2.dcn_v2 import DCNv2
        m = DCNv2(self.C, self.Co, 3, 1, 1, deformable_groups=self.dg).to(DEV)
        with torch.no_grad():
            m.bias.normal_(0, 0.5)
        return m

    def inputs(self, g, size):
        B, H, W = size
        return [_rand(g, B, self.C, H, W), _rand(g, B, 18 * self.dg, H, W) * self.off_scale,
                torch.sigmoid(_rand(g, B, 9 * self.dg, H, W))], (B, self.Co, H, W)

    def ref(self, P, xs):
        return od.dcn_v2_conv(xs[0], xs[1], xs[2], P['weight'], P['bias'], 1, 1, 1, self.dg)

    def check_kernels(self, names):
        joined = ' '.join(names)
        assert 'dcn_naive' not in joined, names
        assert ('dcnw_fwd_kernel' in joined) == self.window, names          # window / halo pack or the plain pack
        assert ('copy_channels_kernel' in joined) == (self.dg > 1), names   # the composed per-group path
        if not self.window:
            assert 'pack_kernel' in names, names


class DCNRow(Row):
    loose_grad_input = True

    def __init__(self, dg):
        self.dg = dg
        self.C, self.Co = (32, 32) if dg == 1 else (32, 16)
        self.sizes = [(2, 24, 24), (2, 16, 20)] if dg == 1 else [(2, 10, 12), (2, 7, 9)]
        # dg = 1: the offset convolution's token and the layer's own; dg = 2: the offset convolution's only (see DCNv2Row)
        self.cached_tokens = 2 if dg == 1 else 1

    def make(self):
        from libs.DCNv2.dcn_v2 import DCN
        m = DCN(self.C, self.Co, (3, 3), 1, 1, deformable_groups=self.dg).to(DEV)
        with torch.no_grad():
            m.conv_offset_mask.weight.normal_(0, 0.5 / (9 * self.C) ** 0.5)
            m.conv_offset_mask.bias.normal_(0, 0.3)
            m.bias.normal_(0, 0.5)
        return m

    def inputs(self, g, size):
        B, H, W = size
        return [_rand(g, B, self.C, H, W)], (B, self.Co, H, W)

    def ref(self, P, xs):
        om = F.conv2d(xs[0], P['conv_offset_mask.weight'], P['conv_offset_mask.bias'], 1, 1)
        o1, o2, mask = torch.chunk(om, 3, dim=1)
        return od.dcn_v2_conv(xs[0], torch.cat((o1, o2), dim=1), torch.sigmoid(mask), P['weight'], P['bias'], 1, 1, 1,
                              self.dg)

    def tokens(self, m):
        return [int(m._pack_token), int(m.conv_offset_mask._pack_token)]

    def check_kernels(self, names):
        joined = ' '.join(names)
        assert 'dcn_naive' not in joined, names
        assert ('split_offset_mask' in joined) == (self.dg > 1), names      # dg = 1: offsets / mask read out of `om`
        if self.dg > 1:
            assert 'copy_channels_kernel' in joined, names                  # the composed per-group path


class ConvRow(Row):
    def __init__(self, kind):
        self.kind = kind
        if kind == 'stride2':      # input gradient by parity classes: several tap-subset images under one token
            self.C, self.Co, self.stride = 32, 32, 2
            self.sizes = [(2, 12, 16), (2, 8, 20)]
        else:                      # halo tiles: forward and input-gradient images of one weight, two pack modes
            self.C, self.Co, self.stride = 32, 48, 1
            self.sizes = [(2, 8, 16), (2, 8, 32)]

    def make(self):
        from hip_runtime import nn as hnn
        return hnn.Conv2d(self.C, self.Co, 3, stride=self.stride, padding=1, bias=True).to(DEV)

    def inputs(self, g, size):
        B, H, W = size
        Ho, Wo = (H + 2 - 3) // self.stride + 1, (W + 2 - 3) // self.stride + 1
        return [_rand(g, B, self.C, H, W)], (B, self.Co, Ho, Wo)

    def ref(self, P, xs):
        return F.conv2d(xs[0], P['weight'], P['bias'], self.stride, 1)

    def context(self):
        import contextlib
        import hip_runtime as hr
        if self.kind == 'stride2':
            return contextlib.nullcontext()
        stack = contextlib.ExitStack()
        stack.enter_context(hr.halo_conv(1, 1))      # every eligible layer, whatever its size; no split-K before it
        stack.enter_context(hr.splitk(0))
        return stack

    def check_kernels(self, names):
        joined = ' '.join(names)
        if self.kind == 'stride2':
            assert 'pack_taps_kernel' in names, names
            assert 'classes_kernel' in joined or 'ConvDgradClass' in joined, names
        else:
            assert 'HconvFwd' in joined and 'HconvDgrad' in joined, names


class ConvTransposeRow(Row):
    """the control: owns no token, so nothing of it may ever be cached"""
    cached_tokens = 0
    sizes = [(2, 6, 7), (2, 5, 8)]

    def make(self):
        from hip_runtime import nn as hnn
        return hnn.ConvTranspose2d(32, 16, 4, stride=2, padding=1).to(DEV)

    def inputs(self, g, size):
        B, H, W = size
        return [_rand(g, B, 32, H, W)], (B, 16, 2 * H, 2 * W)

    def ref(self, P, xs):
        return F.conv_transpose2d(xs[0], P['weight'], None, 2, 1)

    def tokens(self, m):
        assert not hasattr(m, '_pack_token')
        return []


class HeadRow(Row):
    """two tokens in one autograd node; its backward stamps only the first"""
    cached_tokens = 2
    sizes = [(2, 8, 10), (2, 6, 12)]

    def make(self):
        from hip_runtime import nn as hnn
        return hnn.Head(hnn.Conv2d(32, 48, 3, padding=1, act_slope=0.0), hnn.Slot(), hnn.Conv2d(48, 4, 1)).to(DEV)

    def inputs(self, g, size):
        B, H, W = size
        return [_rand(g, B, 32, H, W)], (B, 4, H, W)

    def run(self, m, xs):
        y = m(*xs)
        assert type(y.grad_fn).__name__.startswith('_ConvActConv1x1'), type(y.grad_fn).__name__
        return y

    def ref(self, P, xs):
        return F.conv2d(F.relu(F.conv2d(xs[0], P['0.weight'], P['0.bias'], 1, 1)), P['2.weight'], P['2.bias'])

    def tokens(self, m):
        return [int(m[0]._pack_token), int(m[2]._pack_token)]


class CatRow(Row):
    """ops.conv1x1_cat with the token of the hnn.Conv2d that owns the weight (backends.dla.Root)"""
    sizes = [(4, 32, 32), (4, 32, 16)]

    def make(self):
        from hip_runtime import nn as hnn
        return hnn.Conv2d(128, 64, 1, bias=False).to(DEV)

    def inputs(self, g, size):
        B, H, W = size
        return [_rand(g, B, 64, H, W), _rand(g, B, 64, H, W)], (B, 64, H, W)

    def run(self, m, xs):
        from hip_runtime import ops
        y = ops.conv1x1_cat(xs, m.weight, m._pack_token)
        assert y is not None, 'cnuda_conv2d_cat_supported refused the sources'
        return y

    def ref(self, P, xs):
        return F.conv2d(torch.cat(xs, 1), P['weight'])

    def check_kernels(self, names):
        joined = ' '.join(names)
        for frag in ('ConvFwdCatLoader', 'ConvDgradCatLoader', 'ConvWCatLoader'):
            assert frag in joined, (frag, names)


ROWS = {
    'dcnv2_dg1_dla_64': lambda: DCNv2Row('dla_64'),
    'dcnv2_dg2': lambda: DCNv2Row('dg2'),
    'dcnv2_dg2_64ch': lambda: DCNv2Row('dg2_64ch'),
    'dcnv2_dg4_odd': lambda: DCNv2Row('dg4_odd'),
    'dcn_dg1': lambda: DCNRow(1),
    'dcn_dg2': lambda: DCNRow(2),
    'conv_stride2_parity_classes': lambda: ConvRow('stride2'),
    'conv_halo_tiles': lambda: ConvRow('halo'),
    'conv_transpose_no_token': ConvTransposeRow,
    'head_two_tokens': HeadRow,
    'conv1x1_cat': CatRow,
}


# ---------------------------------------------------------------------------------------------------------------------
# The scenario
# ---------------------------------------------------------------------------------------------------------------------
def _reference(row, m, xs, go):
    P = {n: p.detach().cpu().double().requires_grad_(True) for n, p in m.named_parameters()}
    xr = [t.double().requires_grad_(True) for t in xs]
    y = row.ref(P, xr)
    y.backward(go.double())
    return y.detach(), [t.grad for t in xr], {n: p.grad for n, p in P.items()}


def _measure(row, m, xs, go):
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()          # (in place: a gradient that is a view of the optimizer's arena stays one)
    xd = [t.to(DEV).requires_grad_(True) for t in xs]
    y = row.run(m, xd)
    y.backward(go.to(DEV))
    torch.cuda.synchronize()
    return y.detach().clone(), [t.grad.clone() for t in xd], {n: p.grad.clone() for n, p in m.named_parameters()}


def _scenario(row, cache_on):
    """-> [(label, y, grad_inputs, param_grads)] of every call, each already held against the fp64 reference"""
    import hip_runtime as hr
    from hip_runtime import optim
    L = hr.lib()
    trace = []
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(99)
    m = row.make()
    data = []
    for size in row.sizes:
        xs, oshape = row.inputs(g, size)
        data.append((xs, _rand(g, *oshape)))
    stamped = cache_on and row.cached_tokens > 0

    def counters():
        return L.cnuda_pack_cache_used(), L.cnuda_pack_cache_fills()

    def check(label, mod=None, size=0, log=None):
        mod = m if mod is None else mod
        xs, go = data[size]
        got = _measure(row, mod, xs, go)
        want = _reference(row, mod, xs, go)
        _close(got[0], want[0], '%s: output' % label)
        for i, (a, r) in enumerate(zip(got[1], want[1])):
            _close(a, r, '%s: grad of input %d' % (label, i))
        assert set(got[2]) == set(want[2])
        for n in sorted(want[2]):
            _close(got[2][n], want[2][n], '%s: grad of %s' % (label, n))
        trace.append((label,) + got)

    def changed(label, before):
        """a call after a weight change: at least one fill per cached token; nothing at all without a token"""
        used, fills = counters()
        if stamped:
            assert fills - before[1] >= row.cached_tokens, (label, fills - before[1], row.cached_tokens)
        else:
            assert (used, fills) == before, (label, before, (used, fills))

    def weights(mod):
        return [p for p in mod.parameters() if p.dim() == 4]

    start = counters()
    with row.context():
        # 1. cold slot
        with hr.launch_log() as log:
            check('1 first call')
        row.check_kernels(_names(log))
        c1 = counters()
        if stamped:
            assert c1[0] > start[0] or c1[1] > start[1], (start, c1)
        else:
            assert c1 == start, (start, c1)
        # 2. the same call again: served from the cache
        check('2 same call again')
        assert counters() == c1, (c1, counters())
        # 3. torch's version counter
        with torch.no_grad():
            for w in weights(m):
                w.mul_(-0.5)
        c = counters()
        check('3 weight.mul_')
        changed('3 weight.mul_', c)
        # 4. the fused Adam: parameter epoch, cnuda_pack_refresh; the parameters move into the optimizer's arena and their
        #    gradients land in its sink from here on
        opt = optim.Adam(m.parameters(), lr=0.02)
        before = [p.detach().clone() for p in m.parameters()]
        opt.step()
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
        c = counters()
        check('4 fused Adam step')
        changed('4 fused Adam step', c)
        from hip_runtime.arena import _BY_PTR
        assert all(p.data_ptr() in _BY_PTR for p in m.parameters())      # (the gradients above went through the sink)
        check('4b second call after the step')
        before = [p.detach().clone() for p in m.parameters()]
        opt.step()                                              # arena in place: the refresh launch rebuilds the images
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
        check('4c second fused Adam step')
        # 5. a stock optimizer
        torch.optim.SGD(m.parameters(), lr=1e-3).step()
        c = counters()
        check('5 SGD step')
        changed('5 SGD step', c)
        # 6. load_state_dict of a perturbed copy
        m.load_state_dict({k: v.detach().clone() * 0.8 + 0.01 for k, v in m.state_dict().items()})
        c = counters()
        check('6 load_state_dict')
        changed('6 load_state_dict', c)
        # 7. another input size through the same module, and back
        check('7 second size', size=1)
        check('7 second size again', size=1)
        check('7 first size again')
        c = counters()
        check('7 first size once more')
        assert counters() == c, (c, counters())
        # 8. a deep copy with other weights, in turn with the original
        twin = copy.deepcopy(m)
        assert set(row.tokens(twin)).isdisjoint(row.tokens(m)), (row.tokens(twin), row.tokens(m))
        with torch.no_grad():
            for p in twin.parameters():
                p.mul_(0.7).add_(0.02)
        for turn in range(2):
            check('8 original, turn %d' % turn)
            check('8 copy, turn %d' % turn, mod=twin)
        c = counters()
        check('8 original, steady')
        check('8 copy, steady', mod=twin)
        assert counters() == c, (c, counters())
    if not stamped:
        assert counters() == start, (start, counters())        # unstamped calls never cache
    return trace


def _both(row):
    import hip_runtime as hr
    assert not hr._PACK['off'], 'the suite runs with the pack cache on (CNUDA_PACK_CACHE_MB)'
    on = _scenario(row, True)
    was = hr._PACK['off']
    hr._PACK['off'] = True
    try:
        off = _scenario(row, False)
    finally:
        hr._PACK['off'] = was
    assert [t[0] for t in on] == [t[0] for t in off]
    for (label, y1, gi1, gp1), (_, y0, gi0, gp0) in zip(on, off):
        assert torch.equal(y1, y0), '%s: output differs from the run without the cache' % label
        for i, (a, b) in enumerate(zip(gi1, gi0)):
            if i == 0 and row.loose_grad_input:
                assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), (label, i)
            else:
                assert torch.equal(a, b), '%s: grad of input %d differs from the run without the cache' % (label, i)
        for n in gp1:
            assert torch.equal(gp1[n], gp0[n]), '%s: grad of %s differs from the run without the cache' % (label, n)


@pytest.mark.parametrize('name', sorted(ROWS))
def test_pack_cache_coherence(name):
    """Events 1 to 8 of the module docstring's scenario for one stamping module (or the token-free control), cache on and
    cache off.  deformable_groups > 1 is served by per-group calls that do not cache (csrc/dcn.hip): for `DCNv2` with
    dg > 1 the counters must not move at all, for `DCN` with dg = 2 only the offset convolution's token fills."""
    _both(ROWS[name]())


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm-folded inference: explicit versions (_fold_token / _fold_gen, backends/dla.py)
# ---------------------------------------------------------------------------------------------------------------------
def _bn_eval(y, bn):
    s = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
    return (y - bn.running_mean.detach().cpu().double().view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + \
        bn.bias.detach().cpu().double().view(1, -1, 1, 1)


def _ref_conv_bn_relu(m, x):
    d = lambda t: t.detach().cpu().double()
    return F.relu(_bn_eval(F.conv2d(x.double(), d(m[0].weight), None, m[0].stride, m[0].padding), m[1]))


def _ref_deform_conv(m, x):
    d = lambda t: t.detach().cpu().double()
    c, x = m.conv, x.double()
    om = F.conv2d(x, d(c.conv_offset_mask.weight), d(c.conv_offset_mask.bias), 1, 1)
    o1, o2, mask = torch.chunk(om, 3, dim=1)
    y = od.dcn_v2_forward(x, d(c.weight), d(c.bias), torch.cat((o1, o2), dim=1), torch.sigmoid(mask), 3, 3, 1, 1, 1, 1, 1,
                          1, 1)
    return F.relu(_bn_eval(y, m.actf[0]))


def _make_conv_bn_relu():
    from backends import dla
    return dla.ConvBnRelu(32, 48, 3).to(DEV), (lambda m: m[1]), _ref_conv_bn_relu, [(2, 32, 12, 16), (2, 32, 9, 20)]


def _make_deform_conv():
    from backends import dla
    m = dla.DeformConv(32, 32).to(DEV)
    with torch.no_grad():
        m.conv.conv_offset_mask.weight.normal_(0, 0.5 / (9 * 32) ** 0.5)
        m.conv.conv_offset_mask.bias.normal_(0, 0.3)
        m.conv.bias.normal_(0, 0.5)
    return m, (lambda m: m.actf[0]), _ref_deform_conv, [(2, 32, 16, 16), (2, 32, 12, 20)]


def _folded_scenario(make):
    import hip_runtime as hr
    from backends import dla
    L = hr.lib()
    torch.manual_seed(77)
    g = torch.Generator().manual_seed(78)
    m, bn_of, ref, shapes = make()
    with torch.no_grad():
        bn = bn_of(m)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    xs = [_rand(g, *s) for s in shapes]
    trace = []

    def counters():
        return L.cnuda_pack_cache_used(), L.cnuda_pack_cache_fills()

    def check(label, mod=None, size=0):
        mod = m if mod is None else mod
        mod.eval()
        with torch.no_grad(), dla.folded_inference():
            assert dla._use_folded(mod), label
            y = mod(xs[size].to(DEV))
        torch.cuda.synchronize()
        _close(y, ref(mod, xs[size]), label)
        trace.append((label, y.clone()))

    def first_weight(mod):
        return next(p for p in mod.parameters() if p.dim() == 4 and p.shape[0] != 27)

    m.eval()
    m.fold_batchnorm_()
    check('1 first call')
    c = counters()
    check('2 same call again')
    assert counters() == c, (c, counters())
    for turn in range(3):                   # re-folds drop the old folded tensors: fresh ones may land on their addresses
        with torch.no_grad():
            first_weight(m).mul_(-0.5 if turn == 0 else 1.3)
        m.fold_batchnorm_()
        c = counters()
        check('3 re-folded after a weight change, turn %d' % turn)
        if not hr._PACK['off']:
            assert counters()[1] > c[1], (c, counters())
    m.train()
    m(xs[0].to(DEV) * 2.0 + 0.5)            # a train-mode BatchNorm forward: the running statistics move
    m.eval()
    m.fold_batchnorm_()
    check('4 re-folded after a train-mode forward')
    check('5 second size', size=1)
    check('5 first size again')
    twin = copy.deepcopy(m)
    assert int(twin._fold_token) != int(m._fold_token)
    with torch.no_grad():
        first_weight(twin).mul_(0.7).add_(0.02)
    twin.fold_batchnorm_()
    for turn in range(2):
        check('6 original, turn %d' % turn)
        check('6 copy, turn %d' % turn, mod=twin)
    c = counters()
    check('6 original, steady')
    check('6 copy, steady', mod=twin)
    assert counters() == c, (c, counters())
    return trace


@pytest.mark.parametrize('kind', ['conv_bn_relu', 'deform_conv'])
def test_pack_cache_coherence_of_folded_inference(kind):
    """A folded conv block and a folded `DeformConv` in eval(): the packed images of the folded weights are stamped with
    (`_fold_token`, `_fold_gen`), not with a tensor's version -- values against fp64 after every re-fold (weight change,
    train-mode BatchNorm forward), at a second size, and for a deep copy run in turn with the original; the same bits with
    the cache off."""
    import hip_runtime as hr
    make = {'conv_bn_relu': _make_conv_bn_relu, 'deform_conv': _make_deform_conv}[kind]
    assert not hr._PACK['off']
    on = _folded_scenario(make)
    hr._PACK['off'] = True
    try:
        off = _folded_scenario(make)
    finally:
        hr._PACK['off'] = False
    assert [t[0] for t in on] == [t[0] for t in off]
    for (label, a), (_, b) in zip(on, off):
        assert torch.equal(a, b), label


# ---------------------------------------------------------------------------------------------------------------------
# A replaced Parameter at a recycled address with an equal version counter
# ---------------------------------------------------------------------------------------------------------------------
def _fresh_weight_at(shape, values, raw):
    """a NEW tensor object over `raw`'s storage holding `values`, written through another alias (so the new tensor's own
    version counter does not count the write)"""
    raw.copy_(values.reshape(-1))
    return torch.nn.Parameter(torch.empty(0, device=DEV).set_(raw.untyped_storage(), 0, tuple(shape)))


@pytest.mark.parametrize('kind', ['conv2d', 'dcnv2'])
def test_a_replaced_parameter_at_a_recycled_address_is_not_taken_for_the_old_one(kind):
    """`module.weight = nn.Parameter(fresh)` twice, the first replacement dropped before the second is made: same token,
    same source pointer, same torch version counter, no parameter epoch in between -- the one thing that still tells the
    two weights apart is that they are different tensor objects (hip_runtime.pack_stamp folds a per-object serial number
    into the version; without it the third weight's output was off by 1.3 to 1.6 of its scale on an MI355X).  The aliasing
    is established, not hoped for.  Both routes run: the natural one (drop the second weight, allocate the third: the
    caching allocator may hand the block back) did NOT give the same address on the MI355X for either module, so the
    constructed one is what the test rests on -- both weights are new tensor objects over one raw buffer that is kept
    alive, written through another alias, and the equality of address and version counter is asserted."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn
    g = torch.Generator().manual_seed(31)
    if kind == 'conv2d':
        m = hnn.Conv2d(32, 48, 3, padding=1, bias=True).to(DEV)
        xs = [_rand(g, 2, 32, 9, 11)]
        ref = lambda: F.conv2d(xs[0].double(), m.weight.detach().cpu().double(), m.bias.detach().cpu().double(), 1, 1)
    else:
        from libs.DCNv2.dcn_v2 import DCNv2
        m = DCNv2(64, 64, 3, 1, 1).to(DEV)
        xs = [_rand(g, 1, 64, 16, 16), _rand(g, 1, 18, 16, 16) * 2.0, torch.sigmoid(_rand(g, 1, 9, 16, 16))]
        ref = lambda: od.dcn_v2_forward(xs[0].double(), m.weight.detach().cpu().double(), m.bias.detach().cpu().double(),
                                        xs[1].double(), xs[2].double(), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    shape = tuple(m.weight.shape)
    dx = [t.to(DEV) for t in xs]

    def run(label):
        with torch.no_grad():
            y = m(*dx)
        torch.cuda.synchronize()
        _close(y, ref(), label)

    run('original weight')
    used = hr.lib().cnuda_pack_cache_used()
    aliased = []
    # natural route: the second weight is dropped, the third is allocated into the block it left
    m.weight = torch.nn.Parameter(_rand(g, *shape).to(DEV) * 0.1)
    run('natural route: second weight')
    where, version = m.weight.data_ptr(), m.weight._version
    m.weight = None
    gc.collect()
    third = _rand(g, *shape) * 0.1
    m.weight = torch.nn.Parameter(third.to(DEV))
    if (m.weight.data_ptr(), m.weight._version) == (where, version):
        aliased.append('natural')
    run('natural route: third weight')
    # constructed route: one raw buffer, each weight a new tensor object over it
    raw = torch.empty(m.weight.numel(), device=DEV)
    m.weight = _fresh_weight_at(shape, _rand(g, *shape).to(DEV) * 0.1, raw)
    run('constructed route: second weight')
    where, version = m.weight.data_ptr(), m.weight._version
    m.weight = None
    gc.collect()
    m.weight = _fresh_weight_at(shape, _rand(g, *shape).to(DEV) * 0.1, raw)
    assert (m.weight.data_ptr(), m.weight._version) == (where, version)     # the aliasing this test is about
    aliased.append('constructed')
    run('constructed route: third weight')
    print('aliasing routes:', aliased)
    # the arena did not grow with the replacements (test_pack_cache_slot_follows_a_module_to_a_new_weight_buffer)
    assert hr.lib().cnuda_pack_cache_used() == used
