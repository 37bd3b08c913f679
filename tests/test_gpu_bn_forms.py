"""MI355X: every run-time form of the BatchNorm kernels (csrc/bn.hip) against tests/bn_oracle.py, an fp64 restatement
that tests/test_host_bn_forms.py holds against torch.double.

One kernel body serves several forms, chosen by pick_split / plane_splits from the shape alone: one workgroup per
plane, a plane cut into chunks, several images per workgroup, the apply grid cut over gridDim.y, a 16-byte and a scalar
path, one or several statistics groups, statistics reduced from x or folded from a GEMM epilogue's block sums.  The
kernel names in the launch log cannot tell these apart, so every case asserts its form through cnuda_bn_plan (the
entry points' own planning code) and its values through the oracle.

Tolerances: y and every gradient within 1e-4 of the reference's largest magnitude (`_close`, as in
tests/test_gpu_spatial_forms.py); saved mean / invstd and the running statistics within 1e-6 of the largest magnitude
(tests/test_gpu_ops.py's bound for the running statistics).  Every output buffer starts full of NaN: an element that no
workgroup writes fails.  gamma, beta and the images are random and distinct: a plane, image or group mix-up changes the
numbers.

The gate (bn_oracle.gate_with_band): a float32 kernel may put an element on the other side of a ReLU / ReLU6 edge when
the reference's z lies within the forward tolerance of it, and one flip moves gbeta by a whole gy.  Inside a band of
1e-4 * max|z_ref| around an edge the kernel's own gate (read from its y) is used, outside it the reference's.  Two
assertions keep that from hiding a failure: at most 1e-3 of the elements lie in the band, and every edge in play closes
at least 2 % of them.  Both depend on the reference alone, so the seeds below were checked on the CPU."""
import functools
import zlib

import pytest
import torch

import bn_oracle as bo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS, MOMENTUM = 1e-5, 0.1
NAN = float('nan')


def _close(got, want, what=''):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print('%s: max abs err %.3e, reference max %.3e' % (what, err, scale))
    assert err <= 1e-4 * scale, (what, err, scale)


def _stat_close(got, want, what=''):
    got, want = got.detach().double().cpu().reshape(want.shape), want.detach().double().cpu()
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print('%s: max abs err %.3e, reference max %.3e' % (what, err, scale))
    assert err <= 1e-6 * scale, (what, err, scale)


def _names(log):
    from test_zz_kernel_coverage import short
    counts = {}
    for k, v in log.counts.items():
        counts[short(k)] = counts.get(short(k), 0) + v
    print(sorted(counts.items()))
    return counts


TRAIN_KERNELS = {'bn_reduce_kernel<0>': 1, 'bn_apply_kernel': 1, 'bn_reduce_kernel<1>': 1, 'bn_bwd_apply_kernel': 1}


# ---------------------------------------------------------------------------------------------------------------
# inputs, reference, the two ways in, the checks -- shared with tests/test_gpu_fuzz.py
# ---------------------------------------------------------------------------------------------------------------
# (shape + groups, act, res) -> added to the case's seed: the draws whose reference alone misses one of the two gate
# conditions (on a plane of a few hundred values one element in the band is already more than 1e-3; a single channel
# whose beta comes out near 2 closes less than 2 %)
RESEED = {}


def case_seed(shape, groups, act, res):
    key = (tuple(shape) + (groups,), act, bool(res))
    return zlib.crc32(repr(key).encode()) % 1000003 + RESEED.get(key, 0)


@functools.lru_cache(maxsize=None)
def make_case(shape, groups, act, res, seed=None):
    """-> dict: float32 CPU inputs (x, gamma, beta, residual or None, gy, the running statistics before the call) and
    the fp64 forward reference.  Nothing writes into it.
    ReLU6 takes gamma = 3 * (1 + 0.2 randn), beta = 2 so that the upper edge closes its 2 % -- with a residual too: at
    gamma near 1 and beta near 0.5 the sum with 2 * randn reaches 6 in about 1 % of the elements only."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(case_seed(shape, groups, act, res) if seed is None else seed)
    c = {'shape': shape, 'groups': groups, 'act': act}
    c['x'] = 2 * torch.randn(shape, generator=g) + 0.5
    c['gamma'] = 1 + 0.2 * torch.randn(C, generator=g)
    c['beta'] = 0.5 + 0.5 * torch.randn(C, generator=g)
    if act == 2:
        c['gamma'], c['beta'] = 3 * c['gamma'], torch.full((C,), 2.0)
    c['residual'] = 2 * torch.randn(shape, generator=g) if res else None
    c['gy'] = torch.randn(shape, generator=g)
    c['rm0'], c['rv0'] = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    return add_reference(c)


def add_reference(c):
    c['ref'] = bo.train_forward(c['x'], c['gamma'], c['beta'], c['residual'], c['act'], c['groups'], EPS, MOMENTUM,
                                c['rm0'], c['rv0'])
    return c


def gate_conditions(c, channels=None):
    """the two conditions of the gate rule, from the reference alone -> (band share, closed below, closed above)"""
    z = c['ref'][0] if channels is None else c['ref'][0][:, channels]
    if c['act'] == 0:
        return 0.0, None, None
    share = bo.gate_with_band(z, z, c['act'])[1]
    return share, (z <= 0).double().mean().item(), (z >= 6).double().mean().item() if c['act'] == 2 else None


def run_entry_points(c, backward=True):
    """cnuda_bn_train_forward with running statistics and the batch counter, then cnuda_bn_backward the way
    hip_runtime.ops calls it: `beta` given and y NULL without a residual (the gate is recomputed from x), y given and
    grad_residual with one.  -> dict of device results and the launch counts"""
    import hip_runtime as hr
    L = hr.lib()
    B, C, H, W = c['shape']
    HW, groups, act = H * W, c['groups'], c['act']
    x, gamma, beta, gy = (c[k].to(DEV) for k in ('x', 'gamma', 'beta', 'gy'))
    r = None if c['residual'] is None else c['residual'].to(DEV)
    out = {k: torch.full(c['shape'], NAN, device=DEV) for k in ('y', 'gx')}
    out.update({k: torch.full((groups * C,), NAN, device=DEV) for k in ('mean', 'invstd')})
    out.update({k: torch.full((C,), NAN, device=DEV) for k in ('ggamma', 'gbeta')})
    out['gres'] = None if r is None else torch.full(c['shape'], NAN, device=DEV)
    out['rm'], out['rv'] = c['rm0'].to(DEV), c['rv0'].to(DEV)
    out['nbt'] = torch.zeros((), dtype=torch.int64, device=DEV)
    ws = hr.workspace(L.cnuda_bn_workspace_bytes(B, C, HW), x.device)
    torch.cuda.synchronize()
    with hr.launch_log() as log:
        hr.check(L.cnuda_bn_train_forward(hr.ptr(x), hr.ptr(gamma), hr.ptr(beta), hr.ptr(r), hr.ptr(out['y']),
                                          hr.ptr(out['mean']), hr.ptr(out['invstd']), hr.ptr(out['rm']), hr.ptr(out['rv']),
                                          hr.ptr(out['nbt']), MOMENTUM, EPS, act, B, C, HW, groups, hr.ptr(ws), ws.numel(),
                                          hr.stream()), 'bn_train_forward')
        if backward:
            hr.check(L.cnuda_bn_backward(hr.ptr(gy), hr.ptr(x), None if r is None else hr.ptr(out['y']), hr.ptr(gamma),
                                         hr.ptr(beta) if r is None else None, hr.ptr(out['mean']), hr.ptr(out['invstd']),
                                         hr.ptr(out['gx']), hr.ptr(out['gres']), hr.ptr(out['ggamma']), hr.ptr(out['gbeta']),
                                         act, B, C, HW, groups, hr.ptr(ws), ws.numel(), hr.stream()), 'bn_backward')
        torch.cuda.synchronize()
    out['launched'] = _names(log)
    return out


def run_autograd(c):
    """the same call through hip_runtime.ops.batch_norm_act under hip_runtime.domain_groups"""
    import hip_runtime as hr
    from hip_runtime import ops
    x, gamma, beta = (c[k].to(DEV).requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    r = None if c['residual'] is None else c['residual'].to(DEV).requires_grad_(True)
    out = {'rm': c['rm0'].to(DEV), 'rv': c['rv0'].to(DEV), 'nbt': torch.zeros((), dtype=torch.int64, device=DEV)}
    torch.cuda.synchronize()
    with hr.launch_log() as log, hr.domain_groups(c['groups']):
        y = ops.batch_norm_act(x, gamma, beta, out['rm'], out['rv'], True, MOMENTUM, EPS, r, {0: False, 1: True, 2: 6}[c['act']],
                               num_batches_tracked=out['nbt'])
        y.backward(c['gy'].to(DEV))
        torch.cuda.synchronize()
    out.update(y=y.detach(), gx=x.grad, ggamma=gamma.grad, gbeta=beta.grad, gres=None if r is None else r.grad,
               launched=_names(log))
    return out


def check_case(c, got, channels=None, backward=True):
    """channels: compare y and the gradients on these channels only (the statistics are always compared on all)"""
    z, y, mean, invstd, rm, rv = c['ref']
    groups, act = c['groups'], c['act']
    sel = (lambda t: t) if channels is None else (lambda t: t[:, channels])
    vec = (lambda t: t) if channels is None else (lambda t: t[channels])
    _close(sel(got['y']), sel(y), 'y')
    if 'mean' in got:
        _stat_close(got['mean'], mean, 'save_mean')
        _stat_close(got['invstd'], invstd, 'save_invstd')
    _stat_close(got['rm'], rm, 'running_mean')
    _stat_close(got['rv'], rv, 'running_var')
    assert got['nbt'].item() == groups
    if not backward:
        return
    mask, share = bo.gate_with_band(sel(z), sel(got['y']).cpu(), act)
    if act:
        below, above = (sel(z) <= 0).double().mean().item(), (sel(z) >= 6).double().mean().item()
        print('gate: %.2e of the elements in the band, %.3f closed at 0%s' % (share, below, ', %.3f at 6' % above if act == 2 else ''))
        assert share <= 1e-3, share
        assert below >= 0.02 and (act != 2 or above >= 0.02), (below, above)
    full = torch.ones(z.shape, dtype=torch.bool)
    if channels is None:
        full = mask
    else:
        full[:, channels] = mask
    gx, gres, ggamma, gbeta = bo.backward(c['gy'], c['x'], c['gamma'], mean, invstd, full)
    _close(sel(got['gx']), sel(gx), 'grad_x')
    _close(vec(got['ggamma']), vec(ggamma), 'grad_gamma')
    _close(vec(got['gbeta']), vec(gbeta), 'grad_beta')
    if c['residual'] is not None:
        _close(sel(got['gres']), sel(gres), 'grad_residual')


# ---------------------------------------------------------------------------------------------------------------
# a. every row of the table through the C entry points
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'relu', 'relu6'])
@pytest.mark.parametrize('row', bo.FORMS, ids=[bo.form_id(f[0]) for f in bo.FORMS])
def test_train_every_split_form(row, act, res):
    (B, C, H, W, groups), form = row
    assert bo.plan(B, C, H * W, groups) == form
    c = make_case((B, C, H, W), groups, act, res)
    got = run_entry_points(c)
    assert got['launched'] == TRAIN_KERNELS, got['launched']
    check_case(c, got)


# ---------------------------------------------------------------------------------------------------------------
# b. the autograd path (hip_runtime.ops.batch_norm_act under hip_runtime.domain_groups)
# ---------------------------------------------------------------------------------------------------------------
AUTOGRAD_ROWS = [((1, 3, 91, 91, 1), 1, 'a plane cut in three, scalar'), ((4, 1100, 3, 3, 1), 2, 'four images per workgroup'),
                 ((12, 700, 2, 2, 2), 1, 'two groups, two images per workgroup'), ((1, 3, 33, 37, 1), 2, 'apply grid cut, scalar tail')]


@pytest.mark.parametrize('shape,act,what', AUTOGRAD_ROWS, ids=[bo.form_id(r[0]) for r in AUTOGRAD_ROWS])
def test_autograd_path_on_split_forms(shape, act, what):
    B, C, H, W, groups = shape
    assert bo.plan(B, C, H * W, groups) == dict(bo.FORMS)[shape]
    c = make_case((B, C, H, W), groups, act, True)
    got = run_autograd(c)
    assert got['launched'] == TRAIN_KERNELS, got['launched']
    check_case(c, got)


# ---------------------------------------------------------------------------------------------------------------
# c. statistics folded from a GEMM epilogue's block sums (cnuda_bn_train_forward_stats)
# ---------------------------------------------------------------------------------------------------------------
# (C, rows, groups, blocks per group) -> (B, H, W, pixels per block, act, res).  The split count bn.hip derives from
# the blocks per group, spl = min(64, ceil(bpg / 256)), each split ceil(bpg / spl) blocks:
#   1 -> 1;  255 -> 1;  256 -> 1;  257 -> 2 (129 + 128);  600 -> 3 (200 each);  16385 -> 64 (63 x 257 + 194);  4 -> 1
FOLD_CASES = {
    (3, 3, 1, 1): (2, 4, 8, 64, 0, False),            # one block that spans both images
    (5, 32, 1, 255): (3, 17, 20, 4, 1, True),
    (17, 32, 2, 256): (2, 64, 128, 32, 1, False),     # C straddles a 16-channel workgroup; the apply pass cuts its planes
    (16, 64, 1, 257): (1, 4, 257, 4, 2, False),
    (33, 64, 2, 600): (4, 30, 40, 4, 0, True),
    (2, 128, 1, 16385): (1, 145, 113, 1, 1, False),
    (1040, 1040, 1, 4): (4, 2, 2, 4, 2, True),        # one image per block; the apply pass takes four images per workgroup
}
assert {v[3] for v in FOLD_CASES.values()} == {1, 4, 32, 64} and sum(k[1] > k[0] for k in FOLD_CASES) >= 3


@functools.lru_cache(maxsize=None)
def _fold_case(key):
    C, rows, groups, bpg = key
    B, H, W, blk, act, res = FOLD_CASES[key]
    assert B // groups * H * W == bpg * blk
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 1000003)
    c = {'shape': (B, C, H, W), 'groups': groups, 'act': act}
    c['x'] = torch.randn(B, C, H, W, generator=g) + 0.3           # zero-centred, as the header requires of this path
    c['gamma'], c['beta'] = 1 + 0.2 * torch.randn(C, generator=g), 0.5 + 0.5 * torch.randn(C, generator=g)
    c['residual'] = 2 * torch.randn(B, C, H, W, generator=g) if res else None
    c['rm0'], c['rv0'] = 0.1 * torch.randn(C, generator=g), 1 + 0.3 * torch.rand(C, generator=g)
    # blocks of `blk` consecutive pixels of the flattened (image, pixel) axis, image-major: fp64 sums rounded to float32
    xb = c['x'].double().permute(1, 0, 2, 3).reshape(C, groups * bpg, blk)
    stats = torch.full((groups * bpg, rows, 2), NAN, dtype=torch.float32)          # the unused rows stay NaN
    stats[:, :C, 0] = xb.sum(-1).t().float()
    stats[:, :C, 1] = (xb * xb).sum(-1).t().float()
    c['stats'] = stats
    _, mean, var = bo.fold(stats, bpg, groups, bpg * blk)
    c['ref'] = bo.forward_from_moments(c['x'], mean[:, :C], var[:, :C], c['gamma'], c['beta'], c['residual'], act, EPS, MOMENTUM,
                                       c['rm0'], c['rv0'])
    return c


@pytest.mark.parametrize('key', list(FOLD_CASES), ids=['C%d_rows%d_g%d_blocks%d' % k for k in FOLD_CASES])
def test_statistics_folded_from_block_sums(key):
    """The oracle folds the very float32 block sums the kernel gets, so the statistics must agree to 1e-6 and y to 1e-4.
    Then the same call with y == NULL (statistics only, no residual): bit-identical saved and running statistics."""
    import hip_runtime as hr
    L = hr.lib()
    C, rows, groups, bpg = key
    c = _fold_case(key)
    B, _, H, W = c['shape']
    HW = H * W
    x, gamma, beta, stats = (c[k].to(DEV) for k in ('x', 'gamma', 'beta', 'stats'))
    r = None if c['residual'] is None else c['residual'].to(DEV)
    ws = hr.workspace(L.cnuda_bn_workspace_bytes(B, C, HW), x.device)
    runs = []
    for with_y in (True, False):
        got = {k: torch.full((groups * C,), NAN, device=DEV) for k in ('mean', 'invstd')}
        got['y'] = torch.full(c['shape'], NAN, device=DEV)
        got['rm'], got['rv'] = c['rm0'].to(DEV), c['rv0'].to(DEV)
        got['nbt'] = torch.zeros((), dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        with hr.launch_log() as log:
            hr.check(L.cnuda_bn_train_forward_stats(hr.ptr(x), hr.ptr(stats), bpg, rows, hr.ptr(gamma), hr.ptr(beta),
                                                    hr.ptr(r) if with_y else None, hr.ptr(got['y']) if with_y else None,
                                                    hr.ptr(got['mean']), hr.ptr(got['invstd']), hr.ptr(got['rm']),
                                                    hr.ptr(got['rv']), hr.ptr(got['nbt']), MOMENTUM, EPS, c['act'], B, C, HW,
                                                    groups, hr.ptr(ws), ws.numel(), hr.stream()), 'bn_train_forward_stats')
            torch.cuda.synchronize()
        assert _names(log) == {'bn_fold_stats_kernel': 1, 'bn_apply_kernel': 1}
        runs.append(got)
    check_case(c, runs[0], backward=False)
    assert torch.isnan(runs[1]['y']).all()                          # statistics only: y is not touched
    for k in ('mean', 'invstd', 'rm', 'rv', 'nbt'):
        assert torch.equal(runs[1][k], runs[0][k]), k


# ---------------------------------------------------------------------------------------------------------------
# d. eval mode
# ---------------------------------------------------------------------------------------------------------------
# plane_splits(planes, HW, 256): (1, 3, 33, 37) -> min(2048 / 3, ceil(1221 / 256)) = 5 workgroups per plane;
# (2, 1025, 3, 3) -> 1 (one short workgroup per plane, 2050 planes);  (1, 2, 50, 82) -> ceil(4100 / 256) = 17
@pytest.mark.parametrize('shape,act,res', [((1, 3, 33, 37), 2, True), ((2, 1025, 3, 3), 1, False), ((1, 2, 50, 82), 0, True)],
                         ids=['B1C3H33W37_relu6_res', 'B2C1025H3W3_relu', 'B1C2H50W82_none_res'])
def test_eval_forms(shape, act, res):
    import hip_runtime as hr
    B, C, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr(shape).encode()) % 1000003)
    x = 2 * torch.randn(shape, generator=g) + 0.5
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.5 + 0.5 * torch.randn(C, generator=g)
    if act == 2:
        gamma = 3 * gamma
    rm, rv = 0.5 + 0.3 * torch.randn(C, generator=g), 2 + 2 * torch.rand(C, generator=g)
    r = 2 * torch.randn(shape, generator=g) if res else None
    want = bo.eval_forward(x, gamma, beta, rm, rv, r, act, EPS)
    if act:
        assert (want == 0).double().mean() >= 0.02 and (act != 2 or (want == 6).double().mean() >= 0.02)
    y = torch.full(shape, NAN, device=DEV)
    dev = [t.to(DEV) for t in (x, gamma, beta, rm, rv)]
    dr = None if r is None else r.to(DEV)
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_bn_eval_forward(*[hr.ptr(t) for t in dev], hr.ptr(dr), hr.ptr(y), EPS, act, B, C, H * W,
                                                hr.stream()), 'bn_eval_forward')
        torch.cuda.synchronize()
    assert _names(log) == {'bn_eval_kernel': 1}
    _close(y, want, 'y')


# ---------------------------------------------------------------------------------------------------------------
# e. "safe for any float32 input": channels whose mean dwarfs their spread
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ill_case(act):
    shape = (1, 4, 50, 82)
    g = torch.Generator().manual_seed(4100 + act)
    c = {'shape': shape, 'groups': 1, 'act': act}
    x = torch.randn(shape, generator=g)
    x[:, 1] = 10 + 0.05 * x[:, 1]
    x[:, 2] = 100 + 0.05 * x[:, 2]
    x[:, 3] = 3.25
    c['x'] = x
    c['gamma'], c['beta'] = 1 + 0.2 * torch.randn(4, generator=g), 0.5 + 0.5 * torch.randn(4, generator=g)
    c['beta'][3] = 0.75                     # see the test: a multiple of ulp(1027)
    c['residual'] = None
    c['gy'] = torch.randn(shape, generator=g)
    c['rm0'], c['rv0'] = 0.1 * torch.randn(4, generator=g), 1 + 0.3 * torch.rand(4, generator=g)
    return add_reference(c)


def test_statistics_of_ill_conditioned_channels():
    """(1, 4, 50, 82), a plane cut in two: channels 0 + randn, 10 + 0.05 randn, 100 + 0.05 randn, and the constant 3.25.

    Statistics, all four channels, 1e-6 RELATIVE PER CHANNEL: bn_reduce_kernel<0> forms the squares and both sums in
    fp64, so the cancellation in s1 / n - mu * mu costs about 2^-53 * (mean / std)^2 -- 4e-10 at mean / std = 2000 --
    and what is left is the float32 rounding of the saved value, 6e-8.

    The constant channel: 4100 * 3.25 and 4100 * 3.25^2 are exact in fp64 (3.25 = 13 / 4), so s1 / n - mu^2 is exactly 0,
    invstd = 1 / sqrt(eps) and xhat = 0: y = act(beta).  The kernel applies y = x * sc + sh with sc = invstd * gamma and
    sh = fl(beta - fl(mean * sc)); x == mean == 3.25 exactly, so x * sc is the same rounded product P as mean * sc and
    y = P + fl(beta - P).  |P| = 3.25 * 316.2 * gamma lies in [512, 2048) for gamma in (0.5, 1.99), where float32's ulp is
    at most 2^-13: beta - P is exact when beta is a multiple of 2^-13, and then y == beta bit for bit.  beta[3] = 0.75 is
    one.  (A beta that is not carries up to ulp(P) / 2 = 6e-5 of rounding in sh: the price of the two-operation form at
    mean / std = 1000, of the same kind as channel 2's.)

    Channels 0, 1 and 3 get the whole forward / backward check at 1e-4: at mean / std = 200 the float32 rounding of the
    saved mean moves xhat by about 1e-5.  Channel 2 (mean / std = 2000) is checked for its statistics only: the float32
    x - mean downstream of them is inherent to the format, not to the kernel."""
    assert bo.plan(1, 4, 4100, 1)[0] == 2
    for act in (0, 1):
        c = _ill_case(act)
        got = run_entry_points(c)
        assert got['launched'] == TRAIN_KERNELS, got['launched']
        z, y, mean, invstd, rm, rv = c['ref']
        for k, want in (('mean', mean), ('invstd', invstd)):
            rel = ((got[k].double().cpu().reshape(want.shape) - want).abs() / want.abs()).reshape(-1)
            print(k, 'relative error per channel', ['%.2e' % v for v in rel.tolist()])
            assert (rel <= 1e-6).all(), (k, rel)
        assert mean[0, 3].item() == 3.25 and abs(invstd[0, 3].item() * EPS ** 0.5 - 1) < 1e-12
        assert abs(got['invstd'][3].item() * EPS ** 0.5 - 1) <= 1e-6
        y3 = got['y'][:, 3].double().cpu()
        assert (y3 - max(c['beta'][3].item(), 0.0) if act else y3 - c['beta'][3].item()).abs().max().item() <= 1e-6
        check_case(c, got, channels=[0, 1, 3])
