"""No GPU: (1) tests/bn_oracle.py, the hand-written fp64 BatchNorm that tests/test_gpu_bn_forms.py and the split-geometry
fuzz hold the kernels against, agrees with torch's own double-precision batch_norm + add + relu / relu6 under autograd
to 1e-12; (2) cnuda_bn_plan, the library's own answer to "which run-time form does this shape take", gives the table of
forms that those tests claim to cover."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bn_oracle as bo


def _rel(got, want, what):
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert got.shape == want.shape and err <= 1e-12 * max(scale, 1e-300), (what, err, scale)


@pytest.mark.parametrize('res', [False, True], ids=['plain', 'res'])
@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'relu', 'relu6'])
@pytest.mark.parametrize('shape,groups', [((2, 3, 7, 9), 1), ((4, 5, 6, 6), 2)])
def test_oracle_is_torchs_double_precision_batch_norm(shape, groups, act, res):
    """groups = 2 is two separate torch calls on the two halves of the batch, one after the other on the same running
    statistics; the parameter gradients are the sum of the two calls'."""
    g = torch.Generator().manual_seed(17 + act + 3 * res)
    B, C = shape[:2]
    x = (2 * torch.randn(shape, generator=g, dtype=bo.D) + 0.5).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g, dtype=bo.D)).requires_grad_(True)
    beta = (0.5 + 0.5 * torch.randn(C, generator=g, dtype=bo.D)).requires_grad_(True)
    if act == 2:                                 # reach the upper edge
        gamma, beta = (gamma.detach() * 3).requires_grad_(True), torch.full((C,), 2.0, dtype=bo.D, requires_grad=True)
    r = (2 * torch.randn(shape, generator=g, dtype=bo.D)).requires_grad_(True) if res else None
    gy = torch.randn(shape, generator=g, dtype=bo.D)
    rm0 = (0.1 * torch.randn(C, generator=g)).float()
    rv0 = (1 + 0.3 * torch.rand(C, generator=g)).float()

    rm, rv = rm0.double(), rv0.double()
    Bg = B // groups
    ys, means, invstds = [], [], []
    for k in range(groups):
        xs = x[k * Bg:(k + 1) * Bg]
        z = F.batch_norm(xs, rm, rv, gamma, beta, True, 0.1, 1e-5)          # updates rm, rv in place
        rm, rv = rm.float().double(), rv.float().double()                   # the buffers are float32
        if res:
            z = z + r[k * Bg:(k + 1) * Bg]
        ys.append(F.relu6(z) if act == 2 else (F.relu(z) if act else z))
        m = xs.detach().mean(dim=(0, 2, 3))
        means.append(m)
        invstds.append(1.0 / torch.sqrt(xs.detach().var(dim=(0, 2, 3), unbiased=False) + 1e-5))
    y = torch.cat(ys)
    y.backward(gy)

    z_o, y_o, mean_o, invstd_o, rm_o, rv_o = bo.train_forward(x.detach(), gamma.detach(), beta.detach(),
                                                             None if r is None else r.detach(), act, groups, 1e-5, 0.1,
                                                             rm0, rv0)
    _rel(y_o, y.detach(), 'y')
    _rel(mean_o, torch.stack(means), 'save_mean')
    _rel(invstd_o, torch.stack(invstds), 'save_invstd')
    _rel(rm_o, rm, 'running_mean')
    _rel(rv_o, rv, 'running_var')
    mask = bo.gate(z_o, act)
    if act:
        assert (z_o <= 0).any() and (act != 2 or (z_o >= 6).any())          # every edge in play closes something
    # gate_with_band with the reference's own output is the reference's gate
    assert torch.equal(bo.gate_with_band(z_o, y_o, act)[0], mask)
    gx, gres, gg, gb = bo.backward(gy, x.detach(), gamma.detach(), mean_o, invstd_o, mask)
    _rel(gx, x.grad, 'gx')
    _rel(gg, gamma.grad, 'ggamma')
    _rel(gb, beta.grad, 'gbeta')
    if res:
        _rel(gres, r.grad, 'gres')


def test_oracle_eval_and_fold():
    g = torch.Generator().manual_seed(5)
    x, r = torch.randn(2, 4, 5, 6, generator=g, dtype=bo.D), torch.randn(2, 4, 5, 6, generator=g, dtype=bo.D)
    gamma, beta = torch.rand(4, generator=g, dtype=bo.D) + 0.5, torch.randn(4, generator=g, dtype=bo.D)
    rm, rv = torch.randn(4, generator=g, dtype=bo.D), torch.rand(4, generator=g, dtype=bo.D) + 0.5
    for act, fn in ((0, lambda t: t), (1, F.relu), (2, F.relu6)):
        _rel(bo.eval_forward(x, 3 * gamma, beta, rm, rv, r, act), fn(F.batch_norm(x, rm, rv, 3 * gamma, beta, False, 0.1, 1e-5) + r),
             'eval act %d' % act)
    # fold: block sums of 5 pixels (one row of 30 = 6 blocks per image), two groups of one image each, 7 rows for 4 channels
    blocks = x.reshape(2, 4, 6, 5)
    stats = torch.full((12, 7, 2), float('nan'), dtype=torch.float32)
    stats[:, :4, 0] = blocks.sum(-1).permute(0, 2, 1).reshape(12, 4).float()
    stats[:, :4, 1] = (blocks ** 2).sum(-1).permute(0, 2, 1).reshape(12, 4).float()
    sums, mean, var = bo.fold(stats, 6, 2, 30)
    want_mean, want_var = x.mean(dim=(2, 3)), x.var(dim=(2, 3), unbiased=False)
    assert sums.shape == (2, 7, 2) and torch.isnan(sums[:, 4:]).all()
    assert (mean[:, :4] - want_mean).abs().max() < 1e-6 and (var[:, :4] - want_var).abs().max() < 1e-6


@pytest.mark.parametrize('shape,want', bo.FORMS, ids=[bo.form_id(f[0]) for f in bo.FORMS])
def test_plan_query_reports_the_form_of_every_row(shape, want):
    B, C, H, W, groups = shape
    assert bo.plan(B, C, H * W, groups) == want


def test_plan_table_covers_every_form():
    """what the rows are there for, stated on the table itself"""
    rows = [(s, p) for s, p in bo.FORMS]
    cut = [s for s, p in rows if p[0] > 1]
    assert {s[2] * s[3] % 4 == 0 for s in cut} == {True, False}                       # cut plane: 16-byte and scalar
    assert any(s[4] > 1 for s in cut) and any(s[0] // s[4] > 1 for s in cut)          # ... in groups, several images
    ips = [(s, p) for s, p in rows if p[1] > 1]
    assert {p[1] for s, p in ips} == {2, 4} and {s[2] * s[3] % 4 == 0 for s, p in ips} == {True, False}
    assert any(s[4] > 1 for s, p in ips)
    assert any(p[3] > 1 and p[0] == 1 and s[2] * s[3] % 4 for s, p in rows)           # apply grid cut, scalar tail
    assert {4095, 4096} <= {s[2] * s[3] for s, p in rows if p[0] == 1}                # both sides of the threshold
    assert max(s[0] * s[1] * s[2] * s[3] for s, p in rows) <= 240000


def test_plan_query_needs_no_results_and_rejects_bad_arguments():
    import hip_runtime as hr
    L = hr.lib()
    assert L.cnuda_bn_plan(2, 3, 63, 1, None, None, None, None) == 0
    ips = ctypes.c_int(-1)
    assert L.cnuda_bn_plan(16, 512, 16, 2, None, ctypes.byref(ips), None, None) == 0 and ips.value == 2
    assert L.cnuda_bn_plan(3, 4, 16, 2, None, None, None, None) == -1
    assert b'not divisible' in L.cnuda_last_error()
    for bad in ((0, 4, 16, 1), (2, 0, 16, 1), (2, 4, 0, 1), (2, 4, 16, 0)):
        assert L.cnuda_bn_plan(*bad, None, None, None, None) == -1, bad
    assert hr.ABI_VERSION == 2
