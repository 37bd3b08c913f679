"""The position-sparse backward of a detection head (cnuda_head_backward_sparse, hip_runtime.ops._ConvActConv1x1): the
gradient of the gather + masked-L1 loss is zero outside the batch's ind[b, m], the head's backward then gathers those
rows and takes the same sums over them.  Checked against torch CPU float64 beside the dense path on the same inputs;
the launch log says which path ran."""
import ast

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# The kernel registry follows the change (tests/kernel_manifest.py, which tests/test_zz_kernel_coverage.py reads when it
# runs, after every module has been collected).  The file itself is closed to a change of this kind, so its entries are
# brought up to date here, beside the tests they name; the guard verifies every one of them from the session's launch log.
#  * the two new kernels run in every benched step and are held against float64 below;
#  * the 128 x 128 step fixtures of tests/test_gpu_dla.py (M = 16 on a 32 x 32 map) now take the sparse backward and no
#    longer launch conv1x1_dgrad_act_kernel<2> / <3>: those credits move to tests that do.
# Every statement asserts what it replaces: an edit of the file makes this block fail instead of silently yielding.
import kernel_manifest as _km
_HERE = 'tests/test_gpu_head_sparse.py::'
for _kernel in ('head_rows_kernel', 'head_scatter_kernel'):
    assert _kernel not in _km.MANIFEST, 'tests/kernel_manifest.py names %s itself now: delete it here' % _kernel
    _km.MANIFEST[_kernel] = [_HERE + 'test_sparse_equals_dense_through_the_real_loss',
                             'tests/test_gpu_dla.py::test_uda_step128_plain_1e4',
                             'tests/test_gpu_dla.py::test_base_step_dla_configs1_plain_1e4']
_MOVED = {
    'conv1x1_dgrad_act_kernel<2>': (['tests/test_gpu_dla.py::test_uda_step128_plain_1e4',
                                     'tests/test_gpu_dla.py::test_base_step_dla_configs1_plain_1e4'],
                                    [_HERE + 'test_sparse_equals_dense_through_the_real_loss[c16_m8',
                                     _HERE + 'test_sparse_equals_dense_through_the_real_loss[c64_m150']),
    'conv1x1_dgrad_act_kernel<3>': (['tests/test_gpu_dla.py::test_uda_step128_plain_1e4[advent'],
                                    [_HERE + 'test_three_output_head_with_a_dense_gradient',
                                     _HERE + 'test_sparse_equals_dense_through_the_real_loss[c64_rot_m30']),
}
for _kernel, (_old, _new) in _MOVED.items():
    assert all(_t in _km.MANIFEST[_kernel] for _t in _old), 'tests/kernel_manifest.py has moved the credits of %s itself' % _kernel
    _km.MANIFEST[_kernel] = [_t for _t in _km.MANIFEST[_kernel] if _t not in _old] + _new
DEV = torch.device('cuda', 0) if torch.cuda.is_available() else None
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, (err, scale)


class _switch:
    """with _switch(on): ops.HEAD_SPARSE for the block"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from hip_runtime import ops
        self.prev, ops.HEAD_SPARSE = ops.HEAD_SPARSE, self.on

    def __exit__(self, *exc):
        from hip_runtime import ops
        ops.HEAD_SPARSE = self.prev


class _ratio:
    """with _ratio(r): ops.HEAD_SPARSE_RATIO for the block.  The small maps below sit at 8 M <= H W, under the measured
    constant of the size rule (a tuning threshold, not a limit of the kernels): the tests lower it to reach the path, as
    hip_runtime.halo_conv(1, 1) does for the halo-tile policy."""

    def __init__(self, r):
        self.r = r

    def __enter__(self):
        from hip_runtime import ops
        self.prev, ops.HEAD_SPARSE_RATIO = ops.HEAD_SPARSE_RATIO, self.r

    def __exit__(self, *exc):
        from hip_runtime import ops
        ops.HEAD_SPARSE_RATIO = self.prev


def _short(names):
    return ' '.join(names)


def _took_sparse(log, Co):
    """the head with Co outputs took the sparse backward (other heads of the graph have another Co)"""
    s = _short(log.names)
    assert 'head_rows_kernel' in s and 'head_scatter_kernel' in s and 'conv1x1_dgrad_act_kernel<%d>' % Co not in s, log.names


def _took_dense(log, Co):
    s = _short(log.names)
    assert 'conv1x1_dgrad_act_kernel<%d>' % Co in s and 'head_rows_kernel' not in s and 'head_scatter_kernel' not in s, log.names


def _rows(n_img, H, W, M, empty_last=False):
    """Constructed (ind, mask) [n_img, M].  Every image, in this order as far as M reaches: the top-left corner, the top-edge
    cell beside it (horizontally adjacent) and the left-edge cell below it (diagonally adjacent to the former: overlapping
    scatter, patches that leave the image), the corner AGAIN (a duplicate, both rows active), the bottom-right corner, a
    valid index with mask 0, ind = HW and ind = -1 with mask 1 (skipped, as in the loss); from the ninth row on the other
    two corners, a cell on the bottom and on the right edge, then distinct cells spread over the map.  All images hold the
    same indices (the same index in two images); `empty_last`: the last image has no active row at all.  M = 8 cannot hold
    all four corners: the M = 30 and M = 150 cases do."""
    HW = H * W
    cells = [0, 1, W, 0, HW - 1, (H // 2) * W + W // 2, HW, -1, W - 1, (H - 1) * W, (H - 1) * W + 2, 2 * W + W - 1]
    masks = [1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    used, k = set(cells), 0
    while len(cells) < M:
        k += 1
        c = (k * 37 + (k // 7) * W) % HW
        if c not in used:
            used.add(c)
            cells.append(c)
            masks.append(1)
    ind = torch.tensor([cells[:M]] * n_img, dtype=torch.int64)
    mask = torch.tensor([masks[:M]] * n_img, dtype=torch.uint8)
    if empty_last:
        mask[-1] = 0
    return ind, mask


def _head(C, Ch, Co, k, seed):
    import hip_runtime.nn as hnn
    torch.manual_seed(seed)
    return hnn.Head(hnn.Conv2d(C, Ch, k, padding=k // 2, bias=True, act_slope=0.0), hnn.Slot(),
                    hnn.Conv2d(Ch, Co, 1, bias=True)).to(DEV)


def _reference(head, x, gy, k):
    """float64 gradients (x, w1, b1, w2, b2) of head(x) under the upstream gradient gy, on the CPU; the ReLU's gate is the
    HIP hidden map's (tests/test_gpu_ops.py::test_head_pair_is_one_tape_node_with_the_two_layers_values says why)."""
    xr = x.detach().double().cpu().requires_grad_(True)
    ps = [p.detach().double().cpu().requires_grad_(True) for p in head.parameters()]
    pre = F.conv2d(xr, ps[0], ps[1], padding=k // 2)
    with torch.no_grad():
        gate = (head[0](x) > 0).cpu()
        differ = gate != (pre > 0)
        assert int(differ.sum()) <= 4 and (pre[differ].abs() < 1e-5).all(), (int(differ.sum()), pre[differ])
    F.conv2d(pre * gate, ps[2], ps[3]).backward(gy.detach().double().cpu())
    return [xr.grad] + [p.grad for p in ps]


CASES = {      # B, lead, C, Ch, Co, H, W, k, M
    'c16_m8': (3, 2, 16, 32, 2, 8, 12, 3, 8),
    'c64_rot_m30': (2, 2, 64, 256, 3, 16, 16, 3, 30),
    'k1_m8': (1, 1, 16, 48, 2, 12, 12, 1, 8),
    'c64_m150': (2, 1, 64, 256, 2, 64, 64, 3, 150),
}
_REF = {}     # (case, empty_last) -> the float64 gradients, computed once


@pytest.mark.parametrize('case,sparse_first,empty_last',
                         [(c, f, False) for c in CASES for f in (True, False)] +
                         [('c16_m8', True, True), ('c64_rot_m30', False, True)],
                         ids=lambda v: v if isinstance(v, str) else str(int(v)))
def test_sparse_equals_dense_through_the_real_loss(case, sparse_first, empty_last):
    """reg_l1_loss(head(x, lead)) backward with the switch on and off, x forked with a dense head on the other alias, in
    both backward orders: the launch log names the path; all five gradients of the head and the whole gradient of x
    against float64; the sparse path's error at most twice the dense path's (two orderings of the same products; 4 ulp of
    the largest element where the dense error is zero) and both within the fused node's own 1e-4."""
    import hip_runtime as hr
    import hip_runtime.fanout as fo
    from hip_runtime import ops
    B, lead, C, Ch, Co, H, W, k, M = CASES[case]
    head = _head(C, Ch, Co, k, 11)
    other = _head(C, 16, 1, 3, 12)              # the dense consumer of the other alias, all B images
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(B, C, H, W, generator=g).to(DEV)
    target0 = torch.randn(lead, M, Co, generator=g).to(DEV)
    ind, mask = _rows(lead, H, W, M, empty_last)
    ind, mask = ind.to(DEV), mask.to(DEV)
    assert 8 * M <= H * W

    def run(on):
        for p in list(head.parameters()) + list(other.parameters()):
            p.grad = None
        x = x0.clone().requires_grad_(True)
        a, b = fo.fork(x * 1.0, 2)
        def sparse_branch():
            return ops.reg_l1_loss(head(b, lead), mask, ind, target0.clone()) * 3.0
        def dense_branch():
            return other(a).sum() * 0.01
        # (the branch evaluated LAST runs its backward first)
        terms = [dense_branch(), sparse_branch()] if sparse_first else [sparse_branch(), dense_branch()]
        with _switch(on), _ratio(8), hr.launch_log() as log:
            (terms[0] + terms[1]).backward()
        (_took_sparse if on else _took_dense)(log, Co)
        return [x.grad.clone()] + [p.grad.clone() for p in head.parameters()]

    got_sparse, got_dense = run(True), run(False)
    if (case, empty_last) not in _REF:
        # the upstream gradient of the head is the loss kernel's own dense map, that of `other` the constant 0.01
        y = head(x0[:lead]).detach().requires_grad_(True)
        (ops.reg_l1_loss(y, mask, ind, target0.clone()) * 3.0).backward()
        ref = _reference(head, x0[:lead], y.grad, k)
        gx = torch.zeros(B, C, H, W, dtype=torch.float64)
        gx[:lead] = ref[0]
        gx += _reference(other, x0, torch.full((B, 1, H, W), 0.01), 3)[0]
        _REF[(case, empty_last)] = [gx] + ref[1:]
    ref = _REF[(case, empty_last)]
    for name, s, d, r in zip(('x', 'w1', 'b1', 'w2', 'b2'), got_sparse, got_dense, ref):
        es, ed = (s.double().cpu() - r).abs().max().item(), (d.double().cpu() - r).abs().max().item()
        floor = 4 * float(np.spacing(np.float32(r.abs().max().item())))
        print('%-16s %-3s sparse err %.3e  dense err %.3e  4 ulp %.3e' % (case, name, es, ed, floor))
        _close(s, r, 1e-4)
        _close(d, r, 1e-4)
        assert es <= (2 * ed if ed > 0 else floor), (name, es, ed, floor)


def test_no_active_row_anywhere_writes_zeros_and_leaves_grad_x():
    """The entry point itself with an all-zero mask: the four parameter gradients are WRITTEN as zeros (the sinks hold NaN
    before) and grad_x keeps what it held, bit for bit."""
    import hip_runtime as hr
    from hip_runtime import ops
    B, C, Ch, Co, H, W, M = 2, 16, 32, 2, 8, 12, 8
    g = torch.Generator().manual_seed(3)
    x, hidden = torch.randn(B, C, H, W, generator=g).to(DEV), torch.randn(B, Ch, H, W, generator=g).to(DEV)
    w1, w2 = torch.randn(Ch, C, 3, 3, generator=g).to(DEV), torch.randn(Co, Ch, generator=g).to(DEV)
    gy = torch.randn(B, Co, H, W, generator=g).to(DEV)          # (what a dense map would hold is never read)
    ind, _ = _rows(B, H, W, M)
    ind, mask = ind.to(DEV), torch.zeros(B, M, dtype=torch.uint8, device=DEV)
    gx = torch.randn(B, C, H, W, generator=g).to(DEV)
    before = gx.clone()
    sinks = [torch.full(s, float('nan'), device=DEV) for s in ((Ch, C, 3, 3), (Ch,), (Co, Ch), (Co,))]
    L = hr.lib()
    assert L.cnuda_head_backward_sparse_supported(B, M, C, H, W, Ch, Co, 3, 3, 1, 1, 1, 1) == 1
    ws = hr.workspace(L.cnuda_head_backward_sparse_workspace_bytes(B, M, C, H, W, Ch, Co, 3, 3), DEV)
    hr.check(L.cnuda_head_backward_sparse(hr.ptr(gy), hr.ptr(ind), hr.ptr(mask), hr.ptr(x), hr.ptr(hidden), hr.ptr(w1),
                                          hr.ptr(w2), hr.ptr(gx), *[hr.ptr(t) for t in sinks], B, M, C, H, W, Ch, Co, 3, 3,
                                          0.0, hr.ptr(ws), ws.numel(), hr.stream()), 'head_backward_sparse')
    torch.cuda.synchronize()
    for t in sinks:
        assert torch.equal(t, torch.zeros_like(t))
    assert torch.equal(gx, before)


@pytest.mark.parametrize('why', ['two_losses', 'hook', 'switch_off', 'large_M'])
def test_the_mark_does_not_outlive_its_tensor(why):
    """A gradient summed from two losses, one a hook has scaled, the switch off, 8 M > HW: the dense kernels run and the
    values are the dense path's bit for bit."""
    import hip_runtime as hr
    from hip_runtime import ops
    B, C, Ch, Co, H, W = 2, 16, 32, 2, 8, 12
    M = 16 if why == 'large_M' else 8
    assert (8 * M > H * W) == (why == 'large_M')
    head = _head(C, Ch, Co, 3, 21)
    g = torch.Generator().manual_seed(23)
    x0 = torch.randn(B, C, H, W, generator=g).to(DEV)
    target0 = torch.randn(B, M, Co, generator=g).to(DEV)
    ind, mask = _rows(B, H, W, M)
    ind, mask = ind.to(DEV), mask.to(DEV)

    def run(on):
        for p in head.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        y = head(x)
        loss = ops.reg_l1_loss(y, mask, ind, target0.clone())
        if why == 'two_losses':
            loss = loss + ops.reg_l1_loss(y, mask, ind, target0.clone() * 0.5) * 2.0
        if why == 'hook':
            y.register_hook(lambda t: t * 2.0)
        with _switch(on), _ratio(8), hr.launch_log() as log:
            loss.backward()
        _took_dense(log, Co)
        return [x.grad.clone()] + [p.grad.clone() for p in head.parameters()]

    for a, b in zip(run(why != 'switch_off'), run(False)):
        assert torch.equal(a, b)


def test_three_output_head_with_a_dense_gradient():
    """The rotated-box `wh` head's shape (3 outputs) under a dense random gradient: the fused pass over the hidden map
    (conv1x1_dgrad_act_kernel<3>) against float64."""
    import hip_runtime as hr
    B, C, Ch, Co, H, W, k = 2, 16, 32, 3, 8, 12, 3
    head = _head(C, Ch, Co, k, 31)
    g = torch.Generator().manual_seed(33)
    x0, gy = torch.randn(B, C, H, W, generator=g).to(DEV), torch.randn(B, Co, H, W, generator=g).to(DEV)
    x = x0.clone().requires_grad_(True)
    y = head(x)
    with hr.launch_log() as log:
        y.backward(gy)
    assert any('conv1x1_dgrad_act_kernel<3>' in n for n in log.names), log.names
    for a, r in zip([x.grad] + [p.grad for p in head.parameters()], _reference(head, x0, gy, k)):
        _close(a, r, 1e-4)


def test_small_uda_step_is_the_same_step_with_the_switch_off(golden):
    """One EntropyMinimization step of DLA-34 at 128 x 128 (the fixture of tests/test_gpu_dla.py::test_uda_step128_plain_1e4:
    B = 4 + 4, M = 16 on a 32 x 32 map: the size rule as shipped takes the sparse path), once with the switch on and once
    off,
    under tests/test_gpu_fullsize.py's rule for two runs of one step: statistics and head outputs bit-equal, parameter
    gradients within 1e-4 of each tensor's maximum."""
    import hip_runtime as hr
    import inputs as gin
    import uda
    from backends import dla
    from hip_runtime import ops, optim
    from losses.centernet import DetectionLoss
    from test_gpu_dla import UDA128, _Cfg
    from test_gpu_fullsize import _same_step_twice
    g = golden('step_entropy128')
    cls, args, rotated, seed = UDA128['entropy']
    B, S, M, C, n_obj = 4, 128, 16, 6, (5, 1, 9, 3)
    assert ops.HEAD_SPARSE_RATIO * M <= (S // 4) ** 2
    shapes = dict(ast.literal_eval(str(g['shapes_json'])))
    logs, switch = [], [True, False]

    def run():
        model = dla.build(num_classes=C, rotated_boxes=rotated)
        model.load_state_dict({k: T(v) for k, v in gin.fill_state(shapes, 0.1).items()})
        plugin = getattr(uda, cls)(*args)
        plugin.cfg = _Cfg(max_detections=40, model=_Cfg(backend=_Cfg(params=_Cfg(rotated_boxes=rotated, num_classes=C))))
        plugin.backend = model
        plugin.device = torch.device(DEV)
        plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
        plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, angle_weight=1.0, periodic=rotated)
        plugin.init_done()
        plugin.to(DEV)
        plugin.set_phase(True)
        data = {k: T(v) for k, v in gin.detection_batch(B, C, S // 4, S // 4, M, n_obj, 2, seed).items()}
        data['input'] = T(gin.image_batch(B, S, S, seed + 1))
        data['target_domain_input'] = T(gin.image_batch(B, S, S, seed + 2))
        with _switch(switch.pop(0)), hr.launch_log() as log:
            out = plugin.step(data)
            torch.cuda.synchronize()
        logs.append(_short(log.names))
        return plugin, out

    _same_step_twice(run)
    assert 'head_rows_kernel' in logs[0] and 'conv1x1_dgrad_act_kernel<2>' not in logs[0], logs[0]
    assert 'head_rows_kernel' not in logs[1] and 'conv1x1_dgrad_act_kernel<2>' in logs[1], logs[1]
