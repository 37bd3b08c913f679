"""Deformable PSROI pooling on the MI355X (csrc/psroi.hip) against the float64 oracle tests/psroi_oracle.py:
forward, sample counts and both gradients, with NO element left out of any comparison.  Instead every case asserts
that no sample coordinate comes within 1e-3 of an integer or a map border (psroi_oracle.margin) -- far above fp32
coordinate error at these map sizes -- so that an fp32 / fp64 floor or validity flip cannot occur.  The inputs are
constructed for that on the CPU (psroi_oracle.settle_offsets / settle_rois redraw the few elements that come close).

Tolerances (README: every kernel within 1e-4 of the oracle): 1e-4 absolute for the output on unit-scale inputs,
1e-4 * max|want| for each gradient tensor, counts exactly equal."""
import pytest
import torch

import psroi_oracle as po

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _draw_rois(g, k, B, H, W, scale, integer=False, batch=None):
    """ROIs in image pixels, some hanging over the map's border; corners at least 0.1 away from k + 0.5"""
    Wi, Hi = W / scale, H / scale
    u = lambda lo, hi: torch.rand(k, generator=g) * (hi - lo) + lo
    jit = lambda: torch.zeros(k) if integer else u(-0.4, 0.4)
    x1, y1 = torch.floor(u(-0.2, 0.9) * Wi), torch.floor(u(-0.2, 0.9) * Hi)
    w, h = torch.floor(u(0.03, 0.6) * Wi), torch.floor(u(0.03, 0.6) * Hi)
    bi = torch.randint(B, (k,), generator=g).float() if batch is None else torch.full((k,), float(batch))
    return torch.stack((bi, x1 + jit(), y1 + jit(), x1 + w + jit(), y1 + h + jit()), dim=1)


def _case(seed, B, OD, G, H, W, N, P, part, S, scale, tstd, no_trans, nc=1, special=False, integer=False, batch=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, OD * G * G, H, W, generator=g)
    rois = _draw_rois(g, N, B, H, W, scale, integer, batch)
    if special:
        Wi, Hi = W / scale, H / scale
        rois[0, 1:] = torch.tensor([Wi + 9.2, 3.1, Wi + 40.3, 30.2])            # wholly outside (to the right)
        rois[1, 1:] = torch.tensor([-60.2, -70.3, -20.1, -30.2])                # wholly outside (above, left)
        rois[2, 1:] = torch.tensor([10.2, 12.1, 8.9, 10.8])                     # end before start: the 0.1 floor
    args = (no_trans, scale, OD, G, P, part, S, tstd)
    if no_trans:
        off = torch.zeros(0)
        rois = po.settle_rois(x.shape, rois, lambda k: _draw_rois(g, k, B, H, W, scale, integer, batch), scale, P, S)
    else:
        off = torch.randn(N, 2 * nc, part, part, generator=g)
        off = po.settle_offsets(x.shape, rois, off, scale, P, part, S, tstd, g)
    go = torch.randn(N, OD, P, P, generator=g)
    return x, rois, off, go, args


CASES = {
    #                 seed B  OD  G  H   W   N   P  part S  scale  tstd  no_trans
    'plain':         (1,   2, 8,  1, 24, 32, 12, 7, 7,   4, 0.23,  0.0,  True),
    'deform':        (2,   2, 8,  1, 24, 32, 12, 7, 7,   4, 0.25,  0.1,  False, 1, True),
    'rfcn_group7':   (3,   2, 3,  7, 20, 20, 8,  7, 7,   2, 0.23,  0.1,  False),
    'part3_of_7':    (4,   2, 4,  1, 16, 24, 6,  7, 3,   1, 0.23,  0.2,  False, 1, True),
    'two_classes':   (5,   3, 6,  1, 18, 18, 9,  5, 5,   2, 0.25,  0.1,  False, 2),
    'group3_classes': (6,  2, 4,  3, 14, 22, 7,  6, 3,   2, 0.23,  0.15, False, 2, True),
    'example_pooling':  (7, 2, 32, 1, 64, 64, 20, 7, 7,  4, 0.25,  0.1,  True, 1, False, True),
    'example_dpooling': (8, 2, 32, 1, 64, 64, 20, 7, 7,  4, 0.25,  0.1,  False, 1, False, True),
    'image0_has_no_roi': (9, 2, 4, 1, 12, 12, 5,  3, 3,  2, 0.23,  0.1,  False, 1, False, False, 1),
    'large':         (10,  4, 10, 7, 40, 64, 300, 7, 7,  4, 0.23,  0.1,  False),
}


def _run_ext(x, rois, off, go, args, grad_input=None):
    import _ext
    xd, rd, od, gd = x.to(DEV), rois.to(DEV), off.to(DEV), go.to(DEV)
    out, count = _ext.dcn_v2_psroi_pooling_forward(xd, rd, od, *args)
    gi, goff = _ext.dcn_v2_psroi_pooling_backward(gd, xd, rd, od, count, *args, _grad_input=grad_input)
    return out, count, gi, goff


def _compare(got, want, no_trans):
    out, count, gi, goff = [t.double().cpu() for t in got]
    w_out, w_count, w_gi, w_goff = want
    assert torch.equal(count, w_count)
    err = (out - w_out).abs().max().item()
    print('output: max error %.3g' % err)
    assert err <= 1e-4
    for name, a, b in (('grad_input', gi, w_gi), ('grad_offset', goff, w_goff)):
        if name == 'grad_offset' and no_trans:
            assert a.numel() == 0
            continue
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print('%s: max error %.3g of max|want| %.3g' % (name, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, name


@pytest.mark.parametrize('name', list(CASES))
def test_forward_count_and_gradients_against_the_oracle(name):
    x, rois, off, go, args = _case(*CASES[name])
    m = po.margin(x.shape, rois, off, *args)
    print('margin %.3g' % m)
    assert m >= 1e-3
    want = po.forward_backward(x, rois, off, go, *args)
    if name in ('deform', 'part3_of_7', 'group3_classes'):
        assert bool((want[1] == 0).any()) and bool((want[1] > 0).any())          # count-0 bins are really there
    got = _run_ext(x, rois, off, go, args)
    _compare(got, want, args[0])
    if args[3] == 1:
        # group_size 1: the same through the module and autograd, bit for bit
        from libs.DCNv2.dcn_v2 import DCNv2Pooling
        pool = DCNv2Pooling(args[1], args[4], args[2], args[0], args[3], args[5], args[6], args[7]).to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        od = off.to(DEV).requires_grad_(not args[0])
        y = pool(xd, rois.to(DEV), od)
        y.backward(go.to(DEV))
        assert torch.equal(y.detach(), got[0]) and torch.equal(xd.grad, got[2])
        if not args[0]:
            assert torch.equal(od.grad, got[3])


def test_exact_hits_on_integers_and_borders():
    """Integer ROIs, scale 1/4, P = 4, S = 4, trans_std 1/4 and offsets in eighths: every coordinate is dyadic, many are
    integers or exactly -0.5 / W - 0.5.  fp32 and fp64 then compute the same coordinates exactly, so the comparison
    needs no margin."""
    g = torch.Generator().manual_seed(21)
    B, OD, H, W, N, P, S = 2, 4, 16, 16, 10, 4, 4
    x = torch.randn(B, OD, H, W, generator=g)
    x1, y1 = torch.randint(-2, 12, (N,), generator=g) * 4.0, torch.randint(-2, 12, (N,), generator=g) * 4.0
    w, h = torch.randint(1, 6, (N,), generator=g) * 16.0 - 1, torch.randint(1, 6, (N,), generator=g) * 16.0 - 1
    rois = torch.stack((torch.randint(B, (N,), generator=g).float(), x1, y1, x1 + w, y1 + h), dim=1)
    rois[0] = torch.tensor([0.0, 0.0, 0.0, 63.0, 63.0])                     # the whole map: starts at -0.5, ends at 15.5
    off = torch.randint(-8, 9, (N, 2, P, P), generator=g).float() / 8
    off[0] = 0
    go = torch.randn(N, OD, P, P, generator=g)
    args = (False, 0.25, OD, 1, P, P, S, 0.25)
    w_, h_ = po.sample_coords(rois, off, False, 0.25, P, P, S, 0.25)
    assert bool((w_ == w_.round()).any()) and bool((w_ == -0.5).any()) and bool((w_.float().double() == w_).all())
    want = po.forward_backward(x, rois, off, go, *args)
    _compare(_run_ext(x, rois, off, go, args), want, False)


def test_bit_stable_from_run_to_run_and_beside_another_stream():
    from hip_runtime import ops
    x, rois, off, go, args = _case(*CASES['large'])
    first = _run_ext(x, rois, off, go, args)
    torch.cuda.synchronize()
    again = _run_ext(x, rois, off, go, args)
    for a, b, what in zip(first, again, ('output', 'count', 'grad_input', 'grad_offset')):
        assert torch.equal(a, b), what
    # ... and with convolutions resident on the same CUs (tests/test_gpu_fullsize.py)
    x3 = torch.randn(32, 128, 64, 64, device=DEV, requires_grad=True)
    w3 = (torch.randn(128, 128, 3, 3, device=DEV) * 0.05).requires_grad_(True)
    g3 = torch.randn(32, 128, 64, 64, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for it in range(2):
        with torch.cuda.stream(side):
            for _ in range(3):
                y3 = ops.conv2d(x3, w3, None, 1, 1)
                if it % 2:
                    y3.backward(g3)
        beside = _run_ext(x, rois, off, go, args)
        torch.cuda.synchronize()
        for a, b, what in zip(first, beside, ('output', 'count', 'grad_input', 'grad_offset')):
            assert torch.equal(a, b), (it, what)


def test_accumulate_flag_adds_to_a_prefilled_grad_input():
    """acc = 1 does one fp32 addition per element, prefill + (the acc = 0 value, itself bit-stable): a sum of length
    two, so the result is within half an ulp -- 2^-24 relative -- of the exact sum of the two fp32 numbers."""
    x, rois, off, go, args = _case(*CASES['deform'])
    plain = _run_ext(x, rois, off, go, args)[2]
    pre = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    buf = pre.clone()
    got = _run_ext(x, rois, off, go, args, grad_input=buf)[2]
    assert got.data_ptr() == buf.data_ptr()
    exact = pre.double() + plain.double()
    assert bool(((got.double() - exact).abs() <= 2.0 ** -24 * exact.abs() + 1e-45).all())
    assert not torch.equal(got, pre)


def _module_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W, N, P = 2, 4, 12, 12, 3, 3
    x = torch.randn(B, C, H, W, generator=g)
    rois = _draw_rois(g, N, B, H, W, 0.23)
    rois = po.settle_rois(x.shape, rois, lambda k: _draw_rois(g, k, B, H, W, 0.23), 0.23, P, 2)
    target = torch.randn(N, C, P, P, generator=g)
    return x, rois, target, g


MODULE_SEED = 1


def _oracle_dcn_pooling(fc, x, rois, P, C, S, tstd):
    """DCNPooling.forward with the two pooling calls replaced by the oracle (float64) -> output, offsets"""
    n = rois.shape[0]
    roi = po.forward(x, rois, None, True, 0.23, C, 1, P, P, S, tstd)[0]
    om = fc(roi.reshape(n, -1)).view(n, 3, P, P)
    o1, o2, mask = torch.chunk(om, 3, dim=1)
    offset = torch.cat((o1, o2), dim=1)
    return po.forward(x, rois, offset, False, 0.23, C, 1, P, P, S, tstd)[0] * torch.sigmoid(mask), offset


def test_dcn_pooling_module_one_step():
    """example_mdpooling's shape of computation (testcuda.py:226-250): DCNPooling(no_trans=False) forward + backward,
    against the same module whose pooling calls are the oracle (weights copied, float64); the last layer is given
    random weights, with the reference's zero initialisation every offset would be zero."""
    import copy
    from libs.DCNv2.dcn_v2 import DCNPooling
    x, rois, target, g = _module_inputs(MODULE_SEED)
    P, C, S, tstd = 3, 4, 2, 0.1
    torch.manual_seed(MODULE_SEED)
    m = DCNPooling(0.23, P, C, False, sample_per_part=S, trans_std=tstd, deform_fc_dim=16)
    with torch.no_grad():
        m.offset_mask_fc[4].weight.normal_(0, 0.3)
        m.offset_mask_fc[4].bias.normal_(0, 0.3)
    fc = copy.deepcopy(m.offset_mask_fc).double()
    xo = x.double().requires_grad_(True)
    want, offset = _oracle_dcn_pooling(fc, xo, rois, P, C, S, tstd)
    assert po.margin(x.shape, rois, offset.detach(), False, 0.23, C, 1, P, P, S, tstd) >= 1e-3
    (want * target.double()).sum().backward()
    m = m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    got = m(xd, rois.to(DEV))
    (got * target.to(DEV)).sum().backward()
    assert (got.detach().double().cpu() - want.detach()).abs().max().item() <= 1e-4
    pairs = [('input', xd.grad, xo.grad)]
    pairs += [(n, p.grad, dict(fc.named_parameters())[n].grad) for n, p in m.offset_mask_fc.named_parameters()]
    for name, a, b in pairs:
        scale = b.abs().max().item()
        assert scale > 0 and (a.double().cpu() - b).abs().max().item() <= 1e-4 * scale, name


def test_bad_arguments_raise_and_launch_nothing():
    import _ext
    import hip_runtime as hr
    x, rois, off, go, args = _case(*CASES['image0_has_no_roi'])
    xd, od, gd = x.to(DEV), off.to(DEV), go.to(DEV)
    count = torch.ones_like(gd)
    with hr.launch_log() as log:
        for bad_index in (2.0, -1.0):
            bad = rois.clone()
            bad[3, 0] = bad_index
            with pytest.raises(RuntimeError, match='batch index'):
                _ext.dcn_v2_psroi_pooling_forward(xd, bad.to(DEV), od, *args)
            with pytest.raises(RuntimeError, match='batch index'):
                _ext.dcn_v2_psroi_pooling_backward(gd, xd, bad.to(DEV), od, count, *args)
        with pytest.raises(RuntimeError, match='channels'):
            _ext.dcn_v2_psroi_pooling_forward(xd, rois.to(DEV), od, *(args[:3] + (2,) + args[4:]))
        with pytest.raises(RuntimeError, match='offset'):
            _ext.dcn_v2_psroi_pooling_forward(xd, rois.to(DEV), od[:, :, :2], *args)
        with pytest.raises(RuntimeError, match='offset'):
            _ext.dcn_v2_psroi_pooling_backward(gd, xd, rois.to(DEV), od[:-1], count, *args)
        torch.cuda.synchronize()
    assert not [k for k in log.names if 'psroi' in k], log.names
