"""MI355X: every dispatch form of the plane-wise operators (csrc/spatial.hip) against an fp64 CPU restatement of the
same operation -- max-pool, depthwise convolution, depthwise transposed convolution, add, activation gradient, channel
copy, the offset | mask split and the 1x1 head gradient.

Every case has two parts.  (1) Values: forward and every gradient within 1e-4 of the reference's largest magnitude
(`_close`: the tolerance of tests/test_gpu_ops.py and tests/test_gpu_mbconv_ops.py); max-pool, copy, add and the
offset half of the split are exact (torch.equal).  (2) The case ran the form it is there for: the library's launch log
around the call must name the expected kernel.  No run-time switch of the library moves a call between these kernels
(the dispatch reads shapes and pointer alignment only), so that assertion is not gated.

B = 2 and C = 3 or 5 with random (so distinct) per-channel weights unless a case says otherwise: a plane / channel
mix-up changes the numbers.  References are computed once per geometry (lru_cache) and shared by the tests that need
them; nothing writes into them."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(got, want, what=''):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print('%s: max abs err %.3e, reference max %.3e' % (what, err, scale))
    assert err <= 1e-4 * scale, (what, err, scale)


def _names(log):
    from test_zz_kernel_coverage import short
    names = {short(n) for n in log.names}
    print(sorted(names))
    return names


def _dev(t, offset=False):
    """-> t on the device; offset: as a contiguous view one float into a larger buffer (16-byte alignment broken, which
    hip_runtime.f32c passes through unchanged)."""
    if not offset:
        return t.to(DEV)
    buf = torch.full((t.numel() + 8,), float('nan'), device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _same_pads(H, W, k, s):
    """TensorFlow's SAME rule (ops.same_padding) for both axes -> (top, left, bottom, right)"""
    def axis(n):
        total = max((-(-n // s) - 1) * s + k - n, 0)
        return total // 2, total - total // 2
    (pt, pb), (pl, pr) = axis(H), axis(W)
    return pt, pl, pb, pr


# ---------------------------------------------------------------------------------------------------------------
# 1. depthwise convolution
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dw_case(B, C, H, W, k, s, pads):
    """-> x, w, gy (fp32) and the fp64 reference y, grad_x, grad_w: explicit F.pad, then an unpadded grouped conv2d"""
    pt, pl, pb, pr = pads
    g = torch.Generator().manual_seed(100000 * k + 10000 * s + 100 * H + W + 7 * (pt + 3 * pl + 9 * pb + 27 * pr))
    x, w = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, k, k, generator=g) / k
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr, None, s, 0, 1, C)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    return x, w, gy, y.detach(), xr.grad, wr.grad


def _dw_gpu(case, s, pads, plain=False, offset=False, x_grad=True, w_grad=True):
    """plain: ops.depthwise_conv2d (cnuda_dwconv2d_*, pads all equal); else ops.depthwise_conv2d_same -> y, gx, gw, names"""
    import hip_runtime as hr
    from hip_runtime import ops
    x, w, gy = case[:3]
    dx, dw = _dev(x, offset).requires_grad_(x_grad), _dev(w).requires_grad_(w_grad)
    with hr.launch_log() as log:
        if plain:
            assert len(set(pads)) == 1
            y = ops.depthwise_conv2d(dx, dw, s, pads[0])
        else:
            y = ops.depthwise_conv2d_same(dx, dw, s, pads)
        y.backward(_dev(gy))
        torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, _names(log)


def _dw_check(B, C, H, W, k, s, pads, fwd, vec_bwd, plain=False):
    case = _dw_case(B, C, H, W, k, s, pads)
    y, gx, gw, names = _dw_gpu(case, s, pads, plain)
    _close(y, case[3], 'y')
    _close(gx, case[4], 'grad_x')
    _close(gw, case[5], 'grad_w')
    assert {fwd, 'dwconv_bwd_data_kernel<%d, %d>' % (k, 4 if vec_bwd else 1), 'dwconv_bwd_weight_kernel<%d>' % k,
            'dwconvt_wsum_kernel'} <= names, names


# The whole list of reachable dwconv_fwd_vec_kernel<K, S, PL> forms, each at an 8 x 8 map: (K, S, PL, pads (top, left,
# bottom, right), plain entry).  The kernel needs W % 4 == 0, Wo % 4 == 0, S <= 2, PL <= 2; dwconv_same_geom wants the
# bottom / right padding that the output size implies, (Ho - 1) * S + K - top - H, in [0, K).  With top = left = PL:
#   S = 1 (Ho = 8):  bottom = 7 + K - PL - 8 = K - 1 - PL
#   S = 2 (Ho = 4):  bottom = 6 + K - PL - 8 = K - 2 - PL    (any Ho but 4 leaves [0, K) or gives an odd Wo)
# <3, 2, 2> is missing: K - 2 - PL = -1, and Wo = 5 (bottom 1) is no multiple of 4 -- no geometry reaches it.
# The last two rows repeat a form with top != left, so that the two paddings cannot be swapped unnoticed.
VEC_FORMS = [
    (3, 1, 0, (0, 0, 2, 2), False),
    (3, 1, 1, (1, 1, 1, 1), False),         # SAME padding of k 3, s 1; torch's p = 1
    (3, 1, 2, (2, 2, 0, 0), False),
    (3, 2, 0, (0, 0, 1, 1), False),         # SAME padding of k 3, s 2 at an even size
    (3, 2, 1, (1, 1, 0, 0), False),         # torch's p = 1 (the bottom row of padding is never read)
    (5, 1, 0, (0, 0, 4, 4), False),
    (5, 1, 0, (0, 0, 0, 0), True),          # the plain entry with p = 0: 4 x 4 output
    (5, 1, 1, (1, 1, 3, 3), False),
    (5, 1, 2, (2, 2, 2, 2), False),         # SAME padding of k 5, s 1; torch's p = 2
    (5, 2, 0, (0, 0, 3, 3), False),
    (5, 2, 1, (1, 1, 2, 2), False),         # SAME padding of k 5, s 2 at an even size
    (5, 2, 2, (2, 2, 1, 1), False),         # torch's p = 2
    (3, 1, 0, (2, 0, 0, 2), False),
    (5, 2, 1, (2, 1, 1, 2), False),
]
assert len({f[:3] for f in VEC_FORMS}) == 11


@pytest.mark.parametrize('K,S,PL,pads,plain', VEC_FORMS,
                         ids=['k%ds%dpl%d_%s%s' % (f[0], f[1], f[2], ''.join(map(str, f[3])), '_plain' if f[4] else '')
                              for f in VEC_FORMS])
def test_depthwise_every_vector_forward_form(K, S, PL, pads, plain):
    assert pads[1] == PL
    _dw_check(2, 5, 8, 8, K, S, pads, 'dwconv_fwd_vec_kernel<%d, %d, %d>' % (K, S, PL), True, plain)


# (k, H, W, s, pads, plain, 16-byte input gradient): the scalar forward kernel takes odd widths, strides above 2 (plain
# entry only; 8 x 12 with s = 3 has W and Wo multiples of 4, so the stride alone decides) and a left padding above 2
SCALAR_FORMS = [(k, 7, 9, 1, _same_pads(7, 9, k, 1), False, False) for k in (3, 5)] + \
               [(k, 7, 9, 2, _same_pads(7, 9, k, 2), False, False) for k in (3, 5)] + \
               [(k, 7, 9, 3, (k // 2,) * 4, True, False) for k in (3, 5)] + \
               [(k, 8, 12, 3, (k // 2,) * 4, True, True) for k in (3, 5)] + \
               [(5, 8, 8, 1, (3, 3, 1, 1), False, True), (5, 8, 8, 1, (4, 4, 0, 0), False, True)]


@pytest.mark.parametrize('k,H,W,s,pads,plain,vec_bwd', SCALAR_FORMS,
                         ids=['k%d_%dx%d_s%d_%s%s' % (f[0], f[1], f[2], f[3], ''.join(map(str, f[4])), '_plain' if f[5] else '')
                              for f in SCALAR_FORMS])
def test_depthwise_both_scalar_forward_forms(k, H, W, s, pads, plain, vec_bwd):
    _dw_check(2, 5, H, W, k, s, pads, 'dwconv_fwd_kernel<%d>' % k, vec_bwd, plain)


# more than one workgroup of 256 items per plane (blockIdx.y * kT), forward and input gradient:
#   24 x 64, s 1: 384 quads either way, the second workgroup half empty;  s 2: 96 output quads, 384 input quads;
#   72 x 64, s 2: 288 output quads;   17 x 19: 323 items (s 2: 90 outputs, 323 inputs);   33 x 35, s 2: 306 outputs
@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('H,W,s', [(24, 64, 1), (24, 64, 2), (72, 64, 2), (17, 19, 1), (17, 19, 2), (33, 35, 2)])
def test_depthwise_planes_of_more_than_one_workgroup(H, W, s, k):
    pads = _same_pads(H, W, k, s)
    vec = W % 4 == 0
    _dw_check(2, 3, H, W, k, s, pads, 'dwconv_fwd_vec_kernel<%d, %d, %d>' % (k, s, pads[1]) if vec else 'dwconv_fwd_kernel<%d>' % k, vec)


# beyond dwconv_grid's cap of 64 workgroups per plane (16,384 items): threads make a second trip (+= gridDim.y * kT).
# 260 x 256: 16,640 quads;  129 x 129: 16,641 items;  stride 2 at 260 x 256: 4,160 output quads, 16,640 input quads
@pytest.mark.parametrize('H,W,k,s', [(260, 256, 3, 1), (260, 256, 5, 1), (129, 129, 3, 1), (129, 129, 5, 1), (260, 256, 3, 2)])
def test_depthwise_beyond_the_workgroup_cap(H, W, k, s):
    pads = _same_pads(H, W, k, s)
    vec = W % 4 == 0
    _dw_check(2, 3, H, W, k, s, pads, 'dwconv_fwd_vec_kernel<%d, %d, %d>' % (k, s, pads[1]) if vec else 'dwconv_fwd_kernel<%d>' % k, vec)


@pytest.mark.parametrize('k,s', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_vector_forms_give_the_scalar_forms_bits(k, s):
    """"Taps are accumulated in the scalar kernel's order, so both paths round alike": the same values with x one float
    off 16-byte alignment take the scalar forward kernel and give the same y and grad_x bit for bit.  The input
    gradient's form follows grad_x's alignment alone: its scalar form through cnuda_dwconv2d_backward called directly."""
    import hip_runtime as hr
    B, C, H, W, p = 2, 3, 24, 64, k // 2
    case = _dw_case(B, C, H, W, k, s, (p,) * 4)
    y, gx, gw, names = _dw_gpu(case, s, (p,) * 4, plain=True)
    assert {'dwconv_fwd_vec_kernel<%d, %d, %d>' % (k, s, p), 'dwconv_bwd_data_kernel<%d, 4>' % k} <= names, names
    y1, gx1, gw1, names1 = _dw_gpu(case, s, (p,) * 4, plain=True, offset=True)
    assert 'dwconv_fwd_kernel<%d>' % k in names1 and not any(n.startswith('dwconv_fwd_vec_kernel') for n in names1), names1
    for got, want, what in ((y1, case[3], 'y'), (gx1, case[4], 'grad_x'), (gw1, case[5], 'grad_w')):
        _close(got, want, 'offset x: ' + what)
    assert torch.equal(y1, y) and torch.equal(gx1, gx) and torch.equal(gw1, gw)
    x, w, gy = (_dev(t) for t in case[:3])
    gx2 = _dev(torch.zeros_like(case[0]), offset=True)
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_dwconv2d_backward(hr.ptr(x), hr.ptr(w), hr.ptr(gy), hr.ptr(gx2), None, B, C, H, W, k, s, p,
                                                  None, 0, hr.stream()), 'backward')
        torch.cuda.synchronize()
    names2 = _names(log)
    assert names2 == {'dwconv_bwd_data_kernel<%d, 1>' % k}, names2
    _close(gx2, case[4], 'offset grad_x')
    assert torch.equal(gx2, gx)


@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('H,W,s', [(8, 8, 1), (8, 8, 2), (7, 9, 2)])
def test_depthwise_frozen_operands(H, W, s, k):
    """requires_grad = False on the weight (grad_w == nullptr) or on the input (grad_x == nullptr): the other gradient is
    unchanged bit for bit and the frozen operand's kernels are not launched"""
    pads = _same_pads(H, W, k, s)
    case = _dw_case(2, 5, H, W, k, s, pads)
    y, gx, gw, _ = _dw_gpu(case, s, pads)
    _close(gx, case[4], 'grad_x')
    _close(gw, case[5], 'grad_w')
    y1, gx1, gw1, names1 = _dw_gpu(case, s, pads, w_grad=False)
    assert gw1 is None and torch.equal(y1, y) and torch.equal(gx1, gx)
    assert not any(n.startswith(('dwconv_bwd_weight_kernel', 'dwconvt_wsum_kernel')) for n in names1), names1
    y2, gx2, gw2, names2 = _dw_gpu(case, s, pads, x_grad=False)
    assert gx2 is None and torch.equal(y2, y) and torch.equal(gw2, gw)
    assert not any(n.startswith('dwconv_bwd_data_kernel') for n in names2), names2


# ---------------------------------------------------------------------------------------------------------------
# 2. depthwise transposed convolution
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dwt_case(C, H, W, k, s, p, with_skip):
    """-> x, w, skip (or None), gy (fp32) and the fp64 reference y, grad_x, grad_w"""
    g = torch.Generator().manual_seed(100000 * k + 10000 * s + 1000 * p + 30 * H + W + with_skip)
    x, w = torch.randn(2, C, H, W, generator=g), torch.randn(C, 1, k, k, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, None, stride=s, padding=p, groups=C)
    skip = torch.randn(y.shape, generator=g) if with_skip else None
    if with_skip:
        y = y + skip.double()
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    return x, w, skip, gy, y.detach(), xr.grad, wr.grad


def _dwt_gpu(case, s, p, offset=False, x_grad=True, w_grad=True):
    """-> y, gx, gw, grad_skip, names of the forward, names of the backward"""
    import hip_runtime as hr
    from hip_runtime import ops
    x, w, skip, gy = case[:4]
    dx, dw = _dev(x, offset).requires_grad_(x_grad), _dev(w).requires_grad_(w_grad)
    dskip = None if skip is None else _dev(skip).requires_grad_(True)
    with hr.launch_log() as fwd:
        y = ops.depthwise_conv_transpose2d(dx, dw, s, p, dskip)
        torch.cuda.synchronize()
    with hr.launch_log() as bwd:
        y.backward(_dev(gy))
        torch.cuda.synchronize()
    return y.detach(), dx.grad, dw.grad, None if skip is None else dskip.grad, _names(fwd), _names(bwd)


def _dwt_check(case, got):
    _close(got[0], case[4], 'y')
    _close(got[1], case[5], 'grad_x')
    _close(got[2], case[6], 'grad_w')
    if case[2] is not None:
        assert torch.equal(got[3].cpu(), case[3])          # the summand's gradient is the incoming gradient itself


DWT_GEOMETRIES = [(4, 2, 1), (4, 2, 0), (4, 1, 1), (4, 4, 0), (8, 4, 2), (8, 2, 3), (8, 1, 0),
                  (3, 2, 1), (5, 3, 2), (6, 3, 1), (2, 2, 0), (1, 1, 0), (16, 8, 4)]


@pytest.mark.parametrize('H,W', [(5, 7), (18, 20)])          # odd; more than 256 outputs and more than 256 inputs
@pytest.mark.parametrize('k,s,p', DWT_GEOMETRIES)
def test_depthwise_transposed_any_geometry(k, s, p, H, W):
    """"any k, s, p accepted": dwconvt_bwd_kernel<4> / <8> take s and p at run time, every other kernel size goes to the
    one-thread-per-pixel data gradient and the one-workgroup-per-tap weight gradient"""
    if (H - 1) * s - 2 * p + k <= 0 or (W - 1) * s - 2 * p + k <= 0:
        pytest.skip('empty output')
    case = _dwt_case(3, H, W, k, s, p, False)
    got = _dwt_gpu(case, s, p)
    _dwt_check(case, got)
    if (k, s, p) == (4, 2, 1) and W % 2 == 0:
        want = {'dwconvt_bwd_k4s2_kernel', 'dwconvt_wsum_kernel'}
    elif k in (4, 8):
        want = {'dwconvt_bwd_kernel<%d>' % k, 'dwconvt_wsum_kernel'}
    else:
        want = {'dwconvt_bwd_data_kernel', 'dwconvt_bwd_weight_kernel'}
    assert got[5] == want, got[5]


# form -> (H, W, k, s, p): the generic kernel (W odd, at k = 4), 2 x 2 taps one row per thread (Ho = 66 is no multiple
# of 4), the same at f = 4 below 4,096 outputs per plane, four rows per thread from 4,096 on, and the 4 x 4 block kernel
DWT_FORWARD_FORMS = {
    'dwconvt_fwd_kernel': (5, 7, 4, 2, 1),
    'dwconvt_fwd_f_kernel<2, 1>': (33, 36, 4, 2, 1),
    'dwconvt_fwd_f_kernel<4, 1>': (4, 4, 8, 4, 2),
    'dwconvt_fwd_f_kernel<4, 4>': (16, 16, 8, 4, 2),
    'dwconvt_fwd_k4s2_kernel': (32, 32, 4, 2, 1),
}


@pytest.mark.parametrize('with_skip', [False, True], ids=['plain', 'skip'])
@pytest.mark.parametrize('form', sorted(DWT_FORWARD_FORMS))
def test_depthwise_transposed_every_forward_form(form, with_skip):
    """... and, for the four 16-byte forms, "the result is theirs bit for bit": x one float off alignment takes the
    generic kernel and gives the same y, with and without the summand"""
    H, W, k, s, p = DWT_FORWARD_FORMS[form]
    case = _dwt_case(5, H, W, k, s, p, with_skip)
    got = _dwt_gpu(case, s, p)
    _dwt_check(case, got)
    assert got[4] == {form}, got[4]
    if form != 'dwconvt_fwd_kernel':
        off = _dwt_gpu(case, s, p, offset=True)
        _dwt_check(case, off)
        assert off[4] == {'dwconvt_fwd_kernel'}, off[4]
        assert torch.equal(off[0], got[0])


@pytest.mark.parametrize('H,W', [(18, 20), (32, 32), (5, 8)])
def test_depthwise_transposed_k4s2_backward_gives_the_generic_kernels_input_gradient(H, W):
    """k = 4, s = 2, p = 1: the aligned run takes dwconvt_bwd_k4s2_kernel, x one float off takes dwconvt_bwd_kernel<4>; both
    add an input pixel's taps in (ky, kx) order, so grad_x agrees bit for bit; the per-thread partial sums of grad_w are
    ordered differently, so grad_w is held to the fp64 tolerance in both"""
    case = _dwt_case(3, H, W, 4, 2, 1, False)
    a, b = _dwt_gpu(case, 2, 1), _dwt_gpu(case, 2, 1, offset=True)
    _dwt_check(case, a)
    _dwt_check(case, b)
    assert a[5] == {'dwconvt_bwd_k4s2_kernel', 'dwconvt_wsum_kernel'}, a[5]
    assert b[5] == {'dwconvt_bwd_kernel<4>', 'dwconvt_wsum_kernel'}, b[5]
    assert torch.equal(a[1], b[1])


@pytest.mark.parametrize('H,W,k,s,p,kernel', [(18, 20, 4, 2, 1, 'dwconvt_bwd_k4s2_kernel'), (5, 7, 4, 2, 1, 'dwconvt_bwd_kernel<4>'),
                                              (5, 7, 16, 8, 4, None)], ids=['k4s2', 'k4', 'k16'])
def test_depthwise_transposed_frozen_operands(H, W, k, s, p, kernel):
    """weight frozen (part == nullptr / no weight kernel) and input frozen (gx == nullptr / no data kernel)"""
    case = _dwt_case(3, H, W, k, s, p, False)
    full = _dwt_gpu(case, s, p)
    _dwt_check(case, full)
    wf = _dwt_gpu(case, s, p, w_grad=False)
    assert wf[2] is None and torch.equal(wf[0], full[0]) and torch.equal(wf[1], full[1])
    assert wf[5] == ({kernel} if kernel else {'dwconvt_bwd_data_kernel'}), wf[5]
    xf = _dwt_gpu(case, s, p, x_grad=False)
    assert xf[1] is None and torch.equal(xf[0], full[0]) and torch.equal(xf[2], full[2])
    assert xf[5] == ({kernel, 'dwconvt_wsum_kernel'} if kernel else {'dwconvt_bwd_weight_kernel'}), xf[5]


# ---------------------------------------------------------------------------------------------------------------
# 3. max-pool (window == stride, no padding)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_case(shape, k, ties):
    """test_maxpool's inputs (ties_and_nan: a grid of halves, so most windows hold their maximum more than once, and five
    NaN) -> x, gy, CPU torch's y and grad_x"""
    g = torch.Generator().manual_seed(5 + shape[2])
    x = torch.randn(shape, generator=g)
    if ties:
        x = torch.round(x * 2) / 2
        x.view(-1)[torch.randperm(x.numel(), generator=g)[:5]] = float('nan')
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, k)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    return x, gy, y.detach(), xr.grad


def _pool_gpu(case, k, offset=False):
    import hip_runtime as hr
    from hip_runtime import ops
    dx = _dev(case[0], offset).requires_grad_(True)
    with hr.launch_log() as log:
        y = ops.max_pool2d(dx, k)
        y.backward(_dev(case[1]))
        torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu().nan_to_num(nan=1e30), case[2].nan_to_num(nan=1e30))
    assert torch.equal(dx.grad.cpu(), case[3])
    return y.detach(), dx.grad, _names(log)


SCALAR_POOL = {'maxpool_fwd_kernel', 'maxpool_bwd_kernel'}


@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties_and_nan'])
@pytest.mark.parametrize('shape,k,tail', [((1, 3, 7, 8), 2, True), ((2, 2, 9, 10), 3, True), ((2, 2, 9, 12), 3, False)])
def test_maxpool_scalar_kernels_and_the_uncovered_tail(shape, k, tail, ties):
    """k = 2 with odd H and W % 4 == 0 (scalar kernels, the last row zeroed by the tail kernel) and k = 3 with and without
    an uncovered column"""
    names = _pool_gpu(_pool_case(shape, k, ties), k)[2]
    assert names == SCALAR_POOL | ({'maxpool_bwd_tail_kernel'} if tail else set()), names


@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties_and_nan'])
def test_maxpool_vector_kernels_give_the_scalar_kernels_bits(ties):
    case = _pool_case((2, 5, 8, 12), 2, ties)
    y, gx, names = _pool_gpu(case, 2)
    assert names == {'maxpool2_fwd_vec_kernel', 'maxpool2_bwd_vec_kernel'}, names
    y1, gx1, names1 = _pool_gpu(case, 2, offset=True)
    assert names1 == SCALAR_POOL, names1
    assert torch.equal(y1.nan_to_num(nan=1e30), y.nan_to_num(nan=1e30)) and torch.equal(gx1, gx)


@pytest.mark.parametrize('shape,vec', [((1, 3, 850, 850), False), ((2, 4, 768, 768), True)], ids=['scalar', 'vector'])
def test_maxpool_beyond_the_grid_cap(shape, vec):
    """stream_grid caps the grid at 2,048 workgroups of 256: 541,875 windows (scalar kernels; W % 4 == 2) and 589,824
    window pairs (16-byte kernels) make threads take a second trip through the grid-stride loop"""
    names = _pool_gpu(_pool_case(shape, 2, False), 2)[2]
    assert names == ({'maxpool2_fwd_vec_kernel', 'maxpool2_bwd_vec_kernel'} if vec else SCALAR_POOL), names


def test_maxpool_backward_accumulate_touches_the_arg_max_cells_only():
    """cnuda_maxpool2d_backward_acc(accumulate = 1) at 5 x 8 (odd H: the scalar kernel): held + g in the arg-max cells, every
    other cell -- the uncovered last row included -- keeps its bits, and no tail kernel runs"""
    import hip_runtime as hr
    shape = (1, 2, 5, 8)
    x, gy, _, gx_ref = _pool_case(shape, 2, False)
    held = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    acc = _dev(held).clone()
    dx, dgy = _dev(x), _dev(gy)
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_maxpool2d_backward_acc(hr.ptr(dx), hr.ptr(dgy), hr.ptr(acc), 1, *shape, 2, hr.stream()))
        torch.cuda.synchronize()
    assert _names(log) == {'maxpool_bwd_kernel'}
    touched = gx_ref != 0
    assert touched.sum().item() == gy.numel() and not touched[:, :, 4].any()
    assert torch.equal(acc.cpu()[~touched], held[~touched])
    assert torch.equal(acc.cpu(), torch.where(touched, held + gx_ref, held))


# ---------------------------------------------------------------------------------------------------------------
# 4. add, activation gradient, channel copy, offset | mask split, 1x1 head gradient
# ---------------------------------------------------------------------------------------------------------------
def _guarded(n, offset):
    """-> (buffer of sentinels, its n-float window at float 4 (16-byte aligned) or 5)"""
    buf = torch.full((n + 12,), -7.0, device=DEV)
    at = 5 if offset else 4
    return buf, buf[at:at + n]


def _guards_intact(buf, out):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    at = (out.data_ptr() - buf.data_ptr()) // 4
    keep[at:at + out.numel()] = False
    return bool((buf[keep] == -7.0).all())


@pytest.mark.parametrize('which', ['aligned', 'a_offset', 'b_offset', 'out_offset', 'in_place', 'in_place_offset'])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4099])
def test_add_every_length_alignment_and_in_place(n, which):
    """cnuda_add: the 16-byte loop with its scalar tail, the scalar loop for an operand off alignment, and out == a
    (hip_runtime.fanout sums gradients in place).  One fp32 addition per element: exact."""
    import hip_runtime as hr
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    da, db_ = _dev(a, which in ('a_offset', 'in_place_offset')), _dev(b, which == 'b_offset')
    buf, out = _guarded(n, which == 'out_offset')
    if which.startswith('in_place'):
        out = da
    assert (out.data_ptr() % 16 != 0) == (which in ('out_offset', 'in_place_offset'))
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_add(hr.ptr(da), hr.ptr(db_), hr.ptr(out), n, hr.stream()), 'add')
        torch.cuda.synchronize()
    assert _names(log) == {'add_kernel'}
    assert torch.equal(out.cpu(), a + b)
    assert which.startswith('in_place') or _guards_intact(buf, out)
    assert torch.equal(db_.cpu(), b)


@pytest.mark.parametrize('which', ['aligned', 'gy_offset', 'y_offset', 'gx_offset'])
@pytest.mark.parametrize('slope', [0.0, 0.2])
@pytest.mark.parametrize('n', [1, 5, 4099])
def test_activation_gradient_every_length_and_alignment(n, slope, which):
    """cnuda_act_backward: gx = gy * (y > 0 ? 1 : slope); y == 0.0 and y == -0.0 take the slope side.  An operand off
    16-byte alignment takes the scalar loop (the host checks, as cnuda_add does) and gives the same values."""
    import hip_runtime as hr
    g = torch.Generator().manual_seed(n)
    gy, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[0] = -0.0
    if n > 1:
        y[1], y[-1] = 0.0, 0.0
    dgy, dy = _dev(gy, which == 'gy_offset'), _dev(y, which == 'y_offset')
    buf, gx = _guarded(n, which == 'gx_offset')
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_act_backward(hr.ptr(dgy), hr.ptr(dy), hr.ptr(gx), n, slope, hr.stream()), 'act_backward')
        torch.cuda.synchronize()
    assert _names(log) == {'act_bwd_kernel'}
    slope32 = torch.tensor(slope, dtype=torch.float32).double()
    _close(gx, gy.double() * torch.where(y.double() > 0, torch.ones((), dtype=torch.float64), slope32), 'grad_x')
    assert torch.equal(gx.cpu(), torch.where(y > 0, gy, gy * torch.tensor(slope)))          # one fp32 product: exact
    assert _guards_intact(buf, gx)


# (B, Cn, HW, Csrc, src_off, Cdst, dst_off): 4-byte copies (HW % 4 != 0), 16-byte copies, two chunks per row
# (HW / 4 > 1,024), and more rows than the grid's 65,535 (row += gridDim.y)
COPY_CASES = {'hw30': (2, 3, 30, 5, 1, 7, 2), 'hw20': (2, 3, 20, 5, 1, 7, 2), 'hw4224': (2, 3, 4224, 5, 2, 4, 1),
              'rows65540': (2, 32770, 4, 32771, 1, 32773, 2)}


@pytest.mark.parametrize('which', ['aligned', 'src_offset', 'dst_offset'])
@pytest.mark.parametrize('name', sorted(COPY_CASES))
def test_copy_channels_keeps_everything_outside_the_range(name, which):
    """cnuda_copy_channels between tensors of different channel counts at non-zero channel offsets into a destination full
    of sentinels; a tensor off 16-byte alignment takes the 4-byte copies (the host checks) with the same result"""
    import hip_runtime as hr
    B, Cn, HW, Csrc, so, Cdst, do = COPY_CASES[name]
    src = torch.randn(B, Csrc, HW, generator=torch.Generator().manual_seed(HW))
    want = torch.full((B, Cdst, HW), -7.0)
    want[:, do:do + Cn] = src[:, so:so + Cn]
    dsrc, dst = _dev(src, which == 'src_offset'), _dev(torch.full((B, Cdst, HW), -7.0), which == 'dst_offset')
    with hr.launch_log() as log:
        hr.check(hr.lib().cnuda_copy_channels(hr.ptr(dsrc), hr.ptr(dst), B, Cn, HW, Csrc, so, Cdst, do, hr.stream()), 'copy')
        torch.cuda.synchronize()
    assert _names(log) == {'copy_channels_kernel'}
    assert torch.equal(dst.cpu(), want)


@functools.lru_cache(maxsize=None)
def _split_case(B, H, W):
    """taps = 9: the chunk / cat / sigmoid chain of DCN.forward in fp64 -> om, go, gm (fp32), offset, mask, grad_om (fp64)"""
    g = torch.Generator().manual_seed(B + H * W)
    om = torch.randn(B, 27, H, W, generator=g) * 3
    omr = om.double().requires_grad_(True)
    o1, o2, m = torch.chunk(omr, 3, dim=1)
    off, mask = torch.cat((o1, o2), 1), torch.sigmoid(m)
    go, gm = torch.randn(off.shape, generator=g), torch.randn(mask.shape, generator=g)
    torch.autograd.backward([off, mask], [go.double(), gm.double()])
    return om, go, gm, off.detach(), mask.detach(), omr.grad


@pytest.mark.parametrize('offset', [False, True], ids=['aligned', 'offset_views'])
@pytest.mark.parametrize('B,H,W', [(2, 5, 6), (2, 4, 5), (2, 66, 64), (2430, 2, 2)],
                         ids=['hw30', 'hw20', 'hw4224', 'rows65610'])
def test_split_offset_mask_forward_and_backward(B, H, W, offset):
    """offset_views: om and both incoming gradients one float off 16-byte alignment -- the 4-byte loops, same values"""
    import hip_runtime as hr
    from hip_runtime import ops
    om, go, gm, off, mask, gom = _split_case(B, H, W)
    dom = _dev(om, offset).requires_grad_(True)
    with hr.launch_log() as log:
        doff, dmask = ops.split_offset_mask(dom)
        torch.autograd.backward([doff, dmask], [_dev(go, offset), _dev(gm, offset)])
        torch.cuda.synchronize()
    assert _names(log) == {'split_offset_mask_kernel', 'split_offset_mask_bwd_kernel'}
    assert torch.equal(doff.detach().cpu().double(), off)
    _close(dmask, mask, 'mask')
    _close(dom.grad, gom, 'grad_om')


@pytest.mark.parametrize('Ch', [16, 80, 99, 100])
@pytest.mark.parametrize('Co', [1, 2, 3, 4, 5, 6, 7, 8])
def test_head_gradient_every_output_count(Co, Ch):
    """cnuda_conv1x1_backward_data_act: gh[b, m, p] = (hid > 0 ? 1 : slope) * sum_c w[c, m] * go[b, c, p].  Ch = 80, 99 and
    100 are cut in two channel chunks (grid y); 99 -> 50 + 49 is the ragged one (min(m0 + chunk, Ch))."""
    import hip_runtime as hr
    B, HW = 2, 20
    g = torch.Generator().manual_seed(10 * Ch + Co)
    go, w, hid = torch.randn(B, Co, HW, generator=g), torch.randn(Co, Ch, generator=g), torch.randn(B, Ch, HW, generator=g)
    hid.view(-1)[::7] = 0.0
    hid.view(-1)[3::11] = -0.0
    lin = torch.einsum('cm,bcp->bmp', w.double(), go.double())
    dgo, dw, dhid = _dev(go), _dev(w), _dev(hid)
    for slope in (0.0, 0.2):
        gh = torch.full((B, Ch, HW), float('nan'), device=DEV)
        with hr.launch_log() as log:
            hr.check(hr.lib().cnuda_conv1x1_backward_data_act(hr.ptr(dgo), hr.ptr(dw), hr.ptr(dhid), hr.ptr(gh), B, Co, Ch, HW,
                                                              slope, hr.stream()), 'head gradient')
            torch.cuda.synchronize()
        assert _names(log) == {'conv1x1_dgrad_act_kernel<%d>' % Co}
        slope32 = torch.tensor(slope, dtype=torch.float32).double()
        _close(gh, lin * torch.where(hid.double() > 0, torch.ones((), dtype=torch.float64), slope32), 'grad_hidden slope %g' % slope)


def test_head_gradient_declines_a_view_off_alignment():
    import hip_runtime as hr
    B, Co, Ch, HW = 2, 3, 16, 20
    go, w, hid = torch.zeros(B, Co, HW), torch.zeros(Co, Ch), torch.zeros(B, Ch, HW)
    gh = torch.zeros(B, Ch, HW, device=DEV)
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        hr.check(hr.lib().cnuda_conv1x1_backward_data_act(hr.ptr(_dev(go)), hr.ptr(_dev(w)), hr.ptr(_dev(hid, offset=True)),
                                                          hr.ptr(gh), B, Co, Ch, HW, 0.0, hr.stream()), 'head gradient')
