"""Bit pins of every plane-wise operator of csrc/spatial.hip, forward and every gradient, one case per dispatch form.

tests/golden/spatial_bits.npz was recorded by run_all() below with the library of the commit BEFORE the kernels of
spatial.hip were folded onto one grid-stride walk, one max-pool pick, one depthwise-transposed backward frame and one
row / elementwise mapper (profiles/spatial_dedupe_ab.txt), in two separate processes whose recordings were equal.  The
library is built with -ffp-contract=off, so a helper that keeps the order of operations gives the same bits: a
difference here means an expression was reordered.  Find it; never re-record from the code under test.

Every case calls the C entry points through hip_runtime.lib() (so that a null gradient, `accumulate` and a view off
16-byte alignment are what the case says) with inputs from seeded RandomStates, writes into buffers pre-filled with a
sentinel, and records with the arrays the kernels the library launched (`<family>/kernels`): the dispatch is pinned with
the bits.  The geometries are those of tests/test_gpu_spatial_forms.py at B = 2, C = 3.  Max-pool inputs are halves (exact
ties) with one NaN per plane.  Arrays above DIGEST_ABOVE elements are stored as the bits of head and tail, the bit sum and a
position-weighted bit sum (`.digest`); the bound is 1,024 and not the 65,536 of tests/test_gpu_loss_bits.py because there
are about eighty cases here: the forms that start at 4,096 outputs per plane (24,576 to 47,520 floats each, with and
without the summand) would alone make the fixture larger than that of the losses, and the arrays of 1,100 to 2,200 floats
would do so again."""
import os

import numpy as np
import pytest
import torch

from test_gpu_spatial_forms import DWT_FORWARD_FORMS, VEC_FORMS, _dev, _same_pads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spatial_bits.npz')
FAMILIES = ('pool', 'winpool', 'dwconv', 'dwconvt', 'addact', 'head', 'rows')
DIGEST_ABOVE = 1 << 10
B, C = 2, 3
FILL = -7.0                                                     # what an output buffer holds before the call


def _put(res, key, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    if a.size <= DIGEST_ABOVE:
        res[key] = a
        return
    flat = a.reshape(-1).view(np.uint32)
    bits, weight = flat.astype(np.uint64), np.arange(flat.size, dtype=np.uint64) % np.uint64(65521) + np.uint64(1)
    sums = np.array([bits.sum(dtype=np.uint64), (bits * weight).sum(dtype=np.uint64)], np.uint64)     # (wrap modulo 2^64)
    res[key + '.digest'] = np.concatenate([flat[:16], flat[-16:], sums.view(np.uint32)])


def _f32(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


def _out(*shape):
    return torch.full(shape, FILL, dtype=torch.float32, device=DEV)


class _Case:
    """with _Case(res, tag, kernels) as put: ...; put(name, tensor).  Records the kernels launched inside the block and
    requires `kernels` (the forms the case is there for) among them."""

    def __init__(self, res, tag, kernels=()):
        self.res, self.tag, self.kernels = res, tag, set(kernels)

    def __enter__(self):
        import hip_runtime as hr
        self.log = hr.launch_log()
        self.log.__enter__()
        return lambda name, t: _put(self.res, self.tag + name, t)

    def __exit__(self, *exc):
        from test_zz_kernel_coverage import short
        torch.cuda.synchronize()
        self.log.__exit__(*exc)
        if exc[0] is None:
            names = sorted(short(n) for n in self.log.names)
            assert self.kernels <= set(names), (self.tag, names)
            key = self.tag.split('/')[0] + '/kernels'           # one array of lines per family: "<case> <kernels>"
            self.res[key] = np.append(self.res.get(key, np.array([], str)), self.tag + ' ' + ', '.join(names))


def _pool_input(rs, H, W, offset, Hc=None, Wc=None):
    """halves, so that most windows hold their maximum more than once; one NaN per plane, inside the Hc x Wc corner that
    the windows cover"""
    x = np.round(rs.standard_normal((B, C, H, W)) * 2) / 2
    x.reshape(B * C, H, W)[np.arange(B * C), rs.randint(0, Hc or H, B * C), rs.randint(0, Wc or W, B * C)] = np.nan
    return _dev(torch.from_numpy(x.astype(np.float32)), offset)


def _run_pool(res):
    import hip_runtime as hr
    L = hr.lib()
    vec, scalar = {'maxpool2_fwd_vec_kernel', 'maxpool2_bwd_vec_kernel'}, {'maxpool_fwd_kernel', 'maxpool_bwd_kernel'}
    for H, W, k, offset, want in ((8, 8, 2, False, vec), (7, 9, 2, False, scalar | {'maxpool_bwd_tail_kernel'}),
                                  (9, 9, 3, False, scalar), (8, 8, 2, True, scalar)):
        rs = np.random.RandomState(1000 + 100 * H + 10 * W + k)
        x = _pool_input(rs, H, W, offset, H // k * k, W // k * k)
        gy, held = _dev(_f32(rs, B, C, H // k, W // k)), _dev(_f32(rs, B, C, H, W))
        with _Case(res, 'pool/%dx%d_k%d%s/' % (H, W, k, '_offset' if offset else ''), want) as put:
            y, gx = _out(B, C, H // k, W // k), _out(B, C, H, W)
            hr.check(L.cnuda_maxpool2d_forward(hr.ptr(x), hr.ptr(y), B, C, H, W, k, hr.stream()))
            hr.check(L.cnuda_maxpool2d_backward(hr.ptr(x), hr.ptr(gy), hr.ptr(gx), B, C, H, W, k, hr.stream()))
            hr.check(L.cnuda_maxpool2d_backward_acc(hr.ptr(x), hr.ptr(gy), hr.ptr(held), 1, B, C, H, W, k, hr.stream()))
            put('y', y), put('grad_x', gx), put('grad_x_accumulated', held)


def _run_winpool(res):
    import hip_runtime as hr
    L = hr.lib()
    for H, W, k, s, p in ((7, 9, 3, 2, 1), (5, 6, 2, 1, 1)):
        rs = np.random.RandomState(2000 + 100 * H + 10 * W + k)
        x = _pool_input(rs, H, W, False)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        gy = _dev(_f32(rs, B, C, Ho, Wo))
        with _Case(res, 'winpool/%dx%d_k%ds%dp%d/' % (H, W, k, s, p), {'maxpool_win_fwd_kernel', 'maxpool_win_bwd_kernel'}) as put:
            y, gx = _out(B, C, Ho, Wo), _out(B, C, H, W)
            hr.check(L.cnuda_maxpool2d_window_forward(hr.ptr(x), hr.ptr(y), B, C, H, W, k, s, p, hr.stream()))
            hr.check(L.cnuda_maxpool2d_window_backward(hr.ptr(x), hr.ptr(gy), hr.ptr(gx), B, C, H, W, k, s, p, hr.stream()))
            put('y', y), put('grad_x', gx)


def _workspace(nbytes):
    import hip_runtime as hr
    ws = hr.workspace(nbytes, torch.device(DEV))
    return hr.ptr(ws), ws.numel()


def _run_dwconv(res):
    import hip_runtime as hr
    L = hr.lib()
    # (H, W, k, s, pads, plain entry, grad_x, grad_w, the forward form)
    cases = [(8, 8, K, S, pads, plain, True, True, 'dwconv_fwd_vec_kernel<%d, %d, %d>' % (K, S, PL))
             for K, S, PL, pads, plain in VEC_FORMS]
    cases += [(7, 9, k, s, _same_pads(7, 9, k, s), False, True, True, 'dwconv_fwd_kernel<%d>' % k) for k in (3, 5) for s in (1, 2)]
    cases += [(7, 9, 3, 3, (1, 1, 1, 1), True, True, True, 'dwconv_fwd_kernel<3>'),
              (7, 9, 3, 2, _same_pads(7, 9, 3, 2), False, True, False, 'dwconv_bwd_data_kernel<3, 1>'),
              (7, 9, 3, 2, _same_pads(7, 9, 3, 2), False, False, True, 'dwconv_bwd_weight_kernel<3>'),
              (8, 8, 5, 1, (2, 2, 2, 2), False, True, False, 'dwconv_bwd_data_kernel<5, 4>'),
              (8, 8, 5, 1, (2, 2, 2, 2), False, False, True, 'dwconv_bwd_weight_kernel<5>'),
              (260, 256, 3, 1, _same_pads(260, 256, 3, 1), False, True, True, 'dwconv_fwd_vec_kernel<3, 1, 1>')]   # > 64 workgroups a plane
    for H, W, k, s, pads, plain, x_grad, w_grad, form in cases:
        pt, pl, pb, pr = pads
        Ho, Wo = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
        rs = np.random.RandomState(3000 + 1000 * k + 100 * s + H + 7 * (pt + 3 * pl + 9 * pb + 27 * pr))
        x, w, gy = _dev(_f32(rs, B, C, H, W)), _dev(_f32(rs, C, 1, k, k) / k), _dev(_f32(rs, B, C, Ho, Wo))
        tag = 'dwconv/%dx%d_k%ds%d_%d%d%d%d%s%s/' % (H, W, k, s, pt, pl, pb, pr, '_plain' if plain else '',
                                                     '' if x_grad and w_grad else '_gx_only' if x_grad else '_gw_only')
        with _Case(res, tag, {form}) as put:
            y = _out(B, C, Ho, Wo)
            gx, gw = _out(B, C, H, W) if x_grad else None, _out(C, 1, k, k) if w_grad else None
            if plain:
                wp, wn = _workspace(L.cnuda_dwconv2d_workspace_bytes(B, C, k))
                hr.check(L.cnuda_dwconv2d_forward(hr.ptr(x), hr.ptr(w), hr.ptr(y), B, C, H, W, k, s, pt, hr.stream()))
                hr.check(L.cnuda_dwconv2d_backward(hr.ptr(x), hr.ptr(w), hr.ptr(gy), hr.ptr(gx), hr.ptr(gw), B, C, H, W, k, s, pt,
                                                   wp, wn, hr.stream()))
            else:
                wp, wn = _workspace(L.cnuda_dwconv2d_same_workspace_bytes(B, C, k))
                hr.check(L.cnuda_dwconv2d_same_forward(hr.ptr(x), hr.ptr(w), hr.ptr(y), B, C, H, W, k, s, pt, pl, Ho, Wo, hr.stream()))
                hr.check(L.cnuda_dwconv2d_same_backward(hr.ptr(x), hr.ptr(w), hr.ptr(gy), hr.ptr(gx), hr.ptr(gw), B, C, H, W, k, s,
                                                        pt, pl, Ho, Wo, wp, wn, hr.stream()))
            put('y', y)
            if x_grad:
                put('grad_x', gx)
            if w_grad:
                put('grad_w', gw)


def _run_dwconvt(res):
    import hip_runtime as hr
    L = hr.lib()
    for form in sorted(DWT_FORWARD_FORMS):
        H, W, k, s, p = DWT_FORWARD_FORMS[form]
        Ho, Wo = (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
        rs = np.random.RandomState(4000 + 100 * k + 10 * s + H)
        x, w, skip = _dev(_f32(rs, B, C, H, W)), _dev(_f32(rs, C, 1, k, k)), _dev(_f32(rs, B, C, Ho, Wo))
        for with_skip in (False, True):
            with _Case(res, 'dwconvt_fwd/%s/%s/' % (form, 'skip' if with_skip else 'plain'), {form}) as put:
                y = _out(B, C, Ho, Wo)
                hr.check(L.cnuda_dwconvt2d_add_forward(hr.ptr(x), hr.ptr(w), hr.ptr(skip if with_skip else None), hr.ptr(y),
                                                       B, C, H, W, k, s, p, hr.stream()))
                put('y', y)
    wsum = 'dwconvt_wsum_kernel'
    generic = {'dwconvt_bwd_data_kernel', 'dwconvt_bwd_weight_kernel'}
    # (H, W, k, s, p, the kernels of the full backward, also with each gradient null): 18 x 20 and 17 x 19 are more than
    # one trip of 256 threads through a plane
    cases = [(18, 20, 4, 2, 1, {'dwconvt_bwd_k4s2_kernel', wsum}, False), (5, 8, 4, 2, 1, {'dwconvt_bwd_k4s2_kernel', wsum}, True),
             (17, 19, 4, 2, 1, {'dwconvt_bwd_kernel<4>', wsum}, False), (5, 7, 4, 2, 1, {'dwconvt_bwd_kernel<4>', wsum}, True),
             (5, 7, 4, 1, 1, {'dwconvt_bwd_kernel<4>', wsum}, False), (5, 7, 8, 4, 2, {'dwconvt_bwd_kernel<8>', wsum}, True),
             (17, 19, 3, 2, 1, generic, False), (5, 7, 3, 2, 1, generic, True), (5, 7, 16, 8, 4, generic, False)]
    for H, W, k, s, p, kernels, frozen in cases:
        Ho, Wo = (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
        rs = np.random.RandomState(5000 + 100 * k + 10 * s + H)
        x, w, gy = _dev(_f32(rs, B, C, H, W)), _dev(_f32(rs, C, 1, k, k)), _dev(_f32(rs, B, C, Ho, Wo))
        for x_grad, w_grad in ((True, True), (True, False), (False, True)) if frozen else ((True, True),):
            tag = 'dwconvt_bwd/%dx%d_k%ds%dp%d%s/' % (H, W, k, s, p, '' if x_grad and w_grad else '_gx_only' if x_grad else '_gw_only')
            with _Case(res, tag, kernels if x_grad and w_grad else ()) as put:
                gx, gw = _out(B, C, H, W) if x_grad else None, _out(C, 1, k, k) if w_grad else None
                wp, wn = _workspace(L.cnuda_dwconvt2d_workspace_bytes(B, C, k))
                hr.check(L.cnuda_dwconvt2d_backward(hr.ptr(x), hr.ptr(w), hr.ptr(gy), hr.ptr(gx), hr.ptr(gw), B, C, H, W, k, s, p,
                                                    wp, wn, hr.stream()))
                if x_grad:
                    put('grad_x', gx)
                if w_grad:
                    put('grad_w', gw)


def _run_addact(res):
    import hip_runtime as hr
    L = hr.lib()
    for n, offset in ((67, False), (67, True), (3, False)):          # 4 q + 3: sixteen quads and a rest of three
        rs = np.random.RandomState(6000 + n + offset)
        a, b = _f32(rs, n), _f32(rs, n)
        yv = _f32(rs, n)
        yv[::5] = 0.0
        yv[1::7] = -0.0
        tag = 'n%d%s/' % (n, '_offset' if offset else '')
        with _Case(res, 'add/' + tag, {'add_kernel'}) as put:
            da, db_, out = _dev(a, offset), _dev(b, offset), _dev(torch.full((n,), FILL), offset)
            hr.check(L.cnuda_add(hr.ptr(da), hr.ptr(db_), hr.ptr(out), n, hr.stream()))
            hr.check(L.cnuda_add(hr.ptr(da), hr.ptr(db_), hr.ptr(da), n, hr.stream()))         # in place: out is a
            put('out', out), put('in_place', da)
        with _Case(res, 'act/' + tag, {'act_bwd_kernel'}) as put:
            dg, dy = _dev(a, offset), _dev(yv, offset)
            for slope in (0.0, 0.2):
                gx = _dev(torch.full((n,), FILL), offset)
                hr.check(L.cnuda_act_backward(hr.ptr(dg), hr.ptr(dy), hr.ptr(gx), n, slope, hr.stream()))
                put('grad_x_slope%g' % slope, gx)


def _run_head(res):
    import hip_runtime as hr
    L = hr.lib()
    Ch, HW = 70, 8                                              # two channel chunks of 35
    for Co in range(1, 9):
        rs = np.random.RandomState(7000 + Co)
        go, w, hid = _f32(rs, B, Co, HW), _f32(rs, Co, Ch), _f32(rs, B, Ch, HW)
        hid.view(-1)[::7] = 0.0
        hid.view(-1)[3::11] = -0.0
        dgo, dw, dhid = _dev(go), _dev(w), _dev(hid)           # (named: they must outlive the launches)
        with _Case(res, 'head/co%d/' % Co, {'conv1x1_dgrad_act_kernel<%d>' % Co}) as put:
            for slope in (0.2, 0.0) if Co in (2, 3) else (0.2,):
                gh = _out(B, Ch, HW)
                hr.check(L.cnuda_conv1x1_backward_data_act(hr.ptr(dgo), hr.ptr(dw), hr.ptr(dhid), hr.ptr(gh), B, Co, Ch, HW, slope,
                                                           hr.stream()))
                put('grad_hidden_slope%g' % slope, gh)


def _run_rows(res):
    import hip_runtime as hr
    L = hr.lib()
    # copy (B, Cn, HW, Csrc, src_off, Cdst, dst_off, offset view); the last has 65,540 rows: row += gridDim.y
    for Bc, Cn, HW, Csrc, so, Cdst, do, offset in ((2, 3, 16, 5, 1, 7, 2, False), (2, 3, 15, 5, 1, 7, 2, False),
                                                   (2, 3, 16, 5, 1, 7, 2, True), (2, 32770, 4, 32771, 1, 32773, 2, False)):
        rs = np.random.RandomState(8000 + HW + offset + Cn)
        with _Case(res, 'copy/%dx%dx%d%s/' % (Bc, Cn, HW, '_offset' if offset else ''), {'copy_channels_kernel'}) as put:
            src, dst = _dev(_f32(rs, Bc, Csrc, HW), offset), _dev(torch.full((Bc, Cdst, HW), FILL), offset)
            hr.check(L.cnuda_copy_channels(hr.ptr(src), hr.ptr(dst), Bc, Cn, HW, Csrc, so, Cdst, do, hr.stream()))
            put('dst', dst)
    # split (B, taps, HW, offset views); the last has 65,610 rows
    for Bs, T, HW, offset in ((2, 2, 16, False), (2, 2, 15, False), (2, 2, 16, True), (2430, 9, 4, False)):
        rs = np.random.RandomState(9000 + HW + offset + T)
        om, go, gm = _f32(rs, Bs, 3 * T, HW) * 3, _f32(rs, Bs, 2 * T, HW), _f32(rs, Bs, T, HW)
        with _Case(res, 'split/%dx%dx%d%s/' % (Bs, T, HW, '_offset' if offset else ''),
                   {'split_offset_mask_kernel', 'split_offset_mask_bwd_kernel'}) as put:
            dom, dgo, dgm = _dev(om, offset), _dev(go, offset), _dev(gm, offset)
            off, mask = _dev(torch.full((Bs, 2 * T, HW), FILL), offset), _dev(torch.full((Bs, T, HW), FILL), offset)
            gom = _dev(torch.full((Bs, 3 * T, HW), FILL), offset)
            hr.check(L.cnuda_split_offset_mask(hr.ptr(dom), hr.ptr(off), hr.ptr(mask), Bs, T, HW, hr.stream()))
            hr.check(L.cnuda_split_offset_mask_backward(hr.ptr(dgo), hr.ptr(dgm), hr.ptr(mask), hr.ptr(gom), Bs, T, HW, hr.stream()))
            put('offset', off), put('mask', mask), put('grad_om', gom)


_RUN = {'pool': _run_pool, 'winpool': _run_winpool, 'dwconv': _run_dwconv, 'dwconvt': _run_dwconvt, 'addact': _run_addact,
        'head': _run_head, 'rows': _run_rows}
_PREFIXES = {'pool': ('pool/',), 'winpool': ('winpool/',), 'dwconv': ('dwconv/',), 'dwconvt': ('dwconvt_fwd/', 'dwconvt_bwd/'),
             'addact': ('add/', 'act/'), 'head': ('head/',), 'rows': ('copy/', 'split/')}


def run_all(families=FAMILIES):
    """Builds every input from seeded RandomStates and runs every case of `families` -> {name: array}"""
    res = {}
    for family in families:
        _RUN[family](res)
    torch.cuda.synchronize()
    return res


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.int32), b.view(np.int32)) if a.dtype == np.float32 else np.array_equal(a, b)


@pytest.mark.parametrize('family', FAMILIES)
def test_spatial_bits_are_those_of_the_recording(family):
    want = np.load(FIXTURE, allow_pickle=False)
    keys = sorted(k for k in want.files if k.startswith(_PREFIXES[family]))
    got = run_all((family,))
    assert keys and sorted(got) == keys, (sorted(set(got) ^ set(keys)))
    differ = [k for k in keys if not _same_bits(got[k], want[k])]
    assert not differ, ('%d of %d arrays differ in bits from the recording (%s): %s'
                        % (len(differ), len(keys), str(want['recorded_with']), differ))


def test_pool_cases_hold_ties_and_a_nan_per_plane():
    """What the max-pool pins are for: every plane's NaN reaches its window's output, and the accumulate form leaves
    exactly one cell per window changed"""
    got = run_all(('pool', 'winpool'))
    for tag, windows in (('pool/8x8_k2/', 16), ('pool/7x9_k2/', 12), ('pool/9x9_k3/', 9), ('pool/8x8_k2_offset/', 16)):
        y, gx = got[tag + 'y'], got[tag + 'grad_x']
        assert (np.isnan(y).reshape(B * C, -1).sum(1) == 1).all(), tag
        assert (np.count_nonzero(gx.reshape(B * C, -1), axis=1) == windows).all() and not (gx == FILL).any(), tag
    for tag in ('winpool/7x9_k3s2p1/', 'winpool/5x6_k2s1p1/'):
        assert (np.isnan(got[tag + 'y']).reshape(B * C, -1).sum(1) >= 1).all() and not (got[tag + 'grad_x'] == FILL).any(), tag
