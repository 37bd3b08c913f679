"""MI355X parity of the dense building blocks (implicit-GEMM conv, fused BN,
pooling, depthwise transposed conv, concat/add, Adam) against the CPU torch
primitives the oracle (oracle/dla.py) is made of.  fp32 tolerance 1e-4 of the
tensor's scale (north_star)."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4


def _close(a, b, tol=TOL):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert err <= tol * scale, (err, scale)


CONV_CASES = {
    # name: B, C, H, W, Co, k, s, p, bias, act
    'stem7x7': (2, 3, 20, 24, 16, 7, 1, 3, False, -1.0),
    'c16_3x3': (2, 16, 16, 16, 16, 3, 1, 1, False, -1.0),
    'c16_s2': (2, 16, 17, 15, 32, 3, 2, 1, False, -1.0),
    'c64_3x3': (1, 64, 12, 12, 64, 3, 1, 1, False, -1.0),
    'root1x1': (2, 320, 6, 6, 128, 1, 1, 0, False, -1.0),
    'offset27': (2, 64, 9, 9, 27, 3, 1, 1, True, -1.0),
    'head_relu': (2, 64, 8, 8, 256, 3, 1, 1, True, 0.0),
    'head_out': (2, 256, 8, 8, 6, 1, 1, 0, True, -1.0),
    'disc4x4': (2, 6, 16, 16, 64, 4, 2, 1, True, 0.2),
    'disc_last': (2, 512, 4, 4, 1, 4, 2, 1, True, -1.0),
    'odd': (3, 20, 7, 9, 37, 3, 1, 1, True, -1.0),
    'c512': (1, 256, 4, 4, 512, 3, 2, 1, False, -1.0),
    's2_even': (2, 32, 16, 12, 64, 3, 2, 1, False, -1.0),       # parity-class input gradient
    's2_k1': (2, 16, 8, 8, 32, 1, 2, 0, False, -1.0),           # 1x1 stride 2: three of four classes get zero
    'c16_wgrad16': (2, 16, 12, 12, 48, 3, 1, 1, False, -1.0),   # C % 16 == 0 wgrad path
    # C % 16 != 0 at sizes that select the 8-wave 64-row tile with the generic im2col loader -- what configs[4]'s
    # discriminator (first layer: 6 entropy-map channels, 4x4 stride 2) and configs[0]'s ResNet stem (3 -> 64, 7x7
    # stride 2) run at full size (tests/kernel_manifest.py: igemm_fwd_ws_kernel<64, ConvFwdLoader<false>, 16>)
    'disc4x4_full': (2, 6, 256, 256, 64, 4, 2, 1, True, 0.2),
    'resnet_stem_full': (2, 3, 256, 256, 64, 7, 2, 3, False, -1.0),
    # the DCN offset / mask convolutions (C -> 27, 3x3) at map widths 128 / 64 / 32 / 16: their weight gradient runs on
    # halo tiles (hwgrad_kernel<W>: 256-pixel tiles of full rows); `_b8`: four tiles per workgroup (the prefetch loop),
    # `w16`: a tile is a whole image and fewer than 27 output channels
    'offset27_w128': (2, 64, 128, 128, 27, 3, 1, 1, True, -1.0),
    'offset27_w128_b8': (8, 64, 128, 128, 27, 3, 1, 1, True, -1.0),
    'offset27_w64': (2, 128, 64, 64, 27, 3, 1, 1, True, -1.0),
    'offset27_w32': (3, 48, 32, 32, 27, 3, 1, 1, True, -1.0),
    'offset18_w16': (5, 32, 16, 16, 18, 3, 1, 1, False, -1.0),
    'offset27_24x64': (3, 32, 24, 64, 27, 3, 1, 1, True, -1.0),      # H != W: six 4-row tiles per image
    # DLA-34's level1 shape class (16 -> 32, 3x3 stride 2) at output widths that are multiples of 128: its weight gradient runs
    # on parity-split halo tiles (hwgrad_s2_kernel); two tiles per output row, several tiles per workgroup, a bias, and
    # (l2_*) the 32 -> 64 shape of level2's first convolution
    'l1_s2_w256': (2, 16, 64, 512, 32, 3, 2, 1, False, -1.0),
    'l1_s2_w128_b': (3, 32, 48, 256, 24, 3, 2, 1, True, -1.0),
    'l1_s2_many': (9, 16, 128, 256, 32, 3, 2, 1, False, -1.0),
    'l2_s2_co64': (2, 32, 32, 256, 64, 3, 2, 1, False, -1.0),        # 33..64 output channels: two 32-row blocks
    'l2_s2_co48_b': (2, 16, 16, 256, 48, 3, 2, 1, True, -1.0),
    # round 6: the same two kernels on the map widths of a 640 x 640 input (160 / 80 / 40; 96 as the odd case) -- the tile is a
    # rectangle of TR rows x TW columns, TW the largest power of two dividing the width (hwgrad_kernel<TW, side>: 5 x 32,
    # 5 x 16, 5 x 8, 3 x 32), `rag`: the last tile row hangs over the image, `w256`: 128-column tiles with neighbours;
    # `l1_s2_w320`: stride 2 to a 320-wide map, the third 128-pixel tile of a row half empty
    'offset27_w160': (2, 64, 160, 160, 27, 3, 1, 1, True, -1.0),
    'offset27_w160_rag': (1, 32, 36, 160, 27, 3, 1, 1, True, -1.0),
    'offset27_w80': (2, 128, 80, 80, 27, 3, 1, 1, True, -1.0),
    'offset27_w96': (1, 32, 96, 96, 27, 3, 1, 1, False, -1.0),
    'offset27_w40': (3, 32, 64, 40, 27, 3, 1, 1, True, -1.0),
    'offset27_w256': (1, 16, 8, 256, 27, 3, 1, 1, True, -1.0),
    'offset27_w192': (1, 16, 12, 192, 20, 3, 1, 1, True, -1.0),
    'l1_s2_w320': (1, 16, 16, 640, 32, 3, 2, 1, True, -1.0),
    # round 6, split-K (igemm_fwd_*splitk_kernel + splitk_reduce_kernel): few pixel x row tiles, long K -- the ADVENT
    # discriminator's 4 x 4 / stride 2 layers on 20 x 20 and 10 x 10 maps (forward on the 128-row tile, parity-class input
    # gradient), the 512 -> 27 offset convolution of the 16 x 16 level (32-row tile), a 3 x 3 with 64 input rows (64-row tile)
    'sk_disc_256to512': (4, 256, 20, 20, 512, 4, 2, 1, True, 0.2),
    'sk_disc_128to256': (4, 128, 40, 40, 256, 4, 2, 1, True, 0.2),
    'sk_512to27_16sq': (8, 512, 16, 16, 27, 3, 1, 1, True, -1.0),
    'sk_256to64_8sq': (3, 256, 8, 8, 64, 3, 1, 1, False, 0.0),
    # stride 2 with 256 outputs on a 16 x 16 input: the 4-tap parity class of the input gradient (K = 1,024) cuts K, the 1- and
    # 2-tap classes (K = 256 / 512 < 32 chunks... / = 32) do not -- one launch per class (igemm_fwd_kernel<32, ConvDgradClassBufLoader>
    # beside the split-K instance), as in the ResNet-18 step of configs[0]
    'sk_s2_mixed': (2, 64, 16, 16, 256, 3, 2, 1, False, -1.0),
}


@pytest.mark.parametrize('name', sorted(CONV_CASES))
def test_conv2d_fwd_bwd(name):
    from hip_runtime import ops
    B, C, H, W, Co, k, s, p, bias, act = CONV_CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    x = torch.randn(B, C, H, W, generator=g, requires_grad=True)
    w = (torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5).requires_grad_(True)
    b = torch.randn(Co, generator=g).requires_grad_(True) if bias else None
    y = F.conv2d(x, w, b, s, p)
    if act >= 0:
        y = F.leaky_relu(y, act)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    dx, dw = x.detach().to(DEV).requires_grad_(True), w.detach().to(DEV).requires_grad_(True)
    db = b.detach().to(DEV).requires_grad_(True) if bias else None
    dy = ops.conv2d(dx, dw, db, s, p, act)
    _close(dy, y)
    dy.backward(gy.to(DEV))
    _close(dx.grad, x.grad)
    _close(dw.grad, w.grad)
    if bias:
        _close(db.grad, b.grad)


@pytest.mark.parametrize('name', ['sk_disc_256to512', 'sk_512to27_16sq', 'sk_256to64_8sq'])
def test_split_k_takes_the_starved_long_k_convolutions(name):
    """The `sk_*` cases of test_conv2d_fwd_bwd hold the values; here: the launch plan really cuts K for them (forward and
    input gradient), `hr.splitk(0)` restores pick_bm's small-tile plan, and the two plans agree to summation order."""
    import hip_runtime as hr
    from hip_runtime import ops
    from test_zz_kernel_coverage import short
    B, C, H, W, Co, k, s, p, bias, act = CONV_CASES[name]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5).to(DEV)
    gy = None
    res = []
    for max_tiles in (128, 0):
        xx, ww = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        with hr.splitk(max_tiles), hr.launch_log() as log:
            y = ops.conv2d(xx, ww, None, s, p, act)
            gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(DEV) if gy is None else gy
            y.backward(gy)
        names = sorted(short(n) for n in log.names)
        print(max_tiles, names)
        if hr.get_matrix_mode() == 0 and os.environ.get('CNUDA_SPLITK') != '0' and os.environ.get('CNUDA_BUF') != '0':
            assert any('splitk_kernel' in n for n in names) == (max_tiles > 0), names
            assert any(n.startswith('splitk_reduce_kernel') for n in names) == (max_tiles > 0), names
        res.append((y.detach(), xx.grad, ww.grad))
    for a, b in zip(*res):
        _close(a, b, 2e-5)


# (B, H, W, source channels, Cout): DLA-34's Root shapes (backends/dla.py Tree: level 2 .. 5) at sizes the CPU finishes
CAT_CASES = {
    'level2_64_64': (4, 32, 32, (64, 64), 64),                      # 128-row... M = 64: the 64-row tile
    'level3_four_sources': (4, 16, 32, (128, 128, 64, 128), 128),   # a level root: x2, x1, the pooled input, tree1's output
    'level4_three_sources': (16, 16, 32, (256, 256, 128), 256),     # (enough pixel tiles that the plan does not cut K)
    'level5_four_m_tiles': (32, 16, 16, (512, 512, 256), 512),
    'ragged_pixels': (3, 6, 10, (64, 128), 192),                    # 180 pixels: the last pixel tile is partial
    'level3_128_row_tiles': (16, 64, 64, (128, 128, 64, 128), 128), # enough pixels for the 128-row forward / input-gradient tiles
}


@pytest.mark.parametrize('name', sorted(CAT_CASES))
def test_conv1x1_over_a_concatenation_without_the_concatenation(name):
    """ops.conv1x1_cat (round 6, DLA's Root): y, the BatchNorm statistics, every source's input gradient and the weight
    gradient hold the SAME BITS as conv2d(cat(xs)) -- the same GEMMs in the same order, only the gather / the store switch
    tensors -- and the values are torch's CPU results.  Source 1 has a second consumer: its share of the gradient is in the
    fan-in slot when the input-gradient epilogue runs and must be added there."""
    import hip_runtime as hr
    from hip_runtime import ops
    from hip_runtime.fanout import fork
    from test_zz_kernel_coverage import short
    B, H, W, cs, Co = CAT_CASES[name]
    if hr.get_matrix_mode() != 0:
        pytest.skip('the concatenation-free kernels are f32-matrix-mode only: Root concatenates in mode 1')
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)
    xs = [torch.randn(B, c, H, W, generator=g) for c in cs]
    w = torch.randn(Co, sum(cs), 1, 1, generator=g) / sum(cs) ** 0.5
    gy = torch.randn(B, Co, H, W, generator=g)
    side = torch.randn(B, cs[1], H, W, generator=g)
    # CPU reference
    rx = [t.clone().requires_grad_(True) for t in xs]
    rw = w.clone().requires_grad_(True)
    ry = F.conv2d(torch.cat(rx, 1), rw)
    (ry * gy).sum().backward(retain_graph=True)
    (rx[1] * side).sum().backward()
    res = []
    for fused in (True, False):
        dx = [t.to(DEV).requires_grad_(True) for t in xs]
        dw = w.to(DEV).requires_grad_(True)
        a, b2 = fork(dx[1], 2)                       # source 1: the convolution and an elementwise consumer
        srcs = [dx[0], a] + dx[2:]
        with hr.launch_log() as log:
            if fused:
                y = ops.conv1x1_cat(srcs, dw, 0, emit_stats=True)
                assert y is not None, 'cnuda_conv2d_cat_supported refused %s' % name
            else:
                y = ops.conv2d(ops.cat_channels(srcs), dw, None, 1, 0, -1.0, 0, emit_stats=True)
            stats = getattr(y, '_cnuda_bn_stats', None)
            ((b2 * side.to(DEV)).sum() + (y * gy.to(DEV)).sum()).backward()
        names = sorted(short(n) for n in log.names)
        print(fused, names)
        if fused:
            assert not any(n.startswith('copy_channels') for n in names), names
            for frag in ('ConvFwdCatLoader', 'ConvDgradCatLoader', 'ConvWCatLoader'):
                assert any(frag in n for n in names), (frag, names)
        res.append((y.detach(), None if stats is None else stats[0], dw.grad) + tuple(t.grad for t in dx))
    fused, plain = res
    assert fused[1] is not None and plain[1] is not None
    for i, (u, v) in enumerate(zip(fused, plain)):
        if i == 4:                                   # (source 1: its two shares are added in another order)
            _close(u, v, 1e-6)
        else:
            assert torch.equal(u, v), i
    _close(fused[0], ry.detach())
    _close(fused[2], rw.grad)
    for u, r in zip(fused[3:], rx):
        _close(u, r.grad)


@pytest.mark.parametrize('name', ['level2_64_64', 'level3_four_sources', 'ragged_pixels'])
def test_conv1x1_cat_inference_form_with_bias_and_relu(name):
    """The BatchNorm-folded Root (export.py): act(conv1x1(cat(xs)) + bias) in one launch, the same bits as the concatenated form."""
    import hip_runtime as hr
    from hip_runtime import ops
    B, H, W, cs, Co = CAT_CASES[name]
    if hr.get_matrix_mode() != 0:
        pytest.skip('the concatenation-free kernels are f32-matrix-mode only: Root concatenates in mode 1')
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(B, c, H, W, generator=g).to(DEV) for c in cs]
    w = (torch.randn(Co, sum(cs), 1, 1, generator=g) / sum(cs) ** 0.5).to(DEV)
    b = torch.randn(Co, generator=g).to(DEV)
    got = ops.conv1x1_cat_infer(xs, w, b, 0.0)
    assert got is not None
    want = ops.conv2d_infer(ops.cat_channels(xs), w, b, 1, 0, 0.0)
    assert torch.equal(got, want)
    _close(got, F.relu(F.conv2d(torch.cat([t.cpu() for t in xs], 1), w.cpu(), b.cpu())))


def test_conv1x1_cat_declines_what_no_kernel_takes():
    from hip_runtime import ops
    w = torch.randn(64, 96, 1, 1, device=DEV)
    assert ops.conv1x1_cat([torch.randn(2, 64, 8, 8, device=DEV), torch.randn(2, 32, 8, 8, device=DEV)], w) is None       # 32 channels
    w = torch.randn(64, 128, 1, 1, device=DEV)
    assert ops.conv1x1_cat([torch.randn(2, 64, 3, 3, device=DEV), torch.randn(2, 64, 3, 3, device=DEV)], w) is None       # 9 pixels per image
    assert ops.conv1x1_cat([torch.randn(2, 128, 8, 8, device=DEV)], w) is None                                            # one source


# (B, K = input channels, H, W, rows = output channels): the DCN column-gradient GEMM's shapes -- 9 C rows over K = Cout
ROWQUAD_CASES = {
    # (sizes: pick_bm keeps the 128-row tile only with >= 512 tiles, the 64-row tile with >= 256)
    'shortk_64to576': (4, 64, 64, 64, 576),          # igemm_fwd_shortk_kernel (K = 64, 4.5 row tiles: the 64-row tail tile too)
    'ws128_128to1152': (2, 128, 64, 64, 1152),       # igemm_fwd_ws_kernel<128>
    'ws64_256to576': (1, 256, 64, 64, 576),          # 32 pixel tiles: the 64-row tile
    'rows36_ragged': (1, 32, 5, 7, 36),              # 35 pixels (no multiple of 4), 36 rows: the 32-row tile's bounds
    'k1_rows144': (3, 16, 6, 10, 144),
}


@pytest.mark.parametrize('name', sorted(ROWQUAD_CASES))
def test_conv2d_forward_with_quad_interleaved_output_rows(name):
    """cnuda_conv2d_forward_rowquads (round 6: the layout of the DCN column gradient): y[b][m / 4][pixel][4] holds the SAME
    bits as cnuda_conv2d_forward's y[b][m][pixel] -- same GEMM, same accumulation order, another epilogue -- and the values
    are those of torch's CPU convolution."""
    import hip_runtime as hr
    from hip_runtime import ops
    from test_zz_kernel_coverage import short
    B, K, H, W, M = ROWQUAD_CASES[name]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, K, H, W, generator=g)
    w = torch.randn(M, K, 1, 1, generator=g) / K ** 0.5
    want = F.conv2d(x, w)
    xd, wd = x.to(DEV), w.to(DEV)
    L = hr.lib()
    geom = (B, K, H, W, M, 1, 1, 1, 1, 0, 0)
    assert L.cnuda_conv2d_rowquads_supported(*geom) == (0 if os.environ.get('CNUDA_BUF') == '0' else 1)
    if not L.cnuda_conv2d_rowquads_supported(*geom):
        pytest.skip('no buffer addressing: the plain layout is what runs')
    nbytes = L.cnuda_conv2d_workspace_bytes(*geom)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    plain = torch.full((B, M, H, W), float('nan'), device=DEV)
    quads = torch.full((B, M // 4, H * W, 4), float('nan'), device=DEV)
    hr.check(L.cnuda_conv2d_forward(hr.ptr(xd), hr.ptr(wd), None, hr.ptr(plain), *geom, -1.0, hr.ptr(ws), nbytes, hr.stream()))
    with hr.launch_log() as log:
        hr.check(L.cnuda_conv2d_forward_rowquads(hr.ptr(xd), hr.ptr(wd), hr.ptr(quads), *geom, hr.ptr(ws), nbytes, hr.stream()))
    torch.cuda.synchronize()
    print(sorted(short(n) for n in log.names))
    assert any('ConvFwdBufQuadLoader' in n for n in log.names), log.names
    back = quads.permute(0, 1, 3, 2).reshape(B, M, H, W)           # [b][q][p][r] -> [b][4 q + r][p]
    assert torch.equal(back, plain)
    _close(back, want)
    # and an unsupported geometry is refused, not written in another layout
    assert L.cnuda_conv2d_rowquads_supported(B, K, H, W, M + 2, 1, 1, 1, 1, 0, 0) == 0


def test_short_k_kernel_stores_a_plane_that_is_no_multiple_of_four_pixels():
    """igemm_fwd_shortk_kernel's one-dword-per-lane epilogue, for its full 128-row tiles and for the 64-row tail tile
    (576 rows = 4.5 tiles): a 63 x 65 plane is no multiple of four pixels, so Out::vec4_ok refuses the 16-byte stores
    that every other short-K case (64 x 64 planes, row quads) leaves through.  128 pixel tiles x 5 row tiles keep the
    128-row tile (pick_bm: >= 512 tiles); the last pixel tile is partial (16,380 pixels).  Values: the convolution
    restated in fp64."""
    import hip_runtime as hr
    from hip_runtime import ops
    from test_zz_kernel_coverage import short
    B, K, H, W, M = 4, 64, 63, 65, 576
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, K, H, W, generator=g)
    w = torch.randn(M, K, 1, 1, generator=g) / K ** 0.5
    want = F.conv2d(x.double(), w.double())
    with hr.launch_log() as log, torch.no_grad():
        got = ops.conv2d(x.to(DEV), w.to(DEV), None, 1, 0, -1.0)
    names = sorted(short(n) for n in log.names)
    print(names)
    if hr.get_matrix_mode() == 0 and os.environ.get('CNUDA_SHORTK') != '0':
        assert any(n.startswith('igemm_fwd_shortk_kernel<128, ConvFwd') for n in names), names
    _close(got, want)


@pytest.mark.parametrize('relu,res', [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize('shape', [(2, 16, 10, 12), (3, 5, 7, 7), (1, 64, 2, 2), (16, 512, 4, 4)])   # (last: 4 images per workgroup)
def test_batch_norm_train_fwd_bwd_and_running_stats(shape, relu, res):
    from hip_runtime import ops
    g = torch.Generator().manual_seed(3)
    B, C, H, W = shape
    x = (torch.randn(shape, generator=g) * 2 + 0.5).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g)).requires_grad_(True)
    r = torch.randn(shape, generator=g).requires_grad_(True) if res else None
    rm, rv = torch.randn(C, generator=g) * 0.1, 1 + 0.3 * torch.rand(C, generator=g)
    rm_d, rv_d = rm.clone().to(DEV), rv.clone().to(DEV)
    y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    gy = torch.randn(shape, generator=g)
    y.backward(gy)
    leaves = [t.detach().to(DEV).requires_grad_(True) for t in (x, gamma, beta)]
    dr = r.detach().to(DEV).requires_grad_(True) if res else None
    dy = ops.batch_norm_act(leaves[0], leaves[1], leaves[2], rm_d, rv_d, True, 0.1, 1e-5, dr, relu)
    _close(dy, y)
    dy.backward(gy.to(DEV))
    _close(leaves[0].grad, x.grad)
    _close(leaves[1].grad, gamma.grad)
    _close(leaves[2].grad, beta.grad)
    if res:
        _close(dr.grad, r.grad)
    _close(rm_d, rm, 1e-6)
    _close(rv_d, rv, 1e-6)


@pytest.mark.parametrize('shape,relu', [((4, 16, 8, 12), True), ((2, 5, 7, 9), True), ((3, 8, 16, 16), 'relu6'),
                                        ((2, 32, 64, 64), True), ((16, 512, 4, 4), True)])
def test_batch_norm_backward_gate_recomputed_from_x_is_the_gate_read_from_y(shape, relu):
    """Without a residual the backward passes recompute the activation's gate from x (the forward's own multiply and
    add) instead of reading y: every output must be bit-identical to the y-reading form of the same entry point."""
    import hip_runtime as hr
    L = hr.lib()
    g = torch.Generator().manual_seed(21)
    B, C, H, W = shape
    HW = H * W
    x = (torch.randn(shape, generator=g) * 2 + 0.3).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.5).to(DEV)
    gy = torch.randn(shape, generator=g).to(DEV)
    code = 2 if relu == 'relu6' else 1
    for groups in (1, 2) if B % 2 == 0 else (1,):
        y = torch.empty_like(x)
        mean, invstd = torch.empty(groups * C, device=DEV), torch.empty(groups * C, device=DEV)
        ws = hr.workspace(L.cnuda_bn_workspace_bytes(B, C, HW), x.device)
        hr.check(L.cnuda_bn_train_forward(hr.ptr(x), hr.ptr(gamma), hr.ptr(beta), None, hr.ptr(y), hr.ptr(mean),
                                          hr.ptr(invstd), None, None, None, 0.1, 1e-5, code, B, C, HW, groups, hr.ptr(ws),
                                          ws.numel(), hr.stream()), 'bn_train_forward')
        assert (y == 0).float().mean().item() > 0.1            # the gate matters
        outs = []
        for regate in (False, True):
            gx, gg, gb = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            hr.check(L.cnuda_bn_backward(hr.ptr(gy), hr.ptr(x), None if regate else hr.ptr(y), hr.ptr(gamma),
                                         hr.ptr(beta) if regate else None, hr.ptr(mean), hr.ptr(invstd), hr.ptr(gx), None,
                                         hr.ptr(gg), hr.ptr(gb), code, B, C, HW, groups, hr.ptr(ws), ws.numel(),
                                         hr.stream()), 'bn_backward')
            outs.append((gx, gg, gb))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match='residual'):
        hr.check(L.cnuda_bn_backward(hr.ptr(gy), hr.ptr(x), hr.ptr(y), hr.ptr(gamma), hr.ptr(beta), hr.ptr(mean),
                                     hr.ptr(invstd), hr.ptr(gx), hr.ptr(torch.empty_like(x)), hr.ptr(gg), hr.ptr(gb), code,
                                     B, C, HW, 1, hr.ptr(ws), ws.numel(), hr.stream()), 'bn_backward')


def test_batch_norm_eval_and_single_value_error():
    from hip_runtime import ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 8, 5, 5, generator=g)
    gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    rm, rv = torch.randn(8, generator=g), torch.rand(8, generator=g) + 0.5
    want = F.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5))
    with torch.no_grad():
        got = ops.batch_norm_act(x.to(DEV), gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), False, relu=True)
    _close(got, want)
    with pytest.raises(RuntimeError):       # nn.BatchNorm2d refuses one value per channel in training
        ops.batch_norm_act(torch.zeros(1, 4, 1, 1, device=DEV), gamma[:4].to(DEV), beta[:4].to(DEV),
                           rm[:4].to(DEV), rv[:4].to(DEV), True)


@pytest.mark.parametrize('ties', [False, True], ids=['distinct', 'ties_and_nan'])
@pytest.mark.parametrize('shape,k', [((2, 5, 8, 12), 2), ((1, 3, 9, 7), 2), ((2, 4, 12, 12), 4), ((3, 4, 16, 32), 2), ((1, 2, 6, 10), 2)])
def test_maxpool(shape, k, ties):
    """(W % 4 == 0 and H even with k = 2: the 16-byte kernels of round 6; else the scalar ones.)  ties_and_nan: values on a
    grid of halves -- most windows hold their maximum more than once: the FIRST in scan order takes the gradient -- and a few
    NaN, which win their window (ATen's rule)."""
    from hip_runtime import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g)
    if ties:
        x = torch.round(x * 2) / 2
        x.view(-1)[torch.randperm(x.numel(), generator=g)[:5]] = float('nan')
    x.requires_grad_(True)
    y = F.max_pool2d(x, k, k)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    dx = x.detach().to(DEV).requires_grad_(True)
    dy = ops.max_pool2d(dx, k)
    assert torch.equal(dy.cpu().nan_to_num(nan=1e30), y.detach().nan_to_num(nan=1e30))
    dy.backward(gy.to(DEV))
    assert torch.equal(dx.grad.cpu(), x.grad)


@pytest.mark.parametrize('shape', [(2, 3, 8, 16), (1, 2, 5, 7)], ids=['vector', 'scalar'])
def test_maxpool_backward_accumulates_into_a_held_gradient(shape):
    """cnuda_maxpool2d_backward_acc(accumulate = 1) (hip_runtime.fanout: the pooled tensor has another consumer whose share is
    already in the buffer): held + the plain backward, in both kernel forms."""
    import hip_runtime as hr
    g = torch.Generator().manual_seed(9)
    B, C, H, W = shape
    x = torch.randn(shape, generator=g).to(DEV)
    gy = torch.randn(B, C, H // 2, W // 2, generator=g).to(DEV)
    held = torch.randn(shape, generator=g).to(DEV)
    plain = torch.full(shape, float('nan'), device=DEV)
    L = hr.lib()
    hr.check(L.cnuda_maxpool2d_backward_acc(hr.ptr(x), hr.ptr(gy), hr.ptr(plain), 0, B, C, H, W, 2, hr.stream()))
    acc = held.clone()
    hr.check(L.cnuda_maxpool2d_backward_acc(hr.ptr(x), hr.ptr(gy), hr.ptr(acc), 1, B, C, H, W, 2, hr.stream()))
    assert torch.equal(acc, held + plain)


@pytest.mark.parametrize('C,H,W,f', [(8, 5, 6, 2), (64, 4, 4, 4), (3, 3, 5, 8), (4, 3, 5, 2), (16, 32, 32, 2), (16, 16, 16, 4),
                                     (4, 34, 36, 2), (4, 33, 36, 2), (5, 64, 32, 2), (3, 32, 34, 2)])
def test_depthwise_conv_transpose(C, H, W, f):
    from hip_runtime import ops
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, C, H, W, generator=g).requires_grad_(True)
    w = torch.randn(C, 1, 2 * f, 2 * f, generator=g).requires_grad_(True)
    y = F.conv_transpose2d(x, w, None, stride=f, padding=f // 2, groups=C)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    dx, dw = x.detach().to(DEV).requires_grad_(True), w.detach().to(DEV).requires_grad_(True)
    dy = ops.depthwise_conv_transpose2d(dx, dw, f, f // 2)
    _close(dy, y, 1e-5)
    dy.backward(gy.to(DEV))
    _close(dx.grad, x.grad, 1e-5)
    _close(dw.grad, w.grad)


@pytest.mark.parametrize('C,H,W,f', [(8, 5, 6, 2), (3, 3, 5, 8), (16, 32, 32, 2), (16, 16, 16, 4)])
def test_depthwise_conv_transpose_with_summand_is_the_separate_add(C, H, W, f):
    """IDAUp's `up(project(x)) + layers[i-1]` in one pass: bit-identical to the operator followed by ops.add, and
    the summand's gradient is the incoming gradient itself."""
    from hip_runtime import ops
    g = torch.Generator().manual_seed(16)
    x = torch.randn(2, C, H, W, generator=g).to(DEV)
    w = torch.randn(C, 1, 2 * f, 2 * f, generator=g).to(DEV)
    skip = torch.randn(2, C, H * f, W * f, generator=g).to(DEV)
    gy = torch.randn(2, C, H * f, W * f, generator=g).to(DEV)
    ref_in = [t.clone().requires_grad_(True) for t in (x, w, skip)]
    ref = ops.add(ops.depthwise_conv_transpose2d(ref_in[0], ref_in[1], f, f // 2), ref_in[2])
    ref.backward(gy)
    got_in = [t.clone().requires_grad_(True) for t in (x, w, skip)]
    got = ops.depthwise_conv_transpose2d(got_in[0], got_in[1], f, f // 2, got_in[2])
    assert torch.equal(got, ref)
    got.backward(gy)
    for a, b in zip(got_in, ref_in):
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(got_in[2].grad, gy)
    with pytest.raises(RuntimeError, match='summand'):
        ops.depthwise_conv_transpose2d(x, w, f, f // 2, skip[:, :, 1:])


@pytest.mark.parametrize('B,C,Ch,Co,H,W,k', [(2, 16, 32, 6, 8, 12, 3), (3, 64, 256, 2, 16, 16, 3), (1, 16, 48, 8, 6, 10, 1),
                                            (2, 32, 64, 1, 4, 8, 3)])
def test_head_pair_is_one_tape_node_with_the_two_layers_values(B, C, Ch, Co, H, W, k):
    """hnn.Head = Conv2d + ReLU + Conv2d(.., 1): forward bit-identical to the two layers run in turn; the hidden
    map's gradient (1x1 input gradient x ReLU gradient in one pass, channels summed in order) and everything behind
    it within 1e-5 of the unfused tape and of torch's own conv2d."""
    import hip_runtime.nn as hnn
    torch.manual_seed(40 + Co)
    head = hnn.Head(hnn.Conv2d(C, Ch, k, padding=k // 2, bias=True, act_slope=0.0), hnn.Slot(),
                    hnn.Conv2d(Ch, Co, 1, bias=True)).to(DEV)
    x = torch.randn(B, C, H, W, device=DEV)
    gy = torch.randn(B, Co, H, W, device=DEV)
    xa = x.clone().requires_grad_(True)
    ya = head(xa)
    assert type(ya.grad_fn).__name__.startswith('_ConvActConv1x1')
    ya.backward(gy)
    fused = [xa.grad.clone()] + [p.grad.clone() for p in head.parameters()]
    for p in head.parameters():
        p.grad = None
    xb = x.clone().requires_grad_(True)
    yb = head[2](head[0](xb))                                  # the two _Conv2d nodes
    assert torch.equal(ya, yb)
    yb.backward(gy)
    unfused = [xb.grad] + [p.grad for p in head.parameters()]
    xr = x.detach().cpu().requires_grad_(True)
    ps = [p.detach().cpu().requires_grad_(True) for p in head.parameters()]
    # The ReLU's gate is a discontinuity: a hidden value within rounding noise of zero may pass on one side and not on the
    # other (a different summation order -- split-K since round 6 -- moves one of the 196,608 values of the 64 -> 256 case
    # across).  The reference therefore takes the gate from the HIP hidden map, after checking that the two gates differ
    # only where the pre-activation is zero to 1e-5.
    pre = F.conv2d(xr, ps[0], ps[1], padding=k // 2)
    with torch.no_grad():
        gate = (head[0](x) > 0).cpu()
        differ = gate != (pre > 0)
        assert int(differ.sum()) <= 4 and (pre[differ].abs() < 1e-5).all(), (int(differ.sum()), pre[differ])
    yr = F.conv2d(pre * gate, ps[2], ps[3])
    yr.backward(gy.cpu())
    for a, b, r in zip(fused, unfused, [xr.grad] + [p.grad for p in ps]):
        _close(a, b, 1e-5)
        _close(a, r, 1e-4)
    with torch.no_grad():                                      # no tape: the layers run in turn
        assert torch.equal(head(x), ya)
    # 9 outputs, odd planes: the fused node does not apply and the module still works
    wide = hnn.Head(hnn.Conv2d(C, Ch, k, padding=k // 2, act_slope=0.0), hnn.Slot(), hnn.Conv2d(Ch, 9, 1)).to(DEV)
    assert not type(wide(x.clone().requires_grad_(True)).grad_fn).__name__.startswith('_ConvActConv1x1')
    odd = torch.randn(1, C, 3, 5, device=DEV, requires_grad=True)
    assert not type(head(odd).grad_fn).__name__.startswith('_ConvActConv1x1')


@pytest.mark.parametrize('B,C,Co,H,W', [(2, 32, 27, 8, 16), (1, 32, 64, 16, 16), (3, 64, 100, 4, 32), (2, 48, 27, 8, 32),
                                        (2, 64, 64, 8, 64), (1, 128, 256, 6, 64), (2, 32, 48, 2, 128), (1, 64, 27, 3, 128),
                                        (2, 256, 144, 16, 16),
                                        # round 6: rectangular tiles -- 5 x 32 / 5 x 16 / 5 x 8 / 3 x 32 columns, a last
                                        # tile row that hangs over the image (10 rows of 4), 128-column tiles with neighbours
                                        (2, 32, 27, 8, 160), (1, 64, 64, 16, 80), (2, 32, 27, 16, 40), (1, 32, 27, 8, 96),
                                        (1, 48, 32, 10, 160), (1, 32, 27, 4, 256), (1, 16, 48, 6, 192)])
def test_halo_tile_convolution_3x3(B, C, Co, H, W):
    """3x3 / stride 1 / padding 1 with channels % 16 == 0 on maps 16 / 32 / 64 / 128 wide takes the halo-tile kernels
    (csrc/hconv.cuh: the input tile of a 16-channel group staged once with its halo, K ordered (group, tap, channel)):
    forward (bias + ReLU epilogue) and input gradient (the same kernel over grad_y, flipped taps, when Co % 16 == 0)
    against torch's CPU convolution; 1, 2, 4 or 8 image rows per 128-pixel tile, tiles at the image's top and bottom
    edge, several tiles per image, several channel groups, row counts that leave padded output rows."""
    import hip_runtime as hr
    from hip_runtime import ops
    from test_zz_kernel_coverage import short
    g = torch.Generator().manual_seed(B * 1000 + C + Co + W)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    bias = torch.randn(Co, generator=g)
    gy = torch.randn(B, Co, H, W, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yr = F.relu(F.conv2d(xr, wr, br, 1, 1))
    yr.backward(gy)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, bias))
    # every eligible layer, whatever its size -- and no split-K, which would otherwise take these few-tile problems first
    with hr.halo_conv(1, 1), hr.splitk(0), hr.launch_log() as log:
        yd = ops.conv2d(xd, wd, bd, 1, 1, act_slope=0.0)
        yd.backward(gy.to(DEV))
    names = [short(n) for n in log.names]
    if hr.get_matrix_mode() == 0:
        assert any(n.startswith('hconv_kernel') and 'HconvFwd' in n for n in names), names
        assert any('HconvDgrad' in n for n in names) == (Co % 16 == 0), names
    _close(yd, yr.detach(), 1e-4)
    _close(xd.grad, xr.grad, 1e-4)
    _close(wd.grad, wr.grad, 1e-4)
    _close(bd.grad, br.grad, 1e-4)


def test_head_fused_node_leaves_hooks_and_gradient_free_calls_to_the_children():
    """The fused head node replaces the children's forward (hip_runtime/nn.py Head.forward): with a forward hook on a
    child -- feature extraction, activation statistics -- or with nothing that needs a gradient, the layers run in turn
    (same values: the same two kernels)."""
    import hip_runtime.nn as hnn
    torch.manual_seed(3)
    head = hnn.Head(hnn.Conv2d(16, 32, 3, padding=1, act_slope=0.0), hnn.Slot(), hnn.Conv2d(32, 2, 1)).to(DEV)
    x = torch.randn(2, 16, 8, 12, device=DEV)
    fused = head(x)
    assert type(fused.grad_fn).__name__.startswith('_ConvActConv1x1')
    seen = []
    handle = head[0].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    hooked = head(x)
    handle.remove()
    assert seen == [(2, 32, 8, 12)] and not type(hooked.grad_fn).__name__.startswith('_ConvActConv1x1')
    assert torch.equal(hooked, fused)
    pre = head[2].register_forward_pre_hook(lambda m, i: seen.append('pre'))
    head(x)
    pre.remove()
    assert seen[-1] == 'pre'
    for p in head.parameters():
        p.requires_grad_(False)
    frozen = head(x)                       # tape enabled, but nothing requires a gradient: no hidden map is kept
    assert frozen.grad_fn is None and torch.equal(frozen, fused)
    assert type(head(x.clone().requires_grad_(True)).grad_fn).__name__.startswith('_ConvActConv1x1')


def test_launch_stream_is_torchs_current_stream():
    """hip_runtime.stream() (the raw handle from torch's C layer) follows torch's current stream, also inside a
    `torch.cuda.stream(...)` context and on the workspace key."""
    import hip_runtime as hr
    assert (hr.stream().value or 0) == torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert (hr.stream().value or 0) == side.cuda_stream
        a = hr.workspace(1024, torch.device(DEV))
    b = hr.workspace(1024, torch.device(DEV))
    assert a.data_ptr() != b.data_ptr()                  # one scratch buffer per stream
    assert (hr.stream().value or 0) == torch.cuda.current_stream().cuda_stream


def test_cat_add_split():
    from hip_runtime import ops
    g = torch.Generator().manual_seed(7)
    a, b, c = [torch.randn(2, n, 5, 6, generator=g).requires_grad_(True) for n in (3, 8, 1)]
    y = torch.cat((a, b, c), 1)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    da, db_, dc = [t.detach().to(DEV).requires_grad_(True) for t in (a, b, c)]
    dy = ops.cat_channels((da, db_, dc))
    assert torch.equal(dy.cpu(), y.detach())
    dy.backward(gy.to(DEV))
    for d, r in ((da, a), (db_, b), (dc, c)):
        assert torch.equal(d.grad.cpu(), r.grad)
    s = ops.add(da.detach(), da.detach())
    assert torch.equal(s.cpu(), (a + a).detach())
    om = torch.randn(2, 27, 4, 5, generator=g).requires_grad_(True)
    o1, o2, m = torch.chunk(om, 3, dim=1)
    off, mask = torch.cat((o1, o2), 1), torch.sigmoid(m)
    go, gm = torch.randn(off.shape, generator=g), torch.randn(mask.shape, generator=g)
    torch.autograd.backward([off, mask], [go, gm])
    dom = om.detach().to(DEV).requires_grad_(True)
    doff, dmask = ops.split_offset_mask(dom)
    assert torch.equal(doff.cpu(), off.detach())
    _close(dmask, mask, 1e-6)
    torch.autograd.backward([doff, dmask], [go.to(DEV), gm.to(DEV)])
    _close(dom.grad, om.grad, 1e-6)


def test_adam_matches_torch_and_skips_untouched_params():
    from hip_runtime import optim
    g = torch.Generator().manual_seed(8)
    shapes = [(5, 3), (7,), (2, 2, 3), (11,)]
    ref = [torch.randn(s, generator=g).requires_grad_(True) for s in shapes]
    mine = [t.detach().clone().to(DEV).requires_grad_(True) for t in ref]
    o_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=1e-2)
    o_mine = optim.Adam(mine, lr=1e-2, weight_decay=1e-2)
    for it in range(4):
        o_ref.zero_grad()
        o_mine.zero_grad()
        grads = [torch.randn(s, generator=g) for s in shapes]
        for i, (r, m, gr) in enumerate(zip(ref, mine, grads)):
            if i == 2:
                continue                       # never receives a gradient -> must not move (weight decay!)
            (r * gr).sum().backward()
            (m * gr.to(DEV)).sum().backward()
        o_ref.step()
        o_mine.step()
    for r, m in zip(ref, mine):
        _close(m, r, 1e-6)
    assert torch.equal(mine[2].cpu(), ref[2].detach())
    sd = o_mine.state_dict()
    assert len(sd['state']) == 4 and sd['param_groups'][0]['lr'] == 1e-2


def test_conv_full_size_linearity_64ch_128sq():
    # cfg-size layer 64->64 3x3 @128x128 (B=4): conv is linear in x -- size-independent property
    from hip_runtime import ops
    g = torch.Generator().manual_seed(9)
    x1 = torch.randn(4, 64, 128, 128, generator=g).to(DEV)
    x2 = torch.randn(4, 64, 128, 128, generator=g).to(DEV)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(DEV)
    f = lambda t: ops.conv2d(t, w, None, 1, 1)
    _close(f(x1 + 2 * x2), f(x1) + 2 * f(x2), 2e-5)


def test_pack_cache_follows_the_weights():
    """The library keeps the packed weight image of a module's convolution until the weights change (csrc/pack.hip):
    results must track in-place updates by torch (version counter), by the fused Adam (parameter epoch) and a
    replaced Parameter; anonymous functional calls never cache."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn, optim
    g = torch.Generator().manual_seed(21)
    conv = hnn.Conv2d(32, 48, 3, padding=1, bias=True).to(DEV)
    x = torch.randn(2, 32, 9, 11, generator=g).to(DEV)

    def ref():
        return F.conv2d(x.cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu(), 1, 1)
    y0 = conv(x)
    _close(y0, ref())
    used = hr.lib().cnuda_pack_cache_used()
    assert used > 0
    _close(conv(x), ref())                                  # served from the cache
    assert hr.lib().cnuda_pack_cache_used() == used         # ... no new slot
    with torch.no_grad():
        conv.weight.mul_(-0.5)                              # torch in-place: version counter
    _close(conv(x), ref())
    opt = optim.Adam(conv.parameters(), lr=0.1)             # fused Adam on the flat arena: parameter epoch
    conv(x).square().mean().backward()
    opt.step()
    _close(conv(x), ref())
    torch.optim.SGD(conv.parameters(), lr=0.5).step()       # stock optimizer
    _close(conv(x), ref())
    conv.weight = torch.nn.Parameter(torch.randn(48, 32, 3, 3, generator=g).to(DEV) * 0.1)
    _close(conv(x), ref())
    # backward through cached packs (input-gradient image) after a change
    xg = x.clone().requires_grad_(True)
    conv(xg).sum().backward()
    xr = x.cpu().requires_grad_(True)
    F.conv2d(xr, conv.weight.detach().cpu(), conv.bias.detach().cpu(), 1, 1).sum().backward()
    _close(xg.grad, xr.grad)


def test_pack_cache_starts_over_when_the_arena_is_full():
    """Slots of modules that are gone are never returned one by one; once an image does not fit, the cache forgets
    every slot at the next stamped call (csrc/pack.hip, "Eviction") instead of silently not caching for the rest of the
    process -- the state the 768 MB arena reached half-way through a test session or bench.py's other_configs legs."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn
    L = hr.lib()
    x = torch.randn(2, 64, 9, 11, device=DEV)
    hnn.Conv2d(64, 64, 3, padding=1).to(DEV)(x)                   # (the process-wide arena exists from here on)
    big = hr._PACK['arena']
    small = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)    # room for two 64 -> 64 3x3 images (368 KB each)
    hr.check(L.cnuda_pack_cache_attach(hr.ptr(small), small.numel()), 'attach')
    try:
        r0 = L.cnuda_pack_cache_resets()
        convs = [hnn.Conv2d(64, 64, 3, padding=1, bias=True).to(DEV) for _ in range(5)]
        with torch.no_grad():
            for rounds in range(2):
                for c in convs:
                    _close(c(x), F.conv2d(x.cpu(), c.weight.detach().cpu(), c.bias.detach().cpu(), 1, 1), 1e-4)
                    assert L.cnuda_pack_cache_used() <= small.numel()
        assert L.cnuda_pack_cache_resets() > r0
        # a live working set LARGER than the arena must not start over on every pass: the slots that fit
        # stay, the overflow is packed into the caller's workspace, resets are at least 1,024 stamped calls apart
        r_mid = L.cnuda_pack_cache_resets()
        with torch.no_grad():
            for rounds in range(4):
                for c in convs:
                    _close(c(x), F.conv2d(x.cpu(), c.weight.detach().cpu(), c.bias.detach().cpu(), 1, 1), 1e-4)
        assert L.cnuda_pack_cache_resets() == r_mid
        hr.check(L.cnuda_pack_cache_attach(hr.ptr(small), small.numel()), 'attach')      # (fresh arena for the next part)
        # steady state of a working set that fits: two modules, no further fills, no further resets
        pair = convs[:2]
        with torch.no_grad():
            for _ in range(2):        # (the call that finds the arena full is served from the workspace: two warm passes)
                for c in pair:
                    c(x)
        f0, r1 = L.cnuda_pack_cache_fills(), L.cnuda_pack_cache_resets()
        with torch.no_grad():
            for _ in range(3):
                for c in pair:
                    c(x)
        assert L.cnuda_pack_cache_fills() == f0 and L.cnuda_pack_cache_resets() == r1
    finally:
        hr.check(L.cnuda_pack_cache_attach(hr.ptr(big), big.numel()), 'attach')


def test_pack_refresh_after_the_fused_adam_step():
    """After optim.Adam.step() every cached packed image built from the parameter arena is rebuilt by one launch and
    carried into the new parameter epoch (cnuda_pack_refresh): a few training steps of a small stack (3x3, strided,
    1x1 and transposed-conv input gradients: all three pack kinds) give the same losses and weights, bit for bit, as
    the same steps with the cache off, and the forward after a step is served without a new slot."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn, optim

    def run(cache_off):
        was = hr._PACK['off']
        hr._PACK['off'] = cache_off
        try:
            torch.manual_seed(5)
            net = torch.nn.Sequential(hnn.Conv2d(16, 32, 3, padding=1), hnn.Conv2d(32, 64, 3, stride=2, padding=1),
                                      hnn.Conv2d(64, 27, 3, padding=1), hnn.Conv2d(27, 16, 1)).to(DEV)
            opt = optim.Adam(net.parameters(), lr=1e-2)
            x = torch.randn(4, 16, 20, 24, generator=torch.Generator().manual_seed(6)).to(DEV)
            losses, used = [], []
            for _ in range(4):
                opt.zero_grad()
                loss = net(x).square().mean()
                loss.backward()
                opt.step()
                losses.append(loss.item())
                used.append(hr.lib().cnuda_pack_cache_used())
            return losses, [p.detach().clone() for p in net.parameters()], used
        finally:
            hr._PACK['off'] = was
    l_on, p_on, used = run(False)
    l_off, p_off, _ = run(True)
    assert l_on == l_off
    assert all(torch.equal(a, b) for a, b in zip(p_on, p_off))
    assert l_on[-1] < l_on[0]                      # the steps did move the weights
    assert used[0] > 0 and used[1] == used[-1]     # steady state: no new slots after the first step


def test_pack_cache_slot_follows_a_module_to_a_new_weight_buffer():
    """A module that asks for the same image of a NEW source buffer (a re-fold of BatchNorm allocates fresh folded
    weights, a replaced Parameter) takes over its own old slot: the arena must not grow with every replacement."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn
    g = torch.Generator().manual_seed(23)
    conv = hnn.Conv2d(32, 48, 3, padding=1, bias=False).to(DEV)
    x = torch.randn(2, 32, 9, 11, generator=g).to(DEV)
    conv(x)
    used = hr.lib().cnuda_pack_cache_used()
    keep = []
    for _ in range(5):
        w = torch.nn.Parameter(torch.randn(48, 32, 3, 3, generator=g).to(DEV) * 0.1)
        keep.append(w)                                       # (old buffers stay alive: every address is new)
        conv.weight = w
        _close(conv(x), F.conv2d(x.cpu(), w.detach().cpu(), None, 1, 1))
        assert hr.lib().cnuda_pack_cache_used() == used


def test_pack_refresh_with_a_table_that_is_too_small_does_not_fail_the_step():
    """cnuda_pack_refresh runs AFTER the parameters were updated: a job table that does not fit must not turn the
    optimizer step into an error -- nothing is refreshed, the slots refill lazily, results stay right."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn, optim
    torch.manual_seed(7)
    net = torch.nn.Sequential(hnn.Conv2d(16, 32, 3, padding=1), hnn.Conv2d(32, 16, 1)).to(DEV)
    opt = optim.Adam(net.parameters(), lr=1e-2)
    x = torch.randn(2, 16, 12, 12, device=DEV)
    table = hr._PACK.get('table')
    hr._PACK['table'] = torch.empty(16, dtype=torch.uint8, device=DEV)          # room for no job at all
    try:
        for _ in range(2):
            opt.zero_grad()
            net(x).square().mean().backward()
            opt.step()                                                          # must not raise
        y = net(x)
    finally:
        hr._PACK['table'] = table
    want = F.conv2d(F.conv2d(x.cpu(), net[0].weight.detach().cpu(), net[0].bias.detach().cpu(), 1, 1),
                    net[1].weight.detach().cpu(), net[1].bias.detach().cpu())
    _close(y, want)


def test_tensors_of_2gib_take_the_pointer_loaders():
    """The buffer-addressed loaders carry 32-bit byte offsets with a sentinel at 2 GiB (csrc/igemm.cuh); an input of
    2.2 GiB must fall back to the pointer-addressed loaders by itself.  Checked without a CPU reference: a crop of the
    big input goes through the buffer path, and away from the crop's border both give the same numbers -- forward, and
    the input / weight gradients of a loss that only looks at a window inside the crop."""
    from hip_runtime import ops
    g = torch.Generator().manual_seed(33)
    C, Co, S = 32, 32, 4200                                   # 32 * 4200^2 * 4 B = 2.26 GB
    x = torch.empty(1, C, S, S, device=DEV).uniform_(-1, 1).requires_grad_(True)
    w = (torch.randn(Co, C, 3, 3, generator=g) * 0.1).to(DEV).requires_grad_(True)
    assert x.numel() * 4 > 2 ** 31
    r0, r1 = 1000, 1000 + 96
    r = torch.randn(1, Co, r1 - r0 - 2, r1 - r0 - 2, generator=g).to(DEV)
    y_big = ops.conv2d(x, w, None, 1, 1)
    (y_big[:, :, r0 + 1:r1 - 1, r0 + 1:r1 - 1] * r).sum().backward()
    gx_big, gw_big = x.grad[:, :, r0:r1, r0:r1].clone(), w.grad.clone()
    crop = x.detach()[:, :, r0:r1, r0:r1].contiguous().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    y_crop = ops.conv2d(crop, w2, None, 1, 1)
    (y_crop[:, :, 1:-1, 1:-1] * r).sum().backward()
    a, b = y_big.detach()[:, :, r0 + 1:r1 - 1, r0 + 1:r1 - 1], y_crop.detach()[:, :, 1:-1, 1:-1]
    assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()
    assert (gx_big - crop.grad).abs().max().item() <= 1e-5 * crop.grad.abs().max().item()
    assert (gw_big - w2.grad).abs().max().item() <= 1e-4 * w2.grad.abs().max().item()
    # the image corner (padding) of the big tensor against a small problem cut from the same corner
    with torch.no_grad():
        y0 = ops.conv2d_infer(x.detach()[:, :, :64, :64].contiguous(), w.detach(), None, 1, 1)
    assert (y_big.detach()[:, :, :63, :63] - y0[:, :, :63, :63]).abs().max().item() <= 1e-5 * y0.abs().max().item()
    del y_big, y_crop, x, gx_big
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', [
    # B, C, H, W, Co, k, stride, groups      (Co picks the row tile: 128 / 64 / 32 rows -> 64- / 64- / 32-pixel blocks)
    (4, 32, 32, 32, 160, 3, 1, 2), (4, 32, 32, 32, 64, 3, 1, 2), (2, 16, 64, 64, 32, 3, 2, 1), (2, 64, 16, 16, 128, 1, 1, 2),
    # enough pixel tiles for the 8-wave 128- and 64-row kernels (igemm_fwd_ws_kernel<128 | 64, ConvFwdBufStatsLoader>)
    (4, 16, 128, 128, 128, 3, 1, 2), (4, 16, 128, 128, 64, 3, 1, 2),
    (1, 16, 12, 12, 48, 3, 1, 1),          # 144 pixels: a partial last tile; no whole blocks per group -> BatchNorm's own pass
    # the LDS-tile kernels of the 3- / 16-channel full-resolution layers: a block = a 64-column piece of an output row
    (2, 3, 24, 72, 16, 7, 1, 2), (2, 16, 20, 64, 16, 3, 1, 1),
], ids=lambda s: 'B%dC%dH%dW%dCo%dk%ds%dg%d' % s)
def test_convolution_epilogue_leaves_batchnorm_statistics(shape):
    """conv -> train-mode BatchNorm (backends/dla.py:37-62): the GEMM's epilogue leaves sum / sum of squares per
    (pixel block, channel) with its output (cnuda_conv2d_forward_stats) and the BatchNorm uses them instead of its own pass
    over x (cnuda_bn_train_forward_stats).  The block sums against fp64 sums of the stored output; the normalised
    output, saved / running statistics and every gradient against the plain path (bn_reduce_kernel<0>)."""
    import hip_runtime as hr
    from hip_runtime import ops
    B, C, H, W, Co, k, st, groups = shape
    g = torch.Generator().manual_seed(B * 131 + Co + C)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5).to(DEV)
    gamma, beta = (1 + 0.2 * torch.randn(Co, generator=g)).to(DEV), (0.1 * torch.randn(Co, generator=g)).to(DEV)

    def run(emit):
        xs, ws, ga, be = [t.clone().requires_grad_(True) for t in (x, w, gamma, beta)]
        rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        with hr.domain_groups(groups), hr.launch_log() as log:
            y = ops.conv2d(xs, ws, None, st, k // 2, emit_stats=emit)
            pre = getattr(y, '_cnuda_bn_stats', None)
            out = ops.batch_norm_act(y, ga, be, rm, rv, True, relu=True, num_batches_tracked=nbt)
        torch.manual_seed(3)
        out.backward(torch.randn_like(out))
        return y.detach(), pre, out.detach(), (rm, rv, nbt), [t.grad for t in (xs, ws, ga, be)], set(log.names)

    y0, pre0, out0, run0, grads0, k0 = run(False)
    y1, pre1, out1, run1, grads1, k1 = run(True)
    assert pre0 is None and pre1 is not None
    assert torch.equal(y0, y1)
    stats, blk, rows, bpi = pre1
    Ho, Wo = y1.shape[2], y1.shape[3]
    N = B * Ho * Wo
    flat = y1.double().permute(1, 0, 2, 3).reshape(Co, N)
    if bpi:                                 # row pieces (image, row, 64-column tile): per block against the tensor's rows
        tiles_x = (Wo + 63) // 64
        assert bpi == Ho * tiles_x and stats.shape[0] == B * bpi
        got = stats[:, :Co].double().reshape(B, Ho, tiles_x, Co, 2)
        for tx in range(tiles_x):
            piece = y1.double()[:, :, :, tx * 64:(tx + 1) * 64]                       # [B, Co, Ho, <= 64]
            scale = max(1.0, (piece ** 2).sum(-1).max().item())
            assert (got[:, :, tx, :, 0] - piece.sum(-1).permute(0, 2, 1)).abs().max().item() <= 2e-6 * scale
            assert (got[:, :, tx, :, 1] - (piece ** 2).sum(-1).permute(0, 2, 1)).abs().max().item() <= 2e-6 * scale
        whole_blocks = True
    else:
        nblk = N // blk
        want = flat[:, :nblk * blk].reshape(Co, nblk, blk)
        got = stats[:nblk, :Co].double()
        scale = max(1.0, (want ** 2).sum(-1).max().item())
        assert (got[..., 0].t() - want.sum(-1)).abs().max().item() <= 2e-6 * scale
        assert (got[..., 1].t() - (want ** 2).sum(-1)).abs().max().item() <= 2e-6 * scale
        whole_blocks = (N // groups) % blk == 0
    assert any('bn_fold_stats_kernel' in n for n in k1) == whole_blocks, k1
    assert any('bn_reduce_kernel<0>' in n for n in k1) == (not whole_blocks), k1
    assert any('bn_reduce_kernel<0>' in n for n in k0)
    _close(out1, out0, 2e-6)
    for a, b in zip(run1[:2], run0[:2]):
        _close(a, b, 2e-6)
    assert int(run1[2]) == int(run0[2]) == groups
    for a, b in zip(grads1, grads0):
        _close(a, b, 1e-5)


@pytest.mark.parametrize('shape', [(4, 32, 32, 32, 32, 2), (2, 64, 16, 16, 128, 2), (4, 16, 24, 24, 160, 1)],
                         ids=lambda s: 'B%dC%dH%dW%dCo%dg%d' % s)
def test_deformable_convolution_epilogue_leaves_batchnorm_statistics(shape):
    """DeformConv = DCN + BatchNorm + ReLU (backends/dla.py:351-372): the DCN forward's epilogue -- the LDS-window kernel's
    (<= 64 outputs on a 16..128 wide map: one block per wave's 32 pixels, tiles numbered image-major) and the implicit
    GEMM's -- leaves the statistics; outputs, statistics buffers and gradients against the plain path."""
    import hip_runtime as hr
    from hip_runtime import ops
    from libs.DCNv2.dcn_v2 import DCN
    B, C, H, W, Co, groups = shape
    torch.manual_seed(B * 17 + Co)
    m = DCN(C, Co, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1).to(DEV)
    with torch.no_grad():
        m.conv_offset_mask.weight.normal_(0, 0.05)
        m.bias.normal_(0, 0.1)
    gamma, beta = (1 + 0.2 * torch.randn(Co)).to(DEV), (0.1 * torch.randn(Co)).to(DEV)
    x = torch.randn(B, C, H, W).to(DEV)

    def run(emit):
        m.emit_stats = emit
        m.zero_grad()
        xs, ga, be = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
        rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
        with hr.domain_groups(groups), hr.launch_log() as log:
            y = m(xs)
            pre = getattr(y, '_cnuda_bn_stats', None)
            out = ops.batch_norm_act(y, ga, be, rm, rv, True, relu=True)
        torch.manual_seed(3)
        out.backward(torch.randn_like(out))
        return y.detach(), pre, out.detach(), (rm, rv), [xs.grad, ga.grad, be.grad, m.weight.grad.clone()], set(log.names)

    y0, pre0, out0, run0, grads0, k0 = run(False)
    y1, pre1, out1, run1, grads1, k1 = run(True)
    assert pre0 is None and pre1 is not None and torch.equal(y0, y1)
    stats, blk, rows, _ = pre1
    assert stats.shape[0] * blk == B * H * W and rows >= Co
    tot = stats[:, :Co].double().sum(0)                       # whole-batch sums: independent of the blocks' pixel order
    flat = y1.double().permute(1, 0, 2, 3).reshape(Co, -1)
    scale = max(1.0, (flat ** 2).sum(-1).max().item())
    assert (tot[:, 0] - flat.sum(-1)).abs().max().item() <= 2e-6 * scale
    assert (tot[:, 1] - (flat ** 2).sum(-1)).abs().max().item() <= 2e-6 * scale
    assert any('bn_fold_stats_kernel' in n for n in k1) and not any('bn_reduce_kernel<0>' in n for n in k1), k1
    assert any('bn_reduce_kernel<0>' in n for n in k0)
    _close(out1, out0, 2e-6)
    for a, b in zip(run1, run0):
        _close(a, b, 2e-6)
    for a, b in zip(grads1, grads0):
        _close(a, b, 1e-5)


@pytest.mark.parametrize('shape', [(2, 17, 15, 32), (1, 64, 96, 32), (3, 20, 22, 8), (2, 9, 130, 48)],
                         ids=lambda s: 'B%dH%dW%dCo%d' % s)
def test_stride2_sixteen_channel_input_gradient(shape):
    """dgrad_s2_c16_kernel (3x3 / stride 2 / padding 1, 16 input channels: DLA-34's level1): one thread per 2 x 2 block of
    grad_x.  Odd and even heights / widths (last block rows / columns partly outside), grad_y cells beyond the map, the
    8-byte and the scalar store paths, and both addends -- also aliasing the output (hip_runtime.fanout)."""
    import hip_runtime as hr
    from hip_runtime import ops
    B, H, W, Co = shape
    L = hr.lib()
    g = torch.Generator().manual_seed(H * 7 + W)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(B, Co, Ho, Wo, generator=g)
    w = torch.randn(Co, 16, 3, 3, generator=g) / 12
    want = torch.nn.grad.conv2d_input((B, 16, H, W), w.double(), gy.double(), stride=2, padding=1)
    geom = (B, 16, H, W, Co, 3, 3, 2, 2, 1, 1)
    gyd, wd = gy.to(DEV), w.to(DEV)
    wp, wn = ops._ws(L.cnuda_conv2d_workspace_bytes(*geom), gyd)
    with hr.launch_log() as log:
        gx = torch.empty(B, 16, H, W, device=DEV)
        hr.check(L.cnuda_conv2d_backward_data(hr.ptr(gyd), hr.ptr(wd), hr.ptr(gx), *geom, wp, wn, hr.stream()), 'dgrad')
    assert any('dgrad_s2_c16_kernel' in n for n in log.names), log.names
    _close(gx, want.float(), 1e-5)
    a1, a2 = torch.randn(B, 16, H, W, generator=g).to(DEV), torch.randn(B, 16, H, W, generator=g).to(DEV)
    acc = a1.clone()
    hr.check(L.cnuda_conv2d_backward_data_add(hr.ptr(gyd), hr.ptr(wd), hr.ptr(acc), hr.ptr(a2), hr.ptr(acc), *geom, wp, wn,
                                              hr.stream()), 'dgrad_add')
    _close(acc, (want + a1.double().cpu() + a2.double().cpu()).float(), 1e-5)


@pytest.mark.parametrize('groups', [1, 2])
def test_batchnorm_applied_on_load_equals_the_materialised_activation(groups):
    """conv -> BatchNorm + ReLU -> conv with the BatchNorm's apply pass deferred into the second convolution's staging
    (hip_runtime.ops.batch_norm_act(defer_apply=True), cnuda_conv2d_forward_norm_input / _backward_weight_norm_input: DLA-34's
    stem -> level0): outputs, every gradient and the running statistics bit for bit those of the materialised form, and
    (one statistics group) within 1e-4 of torch's own conv / batch_norm / relu on the CPU."""
    import hip_runtime as hr
    from hip_runtime import nn as hnn
    g = torch.Generator().manual_seed(11)
    B, H, W = 4, 40, 72
    x = torch.randn(B, 3, H, W, generator=g)
    gy = torch.randn(B, 16, H, W, generator=g)
    conv1 = hnn.Conv2d(3, 16, 7, padding=3, bias=False, emit_stats=True).to(DEV)
    bn1 = hnn.BatchNorm2d(16).to(DEV)
    conv2 = hnn.Conv2d(16, 16, 3, padding=1, bias=False, emit_stats=True).to(DEV)
    bn2 = hnn.BatchNorm2d(16).to(DEV)
    with torch.no_grad():
        bn1.weight.uniform_(0.5, 1.5, generator=None); bn1.bias.uniform_(-0.5, 0.5)
    mods = [conv1, bn1, conv2, bn2]
    state = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    for m in mods:
        m.train()
    assert hr.lib().cnuda_conv2d_norm_input_supported(B, 16, H, W, 16, 3, 3, 1, 1, 1, 1) == 1

    def run(defer):
        for m, st in zip(mods, state):
            m.load_state_dict(st)
            for p in m.parameters():
                p.grad = None
        bn1.defer_apply = defer
        xd = x.to(DEV).requires_grad_(True)
        with hr.domain_groups(groups), hr.launch_log() as log:
            a = bn1(conv1(xd), relu=True)
            assert hasattr(a, '_cnuda_deferred_bn') == defer
            y = bn2(conv2(a), relu=True)
            y.backward(gy.to(DEV))
        names = ' '.join(log.names)
        assert ('smallc_fwd_kernelILi1ELi3ELb1' in names or 'smallc_fwd_kernel<1, 3, true>' in names) == defer, names
        out = [y.detach(), xd.grad] + [p.grad for m in mods for p in m.parameters()]
        return out + [bn1.running_mean.clone(), bn1.running_var.clone(), bn2.running_mean.clone(), bn2.running_var.clone()]

    plain, deferred = run(False), run(True)
    for i, (a, b) in enumerate(zip(plain, deferred)):
        assert torch.equal(a, b), (i, (a - b).abs().max().item())
    if groups == 1:
        ref = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 7, padding=3, bias=False), torch.nn.BatchNorm2d(16), torch.nn.ReLU(),
                                  torch.nn.Conv2d(16, 16, 3, padding=1, bias=False), torch.nn.BatchNorm2d(16), torch.nn.ReLU())
        ref[0].load_state_dict({k: v.cpu() for k, v in state[0].items()})
        ref[1].load_state_dict({k: v.cpu() for k, v in state[1].items()})
        ref[3].load_state_dict({k: v.cpu() for k, v in state[2].items()})
        ref[4].load_state_dict({k: v.cpu() for k, v in state[3].items()})
        ref.train()
        xr = x.clone().requires_grad_(True)
        yr = ref(xr)
        yr.backward(gy)
        _close(deferred[0], yr)
        _close(deferred[1], xr.grad)
        _close(deferred[2], ref[0].weight.grad)
        _close(deferred[5], ref[3].weight.grad)
