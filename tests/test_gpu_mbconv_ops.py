"""MI355X parity of the MBConv operators (csrc/mbconv.hip) against the fp64 CPU oracle (tests/efficientnet_oracle.py):
forward and every gradient within 1e-4 of the tensor's largest magnitude, and bit-identical results from two runs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import efficientnet_oracle as eo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(got, want, what=''):
    got, want = got.detach().double().cpu(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    print('%s: max abs err %.3e, tensor max %.3e' % (what, err, scale))
    assert err <= 1e-4 * scale, (what, err, scale)


def _run(fn_gpu, fn_ref, tensors, gy_seed=5):
    """tensors: {name: fp32 CPU tensor or (tensor, False) for inputs without a gradient}, passed in order -> checks forward and gradients;
    runs the GPU side twice and wants the same bits."""
    g = torch.Generator().manual_seed(gy_seed)
    need = {k: not isinstance(v, tuple) for k, v in tensors.items()}
    vals = {k: (v[0] if isinstance(v, tuple) else v) for k, v in tensors.items()}
    ref_in = {k: v.double().requires_grad_(need[k]) for k, v in vals.items()}
    yr = fn_ref(*ref_in.values())
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())
    runs = []
    for _ in range(2):
        dev_in = {k: v.to(DEV).requires_grad_(need[k]) for k, v in vals.items()}
        y = fn_gpu(*dev_in.values())
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        runs.append([y.detach()] + [dev_in[k].grad for k in vals if need[k]])
    _close(runs[0][0], yr, 'forward')
    for k, got in zip([k for k in vals if need[k]], runs[0][1:]):
        _close(got, ref_in[k].grad, 'grad ' + k)
    for a, b in zip(*runs):
        assert torch.equal(a, b), 'two runs differ'


@pytest.mark.parametrize('H,W', [(8, 8), (7, 9), (15, 15), (8, 64)])
@pytest.mark.parametrize('k,s', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_same_matches_oracle(k, s, H, W):
    from hip_runtime import ops
    rs = np.random.RandomState(k * 100 + s * 10 + H)
    x = torch.from_numpy(rs.standard_normal((2, 5, H, W)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((5, 1, k, k)) / k).astype(np.float32))
    _run(lambda x, w: ops.depthwise_conv2d_same(x, w, s), lambda x, w: eo.dwconv_same(x, w, s), dict(x=x, w=w))


@pytest.mark.parametrize('k,s,H,W,nominal', [(5, 2, 16, 16, 15), (3, 2, 16, 12, 15), (5, 2, 9, 9, 8), (3, 1, 8, 8, 8)])
def test_depthwise_static_padding_of_another_nominal_size(k, s, H, W, nominal):
    """the static form: padding computed for the nominal map (odd: symmetric 2 + 2 / 1 + 1) applied to a map of another
    parity -- part of the bottom / right padding is then never read, or the last rows are cut short"""
    from hip_runtime import nn as hnn, ops
    rs = np.random.RandomState(k + H)
    m = hnn.DepthwiseConv2dSame(6, k, s, image_size=nominal).to(DEV)
    x = torch.from_numpy(rs.standard_normal((2, 6, H, W)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((6, 1, k, k)) / k).astype(np.float32))
    _run(lambda x, w: ops.depthwise_conv2d_same(x, w, s, m.static_padding),
         lambda x, w: eo.dwconv_same(x, w, s, (nominal, nominal)), dict(x=x, w=w))
    with torch.no_grad():
        m.weight.copy_(w)
        assert torch.equal(m(x.to(DEV)).cpu(), ops.depthwise_conv2d_same(
            x.to(DEV), w.to(DEV), s, m.static_padding).cpu())


@pytest.mark.parametrize('B,C,Cse,H,W', [(3, 24, 4, 5, 7), (3, 672, 28, 5, 7), (1, 24, 4, 1, 1), (2, 16, 4, 4, 8)])
def test_squeeze_excite_matches_oracle(B, C, Cse, H, W):
    from hip_runtime import ops
    rs = np.random.RandomState(C + H)
    f = lambda *shape, scale=1.0: torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))
    t = dict(x=f(B, C, H, W), w1=f(Cse, C, 1, 1, scale=C ** -0.5 * 2), b1=f(Cse, scale=0.3),
             w2=f(C, Cse, 1, 1, scale=Cse ** -0.5 * 2), b2=f(C, scale=0.3))
    _run(ops.squeeze_excite, eo.squeeze_excite, t)


def test_squeeze_excite_module_names_and_frozen_parameters():
    from hip_runtime import nn as hnn
    m = hnn.SqueezeExcite(24, 6).to(DEV)
    assert sorted(n for n, _ in m.named_parameters()) == ['_se_expand.bias', '_se_expand.weight', '_se_reduce.bias',
                                                          '_se_reduce.weight']
    assert m._se_reduce.weight.shape == (6, 24, 1, 1) and m._se_expand.weight.shape == (24, 6, 1, 1)
    m._se_reduce.weight.requires_grad = False
    m._se_expand.bias.requires_grad = False
    x = torch.randn(2, 24, 3, 3, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    y = m(x)
    y.sum().backward()
    assert m._se_reduce.weight.grad is None and m._se_expand.bias.grad is None
    want = eo.squeeze_excite(x.detach().cpu().double(), *[p.detach().cpu().double() for p in (
        m._se_reduce.weight, m._se_reduce.bias, m._se_expand.weight, m._se_expand.bias)])
    _close(y, want, 'module forward')
    assert m._se_reduce.bias.grad is not None and x.grad is not None


@pytest.mark.parametrize('n', [1, 63, 64, 4099])
def test_swish_matches_oracle(n):
    from hip_runtime import nn as hnn
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    x[0] = 20.0
    x[-1] = -20.0 if n > 1 else 20.0
    if n > 2:
        x[1] = -20.0
    _run(lambda x: hnn.Swish()(x), eo.swish, dict(x=x))


def test_swish_far_tails_are_finite():
    from hip_runtime import ops
    x = torch.tensor([-200.0, -90.0, 0.0, 90.0, 200.0], device=DEV, requires_grad=True)
    y = ops.swish(x)
    y.sum().backward()
    assert torch.equal(y.detach().cpu(), torch.tensor([-0.0, -0.0, 0.0, 90.0, 200.0]))
    assert torch.equal(x.grad.cpu(), torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0]))


@pytest.mark.parametrize('shape', [(4, 6, 5, 4), (4, 3, 3, 3)])
def test_drop_connect_add_matches_oracle(shape):
    from hip_runtime import ops
    g = torch.Generator().manual_seed(shape[1])
    keep = 0.8
    mask = torch.tensor([0.0, 1 / keep, 1 / keep, 0.0])
    _run(ops.drop_connect_add, eo.drop_connect_add,
         dict(x=torch.randn(shape, generator=g), mask=(mask, False), residual=torch.randn(shape, generator=g)))


@pytest.mark.parametrize('H,W,pb,pr', [(8, 8, 1, 1), (5, 7, 1, 0), (6, 4, 0, 2)])
def test_pad_right_bottom_is_f_pad(H, W, pb, pr):
    from hip_runtime import ops
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H))
    y = ops.pad_right_bottom(x.to(DEV), pb, pr)
    assert torch.equal(y.cpu(), F.pad(x, (0, pr, 0, pb)))
    with pytest.raises(RuntimeError, match='no backward'):
        ops.pad_right_bottom(x.to(DEV).requires_grad_(True), pb, pr)


def test_mbconv_block_matches_oracle_with_and_without_drop_connect():
    """one block with a skip connection (stride 1, in == out): training forward / backward against the fp64 oracle, with a
    mask drawn by the block (reproduced from the same seed) and without one"""
    import inputs as gin
    from hip_runtime import nn as hnn
    block = hnn.MBConvBlock(16, 16, 5, 1, 6, image_size=9).to(DEV)
    shapes = {k: tuple(v.shape) for k, v in block.state_dict().items()}
    state = gin.fill_state({'base._blocks.0.' + k: s for k, s in shapes.items()})
    x = torch.randn(4, 16, 9, 9, generator=torch.Generator().manual_seed(3))
    spec = (16, 16, 5, 1, 6, 4, 9)
    for rate in (None, 0.5):
        block.load_state_dict({k[len('base._blocks.0.'):]: torch.from_numpy(v) for k, v in state.items()})
        block.train()
        block.zero_grad(set_to_none=True)          # the second leg must not add to the first leg's gradients
        seed = 0
        if rate:          # a seed whose draw keeps some images and drops others
            seed = next(sd for sd in range(64) if torch.manual_seed(sd) is not None
                        and 0 < torch.floor((1 - rate) + torch.rand([4], device=DEV)).sum().item() < 4)
        torch.manual_seed(seed)
        xg = x.to(DEV).requires_grad_(True)
        y = block(xg, drop_connect_rate=rate)
        mask = None
        if rate:
            torch.manual_seed(seed)
            mask = (torch.floor((1 - rate) + torch.rand([4], device=DEV)) / (1 - rate)).cpu()
            assert 0 < (mask == 0).sum() < 4, mask          # both kinds of image in the batch
        y.backward(torch.cos(torch.arange(y.numel(), dtype=torch.float32).reshape(y.shape)).to(DEV))
        sd = eo.make_state(state, torch.float64)
        net = eo.Net(sd, 'b0', [], False)
        net.training = True
        xr = x.double().requires_grad_(True)
        yr = net.block(xr, 0, spec, mask)
        yr.backward(torch.cos(torch.arange(yr.numel(), dtype=torch.float64).reshape(yr.shape)))
        _close(y, yr, 'block forward rate=%s' % rate)
        _close(xg.grad, xr.grad, 'block grad x rate=%s' % rate)
        for n, p in block.named_parameters():
            _close(p.grad, sd['base._blocks.0.' + n].grad, 'block grad %s rate=%s' % (n, rate))
        for n, b in block.named_buffers():
            if not n.endswith('num_batches_tracked'):
                _close(b, sd['base._blocks.0.' + n], 'buffer ' + n)
    block.eval()
    with torch.no_grad():
        assert torch.equal(block(x.to(DEV), drop_connect_rate=0.5), block(x.to(DEV)))
