"""No-GPU checks of the deformable PSROI pooling: the float64 oracle (tests/psroi_oracle.py) is pinned by answers that
do not come from it (hand counts, closed forms, finite differences), and the Python / C surface is what the DCNv2
library's users expect."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import psroi_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_plane_and_hand_counted_samples():
    """8 x 8 map, scale 1, P = 2, S = 3.  ROI (5, 5)-(10, 10): start 4.5, end 10.5, bins 3 wide, samples 1 apart:
    4.5 5.5 6.5 | 7.5 8.5 9.5 on both axes.  7.5 = W - 0.5 is still inside (the test is `>`), 8.5 and 9.5 are not:
    3 and 1 valid per axis.  The second ROI lies wholly outside."""
    x = torch.full((1, 2, 8, 8), 3.0)
    rois = torch.tensor([[0, 5, 5, 10, 10], [0, 20, 20, 25, 25]], dtype=torch.float32)
    out, count = po.forward(x, rois, None, True, 1.0, 2, 1, 2, 2, 3, 0.0)
    want = torch.tensor([[9.0, 3.0], [3.0, 1.0]], dtype=torch.float64)
    assert torch.equal(count[0], want.expand(2, 2, 2))
    assert torch.equal(count[1], torch.zeros(2, 2, 2, dtype=torch.float64))
    assert torch.allclose(out[0], torch.full((2, 2, 2), 3.0, dtype=torch.float64), atol=1e-12)
    assert torch.equal(out[1], torch.zeros(2, 2, 2, dtype=torch.float64))


def _ramp_case():
    a, b = 0.7, -0.4
    H = W = 16
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    x = (a * xs + b * ys).expand(1, 2, H, W).contiguous()
    rois = torch.tensor([[0, 10, 12, 30, 36]], dtype=torch.float32)
    # scale 0.3: start (2.5, 3.1), end (8.8, 10.6), size 6.3 x 7.5; P = 3, S = 2: samples 1.05 / 1.25 apart, none on an integer
    return a, b, x, rois, 0.3, 3, 2


def test_linear_ramp_closed_form_without_and_with_offsets():
    a, b, x, rois, scale, P, S = _ramp_case()
    s = float(np.float32(scale))
    sw, sh = 10 * s - 0.5, 12 * s - 0.5
    rw, rh = 21 * s, 25 * s
    pw = torch.arange(P, dtype=torch.float64).view(1, P)
    ph = torch.arange(P, dtype=torch.float64).view(P, 1)
    mean_w = sw + pw * rw / P + (S - 1) / 2 * rw / P / S
    mean_h = sh + ph * rh / P + (S - 1) / 2 * rh / P / S
    want = a * mean_w + b * mean_h
    out, count = po.forward(x, rois, None, True, scale, 2, 1, P, P, S, 0.0)
    assert torch.equal(count, torch.full_like(count, S * S))
    assert torch.allclose(out[0, 0], want, atol=1e-12) and torch.allclose(out[0, 1], want, atol=1e-12)
    # offsets (tx, ty) per part cell shift the bin by tx * trans_std * roi_w, ty * trans_std * roi_h
    g = torch.Generator().manual_seed(5)
    off = torch.randn(1, 2, P, P, generator=g, dtype=torch.float64) * 0.5
    tstd = float(np.float32(0.1))
    shifted = want + a * off[0, 0] * tstd * rw + b * off[0, 1] * tstd * rh
    args = (False, scale, 2, 1, P, P, S, 0.1)
    assert po.margin(x.shape, rois, off, *args) > 1e-3
    out, _ = po.forward(x, rois, off, *args)
    assert torch.allclose(out[0, 0], shifted, atol=1e-12)
    # ... and its offset gradient: every one of the 2 channels contributes grad * a * trans_std * roi_w (x), b ... roi_h (y)
    go = torch.randn(1, 2, P, P, generator=g, dtype=torch.float64)
    _, _, gi, goff = po.forward_backward(x, rois, off, go, *args)
    assert torch.allclose(goff[0, 0], go[0].sum(0) * a * tstd * rw, atol=1e-12)
    assert torch.allclose(goff[0, 1], go[0].sum(0) * b * tstd * rh, atol=1e-12)
    # the input gradient of a mean of bilinear weights sums to the output gradient
    assert torch.allclose(gi.sum(dim=(2, 3))[0], go[0].sum(dim=(1, 2)), atol=1e-12)


def test_zero_offsets_equal_no_trans():
    """the reference's check_pooling_zero_offset (testcuda.py:100-131)"""
    x = torch.zeros(2, 16, 64, 64)
    x[0, :, 16:26, 16:26] = 1.0
    x[1, :, 10:20, 20:30] = 2.0
    rois = torch.tensor([[0, 65, 65, 103, 103], [1, 81, 41, 119, 79]], dtype=torch.float32)
    plain, c0 = po.forward(x, rois, None, True, 0.25, 16, 1, 7, 7, 4, 0.0)
    zero, c1 = po.forward(x, rois, torch.zeros(2, 2, 7, 7), False, 0.25, 16, 1, 7, 7, 4, 0.0)
    assert torch.equal(plain, zero) and torch.equal(c0, c1)
    assert plain[0].mean() > 0.5 and plain[1].mean() > 1.0          # the ROIs sit on the two plateaus


def _gradcheck_inputs(seed):
    """the sizes of the reference's check_gradient_dpooling (testcuda.py:134-166)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 5, 5, generator=g, dtype=torch.float64) * 0.01
    N = 4
    bi = torch.randint(2, (N, 1), generator=g).float()
    px, py = torch.rand(N, 1, generator=g) * 15, torch.rand(N, 1, generator=g) * 15
    w, h = torch.rand(N, 1, generator=g) * 10, torch.rand(N, 1, generator=g) * 10
    rois = torch.cat((bi, px, py, px + w, py + h), dim=1)
    off = torch.randn(N, 2, 3, 3, generator=g, dtype=torch.float64)
    return x, rois, off


GRADCHECK_SEED = 4


def test_oracle_gradients_against_finite_differences(trans_std=0.1):
    """trans_std is example_dpooling's 0.1, not check_gradient_dpooling's 0.0: with 0.0 the offset gradient is zero by
    construction, and at scale 1/4 every coordinate is a multiple of 1/48, many of them integers -- the operator is
    not differentiable there, so no seed reaches the margin."""
    x, rois, off = _gradcheck_inputs(GRADCHECK_SEED)
    args = (False, 0.25, 3, 1, 3, 3, 4, trans_std)
    assert po.margin(x.shape, rois, off, *args) >= 1e-3
    x.requires_grad_(True)
    off.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda i, t: po.forward(i, rois, t, *args)[0], (x, off), eps=1e-6, atol=1e-7)


def test_index_tables_are_float32():
    # p / 49 * 49 lands below p for p = 27 only in float32 (what the reference's users ran), for 1, 2, 4, 8, 16, 27, 32
    # in float64: the case that falls on the other side of an integer in another precision
    part, g = po.tables(49, 49, 7)
    assert part.tolist() == [p - 1 if p == 27 else p for p in range(49)]
    assert np.floor(np.arange(49) / 49 * 49).tolist() == [p - 1 if p in (1, 2, 4, 8, 16, 27, 32) else p for p in range(49)]
    assert int(g.max()) == 6 and int(g.min()) == 0
    part7, g7 = po.tables(7, 7, 7)
    assert part7.tolist() == list(range(7)) and g7.tolist() == list(range(7))


def test_cpu_tensors_are_refused():
    import _ext
    from libs.DCNv2.dcn_v2 import DCNPooling, DCNv2Pooling, dcn_v2_pooling
    z = torch.zeros
    x, rois, off = z(1, 4, 8, 8), z(2, 5), z(2, 2, 3, 3)
    with pytest.raises(RuntimeError, match='MI355X only'):
        _ext.dcn_v2_psroi_pooling_forward(x, rois, off, 0, 0.25, 4, 1, 3, 3, 2, 0.1)
    with pytest.raises(RuntimeError, match='MI355X only'):
        _ext.dcn_v2_psroi_pooling_backward(z(2, 4, 3, 3), x, rois, off, z(2, 4, 3, 3), 0, 0.25, 4, 1, 3, 3, 2, 0.1)
    with pytest.raises(RuntimeError, match='MI355X only'):
        DCNv2Pooling(0.25, 3, 4, False, trans_std=0.1)(x, rois, off)
    with pytest.raises(RuntimeError, match='MI355X only'):
        dcn_v2_pooling(x, rois, x.new(), 0.25, 3, 4, True)
    with pytest.raises(RuntimeError, match='MI355X only'):
        DCNPooling(0.25, 3, 4, False, trans_std=0.1, deform_fc_dim=8)(x, rois)


NEW_SYMBOLS = ('cnuda_dcn_v2_psroi_pooling_workspace_bytes', 'cnuda_dcn_v2_psroi_pooling_forward',
               'cnuda_dcn_v2_psroi_pooling_backward')


def test_new_symbols_in_header_signature_table_and_library():
    import hip_runtime as hr
    text = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    L = hr.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(hr._Sig, name) and hasattr(L, name), name
    assert L.cnuda_abi_version() == 2
    assert L.cnuda_dcn_v2_psroi_pooling_workspace_bytes(2, 20, 32, 7) >= 2 * 20 * 32 * 49 * 4
    # null pointers and bad geometry are rejected before anything touches the device
    geom = (2, 32, 64, 64, 20, 0, 0.25, 32, 1, 7, 7, 4, 0.1, 1)
    assert L.cnuda_dcn_v2_psroi_pooling_forward(None, None, None, None, None, *geom, None) == -1
    assert b'null' in L.cnuda_last_error()
    assert L.cnuda_dcn_v2_psroi_pooling_backward(None, None, None, None, None, None, 0, None, *geom, None, 0, None) == -1
    bad = (2, 33, 64, 64, 20, 0, 0.25, 32, 1, 7, 7, 4, 0.1, 1)          # channels != output_dim * group^2
    assert L.cnuda_dcn_v2_psroi_pooling_forward(None, None, None, None, None, *bad, None) == -1
    assert b'channels' in L.cnuda_last_error()


def test_pooling_signatures_match_the_reference():
    from libs.DCNv2.dcn_v2 import DCNPooling, DCNv2Pooling, dcn_v2_pooling
    module = ['spatial_scale', 'pooled_size', 'output_dim', 'no_trans', 'group_size', 'part_size', 'sample_per_part',
              'trans_std']
    defaults = {'group_size': 1, 'part_size': None, 'sample_per_part': 4, 'trans_std': .0}
    sig = inspect.signature(DCNv2Pooling.__init__)
    assert list(sig.parameters)[1:] == module
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == defaults
    sig = inspect.signature(DCNPooling.__init__)
    assert list(sig.parameters)[1:] == module + ['deform_fc_dim']
    assert sig.parameters['deform_fc_dim'].default == 1024
    assert list(inspect.signature(DCNv2Pooling.forward).parameters)[1:] == ['input', 'rois', 'offset']
    assert list(inspect.signature(DCNPooling.forward).parameters)[1:] == ['input', 'rois']
    sig = inspect.signature(dcn_v2_pooling)
    assert list(sig.parameters) == ['input', 'rois', 'offset'] + module
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == defaults


def test_dcn_pooling_state_dict_names_and_zero_init():
    from libs.DCNv2.dcn_v2 import DCNPooling
    m = DCNPooling(0.25, 7, 8, False, trans_std=0.1, deform_fc_dim=16)
    assert sorted(m.state_dict()) == sorted('offset_mask_fc.%d.%s' % (i, n) for i in (0, 2, 4) for n in ('weight', 'bias'))
    assert m.offset_mask_fc[0].weight.shape == (16, 7 * 7 * 8) and m.offset_mask_fc[4].weight.shape == (7 * 7 * 3, 16)
    assert not m.offset_mask_fc[4].weight.any() and not m.offset_mask_fc[4].bias.any()
    assert not hasattr(DCNPooling(0.25, 7, 8, True), 'offset_mask_fc')
