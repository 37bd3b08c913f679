"""Python face of the deformable convolution: `dcn_v2_conv`, `DCNv2`, `DCN`
-- and, at the end of the file, of the deformable PSROI pooling: `dcn_v2_pooling`,
`DCNv2Pooling`, `DCNPooling` (libs/DCNv2/dcn_v2.py:132-303) --
with the constructor/forward signatures, parameter names (`weight`, `bias`,
`conv_offset_mask.{weight,bias}` -- checkpoint keys) and initialisation of the
reference (libs/DCNv2/dcn_v2.py:18-128), running on the MI355X kernels behind
`_ext`.  The offset/mask generating 3x3 convolution of `DCN` is this repo's own
implicit-GEMM convolution (hip_runtime.nn.Conv2d), not a vendor library.
"""
import math
import os as _os

import torch
from torch import nn

import _ext as _backend
import hip_runtime as hr
from hip_runtime import nn as hnn
from hip_runtime import ops
from hip_runtime.arena import grad_sink
from hip_runtime.fanout import accumulate_in_place, claim, fork, slot_of


# CNUDA_DCN_KEEP_COLS=0: the forward does not store the sampled columns and the weight gradient samples the input again
# (the reference's scheme, dcn_v2_cuda.cu:302-319) -- an A/B switch for the measurement in DESIGN.md section 12; the
# default keeps them (one 1 GB side output per 128 x 128 layer, read once by a plain-GEMM weight gradient)
_KEEP_COLUMNS = _os.environ.get('CNUDA_DCN_KEEP_COLS', '1') != '0'
# CNUDA_DCN_OM=0 (or dcn_v2.USE_OM = False): DCN.forward materialises offset and mask tensors like the reference
# (split + sigmoid kernel, its backward twin) instead of reading them out of the offset convolution's output
USE_OM = _os.environ.get('CNUDA_DCN_OM', '1') != '0'


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _node_forward(ctx, fwd, input, sampling, weight, bias, geom, keep, pack_token, stats_box, regime):
    """The forward of both autograd nodes.  sampling: (offset, mask) or (om,); fwd: the `_ext` function that takes them."""
    ctx.regime = int(regime)       # offset regime of this layer (DCN._census): which kernels the library picks
    ctx.slot = slot_of(input)      # where the offset convolution (the input's other consumer) meets this gradient
    ctx.geom = geom
    # keep the sampled columns (a side output of the forward kernel) for the weight gradient:
    # on a 288 GB part re-reading ~0.3 GB per layer beats re-sampling the input
    keep = keep and any(ctx.needs_input_grad[:3 + len(sampling)]) and _KEEP_COLUMNS
    with _offset_regime(ctx.regime):
        out = fwd(input, weight, bias, *sampling, *geom, _want_columns=keep, _pack_token=pack_token, _stats_box=stats_box)
    out, cols = out if isinstance(out, tuple) else (out, None)      # (dcn_v2_forward without columns: the output alone)
    ctx.save_for_backward(input, *sampling, weight, bias, cols)
    return out


def _node_backward(ctx, bwd, grad_output):
    """The backward of both nodes -> (grad_input, [the sampling tensors' gradients], grad_weight, grad_bias)."""
    input, *sampling, weight, bias, cols = ctx.saved_tensors
    sw, sb = grad_sink(weight), grad_sink(bias)       # arena slots: written by the kernels, not returned
    # the data-gradient walks ADD into grad_input: on top of what the slot already holds when it is the slot's own
    # buffer, else into a cleared tensor -- which an empty slot takes over
    acc = accumulate_in_place(ctx.slot)
    with _offset_regime(ctx.regime):
        g_in, *g_sampling, g_w, g_b = bwd(input, weight, bias, *sampling, grad_output, *ctx.geom, _columns=cols,
                                          _grad_weight=sw, _grad_bias=sb, _grad_input=acc)
    if acc is None:
        claim(ctx.slot, g_in)
    return g_in, g_sampling, (None if sw is not None else g_w), (None if sb is not None else g_b)


class _DeformConvFn(torch.autograd.Function):
    # autograd-visible argument order (dcn_v2.py:18-19): input, offset, mask, weight, bias, ...
    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups, pack_token=0,
                stats_box=None, regime=0):
        geom = tuple(weight.shape[2:]) + _pair(stride) + _pair(padding) + _pair(dilation) + (deformable_groups,)
        return _node_forward(ctx, _backend.dcn_v2_forward, input, (offset, mask), weight, bias, geom, input.shape[3] >= 2,
                             pack_token, stats_box, regime)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        g_in, (g_off, g_mask), g_w, g_b = _node_backward(ctx, _backend.dcn_v2_backward, grad_output)
        return g_in, g_off, g_mask, g_w, g_b, None, None, None, None, None, None, None


class _DeformConvOmFn(torch.autograd.Function):
    """The same operation with offsets and mask read out of `om`, the 3T-channel output of the layer's own offset convolution
    whose mask channels already went through the sigmoid (ops.conv2d_rowsig): no split / concatenate / sigmoid tensors in the
    forward, and ONE gradient tensor for `om` in the backward -- the offsets' gradient and the gradient of the mask's LOGIT,
    which is what that convolution's backward consumes (round 6; `DCN.forward` only, deformable_groups == 1)."""

    @staticmethod
    def forward(ctx, input, om, weight, bias, stride, padding, dilation, pack_token=0, stats_box=None, regime=0):
        geom = tuple(weight.shape[2:]) + _pair(stride) + _pair(padding) + _pair(dilation)
        return _node_forward(ctx, _backend.dcn_v2_forward_om, input, (om,), weight, bias, geom, True, pack_token, stats_box,
                             regime)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        g_in, (g_om,), g_w, g_b = _node_backward(ctx, _backend.dcn_v2_backward_om, grad_output)
        return g_in, g_om, g_w, g_b, None, None, None, None, None, None


class _offset_regime:
    """The library's offset regime (cnuda_dcn_set_offset_regime) for the calls inside the block; behind it the regime that
    was in force before (the setter returns it), so that nested or interleaved users do not reset each other."""

    def __init__(self, regime):
        self.regime = regime
        self.prev = 0

    def __enter__(self):
        self.prev = hr.lib().cnuda_dcn_set_offset_regime(self.regime)

    def __exit__(self, *exc):
        hr.lib().cnuda_dcn_set_offset_regime(self.prev)


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups, pack_token=0,
                emit_stats=False, regime=0):
    """emit_stats (not part of the reference's signature): the output goes straight into a train-mode BatchNorm -- the
    kernel's epilogue then leaves the statistics with it (hip_runtime.ops.batch_norm_act finds them on the tensor)."""
    return ops.with_bn_stats(emit_stats, lambda box: _DeformConvFn.apply(
        input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups, pack_token, box, regime))


class DCNv2(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1,
                 deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self._pack_token = hr.PackToken()           # identity of these weights for the library's pack cache
        self.reset_parameters()

    def reset_parameters(self):
        # U(-1/sqrt(fan_in), +1/sqrt(fan_in)) weights, zero bias (dcn_v2.py:75-81)
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.zero_()

    def forward(self, input, offset, mask):
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert offset.shape[1] == 2 * taps and mask.shape[1] == taps
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding,
                           self.dilation, self.deformable_groups, self._pack_token)


class DCN(DCNv2):
    """DCNv2 that predicts its own offsets and modulation mask from the input."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1,
                 deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset_mask = hnn.Conv2d(in_channels, 3 * taps, self.kernel_size, self.stride,
                                           self.padding, bias=True)
        self.emit_stats = False      # set by a caller whose next layer is a BatchNorm2d (backends.dla.DeformConv)
        # offset regime of this layer (cnuda_dcn_set_offset_regime): re-measured every CENSUS_EVERY training forwards by
        # a census of its own offsets -- one small launch and one host read, i.e. one synchronisation per layer and 64 steps
        self._regime, self._census_calls = 0, 0
        with torch.no_grad():        # zero init: offsets 0, mask sigmoid(0)=0.5 (dcn_v2.py:114-116, Q7)
            self.conv_offset_mask.weight.zero_()
            self.conv_offset_mask.bias.zero_()

    def forward(self, input):
        # the input feeds the offset / mask convolution AND the sampling: their gradients meet in a slot, not in the engine
        input_om, input = fork(input, 2)
        taps = self.kernel_size[0] * self.kernel_size[1]
        cm = self.conv_offset_mask
        # (a forward hook on `conv_offset_mask` -- bench.measure_dcn_offsets, a user's probe -- wants that module CALLED: then,
        # as with CNUDA_DCN_OM=0, the module runs and its output is split like the reference does)
        hooked = bool(cm._forward_hooks or cm._forward_pre_hooks or cm._backward_hooks)
        if self.deformable_groups == 1 and input.shape[3] >= 2 and USE_OM and not hooked:
            # round 6: the offset convolution's epilogue applies the mask's sigmoid and the deformable convolution reads
            # offsets and mask out of its one output tensor (no split kernels, no offset / mask tensors of their own)
            om = ops.conv2d_rowsig(input_om, cm.weight, cm.bias, cm.stride, cm.padding, 2 * taps, cm._pack_token)
            if om is not None:
                self._take_census(lambda: om.detach()[:, :2 * taps].contiguous())
                return ops.with_bn_stats(self.emit_stats and self.training, lambda box: _DeformConvOmFn.apply(
                    input, om, self.weight, self.bias, self.stride, self.padding, self.dilation, self._pack_token, box,
                    self._regime))
        om = cm(input_om)
        # channels [0, 2*taps) are offsets (chunks o1|o2 re-concatenated, dcn_v2.py:120-121),
        # [2*taps, 3*taps) the mask logits
        offset, mask = ops.split_offset_mask(om)
        if self.deformable_groups == 1:
            self._take_census(lambda: offset)
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding,
                           self.dilation, self.deformable_groups, self._pack_token,
                           emit_stats=self.emit_stats and self.training, regime=self._regime)

    CENSUS_EVERY = 64
    # shares of (pixel, tap) samples beyond +-2 px / +-3 px above which the wide-window walk / the gathering forward win
    # (profiles/r5_dcn_margin_sweep.txt, r4_dcnw_large_offsets.txt: the crossovers sit near sigma = 0.75 px and 1.25 px)
    CENSUS_SHARES = (0.015, 0.03)

    def _take_census(self, offsets):
        """Every CENSUS_EVERY-th training forward: the regime from a census of offsets() -- [B, 2 * taps, Ho, Wo], contiguous."""
        if self.training:
            self._census_calls += 1
            if self._census_calls % self.CENSUS_EVERY == 1:
                self._regime = self._census(offsets())

    def _census(self, offset):
        off = offset.detach()
        B, HW = off.shape[0], off.shape[2] * off.shape[3]
        taps = off.shape[1] // 2
        counts = torch.zeros(2, dtype=torch.int32, device=off.device)
        hr.check(hr.lib().cnuda_dcn_offset_census(hr.ptr(hr.f32c(off)), B, taps, HW, hr.ptr(counts), hr.stream()), 'census')
        n2, n3 = counts.tolist()
        total = float(B * taps * HW)
        return (1 if n2 > self.CENSUS_SHARES[0] * total else 0) | (2 if n3 > self.CENSUS_SHARES[1] * total else 0)


# ---------------------------------------------------------------------------------------------------------------------
# Deformable position-sensitive ROI pooling (libs/DCNv2/dcn_v2.py:132-303) on csrc/psroi.hip
# ---------------------------------------------------------------------------------------------------------------------
class _DCNv2Pooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size=1,
                part_size=None, sample_per_part=4, trans_std=.0):
        ctx.args = (int(no_trans), spatial_scale, output_dim, group_size, pooled_size,
                    pooled_size if part_size is None else part_size, sample_per_part, trans_std)
        output, output_count = _backend.dcn_v2_psroi_pooling_forward(input, rois, offset, *ctx.args)
        ctx.save_for_backward(input, rois, offset, output_count)
        return output

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, rois, offset, output_count = ctx.saved_tensors
        grad_input, grad_offset = _backend.dcn_v2_psroi_pooling_backward(grad_output, input, rois, offset, output_count,
                                                                         *ctx.args)
        return grad_input, None, grad_offset, None, None, None, None, None, None, None, None


def dcn_v2_pooling(input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                   sample_per_part=4, trans_std=.0):
    return _DCNv2Pooling.apply(input, rois, offset, spatial_scale, pooled_size, output_dim, no_trans, group_size,
                               part_size, sample_per_part, trans_std)


class DCNv2Pooling(nn.Module):
    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                 sample_per_part=4, trans_std=.0):
        super().__init__()
        self.spatial_scale = spatial_scale
        self.pooled_size = pooled_size
        self.output_dim = output_dim
        self.no_trans = no_trans
        self.group_size = group_size
        self.part_size = pooled_size if part_size is None else part_size
        self.sample_per_part = sample_per_part
        self.trans_std = trans_std

    def forward(self, input, rois, offset):
        # the reference's assertion (dcn_v2.py:209): through this layer only group_size 1 is reachable; the R-FCN layout
        # (channels = output_dim * group_size^2) goes through _ext directly
        assert input.shape[1] == self.output_dim
        if self.no_trans:
            offset = input.new()
        return dcn_v2_pooling(input, rois, offset, self.spatial_scale, self.pooled_size, self.output_dim, self.no_trans,
                              self.group_size, self.part_size, self.sample_per_part, self.trans_std)


class DCNPooling(DCNv2Pooling):
    """DCNv2Pooling that predicts its own offsets and modulation mask: plain pooling, three fully connected layers, then
    the deformable pooling times the sigmoid mask.  The two poolings run on this library's kernels; `offset_mask_fc`
    (nn.Linear + ReLU, [N, pooled_size^2 * output_dim] x deform_fc_dim matmuls) runs on torch as in the reference -- it is
    not part of the layer path this package replaces.  State-dict names as there: offset_mask_fc.{0,2,4}.{weight,bias}."""

    def __init__(self, spatial_scale, pooled_size, output_dim, no_trans, group_size=1, part_size=None,
                 sample_per_part=4, trans_std=.0, deform_fc_dim=1024):
        super().__init__(spatial_scale, pooled_size, output_dim, no_trans, group_size, part_size, sample_per_part,
                         trans_std)
        self.deform_fc_dim = deform_fc_dim
        if not no_trans:
            self.offset_mask_fc = nn.Sequential(
                nn.Linear(self.pooled_size * self.pooled_size * self.output_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.deform_fc_dim),
                nn.ReLU(inplace=True),
                nn.Linear(self.deform_fc_dim, self.pooled_size * self.pooled_size * 3))
            with torch.no_grad():        # zero init: offsets 0, mask sigmoid(0) = 0.5 (dcn_v2.py:256-257)
                self.offset_mask_fc[4].weight.zero_()
                self.offset_mask_fc[4].bias.zero_()

    def forward(self, input, rois):
        geom = (self.spatial_scale, self.pooled_size, self.output_dim)
        tail = (self.group_size, self.part_size, self.sample_per_part, self.trans_std)
        if self.no_trans:
            return dcn_v2_pooling(input, rois, input.new(), *geom, True, *tail)
        n = rois.shape[0]
        roi = dcn_v2_pooling(input, rois, input.new(), *geom, True, *tail)
        offset_mask = self.offset_mask_fc(roi.view(n, -1)).view(n, 3, self.pooled_size, self.pooled_size)
        o1, o2, mask = torch.chunk(offset_mask, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        return dcn_v2_pooling(input, rois, offset, *geom, False, *tail) * torch.sigmoid(mask)
