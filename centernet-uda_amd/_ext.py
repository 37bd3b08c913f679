"""Drop-in for the reference's native pybind module `_ext`
(libs/DCNv2/src/vision.cpp:4-8; imported as `import _ext as _backend` by
libs/DCNv2/dcn_v2.py:13).  Same two function names, same positional argument
order (input, weight, bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, dg),
same return values; the work is done by libcenternet_uda_hip.so on the current
HIP stream.  The module's other two functions, deformable PSROI pooling forward
and backward (vision.cpp:6-7), are at the end of this file, with the reference's
positional order (libs/DCNv2/src/dcn_v2.h:95-190) as well.
"""
import torch

import hip_runtime as hr


def _shapes(input, weight, offset, mask, kh, kw, dg):
    if input.dim() != 4 or weight.dim() != 4:
        raise RuntimeError("dcn_v2: input and weight must be 4-D")
    B, C, H, W = input.shape
    Co, Ck, wkh, wkw = weight.shape
    if (wkh, wkw) != (kh, kw):
        raise RuntimeError("Input shape and kernel shape wont match: (%d x %d vs %d x %d)." % (kh, kw, wkh, wkw))
    if Ck != C:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (C, Ck))
    return B, C, H, W, Co


def _out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return ((H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1)


def _forward(who, input, weight, bias, offset, mask, om, geom, Ho, Wo, want_columns, act_slope, pack_token, pack_version,
             stats_box):
    """The one forward call behind dcn_v2_forward (offset, mask; om None) and dcn_v2_forward_om (om; offset, mask None), which
    have validated their own tensor layout.  geom: (B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg).  -> (out, cols)"""
    B, C, H, W, Co, kh, kw = geom[:7]
    dg = geom[13]
    out = torch.empty((B, Co, Ho, Wo), dtype=torch.float32, device=input.device)
    cols = None
    if want_columns and W >= 2:          # (deformable_group > 1: the groups' buffers one behind the other, same size)
        cols = torch.empty((B, kh * kw * C, Ho * Wo), dtype=torch.float32, device=input.device)
    L = hr.lib()
    ws = hr.workspace(L.cnuda_dcn_v2_workspace_bytes(*geom), input.device)
    if dg == 1 and W >= 2:
        hr.prof_arm('dcn_fwd', B, C, H, W, Co, kh, kw, Ho, Wo)
    # stats_box (private): the caller's next layer is a train-mode BatchNorm (DeformConv, backends/dla.py:351-372) -- where
    # the kernel can, its epilogue leaves the per-channel sum / sum of squares of `out` per pixel block (appended to the box)
    stats, blk, rows = None, 0, 0
    if stats_box is not None and act_slope < 0:
        rec = hr.stats_side_output(stats_box, L.cnuda_dcn_v2_stats_block, geom, Ho * Wo, input.device)
        if rec is not None:
            stats, blk, rows = rec[:3]
    tail = (*geom, hr.ptr(ws), ws.numel(), hr.stream())
    # act_slope (not part of the reference's signature): fused epilogue activation of the BatchNorm-folded
    # inference path; -1 = none = the reference's operation
    with hr.pack_stamp(pack_token, weight, pack_version):     # (private) identity of the weights: pack cache
        if om is not None:
            rc = L.cnuda_dcn_v2_forward_om(hr.ptr(input), hr.ptr(weight), hr.ptr(bias), hr.ptr(om), hr.ptr(out), hr.ptr(cols),
                                           hr.ptr(stats), blk, rows, float(act_slope), *tail)
        elif stats is not None:
            who += '_stats'
            rc = L.cnuda_dcn_v2_forward_stats(hr.ptr(input), hr.ptr(weight), hr.ptr(bias), hr.ptr(offset), hr.ptr(mask),
                                              hr.ptr(out), hr.ptr(cols), hr.ptr(stats), blk, rows, *tail)
        else:
            rc = L.cnuda_dcn_v2_forward_act(hr.ptr(input), hr.ptr(weight), hr.ptr(bias), hr.ptr(offset), hr.ptr(mask),
                                            hr.ptr(out), hr.ptr(cols), float(act_slope), *tail)
        hr.check(rc, who)
    return out, cols


def _backward(who, input, weight, bias, offset, mask, om, grad_output, geom, columns, grad_weight, grad_bias, grad_input):
    """The one backward call behind dcn_v2_backward and dcn_v2_backward_om (as _forward).
    -> [grad_input, grad_offset, grad_mask, grad_weight, grad_bias], or [grad_input, grad_om, grad_weight, grad_bias]"""
    B, C, H, W, Co, kh, kw = geom[:7]
    g_in = grad_input if grad_input is not None else torch.empty_like(input)
    g_om = [torch.empty_like(om)] if om is not None else [torch.empty_like(offset), torch.empty_like(mask)]
    # the parameter gradients may be written straight into caller-owned buffers (the arena's gradient sink)
    g_wb = [grad_weight if grad_weight is not None else torch.empty_like(weight),
            grad_bias if grad_bias is not None else torch.empty_like(bias)]
    L = hr.lib()
    ws = hr.workspace(L.cnuda_dcn_v2_workspace_bytes(*geom), input.device)
    if geom[13] == 1:
        hr.prof_arm('dcn_bwd', B, C, H, W, Co, kh, kw, grad_output.shape[2], grad_output.shape[3])
    fn = L.cnuda_dcn_v2_backward_acc if om is None else L.cnuda_dcn_v2_backward_om
    hr.check(fn(hr.ptr(input), hr.ptr(weight), hr.ptr(bias), *[hr.ptr(t) for t in ((offset, mask) if om is None else (om,))],
                hr.ptr(grad_output), hr.ptr(columns), hr.ptr(g_in), 1 if grad_input is not None else 0,
                *[hr.ptr(g) for g in g_om + g_wb], *geom, hr.ptr(ws), ws.numel(), hr.stream()), who)
    return [g_in] + g_om + g_wb


def dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w,
                   pad_h, pad_w, dilation_h, dilation_w, deformable_group, _want_columns=False, _act_slope=-1.0,
                   _pack_token=0, _pack_version=None, _stats_box=None):
    hr.require_gpu(input, weight, bias, offset, mask)
    input, weight, bias, offset, mask = [hr.f32c(t) for t in (input, weight, bias, offset, mask)]
    B, C, H, W, Co = _shapes(input, weight, offset, mask, kernel_h, kernel_w, deformable_group)
    Ho, Wo = _out_hw(H, W, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w)
    T = kernel_h * kernel_w
    if tuple(offset.shape) != (B, 2 * T * deformable_group, Ho, Wo) or \
            tuple(mask.shape) != (B, T * deformable_group, Ho, Wo):
        raise RuntimeError("dcn_v2_forward: offset %s / mask %s do not match output %dx%d"
                           % (tuple(offset.shape), tuple(mask.shape), Ho, Wo))
    geom = (B, C, H, W, Co, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
            dilation_h, dilation_w, deformable_group)
    out, cols = _forward('dcn_v2_forward', input, weight, bias, offset, mask, None, geom, Ho, Wo, _want_columns, _act_slope,
                         _pack_token, _pack_version, _stats_box)
    return (out, cols) if _want_columns else out


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                    pad_h, pad_w, dilation_h, dilation_w, deformable_group, _columns=None, _grad_weight=None,
                    _grad_bias=None, _grad_input=None):
    """_grad_input: a buffer that already holds another consumer's share of the input's gradient (hip_runtime.fanout):
    the data-gradient walks add into it instead of into a cleared tensor.
    -> [grad_input, grad_offset, grad_mask, grad_weight, grad_bias]"""
    hr.require_gpu(input, weight, bias, offset, mask, grad_output)
    input, weight, bias, offset, mask, grad_output = [
        hr.f32c(t) for t in (input, weight, bias, offset, mask, grad_output)]
    B, C, H, W, Co = _shapes(input, weight, offset, mask, kernel_h, kernel_w, deformable_group)
    geom = (B, C, H, W, Co, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
            dilation_h, dilation_w, deformable_group)
    return _backward('dcn_v2_backward', input, weight, bias, offset, mask, None, grad_output, geom, _columns, _grad_weight,
                     _grad_bias, _grad_input)


# ---------------------------------------------------------------------------------------------------------------------
# Round 6 (not part of the reference's `_ext`): offsets and mask read straight out of `om`, the 3T-channel output of DCN's own
# offset convolution whose mask channels already went through the sigmoid (hip_runtime.ops.conv2d_rowsig) -- see
# include/centernet_uda_hip.h, cnuda_dcn_v2_forward_om.  Used by libs.DCNv2.dcn_v2.DCN only; deformable_group == 1.
# ---------------------------------------------------------------------------------------------------------------------
def dcn_v2_forward_om(input, weight, bias, om, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                      _want_columns=False, _pack_token=0, _stats_box=None, _act_slope=-1.0, _pack_version=None):
    hr.require_gpu(input, weight, bias, om)
    input, weight, bias, om = [hr.f32c(t) for t in (input, weight, bias, om)]
    B, C, H, W = input.shape
    Co = weight.shape[0]
    if weight.shape[1] != C or tuple(weight.shape[2:]) != (kernel_h, kernel_w):
        raise RuntimeError("dcn_v2_forward_om: weight %s does not match %d input channels / a %dx%d kernel"
                           % (tuple(weight.shape), C, kernel_h, kernel_w))
    Ho, Wo = _out_hw(H, W, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w)
    T = kernel_h * kernel_w
    if tuple(om.shape) != (B, 3 * T, Ho, Wo):
        raise RuntimeError("dcn_v2_forward_om: om %s does not match [%d, %d, %d, %d]" % (tuple(om.shape), B, 3 * T, Ho, Wo))
    geom = (B, C, H, W, Co, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, 1)
    return _forward('dcn_v2_forward_om', input, weight, bias, None, None, om, geom, Ho, Wo, _want_columns, _act_slope,
                    _pack_token, _pack_version, _stats_box)


def dcn_v2_backward_om(input, weight, bias, om, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                       dilation_h, dilation_w, _columns=None, _grad_weight=None, _grad_bias=None, _grad_input=None):
    """-> [grad_input, grad_om, grad_weight, grad_bias]; grad_om: the offsets' gradient in channels 0 .. 2T-1, the gradient of
    the mask's LOGIT in channels 2T .. 3T-1."""
    hr.require_gpu(input, weight, bias, om, grad_output)
    input, weight, bias, om, grad_output = [hr.f32c(t) for t in (input, weight, bias, om, grad_output)]
    B, C, H, W = input.shape
    geom = (B, C, H, W, weight.shape[0], kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, 1)
    return _backward('dcn_v2_backward_om', input, weight, bias, None, None, om, grad_output, geom, _columns, _grad_weight,
                     _grad_bias, _grad_input)


# ---------------------------------------------------------------------------------------------------------------------
# Deformable position-sensitive ROI pooling (libs/DCNv2/src/dcn_v2.h:95-190; csrc/psroi.hip).  fp32 only.
# ---------------------------------------------------------------------------------------------------------------------
def _psroi_geom(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                sample_per_part, trans_std):
    if input.dim() != 4:
        raise RuntimeError("dcn_v2_psroi_pooling: input must be 4-D")
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise RuntimeError("dcn_v2_psroi_pooling: rois must be [N, 5] (batch index, x1, y1, x2, y2), got %s"
                           % (tuple(rois.shape),))
    B, C, H, W = input.shape
    N = rois.shape[0]
    if C != output_dim * group_size * group_size:
        raise RuntimeError("dcn_v2_psroi_pooling: input has %d channels, output_dim * group_size^2 = %d"
                           % (C, output_dim * group_size * group_size))
    if no_trans:
        num_classes = 1
    else:
        if offset.dim() != 4 or offset.shape[0] != N or offset.shape[1] % 2 or offset.shape[1] == 0 or \
                tuple(offset.shape[2:]) != (part_size, part_size):
            raise RuntimeError("dcn_v2_psroi_pooling: offset %s does not match [%d, 2 * num_classes, %d, %d]"
                               % (tuple(offset.shape), N, part_size, part_size))
        num_classes = offset.shape[1] // 2
        if output_dim % num_classes:
            raise RuntimeError("dcn_v2_psroi_pooling: output_dim %d is not a multiple of the offset's %d classes"
                               % (output_dim, num_classes))
    return (B, C, H, W, N, 1 if no_trans else 0, float(spatial_scale), int(output_dim), int(group_size),
            int(pooled_size), int(part_size), int(sample_per_part), float(trans_std), num_classes)


def dcn_v2_psroi_pooling_forward(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                                 part_size, sample_per_part, trans_std):
    """-> (output, output_count), both [N, output_dim, pooled_size, pooled_size]; `offset` is an empty tensor with no_trans."""
    hr.require_gpu(input, rois, offset)
    input, rois = hr.f32c(input), hr.f32c(rois)
    geom = _psroi_geom(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                       sample_per_part, trans_std)
    offset = None if no_trans else hr.f32c(offset)
    shape = (rois.shape[0], output_dim, pooled_size, pooled_size)
    out = torch.empty(shape, dtype=torch.float32, device=input.device)
    count = torch.empty(shape, dtype=torch.float32, device=input.device)
    hr.check(hr.lib().cnuda_dcn_v2_psroi_pooling_forward(hr.ptr(input), hr.ptr(rois), hr.ptr(offset), hr.ptr(out),
                                                         hr.ptr(count), *geom, hr.stream()),
             'dcn_v2_psroi_pooling_forward')
    return out, count


def dcn_v2_psroi_pooling_backward(grad_output, input, rois, offset, output_count, no_trans, spatial_scale, output_dim,
                                  group_size, pooled_size, part_size, sample_per_part, trans_std, _grad_input=None):
    """-> (grad_input, grad_offset).  _grad_input (not part of the reference's signature): a buffer that already holds
    another consumer's share of the input's gradient; this call adds to it (as dcn_v2_backward does)."""
    hr.require_gpu(grad_output, input, rois, offset, output_count)
    grad_output, input, rois, output_count = [hr.f32c(t) for t in (grad_output, input, rois, output_count)]
    geom = _psroi_geom(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                       sample_per_part, trans_std)
    shape = (rois.shape[0], output_dim, pooled_size, pooled_size)
    if tuple(grad_output.shape) != shape or tuple(output_count.shape) != shape:
        raise RuntimeError("dcn_v2_psroi_pooling_backward: grad_output %s / output_count %s do not match %s"
                           % (tuple(grad_output.shape), tuple(output_count.shape), shape))
    offset = None if no_trans else hr.f32c(offset)
    if _grad_input is not None and (_grad_input.shape != input.shape or _grad_input.dtype != torch.float32 or
                                    not _grad_input.is_contiguous() or not _grad_input.is_cuda):
        raise RuntimeError("dcn_v2_psroi_pooling_backward: _grad_input must be a contiguous fp32 GPU tensor like input")
    grad_input = _grad_input if _grad_input is not None else torch.empty_like(input)
    grad_offset = torch.empty(0, dtype=torch.float32, device=input.device) if no_trans else torch.empty_like(offset)
    L = hr.lib()
    ws = hr.workspace(L.cnuda_dcn_v2_psroi_pooling_workspace_bytes(geom[0], geom[4], geom[7], geom[9]), input.device)
    hr.check(L.cnuda_dcn_v2_psroi_pooling_backward(hr.ptr(grad_output), hr.ptr(input), hr.ptr(rois), hr.ptr(offset),
                                                   hr.ptr(output_count), hr.ptr(grad_input),
                                                   1 if _grad_input is not None else 0,
                                                   None if no_trans else hr.ptr(grad_offset), *geom, hr.ptr(ws),
                                                   ws.numel(), hr.stream()),
             'dcn_v2_psroi_pooling_backward')
    return grad_input, grad_offset
