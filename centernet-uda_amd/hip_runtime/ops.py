"""torch.autograd plumbing around the C ABI.  Every op here launches hand-written
gfx950 kernels from libcenternet_uda_hip.so on torch's current HIP stream;
torch contributes tensors (device memory), the autograd tape and nothing else.
"""
import ctypes
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import check, f32c, lib, pack_stamp, prof_arm, ptr, require_gpu, stats_side_output, stream, workspace
from .arena import grad_sink
from .fanout import accumulate_in_place, accumulate_target, claim, first_writer, slot_of


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _ws(nbytes, like):
    w = workspace(nbytes, like.device)
    return ptr(w), w.numel()


def _param_grad(param, needed=True):
    """Where a parameter's gradient goes: -> (buffer the kernel writes, value handed back to autograd).
    Arena-managed parameters get their slot of the arena's staging buffer and autograd gets None (see
    arena.py, "Gradient sink"); anything else gets a fresh tensor that is returned as usual."""
    if not needed or param is None:
        return None, None
    v = grad_sink(param)
    if v is not None:
        return v, None
    t = torch.empty_like(param)
    return t, t


# ---------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------
def _conv_geom(x, weight, stride, padding):
    B, C, H, W = x.shape
    Co, Ck, kh, kw = weight.shape
    if Ck != C:
        raise RuntimeError("conv2d: input has %d channels, weight expects %d" % (C, Ck))
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    return (B, C, H, W, Co, kh, kw, sh, sw, ph, pw)


# One launch core per direction: workspace, prof_arm, pack_stamp (token 0: none) and check around the C-ABI call of geometry g.
def _conv_forward(g, x, weight, bias, act_slope=-1.0, token=0, version=None, residual=None, stats_box=None, sig_from=None,
                  norm=None, what='conv2d_forward'):
    """-> y.  The epilogue by keyword: residual (added before the activation), stats_box (BatchNorm statistics of y where
    this geometry's kernel leaves them: the record is appended), sig_from (sigmoid on the channels from there on), norm
    (x_raw, mean, invstd, gamma, beta, imgs_per_group: apply on load -- `x` is then only the placeholder's shape)."""
    B, C, H, W, Co, kh, kw, sh, sw, ph, pw = g
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    y = torch.empty((B, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    L = lib()
    wp, wn = _ws(L.cnuda_conv2d_workspace_bytes(*g), x)
    stats = None
    if stats_box is not None:
        rec = stats_side_output(stats_box, L.cnuda_conv2d_stats_block, g, Ho * Wo, x.device, per_image=True)
        stats = rec and rec[0]
    prof_arm('conv_fwd', B, C, H, W, Co, kh, kw, Ho, Wo)
    with pack_stamp(token, weight, version):
        if norm is not None:
            check(L.cnuda_conv2d_forward_norm_input(*[ptr(t) for t in norm[:5]], int(norm[5]), ptr(weight), ptr(bias), ptr(y),
                                                    ptr(stats), *g, float(act_slope), wp, wn, stream()),
                  'conv2d_forward_norm_input')
        elif sig_from is not None:
            check(L.cnuda_conv2d_forward_rowsig(ptr(x), ptr(weight), ptr(bias), ptr(y), int(sig_from), *g, wp, wn, stream()),
                  'conv2d_forward_rowsig')
        else:
            check(L.cnuda_conv2d_forward_stats(ptr(x), ptr(weight), ptr(bias), ptr(residual), ptr(y), ptr(stats), *g,
                                               float(act_slope), wp, wn, stream()), what)
    return y


def _conv_dgrad(g, gy, weight, out, addend=None, addend2=None, token=0, what='conv2d_backward_data'):
    """out = input gradient (+ addend + addend2: other consumers' shares, either may BE out) -> out"""
    L = lib()
    wp, wn = _ws(L.cnuda_conv2d_workspace_bytes(*g), gy)
    prof_arm('conv_dgrad', *g[:7], gy.shape[2], gy.shape[3])
    with pack_stamp(token, weight):
        check(L.cnuda_conv2d_backward_data_add(ptr(gy), ptr(weight), ptr(addend), ptr(addend2), ptr(out), *g, wp, wn,
                                               stream()), what)
    return out


def _conv_wgrad(g, x, gy, weight, bias=None, norm=None, what='conv2d_backward_weight'):
    """-> (gw, gb) as autograd takes them (_param_grad).  norm: (mean, invstd, gamma, beta, imgs_per_group) when `x` is the raw
    input of a deferred BatchNorm + ReLU, normalised again while it is staged."""
    gw_buf, gw = _param_grad(weight)
    gb_buf, gb = _param_grad(bias)
    L = lib()
    wp, wn = _ws(L.cnuda_conv2d_workspace_bytes(*g), x)
    prof_arm('conv_wgrad', *g[:7], gy.shape[2], gy.shape[3])
    if norm is not None:
        check(L.cnuda_conv2d_backward_weight_norm_input(ptr(x), *[ptr(t) for t in norm[:4]], int(norm[4]), ptr(gy), ptr(gw_buf),
                                                        ptr(gb_buf), *g, wp, wn, stream()), 'conv2d_backward_weight_norm_input')
    else:
        check(L.cnuda_conv2d_backward_weight(ptr(x), ptr(gy), ptr(gw_buf), ptr(gb_buf), *g, wp, wn, stream()), what)
    return gw, gb


class _Conv2d(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, act_slope, pack_token=0, stats_box=None, norm=None, sig_from=None):
        """sig_from (private, DCN's offset convolution): output channels >= sig_from get a sigmoid in the epilogue
        (cnuda_conv2d_forward_rowsig) and the gradient this node RECEIVES for them is taken as the gradient of their LOGITS
        -- the deformable convolution's backward multiplies by m (1 - m) where it stores (cnuda_dcn_v2_backward_om) -- so
        the backward below is the plain convolution's.
        norm: None, or (x_raw, mean, invstd, gamma, beta, imgs_per_group) when `x` is the never-written output of a
        BatchNorm + ReLU in deferred mode (batch_norm_act(defer_apply=True)): the kernel reads x_raw and normalises while it
        stages it (cnuda_conv2d_forward_norm_input); the gradient this node returns for `x` is the one with respect to the
        normalised activation, exactly what the BatchNorm's backward expects."""
        require_gpu(x, weight, bias)
        ctx.slot = slot_of(x)          # (hip_runtime.fanout: where the other consumers of x leave their share of its gradient)
        # (norm: `x` is the 4-byte placeholder of a deferred BatchNorm -- shape only; the kernel reads norm[0])
        x, weight = (x if norm is not None else f32c(x)), f32c(weight)
        bias = None if bias is None else f32c(bias)
        g = _conv_geom(x, weight, stride, padding)
        # (BatchNorm statistics of y from the GEMM's epilogue, where this geometry's kernel can give them)
        y = _conv_forward(g, x, weight, bias, act_slope, pack_token, stats_box=stats_box if act_slope < 0 else None,
                          sig_from=sig_from, norm=norm)
        ctx.geom, ctx.act_slope, ctx.has_bias, ctx.pack_token = g, act_slope, bias is not None, pack_token
        ctx.norm_ipg = None
        if norm is not None:
            # (x itself holds nothing: the weight gradient normalises x_raw again while it stages it)
            ctx.norm_ipg = int(norm[5])
            ctx.save_for_backward(norm[0], weight, y if act_slope >= 0 else None, bias, norm[1], norm[2], norm[3], norm[4])
        else:
            ctx.save_for_backward(x, weight, y if act_slope >= 0 else None, bias)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, y, bias = ctx.saved_tensors[:4]
        g = ctx.geom
        gy = f32c(gy)
        if ctx.act_slope >= 0:
            t = torch.empty_like(gy)
            check(lib().cnuda_act_backward(ptr(gy), ptr(y), ptr(t), gy.numel(), float(ctx.act_slope), stream()))
            gy = t
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx, addend, addend2 = accumulate_target(ctx.slot, x)     # the slots' content is summed in the GEMM's epilogue
            _conv_dgrad(g, gy, weight, gx, addend, addend2, ctx.pack_token)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            norm = None if ctx.norm_ipg is None else (*ctx.saved_tensors[4:], ctx.norm_ipg)
            gw, gb = _conv_wgrad(g, x, gy, weight, bias, norm)
        return gx, gw, gb, None, None, None, None, None, None, None


def conv2d_rowsig(x, weight, bias, stride, padding, sig_from, pack_token=0):
    """(private to libs.DCNv2.dcn_v2.DCN) y = conv2d(x, weight) + bias with a sigmoid on the channels >= sig_from; the
    gradient handed back to this node must already be that of those channels' logits.  None where no kernel has the
    epilogue (cnuda_conv2d_rowsig_supported): the caller then takes the split path."""
    g = _conv_geom(x, weight, stride, padding)
    if bias is None or not lib().cnuda_conv2d_rowsig_supported(*g):
        return None
    return _Conv2d.apply(x, weight, bias, stride, padding, -1.0, pack_token, None, None, int(sig_from))


EPILOGUE_STATS = True      # (A/B measurements flip it: profiles/microbench/ab_bn_stats.py)


def with_bn_stats(emit, call):
    """y = call(stats_box).  emit: the caller's next layer is a train-mode BatchNorm over y -- where the producing kernel can,
    it leaves sum / sum of squares per (pixel block, channel) beside y (the node appends the record to its stats_box);
    batch_norm_act finds them on the tensor.  Otherwise, or with EPILOGUE_STATS off, the node gets no box."""
    if not (emit and EPILOGUE_STATS):
        return call(None)
    box = []
    y = call(box)
    if box:
        y._cnuda_bn_stats = box[0]
    return y


def conv2d(x, weight, bias=None, stride=1, padding=0, act_slope=-1.0, pack_token=0, emit_stats=False):
    """y = act(conv2d(x, weight) + bias); act_slope < 0 none, 0 ReLU, 0.2 LeakyReLU(0.2).  pack_token: identity of
    the module that owns `weight` (hip_runtime.new_pack_token) -- lets the library keep the packed weight image
    until the weights change; 0 = re-pack on every call."""
    norm = getattr(x, '_cnuda_deferred_bn', None)        # (batch_norm_act(defer_apply=True): x was never written)
    if norm is not None:
        g = _conv_geom(x, weight, stride, padding)
        if not lib().cnuda_conv2d_norm_input_supported(*g):
            raise RuntimeError("conv2d: the input is a deferred BatchNorm output, but no apply-on-load kernel takes this "
                               "convolution (cnuda_conv2d_norm_input_supported); ask batch_norm_act to apply it")
    return with_bn_stats(emit_stats, lambda box: _Conv2d.apply(x, weight, bias, stride, padding, float(act_slope), pack_token,
                                                               box, norm, None))


# CNUDA_HEAD_SPARSE=0 (or ops.HEAD_SPARSE = False): a head whose gradient is the gather + masked-L1 loss's takes the dense
# backward like every other (A/B measurements: profiles/ab_bench.sh - CNUDA_HEAD_SPARSE=0)
HEAD_SPARSE = os.environ.get('CNUDA_HEAD_SPARSE', '1') != '0'
# The size rule of the sparse head backward, held here only: it is taken while HEAD_SPARSE_RATIO * M <= H * W.  Its cost
# grows with M (two 1x1 GEMMs over B * M rows, a gather, a scatter), the dense cost with H * W.  Measured on the real head
# (64 -> 256 -> 2, B = 16, every row active; profiles/head_sparse_ab.txt): the two meet at H * W = 19 M on the 128 x 128
# map (5 M on the 32 x 32 map, where both are launch-bound); twice the larger, rounded up.
HEAD_SPARSE_RATIO = 40


def _mark_sparse_rows(grad, ind, mask, B, M, HW):
    """`grad` [B, ch, HW] is zero outside the cells ind[b, m] with mask[b, m] set (_RegL1.backward wrote it so).  The mark is
    an attribute of this tensor OBJECT and names the version it was written at: a sum of two gradients, a hook's result,
    a retain_grad copy or a clone is another object and carries none."""
    grad._cnuda_sparse_rows = (ind, mask, B, M, HW, grad._version)


def _sparse_rows_of(gy, B, HW):
    """The (ind, mask, M) of a valid mark on `gy` for a head of B images and HW pixels, consumed; else None."""
    mark = gy.__dict__.pop('_cnuda_sparse_rows', None)
    if mark is None or mark[5] != gy._version or mark[2] != B or mark[4] != HW or not gy.is_contiguous():
        return None
    return mark[0], mark[1], mark[3]


class _ConvActConv1x1(Function):
    """A detection head, `nn.Sequential(Conv2d(C, Ch, k, padding) + ReLU, Conv2d(Ch, Co, 1))` (dla.py:474-483), as one
    tape node: the two forward launches are the ones two `_Conv2d` nodes make; backward computes the hidden map's
    gradient -- the 1x1 layer's input gradient times the ReLU's -- in one pass over the hidden map
    (cnuda_conv1x1_backward_data_act) instead of a K <= 8 GEMM launch followed by cnuda_act_backward's own pass."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, padding, act_slope, token1, token2, lead=None):
        require_gpu(x, w1, b1, w2, b2)
        # lead: only the first `lead` images of x go through the head (a UDA step's source half: forward_domains) -- the
        # gradient still covers all of x, zero beyond them, or simply added into what x's gradient slot already holds
        ctx.slot, ctx.full = slot_of(x), None
        if lead is not None and lead < x.shape[0]:
            ctx.full = x.shape
            x = f32c(x)[:lead]
        x, w1, w2 = f32c(x), f32c(w1), f32c(w2)
        b1 = None if b1 is None else f32c(b1)
        b2 = None if b2 is None else f32c(b2)
        g1 = _conv_geom(x, w1, 1, padding)
        hidden = _conv_forward(g1, x, w1, b1, act_slope, token1)
        g2 = _conv_geom(hidden, w2, 1, 0)
        y = _conv_forward(g2, hidden, w2, b2, -1.0, token2)
        ctx.g1, ctx.g2, ctx.act_slope, ctx.token1 = g1, g2, float(act_slope), token1
        ctx.has_b1, ctx.has_b2 = b1 is not None, b2 is not None
        ctx.save_for_backward(x, w1, b1, w2, b2, hidden)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w1, b1, w2, b2, hidden = ctx.saved_tensors
        g1, g2 = ctx.g1, ctx.g2
        L = lib()
        gy = f32c(gy)
        if gy.data_ptr() % 16:                 # (a view at an odd offset: the fused pass reads 16 bytes at a time)
            gy = gy.clone()
        B, Ch, Co = g1[0], g1[4], g2[4]
        rows = _sparse_rows_of(gy, B, hidden.shape[2] * hidden.shape[3])
        if rows is not None and HEAD_SPARSE:
            sparse = _ConvActConv1x1._backward_sparse(ctx, gy, *rows)
            if sparse is not None:
                return sparse
        gx = gw1 = gb1 = gw2 = gb2 = None
        if ctx.needs_input_grad[3] or (ctx.has_b2 and ctx.needs_input_grad[4]):
            gw2, gb2 = _conv_wgrad(g2, hidden, gy, w2, b2)
        gh = torch.empty_like(hidden)
        check(L.cnuda_conv1x1_backward_data_act(ptr(gy), ptr(w2), ptr(hidden), ptr(gh), B, Co, Ch, hidden.shape[2] * hidden.shape[3],
                                                ctx.act_slope, stream()), 'conv1x1_backward_data_act')
        if ctx.needs_input_grad[0]:
            slot = ctx.slot
            if ctx.full is None:
                gx, addend, addend2 = accumulate_target(slot, x)
                part = gx
            elif (gx := accumulate_in_place(slot)) is not None:
                part = addend = gx[:B]                          # the leading images' share lands on top of the slot's total
                addend2 = None
            else:
                gx = claim(slot, torch.empty(ctx.full, dtype=torch.float32, device=x.device))
                gx[B:].zero_()
                part, addend, addend2 = gx[:B], None, None
            _conv_dgrad(g1, gh, w1, part, addend, addend2, ctx.token1)
        if ctx.needs_input_grad[1] or (ctx.has_b1 and ctx.needs_input_grad[2]):
            gw1, gb1 = _conv_wgrad(g1, x, gh, w1, b1)
        return gx, gw1, gb1, gw2, gb2, None, None, None, None, None

    @staticmethod
    def _backward_sparse(ctx, gy, ind, mask, M):
        """backward() for a `gy` that is zero outside ind[b, m] where mask[b, m] (cnuda_head_backward_sparse): no gradient of
        the hidden map, no full-size GEMM.  The share of x's gradient is ADDED to the slot's buffer -- the consumer class of
        DCN's atomics and the max-pool scatter -- or to a zero-filled tensor that takes an empty slot.  -> backward()'s
        result, or None where the dense path has to run: a geometry the library does not take, a map too small for the
        size rule, a slot whose buffer belongs to somebody else."""
        x, w1, b1, w2, b2, hidden = ctx.saved_tensors
        B, C, H, W, Ch, kh, kw, sh, sw, ph, pw = ctx.g1
        Co = ctx.g2[4]
        L = lib()
        HW = hidden.shape[2] * hidden.shape[3]
        if HEAD_SPARSE_RATIO * M > HW or \
                not L.cnuda_head_backward_sparse_supported(B, M, C, H, W, Ch, Co, kh, kw, sh, sw, ph, pw):
            return None
        gx = part = None
        if ctx.needs_input_grad[0]:
            slot = ctx.slot
            if slot is not None and slot.buf is not None and not slot.owned:
                return None
            gx = accumulate_in_place(slot)
            if gx is None:
                gx = claim(slot, torch.zeros(ctx.full or x.shape, dtype=torch.float32, device=x.device))
            part = gx[:B]
        gw1 = gb1 = gw2 = gb2 = gw1_buf = gb1_buf = gw2_buf = gb2_buf = None
        if ctx.needs_input_grad[1] or (ctx.has_b1 and ctx.needs_input_grad[2]):
            (gw1_buf, gw1), (gb1_buf, gb1) = _param_grad(w1), _param_grad(b1)
        if ctx.needs_input_grad[3] or (ctx.has_b2 and ctx.needs_input_grad[4]):
            (gw2_buf, gw2), (gb2_buf, gb2) = _param_grad(w2), _param_grad(b2)
        wp, wn = _ws(L.cnuda_head_backward_sparse_workspace_bytes(B, M, C, H, W, Ch, Co, kh, kw), x)
        check(L.cnuda_head_backward_sparse(ptr(gy), ptr(ind), ptr(mask), ptr(x), ptr(hidden), ptr(w1), ptr(w2), ptr(part),
                                           ptr(gw1_buf), ptr(gb1_buf), ptr(gw2_buf), ptr(gb2_buf), B, M, C, H, W, Ch, Co, kh, kw,
                                           ctx.act_slope, wp, wn, stream()), 'head_backward_sparse')
        return gx, gw1, gb1, gw2, gb2, None, None, None, None, None


def conv_act_conv1x1_supported(x, conv, last):
    """The fused head node applies: stride-1 `conv` with an activation, a 1x1 `last` with 1..8 outputs, planes of a
    multiple of 4 pixels, and a tape being recorded."""
    if not (torch.is_grad_enabled() and x.is_cuda and x.dim() == 4):
        return False
    (kh, kw), (ph, pw) = conv.kernel_size, conv.padding
    hw = (x.shape[2] + 2 * ph - kh + 1) * (x.shape[3] + 2 * pw - kw + 1)
    return (conv.act_slope >= 0 and conv.stride == (1, 1) and last.kernel_size == (1, 1) and last.stride == (1, 1)
            and last.padding == (0, 0) and last.act_slope < 0 and 1 <= last.out_channels <= 8 and hw > 0 and hw % 4 == 0)


def conv_act_conv1x1(x, conv, last, lead=None):
    """last(conv(x)) for the two `hip_runtime.nn.Conv2d` layers of a detection head, recorded as one tape node.
    lead: evaluate the first `lead` images of x only (the result has `lead` images; x's gradient is whole)."""
    return _ConvActConv1x1.apply(x, conv.weight, conv.bias, last.weight, last.bias, conv.padding, conv.act_slope,
                                 conv._pack_token, last._pack_token, lead)


def conv2d_infer(x, weight, bias=None, stride=1, padding=0, act_slope=-1.0, residual=None, pack_token=0,
                 pack_version=None):
    """Tape-free y = act(conv2d(x, weight) + bias + residual): the forward kernel with the skip connection in its
    epilogue -- what a BatchNorm-folded BasicBlock needs (export.py).  No autograd node is created."""
    require_gpu(x, weight, bias, residual)
    x, weight = f32c(x.detach()), f32c(weight.detach())
    bias = None if bias is None else f32c(bias.detach())
    g = _conv_geom(x, weight, stride, padding)
    B, C, H, W, Co, kh, kw, sh, sw, ph, pw = g
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    if residual is not None:
        residual = f32c(residual.detach())
        if tuple(residual.shape) != (B, Co, Ho, Wo):
            raise RuntimeError("conv2d_infer: residual %s does not match the output %s"
                               % (tuple(residual.shape), (B, Co, Ho, Wo)))
    return _conv_forward(g, x, weight, bias, act_slope, pack_token, pack_version, residual=residual)


class _ConvTranspose2d(Function):
    """nn.ConvTranspose2d(Cin, Cout, k, stride, padding, bias=False) (backends/resnet.py:86-94): the input
    gradient of the convolution whose weight is this [Cin, Cout, kh, kw] tensor read as [Cout_conv, Cin_conv, ...];
    its own gradients are that convolution's forward (grad_x) and weight gradient (roles of x and grad_y
    swapped) -- the same three C entry points as _Conv2d."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding, output_padding):
        require_gpu(x, weight)
        x, weight = f32c(x), f32c(weight)
        B, Ci, H, W = x.shape
        if weight.shape[0] != Ci:
            raise RuntimeError("conv_transpose2d: input has %d channels, weight expects %d" % (Ci, weight.shape[0]))
        Co, kh, kw = weight.shape[1], weight.shape[2], weight.shape[3]
        (sh, sw), (ph, pw), (oph, opw) = _pair(stride), _pair(padding), _pair(output_padding)
        Ho, Wo = (H - 1) * sh - 2 * ph + kh + oph, (W - 1) * sw - 2 * pw + kw + opw
        # geometry of the convolution  y[B,Co,Ho,Wo] -> x[B,Ci,H,W]
        g = (B, Co, Ho, Wo, Ci, kh, kw, sh, sw, ph, pw)
        if (Ho + 2 * ph - kh) // sh + 1 != H or (Wo + 2 * pw - kw) // sw + 1 != W:
            raise RuntimeError("conv_transpose2d: output_padding %s inconsistent with stride %s" %
                               ((oph, opw), (sh, sw)))
        y = torch.empty((B, Co, Ho, Wo), dtype=torch.float32, device=x.device)
        ctx.geom = g
        ctx.save_for_backward(x, weight)
        return _conv_dgrad(g, x, weight, y, what='conv_transpose2d(forward)')

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        g = ctx.geom
        gy = f32c(gy)
        gx = gw = None
        if ctx.needs_input_grad[0]:       # (the convolution's forward over gy: its output has x's shape)
            gx = _conv_forward(g, gy, weight, None, what='conv_transpose2d(backward data)')
        if ctx.needs_input_grad[1]:
            gw, _ = _conv_wgrad(g, gy, x, weight, what='conv_transpose2d(backward weight)')
        return gx, gw, None, None, None


def conv_transpose2d(x, weight, stride=1, padding=0, output_padding=0):
    return _ConvTranspose2d.apply(x, weight, stride, padding, output_padding)


# ---------------------------------------------------------------------------
# batch norm (+ residual add + ReLU)
# ---------------------------------------------------------------------------
def _act_code(relu):
    """fused activation of the BN kernels: False / True (ReLU) / 6 (ReLU6)"""
    if relu is True or relu is False or relu is None:
        return 1 if relu else 0
    if relu == 6:
        return 2
    raise ValueError("batch_norm_act: relu must be False, True or 6, got %r" % (relu,))


class _BatchNormAct(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, momentum, eps, relu, num_batches_tracked,
                groups, pre=None, defer=False):
        require_gpu(x, gamma, beta, residual)
        ctx.res_slot = None if residual is None else slot_of(residual)
        x = f32c(x)
        residual = None if residual is None else f32c(residual)
        B, C = x.shape[0], x.shape[1]
        if B % groups:
            raise RuntimeError("batch_norm_act: batch of %d images cannot be split into %d domain groups" % (B, groups))
        HW = x.numel() // (B * C)
        mean = torch.empty(groups * C, dtype=torch.float32, device=x.device)
        invstd = torch.empty(groups * C, dtype=torch.float32, device=x.device)
        L = lib()
        wp, wn = _ws(L.cnuda_bn_workspace_bytes(B, C, HW), x)
        bpg = 0
        if pre is not None and pre[2] >= C:
            # blocks per statistics group: whole images' worth of row pieces, or whole blocks of the flattened pixel axis
            if pre[3]:
                bpg = B // groups * pre[3]
            elif (B // groups * HW) % pre[1] == 0:
                bpg = B // groups * HW // pre[1]
        # defer: the statistics only -- y stays unwritten, its consumer (ops.conv2d) normalises x while it stages it
        ctx.deferred = bool(defer and bpg and residual is None and relu in (True, 1))
        # deferred: nothing is ever written, so the output is a 4-byte placeholder of the right SHAPE (all strides 0) --
        # no 537-MB allocation at the stem, and an accidental reader (f32c raises on the mark) cannot mistake it for data
        y = torch.empty_strided(x.shape, (0,) * x.dim(), dtype=torch.float32, device=x.device) if ctx.deferred \
            else torch.empty_like(x)
        if bpg:
            # sum(x) / sum(x^2) came with x from the producing GEMM's epilogue: no statistics pass over x
            check(L.cnuda_bn_train_forward_stats(ptr(x), ptr(pre[0]), bpg, pre[2], ptr(gamma), ptr(beta), ptr(residual),
                                                 ptr(None if ctx.deferred else y), ptr(mean), ptr(invstd), ptr(running_mean), ptr(running_var),
                                                 ptr(num_batches_tracked), float(momentum), float(eps), _act_code(relu),
                                                 B, C, HW, groups, wp, wn, stream()), 'bn_train_forward_stats')
        else:
            check(L.cnuda_bn_train_forward(ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(invstd),
                                           ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), float(momentum),
                                           float(eps),
                                           _act_code(relu), B, C, HW, groups, wp, wn, stream()), 'bn_train_forward')
        ctx.relu, ctx.dims, ctx.has_res, ctx.groups = relu, (B, C, HW), residual is not None, groups
        # y is read by the backward only where a residual entered the activation; without one the gate is recomputed
        # from x (cnuda_bn_backward, `beta` given) and y is not kept
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, gamma, mean, invstd, beta)
        if ctx.deferred:
            ctx.mark_non_differentiable(mean, invstd)
            return y, mean, invstd
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, *_unused):
        x, y, gamma, mean, invstd, beta = ctx.saved_tensors
        B, C, HW = ctx.dims
        gy = f32c(gy)
        gx = torch.empty_like(x)
        gres = first_writer(ctx.res_slot, x) if ctx.has_res else None
        gg_buf, gg = _param_grad(gamma)
        gb_buf, gb = _param_grad(beta)
        L = lib()
        wp, wn = _ws(L.cnuda_bn_workspace_bytes(B, C, HW), x)
        # without a residual the activation's gate is recomputed from x (y is not read): beta goes along for that
        regate = beta if (ctx.relu and not ctx.has_res) else None
        check(L.cnuda_bn_backward(ptr(gy), ptr(x), ptr(y), ptr(gamma), ptr(regate), ptr(mean), ptr(invstd), ptr(gx),
                                  ptr(gres), ptr(gg_buf), ptr(gb_buf), _act_code(ctx.relu), B, C, HW, ctx.groups, wp, wn,
                                  stream()), 'bn_backward')
        return gx, gg, gb, gres, None, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5,
                   residual=None, relu=False, num_batches_tracked=None, groups=None, defer_apply=False):
    """`num_batches_tracked` (int64 scalar buffer, optional) is incremented by the statistics kernel in training
    mode, like nn.BatchNorm2d.forward does on the host.  `groups` (default: hip_runtime.current_groups()):
    statistics groups of a batch that carries several domains, see hip_runtime.domain_groups.
    defer_apply (training, ReLU, no residual, statistics from the producing GEMM's epilogue; ignored otherwise): the
    returned tensor is NOT written -- it carries `_cnuda_deferred_bn`, and the one consumer the caller vouches for,
    ops.conv2d, normalises x while it stages it (apply on load: one write and one read of the activation less)."""
    if groups is None:
        from . import current_groups
        groups = current_groups()
    if training:
        if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or
                                                not num_batches_tracked.is_cuda):
            raise RuntimeError("batch_norm_act: num_batches_tracked must be an int64 tensor on the GPU")
        from . import bump_buffer_epoch
        bump_buffer_epoch()         # the kernel rewrites the running statistics behind torch's version counters
        out = _BatchNormAct.apply(x, gamma, beta, residual, running_mean, running_var, momentum, eps, relu,
                                  num_batches_tracked, int(groups), getattr(x, '_cnuda_bn_stats', None), bool(defer_apply))
        if isinstance(out, tuple):                  # deferred: (unwritten y, mean, invstd)
            y, mean, invstd = out
            y._cnuda_deferred_bn = (f32c(x).detach(), mean, invstd, f32c(gamma).detach(), f32c(beta).detach(),
                                    x.shape[0] // int(groups))
            return y
        return out
    if torch.is_grad_enabled() and (x.requires_grad or gamma.requires_grad):
        raise RuntimeError("batch_norm_act: eval-mode BN has no backward in this build "
                           "(the reference evaluates under torch.no_grad(), train.py:172)")
    require_gpu(x, gamma, beta, residual)
    x = f32c(x)
    residual = None if residual is None else f32c(residual)
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    check(lib().cnuda_bn_eval_forward(ptr(x), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                      ptr(residual), ptr(y), float(eps), _act_code(relu), B, C, HW, stream()),
          'bn_eval_forward')
    return y


# ---------------------------------------------------------------------------
# spatial
# ---------------------------------------------------------------------------
class _MaxPool(Function):
    @staticmethod
    def forward(ctx, x, k):
        require_gpu(x)
        ctx.slot = slot_of(x)
        x = f32c(x)
        B, C, H, W = x.shape
        y = torch.empty((B, C, H // k, W // k), dtype=torch.float32, device=x.device)
        check(lib().cnuda_maxpool2d_forward(ptr(x), ptr(y), B, C, H, W, k, stream()), 'maxpool2d_forward')
        ctx.k = k
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        # another consumer's share already in the slot's own buffer: only the arg-max cells are touched (+=)
        gx, acc = accumulate_in_place(ctx.slot), 1
        if gx is None:
            gx, acc = first_writer(ctx.slot, x), 0
        check(lib().cnuda_maxpool2d_backward_acc(ptr(x), ptr(f32c(gy)), ptr(gx), acc, B, C, H, W, ctx.k, stream()),
              'maxpool2d_backward')
        return gx, None


class _MaxPoolWindow(Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        require_gpu(x)
        x = f32c(x)
        B, C, H, W = x.shape
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        check(lib().cnuda_maxpool2d_window_forward(ptr(x), ptr(y), B, C, H, W, k, s, p, stream()),
              'maxpool2d_window_forward')
        ctx.ksp = (k, s, p)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        gx = torch.empty_like(x)
        check(lib().cnuda_maxpool2d_window_backward(ptr(x), ptr(f32c(gy)), ptr(gx), B, C, H, W, *ctx.ksp, stream()),
              'maxpool2d_window_backward')
        return gx, None, None, None


def max_pool2d(x, k, stride=None, padding=0):
    """nn.MaxPool2d(k, stride, padding) (floor mode).  stride == k without padding is the DLA downsample
    (dla.py:202-203); the general window is torchvision's ResNet stem pool."""
    k = int(k)
    stride = k if stride is None else int(stride)
    if stride == k and padding == 0:
        return _MaxPool.apply(x, k)
    return _MaxPoolWindow.apply(x, k, stride, int(padding))


class _DwConvT(Function):
    @staticmethod
    def forward(ctx, x, weight, stride, padding, skip=None):
        require_gpu(x, weight)
        x, weight = f32c(x), f32c(weight)
        B, C, H, W = x.shape
        k = weight.shape[2]
        if weight.shape[0] != C or weight.shape[1] != 1 or weight.shape[3] != k:
            raise RuntimeError("depthwise conv_transpose2d: weight %s does not fit %d channels"
                               % (tuple(weight.shape), C))
        Ho, Wo = (H - 1) * stride - 2 * padding + k, (W - 1) * stride - 2 * padding + k
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        if skip is not None:
            require_gpu(skip)
            skip = f32c(skip)
            if skip.shape != y.shape:
                raise RuntimeError("depthwise conv_transpose2d: summand %s does not fit the output %s"
                                   % (tuple(skip.shape), tuple(y.shape)))
        check(lib().cnuda_dwconvt2d_add_forward(ptr(x), ptr(weight), ptr(skip), ptr(y), B, C, H, W, k, stride, padding,
                                                stream()), 'dwconvt2d_forward')
        ctx.geom = (B, C, H, W, k, stride, padding)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw_buf, gw = _param_grad(weight, ctx.needs_input_grad[1])
        L = lib()
        B, C, _, _, k = ctx.geom[:5]
        wp, wn = _ws(L.cnuda_dwconvt2d_workspace_bytes(B, C, k), x)
        check(L.cnuda_dwconvt2d_backward(ptr(x), ptr(weight), ptr(f32c(gy)), ptr(gx), ptr(gw_buf), *ctx.geom,
                                         wp, wn, stream()), 'dwconvt2d_backward')
        return gx, gw, None, None, (gy if ctx.needs_input_grad[4] else None)


def depthwise_conv_transpose2d(x, weight, stride, padding, skip=None):
    """Depthwise ConvTranspose2d; with `skip` the result is `conv_transpose(x) + skip` written in one pass."""
    return _DwConvT.apply(x, weight, int(stride), int(padding), skip)


class _DwConvSame(Function):
    """Depthwise convolution (groups == channels), weight [C,1,k,k], no bias: pads = (top, left, bottom, right) zeros,
    which may differ per side (TensorFlow's "SAME" padding) or be torch's one `padding`.  Both entry pairs of the library
    run the same kernels; `same` picks the pair, and with it the argument contract: cnuda_dwconv2d_same_* (stride 1 or 2,
    every side's padding below k) or cnuda_dwconv2d_* (pads all equal; any stride and padding)."""

    @staticmethod
    def forward(ctx, x, weight, stride, pads, same=True):
        require_gpu(x, weight)
        x, weight = f32c(x), f32c(weight)
        B, C, H, W = x.shape
        k = weight.shape[2]
        if weight.shape[0] != C or weight.shape[1] != 1 or weight.shape[3] != k:
            raise RuntimeError("depthwise conv2d: weight %s does not fit %d channels" % (tuple(weight.shape), C))
        pt, pl, pb, pr = pads
        Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
        if Ho < 1 or Wo < 1:
            raise RuntimeError("depthwise conv2d: a %dx%d map with padding %s is smaller than the kernel" % (H, W, pads))
        y = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
        ctx.entry = 'dwconv2d_same' if same else 'dwconv2d'
        ctx.geom = (B, C, H, W, k, stride, pt, pl, Ho, Wo) if same else (B, C, H, W, k, stride, pt)
        check(getattr(lib(), 'cnuda_%s_forward' % ctx.entry)(ptr(x), ptr(weight), ptr(y), *ctx.geom, stream()),
              ctx.entry + '_forward')
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw_buf, gw = _param_grad(weight, ctx.needs_input_grad[1])
        L = lib()
        B, C, _, _, k = ctx.geom[:5]
        wp, wn = _ws(getattr(L, 'cnuda_%s_workspace_bytes' % ctx.entry)(B, C, k), x)
        check(getattr(L, 'cnuda_%s_backward' % ctx.entry)(ptr(x), ptr(weight), ptr(f32c(gy)), ptr(gx), ptr(gw_buf),
                                                          *ctx.geom, wp, wn, stream()), ctx.entry + '_backward')
        return gx, gw, None, None, None


def same_padding(size, kernel_size, stride):
    """TensorFlow's SAME rule for one axis of `size` pixels -> (before, after): total max((ceil(size/s)-1)*s + k - size, 0),
    the smaller half in front."""
    total = max((-(-size // stride) - 1) * stride + kernel_size - size, 0)
    return total // 2, total - total // 2


def depthwise_conv2d(x, weight, stride=1, padding=0):
    """nn.Conv2d(C, C, k, stride, padding, groups=C, bias=False)."""
    return _DwConvSame.apply(x, weight, int(stride), (int(padding),) * 4, False)


def depthwise_conv2d_same(x, weight, stride=1, pads=None):
    """pads (top, left, bottom, right); None: SAME padding derived from x's own size."""
    if pads is None:
        k = weight.shape[2]
        (pt, pb), (pl, pr) = same_padding(x.shape[2], k, int(stride)), same_padding(x.shape[3], k, int(stride))
        pads = (pt, pl, pb, pr)
    return _DwConvSame.apply(x, weight, int(stride), tuple(int(p) for p in pads))


class _Swish(Function):
    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        x = f32c(x)
        y = torch.empty_like(x)
        if x.numel():
            check(lib().cnuda_swish_forward(ptr(x), ptr(y), x.numel(), stream()), 'swish_forward')
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gx = torch.empty_like(x)
        if x.numel():
            check(lib().cnuda_swish_backward(ptr(f32c(gy)), ptr(x), ptr(gx), x.numel(), stream()), 'swish_backward')
        return gx


def swish(x):
    """x * sigmoid(x); the backward recomputes the sigmoid from x (the output is not kept)."""
    return _Swish.apply(x)


class _SqueezeExcite(Function):
    """y = x * sigmoid(W2 swish(W1 mean_hw(x) + b1) + b2): pool, gate (one workgroup per image) and scale kernels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        require_gpu(x, w1, b1, w2, b2)
        x, w1, b1, w2, b2 = [f32c(t) for t in (x, w1, b1, w2, b2)]
        B, C = x.shape[0], x.shape[1]
        HW = x.numel() // (B * C)
        Cse = w1.shape[0]
        if w1.numel() != Cse * C or w2.numel() != C * Cse or w2.shape[0] != C or b1.numel() != Cse or b2.numel() != C:
            raise RuntimeError("squeeze_excite: weights %s / %s, biases %s / %s do not fit %d channels"
                               % (tuple(w1.shape), tuple(w2.shape), tuple(b1.shape), tuple(b2.shape), C))
        y = torch.empty_like(x)
        pool = torch.empty((B, C), dtype=torch.float32, device=x.device)
        hpre = torch.empty((B, Cse), dtype=torch.float32, device=x.device)
        gate = torch.empty((B, C), dtype=torch.float32, device=x.device)
        ctx.dims = (B, C, Cse, HW)
        check(lib().cnuda_se_forward(ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(pool), ptr(hpre), ptr(gate),
                                     B, C, Cse, HW, stream()), 'se_forward')
        ctx.save_for_backward(x, w1, b1, w2, b2, pool, hpre, gate)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w1, b1, w2, b2, pool, hpre, gate = ctx.saved_tensors
        B, C, Cse, HW = ctx.dims
        gx = torch.empty_like(x)
        bufs, grads = zip(*[_param_grad(p, ctx.needs_input_grad[i + 1]) for i, p in enumerate((w1, b1, w2, b2))])
        L = lib()
        wp, wn = _ws(L.cnuda_se_workspace_bytes(B, C, Cse), x)
        check(L.cnuda_se_backward(ptr(x), ptr(f32c(gy)), ptr(w1), ptr(w2), ptr(pool), ptr(hpre), ptr(gate), ptr(gx),
                                  *[ptr(t) for t in bufs], B, C, Cse, HW, wp, wn, stream()), 'se_backward')
        return (gx if ctx.needs_input_grad[0] else None,) + tuple(grads)


def squeeze_excite(x, w_reduce, b_reduce, w_expand, b_expand):
    """w_reduce [Cse,C,1,1] (or [Cse,C]), w_expand [C,Cse,1,1]: the two 1x1 convolutions of an MBConv block's SE branch."""
    return _SqueezeExcite.apply(x, w_reduce, b_reduce, w_expand, b_expand)


class _DropConnectAdd(Function):
    @staticmethod
    def forward(ctx, x, mask, residual):
        require_gpu(x, mask, residual)
        if x.shape != residual.shape or mask.numel() != x.shape[0]:
            raise RuntimeError("drop_connect_add: x %s, residual %s, mask %s" % (tuple(x.shape), tuple(residual.shape),
                                                                                tuple(mask.shape)))
        x, mask, residual = f32c(x), f32c(mask), f32c(residual)
        y = torch.empty_like(x)
        ctx.dims = (x.shape[0], x.numel() // x.shape[0])
        check(lib().cnuda_drop_connect_add(ptr(x), ptr(mask), ptr(residual), ptr(y), *ctx.dims, stream()), 'drop_connect_add')
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        mask, = ctx.saved_tensors
        gy = f32c(gy)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(gy)
            check(lib().cnuda_drop_connect_add(ptr(gy), ptr(mask), None, ptr(gx), *ctx.dims, stream()), 'drop_connect_add')
        return gx, None, gy if ctx.needs_input_grad[2] else None


def drop_connect_add(x, mask, residual):
    """x * mask[b] + residual: the stochastic-depth branch of an MBConv block joined with its skip connection; mask [B] is
    the caller's (0 or 1 / keep probability per image)."""
    return _DropConnectAdd.apply(x, mask, residual)


def pad_right_bottom(x, pad_bottom, pad_right):
    """[B,C,H,W] -> [B,C,H+pad_bottom,W+pad_right], zeros added below / to the right (the SAME padding of a stride-2 stem in
    front of a padding-0 convolution).  No backward: for network inputs."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("pad_right_bottom has no backward in this build (it pads the network's input)")
    require_gpu(x)
    if pad_bottom == 0 and pad_right == 0:
        return x
    x = f32c(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, H + pad_bottom, W + pad_right), dtype=torch.float32, device=x.device)
    check(lib().cnuda_pad_right_bottom(ptr(x), ptr(y), B * C, H, W, int(pad_bottom), int(pad_right), stream()),
          'pad_right_bottom')
    return y


class _Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        require_gpu(a, b)
        if a.shape != b.shape:
            raise RuntimeError("add: shapes %s and %s differ" % (tuple(a.shape), tuple(b.shape)))
        a, b = f32c(a), f32c(b)
        out = torch.empty_like(a)
        check(lib().cnuda_add(ptr(a), ptr(b), ptr(out), a.numel(), stream()), 'add')
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


class _Cat(Function):
    @staticmethod
    def forward(ctx, *xs):
        require_gpu(*xs)
        slots = [slot_of(t) for t in xs]
        xs = [f32c(t) for t in xs]
        B, _, H, W = xs[0].shape
        chans = [t.shape[1] for t in xs]
        out = torch.empty((B, sum(chans), H, W), dtype=torch.float32, device=xs[0].device)
        off, L = 0, lib()
        for t, c in zip(xs, chans):
            if t.shape[0] != B or t.shape[2] != H or t.shape[3] != W:
                raise RuntimeError("cat: mismatching shapes")
            check(L.cnuda_copy_channels(ptr(t), ptr(out), B, c, H * W, c, 0, sum(chans), off, stream()), 'cat')
            off += c
        ctx.chans = chans
        ctx.slots = slots
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = f32c(g)
        B, Ct, H, W = g.shape
        outs, off, L = [], 0, lib()
        for i, c in enumerate(ctx.chans):
            if ctx.needs_input_grad[i]:
                t = claim(ctx.slots[i], torch.empty((B, c, H, W), dtype=torch.float32, device=g.device))
                check(L.cnuda_copy_channels(ptr(g), ptr(t), B, c, H * W, Ct, off, c, 0, stream()), 'cat_backward')
                outs.append(t)
            else:
                outs.append(None)
            off += c
        return tuple(outs)


def cat_channels(xs):
    return _Cat.apply(*xs)


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _cat_forward(xs, weight, bias, act_slope, token, version=None, stats_box=None):
    """One cnuda_conv2d_cat_forward launch over the sources xs -> (y, their channel counts); stats_box as _conv_forward"""
    B, _, H, W = xs[0].shape
    cs = [int(t.shape[1]) for t in xs]
    Co = weight.shape[0]
    g = (B, sum(cs), H, W, Co, 1, 1, 1, 1, 0, 0)
    L = lib()
    y = torch.empty((B, Co, H, W), dtype=torch.float32, device=weight.device)
    wp, wn = _ws(L.cnuda_conv2d_workspace_bytes(*g), y)
    stats = None
    if stats_box is not None:
        rec = stats_side_output(stats_box, L.cnuda_conv2d_stats_block, g, H * W, weight.device, per_image=True)
        stats = rec and rec[0]
    prof_arm('conv_fwd', B, sum(cs), H, W, Co, 1, 1, H, W)
    with pack_stamp(token, weight, version):
        check(L.cnuda_conv2d_cat_forward(_ptr_array(xs), (ctypes.c_int * len(cs))(*cs), len(xs), ptr(weight), ptr(bias), ptr(y),
                                         ptr(stats), float(act_slope), B, H, W, Co, wp, wn, stream()), 'conv2d_cat_forward')
    return y, cs


class _CatConv1x1(Function):
    """y = conv1x1(cat(xs, 1), weight) without the concatenation (cnuda_conv2d_cat_*): DLA's Root (backends/dla.py
    Root.forward; reference dla.py:150-168).  The input gradient of every source goes to that source's own tensor, with the
    other consumers' shares of its gradient added in the epilogue (hip_runtime.fanout), like _Conv2d's."""

    @staticmethod
    def forward(ctx, weight, pack_token, stats_box, *xs):
        require_gpu(weight, *xs)
        ctx.slots = [slot_of(t) for t in xs]
        xs = [f32c(t) for t in xs]
        weight = f32c(weight)
        B, _, H, W = xs[0].shape
        cin = sum(int(t.shape[1]) for t in xs)
        for t in xs:
            if t.shape[0] != B or t.shape[2] != H or t.shape[3] != W:
                raise RuntimeError("conv1x1_cat: mismatching shapes")
        if weight.shape[1] != cin or weight.shape[2] != 1 or weight.shape[3] != 1:
            raise RuntimeError("conv1x1_cat: weight %s for %d concatenated channels" % (tuple(weight.shape), cin))
        y, cs = _cat_forward(xs, weight, None, -1.0, pack_token, stats_box=stats_box)
        ctx.cs, ctx.pack_token = cs, pack_token
        ctx.save_for_backward(weight, *xs)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        weight, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        cs, n = ctx.cs, len(ctx.cs)
        B, _, H, W = xs[0].shape
        Co = weight.shape[0]
        g = (B, sum(cs), H, W, Co, 1, 1, 1, 1, 0, 0)
        L = lib()
        gy = f32c(gy)
        cs_arr = (ctypes.c_int * n)(*cs)
        wp, wn = _ws(L.cnuda_conv2d_workspace_bytes(*g), gy)
        gxs = [None] * n
        if any(ctx.needs_input_grad[3:]):
            outs, adds, add2s = [], [], []
            for i, x in enumerate(xs):
                if ctx.needs_input_grad[3 + i]:
                    out, a1, a2 = accumulate_target(ctx.slots[i], x)     # the slot's content is summed in the epilogue
                    gxs[i] = out
                else:
                    out, a1, a2 = torch.empty_like(x), None, None        # (a source outside the tape: its rows go to scratch)
                outs.append(out)
                adds.append(a1)
                add2s.append(a2)
            prof_arm('conv_dgrad', B, sum(cs), H, W, Co, 1, 1, H, W)
            with pack_stamp(ctx.pack_token, weight):
                check(L.cnuda_conv2d_cat_backward_data(ptr(gy), ptr(weight), _ptr_array(outs), _ptr_array(adds),
                                                       _ptr_array(add2s), cs_arr, n, B, H, W, Co, wp, wn, stream()),
                      'conv2d_cat_backward_data')
        gw = None
        if ctx.needs_input_grad[0]:
            gw_buf, gw = _param_grad(weight)
            prof_arm('conv_wgrad', B, sum(cs), H, W, Co, 1, 1, H, W)
            check(L.cnuda_conv2d_cat_backward_weight(_ptr_array(xs), cs_arr, n, ptr(gy), ptr(gw_buf), B, H, W, Co, wp, wn,
                                                     stream()), 'conv2d_cat_backward_weight')
        return (gw, None, None) + tuple(gxs)


def _cat_supported(xs, weight):
    xs = list(xs)
    if not (2 <= len(xs) <= 4) or any(t.dim() != 4 or getattr(t, '_cnuda_deferred_bn', None) is not None for t in xs):
        return False
    if weight.dim() != 4 or weight.shape[2] != 1 or weight.shape[3] != 1:
        return False
    B, _, H, W = xs[0].shape
    cs = [int(t.shape[1]) for t in xs]
    return bool(lib().cnuda_conv2d_cat_supported((ctypes.c_int * len(cs))(*cs), len(cs), B, H, W, int(weight.shape[0])))


def conv1x1_cat_infer(xs, weight, bias=None, act_slope=-1.0, pack_token=0, pack_version=None):
    """Tape-free y = act(conv1x1(cat(xs, 1), weight) + bias) without the concatenation (a BatchNorm-folded Root, export.py),
    or None where no kernel takes the sources (the caller concatenates)."""
    xs = list(xs)
    if not _cat_supported(xs, weight):
        return None
    require_gpu(weight, bias, *xs)
    xs = [f32c(t.detach()) for t in xs]
    weight = f32c(weight.detach())
    bias = None if bias is None else f32c(bias.detach())
    return _cat_forward(xs, weight, bias, act_slope, pack_token, pack_version)[0]


def conv1x1_cat(xs, weight, pack_token=0, emit_stats=False):
    """conv2d(cat(xs, 1), weight) for a 1x1 / stride 1 / bias-free convolution, or None where no kernel takes the sources as
    they are (cnuda_conv2d_cat_supported: 2 .. 4 sources of multiples of 64 channels, H * W % 4 == 0, no K split in the
    plan): the caller then concatenates.  emit_stats as ops.conv2d."""
    xs = list(xs)
    if not _cat_supported(xs, weight):
        return None
    return with_bn_stats(emit_stats, lambda box: _CatConv1x1.apply(weight, pack_token, box, *xs))


class _SplitOffsetMask(Function):
    @staticmethod
    def forward(ctx, om):
        require_gpu(om)
        om = f32c(om)
        B, C3, H, W = om.shape
        if C3 % 3:
            raise RuntimeError("conv_offset_mask output must have 3*taps channels, got %d" % C3)
        T = C3 // 3
        offset = torch.empty((B, 2 * T, H, W), dtype=torch.float32, device=om.device)
        mask = torch.empty((B, T, H, W), dtype=torch.float32, device=om.device)
        check(lib().cnuda_split_offset_mask(ptr(om), ptr(offset), ptr(mask), B, T, H * W, stream()),
              'split_offset_mask')
        ctx.save_for_backward(mask)
        return offset, mask

    @staticmethod
    @once_differentiable
    def backward(ctx, goff, gmask):
        (mask,) = ctx.saved_tensors
        B, T, H, W = mask.shape
        gom = torch.empty((B, 3 * T, H, W), dtype=torch.float32, device=mask.device)
        check(lib().cnuda_split_offset_mask_backward(ptr(f32c(goff)), ptr(f32c(gmask)), ptr(mask), ptr(gom), B, T,
                                                     H * W, stream()), 'split_offset_mask_backward')
        return gom


def split_offset_mask(om):
    return _SplitOffsetMask.apply(om)


# ---------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------
def _loss_ws(like):
    return _ws(lib().cnuda_loss_workspace_bytes(), like)


class _Focal(Function):
    """(loss, prob) = focal(clamp(sigmoid(logits)), gt)."""

    @staticmethod
    def forward(ctx, logits, gt, weight):
        require_gpu(logits, gt)
        logits, gt = f32c(logits), f32c(gt)
        if logits.shape != gt.shape:
            raise RuntimeError("focal loss: prediction %s vs target %s" % (tuple(logits.shape), tuple(gt.shape)))
        prob = torch.empty_like(logits)
        out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
        wp, wn = _loss_ws(logits)
        check(lib().cnuda_focal_loss_forward(ptr(logits), ptr(gt), ptr(prob), ptr(out2), logits.numel(),
                                             float(weight), wp, wn, stream()), 'focal_loss_forward')
        ctx.weight = weight
        ctx.save_for_backward(logits, gt, out2)
        den = out2[1].clone()                      # num_pos
        ctx.mark_non_differentiable(prob, den)
        return out2[0].clone(), prob, den

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _gprob, _gden):
        logits, gt, out2 = ctx.saved_tensors
        grad = torch.empty_like(logits)
        up = f32c(gloss.reshape(1))
        check(lib().cnuda_focal_loss_backward(ptr(logits), ptr(gt), ptr(out2), ptr(up), ptr(grad), logits.numel(),
                                              float(ctx.weight), stream()), 'focal_loss_backward')
        return grad, None, None


def focal_loss(logits, gt, weight=1.0, return_den=False):
    """-> (loss, prob[, num_pos]).  num_pos (a device scalar) is the divisor the loss used (0: none, sum of the
    negative terms only)."""
    loss, prob, den = _Focal.apply(logits, gt, weight)
    return (loss, prob, den) if return_den else (loss, prob)


def _l1_batch_check(name, expected, mask, ind, target):
    """dtypes and contiguity of the batch tensors of a gather + masked-L1 loss (`expected`: the loss's own wording)."""
    if mask.dtype != torch.uint8 or ind.dtype != torch.int64 or target.dtype != torch.float32:
        raise RuntimeError("%s: expected %s, got %s/%s/%s" % (name, expected, mask.dtype, ind.dtype, target.dtype))
    if not (mask.is_contiguous() and ind.is_contiguous() and target.is_contiguous()):
        raise RuntimeError("%s: batch tensors must be contiguous (target is updated in place)" % name)


def _l1_forward_tail(ctx, feat, mask, ind, target, out2):
    ctx.save_for_backward(feat, mask, ind, target, out2)
    den = out2[1].clone()                      # expanded-mask sum + 1e-4
    ctx.mark_non_differentiable(den)
    return out2[0].clone(), den


def _l1_backward(ctx, gloss, name, *pairs, rows_mark=False):
    """-> gradient w.r.t. feat; `pairs`: the pointer the keypoint entry point takes between target and out2.
    rows_mark: mask is [B, M] -- the dense map also says where it can be non-zero (_mark_sparse_rows: a detection head's
    backward then skips the zeros, _ConvActConv1x1._backward_sparse)."""
    feat, mask, ind, target, out2 = ctx.saved_tensors
    grad = torch.empty_like(feat)
    up = f32c(gloss.reshape(1))
    check(getattr(lib(), 'cnuda_' + name)(ptr(feat), ptr(mask), ptr(ind), ptr(target), *pairs, ptr(out2), ptr(up),
                                          ptr(grad), *ctx.args, stream()), name)
    if rows_mark and tuple(mask.shape) == tuple(ind.shape):
        _mark_sparse_rows(grad, ind, mask, feat.shape[0], ind.shape[1], feat.shape[2] * feat.shape[3])
    return grad


class _RegL1(Function):
    @staticmethod
    def forward(ctx, feat, mask, ind, target, periodic, weight, angle_weight):
        require_gpu(feat, mask, ind, target)
        feat = f32c(feat)
        _l1_batch_check('reg_l1', 'reg_mask uint8, ind int64, target float32 (datasets/coco.py:168-174)',
                        mask, ind, target)
        B, ch, H, W = feat.shape
        if ind.dim() != 2 or ind.shape[0] != B or tuple(mask.shape) != tuple(ind.shape) or \
                tuple(target.shape) != tuple(ind.shape) + (ch,):      # the kernel walks all three by (B, M, ch)
            raise RuntimeError("reg_l1: output %s vs ind %s / reg_mask %s / target %s"
                               % (tuple(feat.shape), tuple(ind.shape), tuple(mask.shape), tuple(target.shape)))
        M = ind.shape[1]
        out2 = torch.empty(2, dtype=torch.float32, device=feat.device)
        ctx.args = (B, M, ch, H * W, 1 if periodic else 0, float(weight), float(angle_weight))
        check(lib().cnuda_reg_l1_forward(ptr(feat), ptr(mask), ptr(ind), ptr(target), ptr(out2), *ctx.args, stream()),
              'reg_l1_forward')
        return _l1_forward_tail(ctx, feat, mask, ind, target, out2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _gden):
        return _l1_backward(ctx, gloss, 'reg_l1_backward', rows_mark=True), None, None, None, None, None, None


def reg_l1_loss(feat, mask, ind, target, periodic=False, weight=1.0, angle_weight=1.0, return_den=False):
    # `target` is a plain batch tensor (never requires grad); it is masked in place (Q2).
    loss, den = _RegL1.apply(feat, mask, ind, target, periodic, weight, angle_weight)
    return (loss, den) if return_den else loss


class _KpsL1(Function):
    @staticmethod
    def forward(ctx, feat, mask, ind, target, pairs, use_l1, weight, distance_weight):
        require_gpu(feat, mask, ind, target)
        feat = f32c(feat)
        _l1_batch_check('kps_l1', 'kp_reg_mask uint8, ind int64, kps float32 (datasets/coco.py:183-189)',
                        mask, ind, target)
        B, ch, H, W = feat.shape
        M = ind.shape[1]
        if ch % 2 or tuple(target.shape) != (B, M, ch) or tuple(mask.shape) != (B, M, ch):
            raise RuntimeError("kps_l1: output %s vs kps %s / kp_reg_mask %s"
                               % (tuple(feat.shape), tuple(target.shape), tuple(mask.shape)))
        P = 0 if pairs is None else pairs.shape[0]
        out2 = torch.empty(2, dtype=torch.float32, device=feat.device)
        ctx.args = (B, M, ch // 2, H * W, P, 1 if use_l1 else 0, float(weight), float(distance_weight))
        check(lib().cnuda_kps_l1_forward(ptr(feat), ptr(mask), ptr(ind), ptr(target), ptr(pairs), ptr(out2), *ctx.args,
                                         stream()), 'kps_l1_forward')
        ctx.pairs = pairs
        return _l1_forward_tail(ctx, feat, mask, ind, target, out2)

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _gden):
        return _l1_backward(ctx, gloss, 'kps_l1_backward', ptr(ctx.pairs)), None, None, None, None, None, None, None


def kps_l1_loss(feat, mask, ind, target, pairs=None, use_l1=False, weight=1.0, distance_weight=0.1, return_den=False):
    """KPSL1Loss (losses/centernet.py:136-189); `pairs` an int32 device tensor [P, 2] or None; `target` is masked
    in place."""
    loss, den = _KpsL1.apply(feat, mask, ind, target, pairs, use_l1, weight, distance_weight)
    return (loss, den) if return_den else loss


class _LogitsLoss(Function):
    """The losses of the logits alone.  `spec` = (stem, flat, workspace, is_map) names cnuda_<stem>_forward/_backward and
    their argument layout: logits, [extra scalars if flat], out, shape, [extra scalars if not flat], [loss workspace],
    stream -- the backward takes (upstream, grad) in the place of out and no workspace.  The shape is (numel) when
    flat, (B, C, HW) otherwise; the result is a scalar with a scalar upstream, or (is_map) a tensor like the logits
    with a full upstream tensor."""

    @staticmethod
    def forward(ctx, logits, spec, *extra):
        stem, flat, workspace, is_map = spec
        require_gpu(logits)
        logits = f32c(logits)
        if flat:
            lead, shape = extra, (logits.numel(),)
        else:
            B, C = logits.shape[0], logits.shape[1]
            lead, shape = (), (B, C, logits.numel() // (B * C)) + extra
        out = torch.empty_like(logits) if is_map else torch.empty(1, dtype=torch.float32, device=logits.device)
        ws = _loss_ws(logits) if workspace else ()
        check(getattr(lib(), 'cnuda_%s_forward' % stem)(ptr(logits), *lead, ptr(out), *shape, *ws, stream()),
              stem + '_forward')
        ctx.call = (stem, is_map, lead, shape, len(extra))
        ctx.save_for_backward(logits)
        return out if is_map else out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (logits,) = ctx.saved_tensors
        stem, is_map, lead, shape, n_extra = ctx.call
        grad = torch.empty_like(logits)
        up = f32c(g if is_map else g.reshape(1))
        check(getattr(lib(), 'cnuda_%s_backward' % stem)(ptr(logits), *lead, ptr(up), ptr(grad), *shape, stream()),
              stem + '_backward')
        return (grad, None) + (None,) * n_extra


#                     stem            flat  workspace  is_map        extra scalars
_SOFTMAX_LOSS     = ('softmax_loss',     False, True,  False)      # kind: 0 entropy, 1 max-squares
_ENTROPY_ETA_LOSS = ('entropy_eta_loss', False, True,  False)      # eta
_ENTROPY_MAP      = ('entropy_map',      False, False, True)
_BCE_CONST        = ('bce_const',        True,  False, False)      # label


def entropy_loss(hm_logits):
    return _LogitsLoss.apply(hm_logits, _SOFTMAX_LOSS, 0)


def max_square_loss(hm_logits):
    return _LogitsLoss.apply(hm_logits, _SOFTMAX_LOSS, 1)


def entropy_eta_loss(hm_logits, eta):
    """EntropyLoss(eta) (losses/entropy.py:17-22): mean over pixels of (e^2 + 1e-30)^eta, e the normalised softmax
    entropy over the channels."""
    return _LogitsLoss.apply(hm_logits, _ENTROPY_ETA_LOSS, float(eta))


def entropy_map(hm):
    return _LogitsLoss.apply(hm, _ENTROPY_MAP)


def _class_histogram(logits):
    """logits: contiguous fp32 [B, C, ...] on the GPU -> int32 [B, C]"""
    B, C = logits.shape[0], logits.shape[1]
    hist = torch.empty((B, C), dtype=torch.int32, device=logits.device)
    check(lib().cnuda_argmax_histogram(ptr(logits), ptr(hist), B, C, logits.numel() // (B * C), stream()),
          'argmax_histogram')
    return hist


def class_histogram(hm_logits):
    """hm_logits [B, C, H, W] -> int32 [B, C]: how many pixels of each image every class wins, the argmax taken on the
    logits with the lowest channel on a tie (np.argmax(x, 1)).  No gradient, no read-back."""
    require_gpu(hm_logits)
    return _class_histogram(f32c(hm_logits.detach()))


class _IWMaxSquare(Function):
    """_LogitsLoss's sibling with a saved side tensor: the [B, C] class weights the forward derives from the argmax
    histogram are constants of the backward pass."""

    @staticmethod
    def forward(ctx, logits, ratio):
        require_gpu(logits)
        logits = f32c(logits)
        B, C = logits.shape[0], logits.shape[1]
        shape = (B, C, logits.numel() // (B * C))
        hist = _class_histogram(logits)
        weights = torch.empty((B, C), dtype=torch.float32, device=logits.device)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        check(lib().cnuda_iw_max_square_forward(ptr(logits), ptr(hist), ratio, ptr(weights), ptr(out), *shape,
                                                *_loss_ws(logits), stream()), 'iw_max_square_forward')
        ctx.shape = shape
        ctx.save_for_backward(logits, weights)
        return out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logits, weights = ctx.saved_tensors
        grad = torch.empty_like(logits)
        up = f32c(g.reshape(1))
        check(lib().cnuda_iw_max_square_backward(ptr(logits), ptr(weights), ptr(up), ptr(grad), *ctx.shape, stream()),
              'iw_max_square_backward')
        return grad, None


def iw_max_square_loss(hm_logits, ratio=0.2):
    """Max-squares with the image-wise class-balanced weighting factor (Chen, Xue, Cai, ICCV 2019):
    -sum(softmax(hm)^2 * w[argmax]) / (2 B C),  w[b, c] = 1 / max(hist[b, c]^ratio * HW^(1 - ratio), 1),
    hist = class_histogram(hm).  The published form has no 1/2; it is here because MaxSquareLoss has it, so ratio = 0
    is MaxSquareLoss.  The weights carry no gradient."""
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("iw_max_square_loss: ratio must be in [0, 1], got %r" % (ratio,))
    return _IWMaxSquare.apply(hm_logits, ratio)


def _check_threshold(who, threshold):
    threshold = float(threshold)
    if not 0.0 <= threshold < 1.0:
        raise ValueError("%s: threshold must be in [0, 1), got %r" % (who, threshold))
    return threshold


def _guidance_forward(low, high, threshold):
    """low, high: contiguous fp32 [B, C, ...] on the GPU -> (labels int32 [B, ...], out2 = {loss, guided pixels})"""
    if low.shape != high.shape or low.dim() < 2:
        raise RuntimeError("guidance: low-level map %s vs final map %s" % (tuple(low.shape), tuple(high.shape)))
    B, C = low.shape[0], low.shape[1]
    shape = (B, C, low.numel() // (B * C))
    labels = torch.empty((B,) + tuple(low.shape[2:]), dtype=torch.int32, device=low.device)
    out2 = torch.empty(2, dtype=torch.float32, device=low.device)
    check(lib().cnuda_guidance_forward(ptr(high), ptr(low), threshold, ptr(labels), ptr(out2), *shape, *_loss_ws(low),
                                       stream()), 'guidance_forward')
    return labels, out2, shape


def guidance_labels(high, low, threshold=0.95):
    """high, low [B, C, H, W] (the final and the low-level heat map's logits) -> int32 [B, H, W]: the channel where the
    mean of the two class softmaxes is largest (the lowest on a tie) if that mean exceeds `threshold`, else -1.  No
    gradient, no read-back; a fresh tensor every call."""
    threshold = _check_threshold('guidance_labels', threshold)
    require_gpu(high, low)
    return _guidance_forward(f32c(low.detach()), f32c(high.detach()), threshold)[0]


class _Guidance(Function):
    """_IWMaxSquare's sibling with two inputs: the labels and their number, found from both maps in the forward, are
    constants of the backward pass, and only `low` has a gradient."""

    @staticmethod
    def forward(ctx, low, high, threshold):
        require_gpu(low, high)
        low, high = f32c(low), f32c(high)
        labels, out2, ctx.shape = _guidance_forward(low, high, threshold)
        ctx.save_for_backward(low, labels, out2)
        count = out2[1].clone()
        ctx.mark_non_differentiable(count)
        return out2[0].clone(), count

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gcount):
        low, labels, out2 = ctx.saved_tensors
        grad = torch.empty_like(low)
        up = f32c(g.reshape(1))
        check(lib().cnuda_guidance_backward(ptr(low), ptr(labels), ptr(out2), ptr(up), ptr(grad), *ctx.shape, stream()),
              'guidance_backward')
        return grad, None, None


def guidance_loss(low, high, threshold=0.95, return_count=False):
    """Multi-level self-produced guidance (Chen, Xue, Cai, ICCV 2019): the cross-entropy of softmax(low) against
    guidance_labels(high, low, threshold), summed over the guided pixels and divided by max(their number, 1) -- an exact 0
    with an all-zero gradient when there is none.  The gradient goes to `low` only: the labels are constants and `high`,
    whether it requires grad or not, gets None.  return_count: also the number of guided pixels (a device scalar)."""
    threshold = _check_threshold('guidance_loss', threshold)
    loss, count = _Guidance.apply(low, high, threshold)
    return (loss, count) if return_count else loss


def bce_with_logits_const(logits, label):
    return _LogitsLoss.apply(logits, _BCE_CONST, float(label))


# ---------------------------------------------------------------------------
# small helpers without gradients
# ---------------------------------------------------------------------------
def sigmoid_clamp_(x):
    """x <- sigmoid(x) in place; returns clamp(x, 1e-4, 1-1e-4) (utils/tensor.py:5-7)."""
    require_gpu(x)
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("sigmoid_clamp_ is an in-place, gradient-free helper; "
                           "training code goes through focal_loss / reg_l1_loss")
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise RuntimeError("sigmoid_clamp_: expected a contiguous float32 tensor")
    y = torch.empty_like(x)
    check(lib().cnuda_sigmoid_clamp_(ptr(x), ptr(y), x.numel(), stream()), 'sigmoid_clamp_')
    return y


def gather_feat(feat, ind):
    """feat [B,ch,H,W], ind [B,M] int64 -> [B,M,ch] (no gradient; the losses gather internally)."""
    require_gpu(feat, ind)
    feat = f32c(feat.detach())
    B, ch, H, W = feat.shape
    M = ind.shape[1]
    out = torch.empty((B, M, ch), dtype=torch.float32, device=feat.device)
    check(lib().cnuda_gather_feat(ptr(feat), ptr(ind.contiguous()), ptr(out), B, M, ch, H * W, stream()),
          'gather_feat')
    return out


def adam_step_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step):
    require_gpu(param, grad, exp_avg, exp_avg_sq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != param.numel():
            raise RuntimeError("adam_step_: flat contiguous float32 tensors of equal length required")
    check(lib().cnuda_adam_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                                float(beta1), float(beta2), float(eps), float(weight_decay), int(step), stream()),
          'adam_step')


def _flat_operands(what, param, *others):
    """param and every tensor of `others` that is not None: flat contiguous fp32 on the GPU, of one length."""
    require_gpu(param, *others)
    for t in (param,) + others:
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != param.numel()):
            raise RuntimeError("%s: flat contiguous float32 tensors of equal length required" % what)


def sgd_step_(param, grad, momentum_buffer, lr, momentum, dampening, weight_decay, nesterov, maximize, first):
    """torch.optim.SGD over one flat range (csrc/optim.hip).  momentum_buffer None <=> momentum == 0; `first`: the
    range's first update, which sets the buffer to the gradient."""
    _flat_operands('sgd_step_', param, grad, momentum_buffer)
    check(lib().cnuda_sgd_step(ptr(param), ptr(grad), ptr(momentum_buffer), param.numel(), float(lr), float(momentum),
                               float(dampening), float(weight_decay), int(bool(nesterov)), int(bool(maximize)),
                               int(bool(first)), stream()), 'sgd_step')


def adamw_step_(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps, weight_decay, decoupled,
                maximize, step):
    """The Adam family over one flat range: decoupled weight decay (AdamW) or L2, max_exp_avg_sq None <=> no amsgrad."""
    _flat_operands('adamw_step_', param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq)
    check(lib().cnuda_adamw_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(max_exp_avg_sq),
                                 param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                 int(bool(decoupled)), int(bool(maximize)), int(step), stream()), 'adamw_step')


def rmsprop_step_(param, grad, square_avg, grad_avg, momentum_buffer, lr, alpha, eps, weight_decay, momentum, maximize):
    """torch.optim.RMSprop over one flat range: grad_avg None <=> not centered, momentum_buffer None <=> momentum == 0."""
    _flat_operands('rmsprop_step_', param, grad, square_avg, grad_avg, momentum_buffer)
    check(lib().cnuda_rmsprop_step(ptr(param), ptr(grad), ptr(square_avg), ptr(grad_avg), ptr(momentum_buffer),
                                   param.numel(), float(lr), float(alpha), float(eps), float(weight_decay),
                                   float(momentum), int(bool(maximize)), stream()), 'rmsprop_step')


# ---------------------------------------------------------------------------
# Fourier domain adaptation (csrc/fda.hip)
# ---------------------------------------------------------------------------
def fda_source_to_target(src, trg, use_target_amp):
    """The amplitude transfer of FDA_source_to_target (utils/image.py:137-230) for a whole batch: src, trg [B,C,H,W]
    fp32 on the GPU, use_target_amp a uint8 [H, W//2+1] device tensor (non-zero: the bin takes the target's
    amplitude).  Returns a new [B,C,H,W] tensor.  Not differentiable: an input that requires grad is an error."""
    require_gpu(src, trg, use_target_amp)
    if src.requires_grad or trg.requires_grad:
        raise RuntimeError("fda_source_to_target is not differentiable (the reference never back-propagates "
                           "through it): pass detached inputs")
    if src.dim() != 4 or src.shape != trg.shape:
        raise RuntimeError("fda_source_to_target: src and trg must be [B,C,H,W] of one shape, got %s and %s"
                           % (tuple(src.shape), tuple(trg.shape)))
    B, C, H, W = src.shape
    if use_target_amp.dtype != torch.uint8 or tuple(use_target_amp.shape) != (H, W // 2 + 1):
        raise RuntimeError("fda_source_to_target: use_target_amp must be uint8 [%d, %d], got %s %s"
                           % (H, W // 2 + 1, use_target_amp.dtype, tuple(use_target_amp.shape)))
    src, trg, m = f32c(src), f32c(trg), use_target_amp.contiguous()
    out = torch.empty_like(src)
    wp, wn = _ws(lib().cnuda_fda_workspace_bytes(B, C, H, W), src)
    check(lib().cnuda_fda_source_to_target(ptr(src), ptr(trg), ptr(m), ptr(out), B, C, H, W, wp, wn, stream()),
          'fda_source_to_target')
    return out


# ---------------------------------------------------------------------------
# Running statistics on the device (csrc/meters.hip)
# ---------------------------------------------------------------------------
METER_SLOTS = 32


def meter_update(values, n, sums, counts, last):
    """values: 1 to 32 0-dim float32 device tensors; meter i of the device arrays sums / counts (float64) and last
    (float32), each of at least len(values) elements, takes sums[i] += float64(values[i]) * n, counts[i] += n,
    last[i] = values[i] -- one launch, nothing read back, nothing uploaded (the pointers travel in the kernel
    arguments).  The caller keeps stream order: the values are read on the current stream."""
    values = list(values)
    require_gpu(sums, counts, last, *values)
    S = len(values)
    if not 1 <= S <= METER_SLOTS:
        raise RuntimeError("meter_update: 1 to %d values per call, got %d" % (METER_SLOTS, S))
    for v in values:
        if v.dtype != torch.float32 or v.dim() != 0:
            raise RuntimeError("meter_update: values must be 0-dim float32 tensors, got %s %s"
                               % (v.dtype, tuple(v.shape)))
    if sums.dtype != torch.float64 or counts.dtype != torch.float64 or last.dtype != torch.float32 \
            or min(sums.numel(), counts.numel(), last.numel()) < S \
            or not (sums.is_contiguous() and counts.is_contiguous() and last.is_contiguous()):
        raise RuntimeError("meter_update: sums / counts must be contiguous float64 and last float32 arrays of at "
                           "least %d elements" % S)
    table = (ctypes.c_void_p * S)(*[v.data_ptr() for v in values])
    check(lib().cnuda_meter_update(table, S, float(n), ptr(sums), ptr(counts), ptr(last), stream()), 'meter_update')


# ---------------------------------------------------------------------------
# Mean teacher (csrc/teacher.hip)
# ---------------------------------------------------------------------------
EMA_PER_BLOCK = 4096            # elements (float32 EMA) or bytes (copy) per workgroup: csrc/teacher.hip kEmaPerBlock


def ema_segment_table(segments):
    """[(dst address, src address, count, kind)] -> (the table as a numpy record array with the layout of
    csrc/teacher.hip's EmaSegment, total workgroups).  Segments of no elements are left out."""
    import numpy as np
    dtype = np.dtype([('dst', '<u8'), ('src', '<u8'), ('count', '<i8'), ('kind', '<i4'), ('block0', '<u4')])
    rows, blocks = [], 0
    for dst, src, count, kind in segments:
        if count <= 0:
            continue
        rows.append((dst, src, count, kind, blocks))
        blocks += (count + EMA_PER_BLOCK - 1) // EMA_PER_BLOCK
    if blocks >= 1 << 31:
        raise RuntimeError("EmaPlan: %d workgroups exceed one launch" % blocks)
    return np.array(rows, dtype=dtype), blocks


class EmaPlan:
    """dst_tensors[i] <- EMA of itself and src_tensors[i], all pairs in ONE launch (cnuda_ema_update).

    A float32 pair is an element-wise `t = (t * d) + (s * omd)` with omd = float32(1) - float32(d): numpy's float32
    result bit for bit.  Any other dtype (integer buffers: num_batches_tracked) is copied byte for byte.  Tensors are
    contiguous device tensors of pairwise equal dtype and element count; a slice that starts at an odd element is fine.
    The segment table is built and uploaded once; `update` compares the tensors' addresses with the ones it was
    built from and rebuilds it when one moved (load_state_dict with assign, `.to()`, a re-pointed arena)."""

    def __init__(self, dst_tensors, src_tensors):
        self.dst, self.src = list(dst_tensors), list(src_tensors)
        if len(self.dst) != len(self.src):
            raise RuntimeError("EmaPlan: %d destinations for %d sources" % (len(self.dst), len(self.src)))
        require_gpu(*self.dst, *self.src)
        for i, (t, s) in enumerate(zip(self.dst, self.src)):
            if t.dtype != s.dtype or t.numel() != s.numel() or t.device != s.device:
                raise RuntimeError("EmaPlan: pair %d differs in dtype, length or device (%s %d %s / %s %d %s)"
                                   % (i, t.dtype, t.numel(), t.device, s.dtype, s.numel(), s.device))
            if not t.is_contiguous() or not s.is_contiguous():
                raise RuntimeError("EmaPlan: pair %d is not contiguous" % i)
            if t.numel() and t.dtype == torch.float32 and (t.data_ptr() % 4 or s.data_ptr() % 4):
                raise RuntimeError("EmaPlan: pair %d is not 4-byte aligned" % i)
        self._addresses = None
        self._table = None
        self._blocks = 0
        self._rows = 0
        self.uploads = 0                # times the table was (re)built
        self._build()

    def _current(self):
        return [t.data_ptr() for t in self.dst] + [s.data_ptr() for s in self.src]

    def _build(self):
        segments = []
        for t, s in zip(self.dst, self.src):
            n = t.numel()
            lo_t, lo_s, nbytes = t.data_ptr(), s.data_ptr(), n * t.element_size()
            if n and lo_t < lo_s + nbytes and lo_s < lo_t + nbytes:
                raise RuntimeError("EmaPlan: a destination overlaps its source")
            if t.dtype == torch.float32:
                segments.append((lo_t, lo_s, n, 0))
            else:
                segments.append((lo_t, lo_s, nbytes, 1))
        table, self._blocks = ema_segment_table(segments)
        self._rows = len(table)
        self._addresses = self._current()
        self._table = None
        if self._rows:
            host = torch.from_numpy(table.view('u1').reshape(-1).copy())
            self._table = host.to(self.dst[0].device)          # (pageable and blocking: once per layout)
        self.uploads += 1

    def update(self, decay):
        import numpy as np
        d = np.float32(decay)
        if not 0.0 <= float(d) < 1.0:
            raise ValueError("EmaPlan.update: decay=%r outside [0, 1)" % (decay,))
        if self._current() != self._addresses:
            self._build()
        if not self._rows:
            return
        omd = np.float32(1) - d
        check(lib().cnuda_ema_update(ptr(self._table), self._rows, self._blocks, float(d), float(omd), stream()),
              'ema_update')


_CHECKED_PERMS = {}           # id(tensor) -> (weak reference, the tensor's version when it was validated)


def _flip_perm(flip_perm, J, dev):
    """`flip_perm` (None, an int32 [J] device tensor or a sequence) -> None or a validated int32 [J] tensor on `dev`.  A
    device tensor is read back the first time it is seen and again only after it was written."""
    import weakref
    import numpy as np
    if flip_perm is None:
        return None
    if isinstance(flip_perm, torch.Tensor):
        if flip_perm.dtype != torch.int32 or tuple(flip_perm.shape) != (J,) or flip_perm.device != dev:
            raise RuntimeError("pseudo_labels: flip_perm must be an int32 [%d] tensor on dets' device, got %s %s"
                               % (J, flip_perm.dtype, tuple(flip_perm.shape)))
        seen = _CHECKED_PERMS.get(id(flip_perm))
        if seen is not None and seen[0]() is flip_perm and seen[1] == flip_perm._version:
            return flip_perm.contiguous()
        host = flip_perm.detach().cpu().numpy()
    else:
        host = np.asarray(flip_perm)
        if host.shape != (J,) or host.dtype.kind not in 'iu':
            raise RuntimeError("pseudo_labels: flip_perm must list %d joint indices, got %r" % (J, flip_perm))
    if sorted(int(v) for v in host) != list(range(J)):
        raise RuntimeError("pseudo_labels: flip_perm %r is not a permutation of 0..%d" % (host.tolist(), J - 1))
    if isinstance(flip_perm, torch.Tensor):
        key = id(flip_perm)
        _CHECKED_PERMS[key] = (weakref.ref(flip_perm, lambda _, key=key: _CHECKED_PERMS.pop(key, None)),
                               flip_perm._version)
        return flip_perm.contiguous()
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)


def pseudo_labels(dets, thresholds, map_width, *, rotated=False, mirror=False, min_size=0.0, kps=None, flip_perm=None,
                  map_height=None):
    """A decoded detection table -> the inputs of datasets.targets.encode_targets at output-map resolution
    (cnuda_pseudo_labels; include/centernet_uda_hip.h).  dets [B, K, 6] (or [B, K, 7] with rotated) float32 as
    decode_detection leaves it, thresholds [C] float32 on the device.  -> {'classes' [B, K] int32, 'counts' [B] int32,
    'kept' 0-dim float32 (the mean of counts), and 'boxes' [B, K, 4] float64 or, rotated, 'corners' [B, K, 4, 2]
    float64}: the surviving rows first, in input order, zeros behind them.  One launch, nothing read back.

    With kps [B, K, J, 2] float32 (decode_detection's second result) and `map_height` the call goes through
    cnuda_pseudo_labels_kps: the same rows survive -- the joints never decide it --, and the dict gains 'keypoints'
    [B, K, J, 2] float64, 'visibility' [B, K, J] int32 (2: inside [0, map_width) x [0, map_height); else 0) and 'joints'
    (0-dim float32: the mean number of visible joints per image).  flip_perm: an int32 [J] device tensor or a sequence,
    a permutation of 0..J-1 (predict.flip_permutation): output joint j takes input joint flip_perm[j].  It is validated
    on the host: a sequence on every call, a tensor when it is first seen and after it was written (one read-back)."""
    if kps is None:
        if flip_perm is not None or map_height is not None:
            raise RuntimeError("pseudo_labels: flip_perm and map_height belong to kps, which is not given")
    else:
        if map_height is None or int(map_height) < 1:
            raise RuntimeError("pseudo_labels: kps needs map_height >= 1, got %r" % (map_height,))
    require_gpu(dets, thresholds, kps)
    ncol = 7 if rotated else 6
    if dets.dim() != 3 or dets.shape[2] != ncol or dets.numel() == 0:
        raise RuntimeError("pseudo_labels: dets must be a non-empty [B, K, %d], got %s" % (ncol, tuple(dets.shape)))
    if thresholds.dtype != torch.float32 or thresholds.dim() != 1 or thresholds.numel() == 0 \
            or thresholds.device != dets.device:
        raise RuntimeError("pseudo_labels: thresholds must be a float32 [C] tensor on dets' device")
    if int(map_width) < 1:
        raise RuntimeError("pseudo_labels: map_width=%r" % (map_width,))
    dets, thresholds = f32c(dets.detach()), thresholds.contiguous()
    B, K, _ = dets.shape
    dev = dets.device
    geometry = torch.empty((B, K, 4, 2) if rotated else (B, K, 4), dtype=torch.float64, device=dev)
    out = {'classes': torch.empty((B, K), dtype=torch.int32, device=dev),
           'counts': torch.empty((B,), dtype=torch.int32, device=dev),
           'kept': torch.empty((), dtype=torch.float32, device=dev),
           'corners' if rotated else 'boxes': geometry}
    if kps is not None:
        if kps.dim() != 4 or tuple(kps.shape[:2]) != (B, K) or kps.shape[2] < 1 or kps.shape[3] != 2 \
                or kps.dtype != torch.float32 or kps.device != dev:
            raise RuntimeError("pseudo_labels: kps must be a float32 [%d, %d, J, 2] on dets' device, got %s %s"
                               % (B, K, kps.dtype, tuple(kps.shape)))
        J = kps.shape[2]
        kps, perm = kps.detach().contiguous(), _flip_perm(flip_perm, J, dev)
        out['keypoints'] = torch.empty((B, K, J, 2), dtype=torch.float64, device=dev)
        out['visibility'] = torch.empty((B, K, J), dtype=torch.int32, device=dev)
        out['joints'] = torch.empty((), dtype=torch.float32, device=dev)
        check(lib().cnuda_pseudo_labels_kps(ptr(dets), ptr(kps), ptr(thresholds), ptr(perm), ptr(geometry),
                                            ptr(out['classes']), ptr(out['counts']), ptr(out['kept']),
                                            ptr(out['keypoints']), ptr(out['visibility']), ptr(out['joints']), B, K,
                                            thresholds.numel(), J, 1 if rotated else 0, 1 if mirror else 0,
                                            int(map_height), int(map_width), float(min_size), stream()),
              'pseudo_labels_kps')
        return out
    check(lib().cnuda_pseudo_labels(ptr(dets), ptr(thresholds), ptr(geometry), ptr(out['classes']), ptr(out['counts']),
                                    ptr(out['kept']), B, K, thresholds.numel(), 1 if rotated else 0,
                                    1 if mirror else 0, int(map_width), float(min_size), stream()), 'pseudo_labels')
    return out


def transform_labels(labels, forward_map, map_h, map_w, *, rotated=False, min_size=0.0, min_visible=0.5):
    """The pseudo-labels of `pseudo_labels` under a geometric view (cnuda_labels_transform; include/centernet_uda_hip.h,
    "Geometric view").  labels: the dict `pseudo_labels` returns; forward_map [B, 6] (or [B, 2, 3]) float64, host or
    device: the view's matrix at output-map resolution (datasets.geometric_view.GeometricViewParams.forward_map).
    Rotated: the corners are mapped point by point; axis-aligned: the bounding box of the four mapped corners.  A row
    survives iff both extents >= min_size, its area is positive and finite and at least `min_visible` of it lies inside
    [0, map_w] x [0, map_h] (an exact convex clip in float64); an image with the identity matrix keeps every row.
    -> a new dict with the same keys, dtypes and layout -- survivors first, in input order, unclipped, zeros behind them;
    'counts' and 'kept' rewritten -- plus 'dropped' (0-dim float32: the mean number of rows removed per image).  The
    input tensors are not written.  Two launches, no atomics, nothing read back.

    A dict that holds 'keypoints' [B, K, J, 2] float64 and 'visibility' [B, K, J] int32 (pseudo_labels(kps=...)) goes
    through cnuda_labels_transform_kps: the same rows survive, their joints are mapped by the same matrix and stay
    visible (2) only where they were and the mapped point lies inside [0, map_w) x [0, map_h); 'joints' is recomputed."""
    import numpy as np
    key = 'corners' if rotated else 'boxes'
    tail = (4, 2) if rotated else (4,)
    if not isinstance(labels, dict) or any(k not in labels for k in (key, 'classes', 'counts')):
        raise RuntimeError("transform_labels: labels must be the dict of pseudo_labels(rotated=%s) with '%s', 'classes' "
                           "and 'counts'" % (bool(rotated), key))
    if ('keypoints' in labels) != ('visibility' in labels):
        raise RuntimeError("transform_labels: labels hold only one of 'keypoints' and 'visibility'")
    geometry, classes, counts = labels[key], labels['classes'], labels['counts']
    require_gpu(geometry, classes, counts)
    if geometry.dim() != 2 + len(tail) or tuple(geometry.shape[2:]) != tail or geometry.numel() == 0 \
            or geometry.dtype != torch.float64:
        raise RuntimeError("transform_labels: %s must be a non-empty float64 [B, K, %s], got %s %s"
                           % (key, ', '.join(map(str, tail)), geometry.dtype, tuple(geometry.shape)))
    B, K = geometry.shape[:2]
    if tuple(classes.shape) != (B, K) or tuple(counts.shape) != (B,) or classes.dtype != torch.int32 \
            or counts.dtype != torch.int32:
        raise RuntimeError("transform_labels: classes must be int32 [%d, %d] and counts int32 [%d], got %s %s and %s %s"
                           % (B, K, B, classes.dtype, tuple(classes.shape), counts.dtype, tuple(counts.shape)))
    if int(map_h) < 1 or int(map_w) < 1:
        raise RuntimeError("transform_labels: map_h=%r, map_w=%r" % (map_h, map_w))
    if not 0.0 <= float(min_visible) <= 1.0 or not float(min_size) == float(min_size):
        raise RuntimeError("transform_labels: min_visible=%r outside [0, 1] or min_size=%r is NaN" % (min_visible, min_size))
    dev = geometry.device
    if isinstance(forward_map, torch.Tensor):
        forward = forward_map.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    else:
        host = np.ascontiguousarray(np.asarray(forward_map, dtype=np.float64).reshape(-1))
        if not np.isfinite(host).all():
            raise RuntimeError("transform_labels: forward_map must be finite")
        forward = torch.from_numpy(host).to(dev)
    if forward.numel() != 6 * B:
        raise RuntimeError("transform_labels: forward_map must be [%d, 6], got %d values" % (B, forward.numel()))
    geometry, classes, counts = geometry.contiguous(), classes.contiguous(), counts.contiguous()
    out = {'classes': torch.empty_like(classes), 'counts': torch.empty_like(counts),
           'kept': torch.empty((), dtype=torch.float32, device=dev), key: torch.empty_like(geometry),
           'dropped': torch.empty((), dtype=torch.float32, device=dev)}
    if 'keypoints' in labels:
        keypoints, visibility = labels['keypoints'], labels['visibility']
        require_gpu(keypoints, visibility)
        if keypoints.dim() != 4 or tuple(keypoints.shape[:2]) != (B, K) or keypoints.shape[2] < 1 \
                or keypoints.shape[3] != 2 or keypoints.dtype != torch.float64 or keypoints.device != dev:
            raise RuntimeError("transform_labels: keypoints must be a float64 [%d, %d, J, 2], got %s %s"
                               % (B, K, keypoints.dtype, tuple(keypoints.shape)))
        J = keypoints.shape[2]
        if tuple(visibility.shape) != (B, K, J) or visibility.dtype != torch.int32 or visibility.device != dev:
            raise RuntimeError("transform_labels: visibility must be an int32 [%d, %d, %d], got %s %s"
                               % (B, K, J, visibility.dtype, tuple(visibility.shape)))
        keypoints, visibility = keypoints.contiguous(), visibility.contiguous()
        out['keypoints'], out['visibility'] = torch.empty_like(keypoints), torch.empty_like(visibility)
        out['joints'] = torch.empty((), dtype=torch.float32, device=dev)
        check(lib().cnuda_labels_transform_kps(ptr(geometry), ptr(classes), ptr(counts), ptr(keypoints), ptr(visibility),
                                               ptr(forward), ptr(out[key]), ptr(out['classes']), ptr(out['counts']),
                                               ptr(out['keypoints']), ptr(out['visibility']), ptr(out['kept']),
                                               ptr(out['dropped']), ptr(out['joints']), B, K, J, 1 if rotated else 0,
                                               int(map_h), int(map_w), float(min_size), float(min_visible), stream()),
              'labels_transform_kps')
        return out
    check(lib().cnuda_labels_transform(ptr(geometry), ptr(classes), ptr(counts), ptr(forward), ptr(out[key]),
                                       ptr(out['classes']), ptr(out['counts']), ptr(out['kept']), ptr(out['dropped']),
                                       B, K, 1 if rotated else 0, int(map_h), int(map_w), float(min_size),
                                       float(min_visible), stream()), 'labels_transform')
    return out


# ---------------------------------------------------------------------------
# Dense teacher (csrc/dense.hip; DESIGN.md, "Dense teacher")
# ---------------------------------------------------------------------------
def _check_ratio(who, ratio):
    ratio = float(ratio)
    if not 0.0 < ratio <= 1.0:
        raise ValueError("%s: ratio must be in (0, 1], got %r" % (who, ratio))
    return ratio


def dense_select(teacher_hm, ratio):
    """teacher_hm [B, C, H, W] logits -> (tau [B] float32, count [B] int32): per image the k-th largest channel-max
    score, k = max(1, floor(ratio H W)), and how many positions reach it (every tie counts, so count >= k; -0 equals
    +0; a NaN score is never selected).  The mask is `score >= tau[b]`.  Two launches, no gradient, no read-back."""
    ratio = _check_ratio('dense_select', ratio)
    require_gpu(teacher_hm)
    if teacher_hm.dim() != 4 or teacher_hm.numel() == 0:
        raise RuntimeError("dense_select: teacher_hm must be a non-empty [B, C, H, W], got %s" % (tuple(teacher_hm.shape),))
    hm = f32c(teacher_hm.detach())
    B, C, H, W = hm.shape
    tau = torch.empty(B, dtype=torch.float32, device=hm.device)
    count = torch.empty(B, dtype=torch.int32, device=hm.device)
    ws = _ws(lib().cnuda_dense_select_workspace_bytes(B, H * W), hm)
    check(lib().cnuda_dense_select(ptr(hm), ratio, ptr(tau), ptr(count), B, C, H * W, *ws, stream()), 'dense_select')
    return tau, count


class _DenseTeacher(Function):
    """_IWMaxSquare's sibling with two differentiable inputs: the teacher's maps, tau and the forward's five results are
    constants of the backward pass."""

    @staticmethod
    def forward(ctx, hm, wh, teacher_hm, teacher_wh, tau, count, mirror, hm_weight, wh_weight):
        require_gpu(hm, wh, teacher_hm, teacher_wh, tau, count)
        hm, wh, teacher_hm, teacher_wh = f32c(hm), f32c(wh), f32c(teacher_hm), f32c(teacher_wh)
        B, C, H, W = hm.shape
        out5 = torch.empty(5, dtype=torch.float32, device=hm.device)
        check(lib().cnuda_dense_teacher_forward(ptr(hm), ptr(wh), ptr(teacher_hm), ptr(teacher_wh), ptr(tau), ptr(count),
                                                ptr(out5), B, C, H, W, mirror, hm_weight, wh_weight, *_loss_ws(hm),
                                                stream()), 'dense_teacher_forward')
        ctx.call = (B, C, H, W, mirror, hm_weight, wh_weight)
        ctx.save_for_backward(hm, wh, teacher_hm, teacher_wh, tau, out5)
        stats = out5.clone()
        ctx.mark_non_differentiable(stats)
        return out5[0].clone(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gstats):
        hm, wh, teacher_hm, teacher_wh, tau, out5 = ctx.saved_tensors
        grad_hm, grad_wh = torch.empty_like(hm), torch.empty_like(wh)
        up = f32c(g.reshape(1))
        check(lib().cnuda_dense_teacher_backward(ptr(hm), ptr(wh), ptr(teacher_hm), ptr(teacher_wh), ptr(tau), ptr(out5),
                                                 ptr(up), ptr(grad_hm), ptr(grad_wh), *ctx.call, stream()),
              'dense_teacher_backward')
        return (grad_hm, grad_wh) + (None,) * 7


def dense_teacher_loss(hm, wh, teacher_hm, teacher_wh, tau, count, *, mirror, hm_weight=1.0, wh_weight=0.1):
    """Dense Teacher's loss of the student's maps hm [B, C, H, W] (logits) and wh [B, 2, H, W] against the teacher's,
    inside the selection (tau, count) = dense_select(teacher_hm, ratio); `mirror`: the student saw the mirrored image.
    -> (hm_weight hm_loss + wh_weight wh_loss, stats [5] = that loss, hm_loss, wh_loss, N, sum u): a quality focal
    loss (exponent 2) of sigmoid(hm) against sigmoid(teacher_hm) on the selection and 0 elsewhere, over N = sum count;
    the L1 of the sizes weighted by u = sigmoid(score) (include/centernet_uda_hip.h).  The teacher's tensors carry no
    gradient."""
    for name, t in (('teacher_hm', teacher_hm), ('teacher_wh', teacher_wh), ('tau', tau)):
        if t.requires_grad:
            raise RuntimeError("dense_teacher_loss: %s requires grad; the teacher is a constant (detach it)" % name)
    if hm.dim() != 4 or hm.numel() == 0:
        raise RuntimeError("dense_teacher_loss: hm must be a non-empty [B, C, H, W], got %s" % (tuple(hm.shape),))
    B, C, H, W = hm.shape
    for name, t, shape in (('teacher_hm', teacher_hm, (B, C, H, W)), ('wh', wh, (B, 2, H, W)),
                           ('teacher_wh', teacher_wh, (B, 2, H, W)), ('tau', tau, (B,)), ('count', count, (B,))):
        if tuple(t.shape) != shape:
            raise RuntimeError("dense_teacher_loss: %s is %s, expected %s" % (name, tuple(t.shape), shape))
    if tau.dtype != torch.float32 or count.dtype != torch.int32 or not tau.is_contiguous() or not count.is_contiguous():
        raise RuntimeError("dense_teacher_loss: tau must be contiguous float32 and count contiguous int32")
    return _DenseTeacher.apply(hm, wh, teacher_hm, teacher_wh, tau, count, 1 if mirror else 0, float(hm_weight),
                               float(wh_weight))


def rotated_iou(a, b, return_areas=False):
    """The exact IoU of every pair of two sets of convex quadrilaterals per image, in float64 (csrc/polyiou.cuh;
    include/centernet_uda_hip.h, "Rotated IoU").  a [B, N, 4, 2], b [B, M, 4, 2] float32 (x, y) vertices in either
    winding, as predict.project_detections and utils.box.rotate_bboxes_float give them -> iou [B, N, M] float64; with
    `return_areas` also (area_a [B, N], area_b [B, M]) float64.  Subject a, clipper b; a quad with a coordinate that is
    not finite or without area overlaps nothing; a quad that is not convex gives a finite value in [0, 1] that is
    otherwise unspecified.  One launch, no gradient, no read-back."""
    require_gpu(a, b)
    a, b = f32c(a.detach()), f32c(b.detach())
    if a.dim() != 4 or b.dim() != 4 or tuple(a.shape[2:]) != (4, 2) or tuple(b.shape[2:]) != (4, 2) \
            or a.shape[0] != b.shape[0] or a.shape[0] < 1:
        raise RuntimeError("rotated_iou: a must be [B, N, 4, 2] and b [B, M, 4, 2] with B >= 1, got %s and %s"
                           % (tuple(a.shape), tuple(b.shape)))
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    iou = torch.empty((B, N, M), dtype=torch.float64, device=a.device)
    area_a = torch.empty((B, N), dtype=torch.float64, device=a.device) if return_areas else None
    area_b = torch.empty((B, M), dtype=torch.float64, device=a.device) if return_areas else None
    check(lib().cnuda_quad_iou_pairs(ptr(a) if N else None, ptr(b) if M else None, ptr(iou) if N * M else None,
                                     ptr(area_a) if N else None, ptr(area_b) if M else None, B, N, M, stream()),
          'quad_iou_pairs')
    return (iou, area_a, area_b) if return_areas else iou
