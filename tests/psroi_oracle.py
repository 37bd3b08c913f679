"""float64 oracle of the deformable PSROI pooling (test helper, not collected).

Nothing of the reference can be run for this operator: its CPU source does not compile against this torch
(`AT_DISPATCH_FLOATING_TYPES(input.type(), ...)`), and oracle/ is frozen.  So no golden file comes
from it.  This file restates the operator (libs/DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu:59-146) in differentiable
torch ops in float64:

  * sample coordinates are functions of `offset`; the bilinear corners come from floor / ceil and are detached, so
    autograd differentiates the weights only -- at an integer coordinate both corners coincide and the offset
    gradient is zero, as in the reference;
  * the index tables floor(float(p) / P * part) and floor(float(p) * group / P) are computed with numpy.float32 in
    that operation order (what users of the reference ran);
  * spatial_scale and trans_std are rounded to float32 first (they are C floats in the reference's signature);
  * grad_input and grad_offset come from torch.autograd.grad: no hand-written backward formula is involved.

tests/test_host_psroi.py pins this oracle by answers that do not come from it.
"""
import numpy as np
import torch


def tables(pooled_size, part_size, group_size):
    """-> (part_of[P], g_of[P]) int64, float32 arithmetic in the reference's operation order."""
    p = np.arange(pooled_size).astype(np.float32)
    part = np.floor(p / np.float32(pooled_size) * np.float32(part_size)).astype(np.int64)
    g = np.floor(p * np.float32(group_size) / np.float32(pooled_size)).astype(np.int64)
    return torch.from_numpy(part), torch.from_numpy(np.clip(g, 0, group_size - 1))


def _round_half_away(v):
    return torch.sign(v) * torch.floor(v.abs() + 0.5)


def roi_boxes(rois, spatial_scale):
    """-> batch index [N] (long), start_w, start_h, width, height [N] (float64)"""
    r = rois.detach().double()
    scale = float(np.float32(spatial_scale))
    sw = _round_half_away(r[:, 1]) * scale - 0.5
    sh = _round_half_away(r[:, 2]) * scale - 0.5
    ew = (_round_half_away(r[:, 3]) + 1.0) * scale - 0.5
    eh = (_round_half_away(r[:, 4]) + 1.0) * scale - 0.5
    return r[:, 0].long(), sw, sh, (ew - sw).clamp(min=0.1), (eh - sh).clamp(min=0.1)


def sample_coords(rois, offset, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std):
    """-> w, h [N, num_classes, P, P, S] float64 (before the validity test and the clamp); differentiable in offset."""
    N, P, S = rois.shape[0], pooled_size, sample_per_part
    _, sw, sh, rw, rh = roi_boxes(rois, spatial_scale)
    part_of, _ = tables(P, part_size, 1)
    if no_trans:
        nc = 1
        tx = ty = torch.zeros(N, 1, P, P, dtype=torch.float64)
    else:
        nc = offset.shape[1] // 2
        t = offset.double().view(N, nc, 2, part_size, part_size) * float(np.float32(trans_std))
        t = t[:, :, :, part_of][:, :, :, :, part_of]                    # [N, nc, 2, P(ph), P(pw)]
        tx, ty = t[:, :, 0], t[:, :, 1]
    pw = torch.arange(P, dtype=torch.float64).view(1, 1, 1, P)
    ph = torch.arange(P, dtype=torch.float64).view(1, 1, P, 1)
    v = lambda a: a.view(N, 1, 1, 1)
    wstart = pw * v(rw / P) + v(sw) + tx * v(rw)
    hstart = ph * v(rh / P) + v(sh) + ty * v(rh)
    i = torch.arange(S, dtype=torch.float64)
    w = wstart.unsqueeze(-1) + i * (rw / P / S).view(N, 1, 1, 1, 1)
    h = hstart.unsqueeze(-1) + i * (rh / P / S).view(N, 1, 1, 1, 1)
    return w.expand(N, nc, P, P, S), h.expand(N, nc, P, P, S)


def forward(input, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
            sample_per_part, trans_std):
    """-> (output, output_count) float64, [N, output_dim, P, P]; differentiable in input and offset."""
    x = input.double()
    B, C, H, W = x.shape
    N, P, S, G, OD = rois.shape[0], pooled_size, sample_per_part, group_size, output_dim
    assert C == OD * G * G
    w, h = sample_coords(rois, offset, no_trans, spatial_scale, P, part_size, S, trans_std)
    nc = w.shape[1]
    assert OD % nc == 0
    bi = roi_boxes(rois, spatial_scale)[0]
    assert bool(((bi >= 0) & (bi < B)).all())
    vw = ((w >= -0.5) & (w <= W - 0.5))
    vh = ((h >= -0.5) & (h <= H - 0.5))
    cw, ch = w.clamp(0.0, W - 1.0), h.clamp(0.0, H - 1.0)
    x0, x1 = cw.detach().floor().long(), cw.detach().ceil().long()
    y0, y1 = ch.detach().floor().long(), ch.detach().ceil().long()
    dx, dy = cw - x0, ch - y0
    # per output channel: class of the geometry, input channel of every bin
    ctop = torch.arange(OD)
    cls = ctop // (OD // nc)
    _, g_of = tables(P, part_size, G)
    chan = (ctop.view(OD, 1, 1) * G + g_of.view(1, P, 1)) * G + g_of.view(1, 1, P)          # [OD, P, P]
    # everything to [N, OD, P, P, S(ih), S(iw)]
    e = lambda a, axis: (a[:, cls].unsqueeze(-1) if axis == 'h' else a[:, cls].unsqueeze(-2))
    X0, X1, DX, VW = e(x0, 'w'), e(x1, 'w'), e(dx, 'w'), e(vw, 'w')
    Y0, Y1, DY, VH = e(y0, 'h'), e(y1, 'h'), e(dy, 'h'), e(vh, 'h')
    full = (N, OD, P, P, S, S)
    bb = bi.view(N, 1, 1, 1, 1, 1).expand(full)
    cc = chan.view(1, OD, P, P, 1, 1).expand(full)
    X0, X1, Y0, Y1 = [a.expand(full) for a in (X0, X1, Y0, Y1)]
    v00, v01 = x[bb, cc, Y0, X0], x[bb, cc, Y1, X0]          # v<x><y>
    v10, v11 = x[bb, cc, Y0, X1], x[bb, cc, Y1, X1]
    val = (1 - DX) * (1 - DY) * v00 + (1 - DX) * DY * v01 + DX * (1 - DY) * v10 + DX * DY * v11
    valid = (VW & VH).expand(full)
    total = (val * valid).sum(dim=(-1, -2))
    count = valid.sum(dim=(-1, -2)).double()
    out = torch.where(count > 0, total / count.clamp(min=1.0), torch.zeros_like(total))
    return out, count


def forward_backward(input, rois, offset, grad_output, *args):
    """-> output, output_count, grad_input, grad_offset (float64; grad_offset None with no_trans)"""
    no_trans = bool(args[0])
    x = input.detach().double().requires_grad_(True)
    t = None if no_trans else offset.detach().double().requires_grad_(True)
    out, count = forward(x, rois, t, *args)
    wrt = (x,) if no_trans else (x, t)
    grads = torch.autograd.grad(out, wrt, grad_output.double(), allow_unused=True)
    gi = grads[0] if grads[0] is not None else torch.zeros_like(x)
    go = None
    if not no_trans:
        go = grads[1] if grads[1] is not None else torch.zeros_like(t)
    return out.detach(), count, gi, go


def _coord_margin(v, size):
    d = (v - v.round()).abs()                                        # to the nearest integer
    d = torch.minimum(d, (v + 0.5).abs())                            # to -0.5
    return torch.minimum(d, (v - (size - 0.5)).abs())                # to size - 0.5


def corner_margin(rois):
    """smallest distance of a ROI corner to k + 0.5 (where round() flips)"""
    c = rois.detach().double()[:, 1:]
    return float(((c - 0.5) - (c - 0.5).round()).abs().min()) if c.numel() else float('inf')


def margin(input_shape, rois, offset, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
           sample_per_part, trans_std):
    """The smallest distance of any sample coordinate, valid or not, to an integer, to -0.5 or to W - 0.5 / H - 0.5, and
    of any ROI corner to k + 0.5: below it an fp32 and an fp64 evaluation cannot disagree about a floor, a ceil, a
    validity test or a rounding."""
    H, W = input_shape[2], input_shape[3]
    w, h = sample_coords(rois, offset, no_trans, spatial_scale, pooled_size, part_size, sample_per_part, trans_std)
    if w.numel() == 0:
        return float('inf')
    return min(float(_coord_margin(w.detach(), W).min()), float(_coord_margin(h.detach(), H).min()), corner_margin(rois))


def settle_offsets(input_shape, rois, offset, spatial_scale, pooled_size, part_size, sample_per_part, trans_std,
                   generator, floor=2e-3, sigma=1.0):
    """Input construction for the tests: redraws (from `generator`) exactly those offset elements whose sample
    coordinates come within `floor` of an integer or of a map border, until none does.  With tens of thousands of
    random coordinates a margin of 1e-3 never holds by luck; the kernels under test play no part in this choice."""
    H, W = input_shape[2], input_shape[3]
    N, nc2, part = offset.shape[0], offset.shape[1], part_size
    part_of, _ = tables(pooled_size, part_size, 1)
    offset = offset.clone()
    for _ in range(200):
        w, h = sample_coords(rois, offset, False, spatial_scale, pooled_size, part_size, sample_per_part, trans_std)
        bad = torch.zeros(N, nc2 // 2, 2, part, part, dtype=torch.bool)
        for xy, (v, size) in enumerate(((w, W), (h, H))):
            close = (_coord_margin(v, size) < floor).any(dim=-1)                # [N, nc, P, P]
            n, c, ph, pw = close.nonzero(as_tuple=True)
            bad[n, c, xy, part_of[ph], part_of[pw]] = True
        bad = bad.view_as(offset)
        k = int(bad.sum())
        if k == 0:
            return offset
        offset[bad] = torch.randn(k, generator=generator, dtype=offset.dtype) * sigma
    raise AssertionError('settle_offsets: no admissible offsets found')


def settle_rois(input_shape, rois, draw, spatial_scale, pooled_size, sample_per_part, floor=2e-3):
    """The same for the ROIs of a no_trans case: `draw(k)` -> k fresh ROI rows [k, 5]; rows whose (offset-free) sample
    coordinates come within `floor` of an integer or a border are redrawn."""
    H, W = input_shape[2], input_shape[3]
    rois = rois.clone()
    for _ in range(200):
        w, h = sample_coords(rois, None, True, spatial_scale, pooled_size, pooled_size, sample_per_part, 0.0)
        close = (_coord_margin(w, W) < floor).flatten(1).any(dim=1) | (_coord_margin(h, H) < floor).flatten(1).any(dim=1)
        k = int(close.sum())
        if k == 0:
            return rois
        fresh = draw(k)
        fresh[:, 0] = rois[close, 0]
        rois[close] = fresh
    raise AssertionError('settle_rois: no admissible ROIs found')
