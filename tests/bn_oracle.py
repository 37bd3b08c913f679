"""BatchNorm2d + residual add + ReLU / ReLU6 (csrc/bn.hip) restated in plain torch.double: sums, means and the chain
rule written out by hand -- no autograd, no F.batch_norm -- so that it is a second derivation of what the kernels
compute.  tests/test_host_bn_forms.py holds it against torch's own double-precision batch_norm + autograd.

Conventions (include/centernet_uda_hip.h): x, residual, y are [B, C, H, W]; `groups` statistics groups are the images
[g * B / groups, (g + 1) * B / groups), each normalised by its own batch statistics, which are saved as [groups][C];
act: 0 none, 1 ReLU, 2 ReLU6, whose gradient passes strictly inside (0, 6)."""
import torch

D = torch.float64


def _grouped(t, groups):
    """[B, C, H, W] -> [groups, Bg, C, HW] (a view)"""
    B, C = t.shape[0], t.shape[1]
    return t.reshape(groups, B // groups, C, -1)


def activation(z, act):
    if act == 0:
        return z
    y = torch.where(z > 0, z, torch.zeros_like(z))
    return torch.where(y < 6, y, torch.full_like(y, 6.0)) if act == 2 else y


def gate(z, act):
    """where the activation lets a gradient through"""
    if act == 0:
        return torch.ones_like(z, dtype=torch.bool)
    return (z > 0) & (z < 6) if act == 2 else z > 0


def train_forward(x, gamma, beta, residual=None, act=0, groups=1, eps=1e-5, momentum=0.1, running_mean=None,
                  running_var=None):
    """-> z (pre-activation), y, save_mean [groups, C], save_invstd [groups, C] (biased variance), running_mean,
    running_var (None without the inputs) after one momentum update per group, in group order: the update uses the
    unbiased variance and the buffers are float32, so they are rounded to float32 between updates (bn_apply_kernel)."""
    xg = _grouped(x.to(D), groups)                                # [G, Bg, C, HW]
    n = xg.shape[1] * xg.shape[3]
    mean = xg.sum(dim=(1, 3)) / n                                 # [G, C]
    var = ((xg - mean[:, None, :, None]) ** 2).sum(dim=(1, 3)) / n
    return forward_from_moments(x, mean, var, gamma, beta, residual, act, eps, momentum, running_mean, running_var)


def forward_from_moments(x, mean, var, gamma, beta, residual=None, act=0, eps=1e-5, momentum=0.1, running_mean=None,
                         running_var=None):
    """train_forward's second half for given per-group mean and biased variance, [groups, C] each (the statistics that
    arrive from a GEMM epilogue: fold) -> the same six results"""
    x, gamma, beta = x.to(D), gamma.to(D), beta.to(D)
    groups = mean.shape[0]
    xg = _grouped(x, groups)
    n = xg.shape[1] * xg.shape[3]
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xg - mean[:, None, :, None]) * invstd[:, None, :, None]
    z = (xhat * gamma[None, None, :, None] + beta[None, None, :, None]).reshape(x.shape)
    if residual is not None:
        z = z + residual.to(D)
    rm = rv = None
    if running_mean is not None:
        rm, rv = running_mean.to(D).clone(), running_var.to(D).clone()
        for g in range(groups):
            unbiased = var[g] * n / (n - 1) if n > 1 else var[g]
            rm = ((1.0 - momentum) * rm + momentum * mean[g]).float().to(D)
            rv = ((1.0 - momentum) * rv + momentum * unbiased).float().to(D)
    return z, activation(z, act), mean, invstd, rm, rv


def backward(gy, x, gamma, save_mean, save_invstd, gate_mask):
    """-> gx, gres, ggamma, gbeta for the boolean `gate_mask` (shaped like x) of the activation.  With g = gy * gate:
    gres = g;  gbeta = sum g and ggamma = sum g * xhat over ALL groups, each group's xhat from its own statistics;
    gx = gamma * invstd * (g - mean_n(g) - xhat * mean_n(g * xhat)), the two means over the element's own group."""
    groups = save_mean.shape[0]
    gy, x, gamma = gy.to(D), x.to(D), gamma.to(D)
    mean, invstd = save_mean.to(D), save_invstd.to(D)
    g = torch.where(gate_mask, gy, torch.zeros_like(gy))
    gg, xg = _grouped(g, groups), _grouped(x, groups)
    n = xg.shape[1] * xg.shape[3]
    xhat = (xg - mean[:, None, :, None]) * invstd[:, None, :, None]
    s0 = gg.sum(dim=(1, 3))                                       # [G, C]
    s1 = (gg * xhat).sum(dim=(1, 3))
    k = (gamma[None] * invstd)[:, None, :, None]
    gx = k * (gg - (s0 / n)[:, None, :, None] - xhat * (s1 / n)[:, None, :, None])
    return gx.reshape(x.shape), g, s1.sum(dim=0), s0.sum(dim=0)


def eval_forward(x, gamma, beta, running_mean, running_var, residual=None, act=0, eps=1e-5):
    x = x.to(D)
    sc = gamma.to(D) / torch.sqrt(running_var.to(D) + eps)
    z = (x - running_mean.to(D)[None, :, None, None]) * sc[None, :, None, None] + beta.to(D)[None, :, None, None]
    if residual is not None:
        z = z + residual.to(D)
    return activation(z, act)


def fold(stats_f32, blocks_per_group, groups, count):
    """stats_f32: [blocks][rows][2] float32 block sums (sum, sum of squares), the blocks of group g being
    [g, g + 1) * blocks_per_group; `count` values per channel and group.  -> the per-group sums [groups, rows, 2] of
    exactly these float32 numbers, added in fp64 (the order of fp64 additions is worth 1e-16 per term), and what
    bn_apply_kernel makes of them: mean [groups, rows] and biased variance [groups, rows], clamped at 0."""
    assert stats_f32.dtype == torch.float32 and stats_f32.shape[0] == groups * blocks_per_group
    s = stats_f32.to(D).reshape(groups, blocks_per_group, stats_f32.shape[1], 2).sum(dim=1)
    mean = s[..., 0] / count
    var = s[..., 1] / count - mean * mean
    return s, mean, torch.where(var > 0, var, torch.zeros_like(var))


def gate_with_band(z_ref, y_kernel, act, rel=1e-4):
    """The gate for a comparison with a float32 kernel.  The kernel may legitimately put an element on the other side
    of an activation edge when the reference's z lies within the forward tolerance of that edge, and one such flip
    moves gbeta by a whole gy.  Band = rel * max|z_ref| around 0 (and around 6 for ReLU6): outside it the gate is the
    reference's, inside it the kernel's own, read from its forward output.  -> (mask, share of elements in the band)"""
    if act == 0:
        return torch.ones_like(z_ref, dtype=torch.bool), 0.0
    band = rel * z_ref.abs().max().item()
    near = z_ref.abs() <= band
    own = y_kernel.to(D) > 0
    if act == 2:
        near = near | ((z_ref - 6.0).abs() <= band)
        own = own & (y_kernel.to(D) < 6)
    return torch.where(near, own, gate(z_ref, act)), near.double().mean().item()


# ---------------------------------------------------------------------------------------------------------------
# The run-time forms of the train / backward kernels (pick_split and plane_splits in csrc/bn.hip) and a shape that
# selects each: (B, C, H, W, groups) -> (per_plane, images per workgroup, partials per channel, apply splits), as
# cnuda_bn_plan must report them.  tests/test_host_bn_forms.py checks the table against the library without a GPU;
# tests/test_gpu_bn_forms.py runs every row.
# ---------------------------------------------------------------------------------------------------------------
FORMS = [
    ((2, 3, 7, 9, 1), (1, 1, 2, 1)),          # the plain form, scalar (HW % 4 == 3)
    ((2, 5, 32, 40, 1), (1, 1, 2, 2)),        # apply grid cut, 16-byte
    ((1, 3, 33, 37, 1), (1, 1, 1, 2)),        # apply grid cut, scalar tail
    ((3, 2, 65, 63, 1), (1, 1, 3, 4)),        # HW = 4095, one below the cut
    ((1, 2, 64, 64, 1), (1, 1, 1, 4)),        # HW = 4096, the last uncut plane
    ((1, 2, 50, 82, 1), (2, 1, 2, 5)),        # cut plane, chunk 2052, last 2048
    ((1, 2, 17, 241, 1), (2, 1, 2, 5)),       # cut plane, scalar, last chunk 2045
    ((1, 3, 91, 91, 1), (3, 1, 3, 9)),        # three chunks, scalar
    ((1, 1, 4, 3073, 1), (4, 1, 4, 13)),      # chunk 3076, short last chunk 3064
    ((2, 1, 127, 129, 1), (4, 1, 8, 16)),     # two images of cut planes
    ((6, 2, 65, 64, 3), (2, 1, 12, 5)),       # three groups of cut planes
    ((4, 3, 91, 91, 2), (3, 1, 12, 9)),       # two groups, scalar, three chunks
    ((2, 1025, 3, 3, 1), (1, 2, 1, 1)),       # ips 2, scalar
    ((4, 1100, 3, 3, 1), (1, 4, 1, 1)),       # ips 4, scalar
    ((4, 600, 10, 10, 1), (1, 2, 2, 1)),      # ips 2, 16-byte, two workgroups per channel
    ((12, 700, 2, 2, 2), (1, 2, 6, 1)),       # ips 2 with 6 images per group, two groups
    ((8, 520, 1, 5, 2), (1, 2, 4, 1)),        # ips 2, HW = 5, two groups
    ((16, 512, 4, 4, 2), (1, 2, 8, 1)),       # the 512-channel level as a two-domain batch
]


def form_id(shape):
    return 'B%dC%dH%dW%dg%d' % tuple(shape)


def plan(B, C, HW, groups):
    """cnuda_bn_plan -> (per_plane, images per workgroup, partials, apply splits); needs no GPU"""
    import ctypes
    import hip_runtime as hr
    out = [ctypes.c_int(-1) for _ in range(4)]
    hr.check(hr.lib().cnuda_bn_plan(B, C, HW, groups, *[ctypes.byref(o) for o in out]), 'bn_plan')
    return tuple(o.value for o in out)
