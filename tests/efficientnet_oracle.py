"""CPU oracle for the EfficientNet backend (not a test): a pure-torch restatement of the MBConv operators and of the whole
CenterEfficientNet, built from F.conv2d(groups=C), F.pad, adaptive_avg_pool2d, sigmoid and F.batch_norm.  The network
is a FUNCTION of the product's state dict, so the names pin the wiring; it runs in whatever dtype the state has
(float64 for gradients).  Architecture from the published EfficientNet description (block table, width / depth
coefficients, rounding rules, static SAME padding) and the reference's backends/efficientnet.py head / up-sampling."""
import math

import torch
import torch.nn.functional as F

TABLE = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80), (3, 5, 1, 6, 80, 112),
         (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
COEFFS = {'b0': (1.0, 1.0, 224), 'b1': (1.0, 1.1, 240), 'b2': (1.1, 1.2, 260), 'b3': (1.2, 1.4, 300)}
SKIPS = {'b0': {5: 4, 2: 10}, 'b1': {5: 7, 2: 15}, 'b2': {5: 7, 2: 15}, 'b3': {5: 7, 2: 17}}


# ----------------------------------------------------------------------------- operators
def same_pads(size, k, s):
    total = max((math.ceil(size / s) - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def dwconv_same(x, w, stride, size=None):
    """size: the nominal (H, W) the padding is computed for; None: x's own."""
    k = w.shape[-1]
    h, wd = (x.shape[2], x.shape[3]) if size is None else size
    (pt, pb), (pl, pr) = same_pads(h, k, stride), same_pads(wd, k, stride)
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, None, stride, 0, 1, x.shape[1])


def swish(x):
    return x * torch.sigmoid(x)


def squeeze_excite(x, w1, b1, w2, b2):
    s = F.adaptive_avg_pool2d(x, 1)
    s = F.conv2d(swish(F.conv2d(s, w1, b1)), w2, b2)
    return torch.sigmoid(s) * x


def drop_connect_add(x, mask, residual):
    return x * mask.view(-1, 1, 1, 1) + residual


# ----------------------------------------------------------------------------- structure
def round_filters(f, width):
    f = f * width
    new = max(8, int(f + 4) // 8 * 8)
    return new + 8 if new < 0.9 * f else new


def blocks(variant):
    """-> [(cin, cout, k, stride, expand, cse, nominal map size at the block's input)], stem width, head width, nominal size"""
    width, depth, size = COEFFS[variant]
    cur = math.ceil(size / 2)
    out = []
    for r, k, s, e, ci, co in TABLE:
        ci, co = round_filters(ci, width), round_filters(co, width)
        for i in range(int(math.ceil(depth * r))):
            out.append((ci if i == 0 else co, co, k, s if i == 0 else 1, e, max(1, int((ci if i == 0 else co) * 0.25)), cur))
            if i == 0:
                cur = math.ceil(cur / s)
    return out, round_filters(32, width), round_filters(1280, width), size


def _bn(prefix, c):
    return [(prefix + '.weight', (c,)), (prefix + '.bias', (c,)), (prefix + '.running_mean', (c,)),
            (prefix + '.running_var', (c,)), (prefix + '.num_batches_tracked', ())]


def state_shapes(variant, heads, use_skip):
    """ordered [(state-dict key, shape)] of CenterEfficientNet; heads: {name: channels}"""
    bl, stem, head, _ = blocks(variant)
    keys = [('base._conv_stem.weight', (stem, 3, 3, 3))] + _bn('base._bn0', stem)
    for i, (ci, co, k, s, e, cse, _) in enumerate(bl):
        p, mid = 'base._blocks.%d.' % i, ci * e
        if e != 1:
            keys += [(p + '_expand_conv.weight', (mid, ci, 1, 1))] + _bn(p + '_bn0', mid)
        keys += [(p + '_depthwise_conv.weight', (mid, 1, k, k))] + _bn(p + '_bn1', mid)
        keys += [(p + '_se_reduce.weight', (cse, mid, 1, 1)), (p + '_se_reduce.bias', (cse,)),
                 (p + '_se_expand.weight', (mid, cse, 1, 1)), (p + '_se_expand.bias', (mid,))]
        keys += [(p + '_project_conv.weight', (co, mid, 1, 1))] + _bn(p + '_bn2', co)
    keys += [('base._conv_head.weight', (head, bl[-1][1], 1, 1))] + _bn('base._bn1', head)
    keys += [('base._fc.weight', (1000, head)), ('base._fc.bias', (1000,))]
    cin = head
    for i in range(3):
        keys += [('deconv_layers.%d.weight' % (3 * i), (cin, 256, 4, 4))] + _bn('deconv_layers.%d' % (3 * i + 1), 256)
        cin = 256
    if use_skip:
        for did, fid in SKIPS[variant].items():
            keys += [('skip_%d.0.weight' % did, (256, bl[fid][1], 1, 1)), ('skip_%d.0.bias' % did, (256,))] + \
                _bn('skip_%d.1' % did, 256)
    for h in sorted(heads):
        keys += [(h + '.0.weight', (256, 256, 3, 3)), (h + '.0.bias', (256,)), (h + '.2.weight', (heads[h], 256, 1, 1)),
                 (h + '.2.bias', (heads[h],))]
    return keys


# ----------------------------------------------------------------------------- network
class Net:
    """forward(x) over a state dict `sd` (name -> tensor; the running statistics are updated in place in training mode,
    like nn.BatchNorm2d).  masks: {block index: drop-connect mask [B]} for the blocks that drop (training only)."""

    def __init__(self, sd, variant, heads, use_skip):
        self.sd, self.variant, self.heads, self.use_skip = sd, variant, list(heads), use_skip
        self.training = False

    def bn(self, x, p, momentum, eps):
        sd = self.sd
        if self.training:
            sd[p + '.num_batches_tracked'] += 1
        return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'],
                            self.training, momentum, eps)

    def block(self, x, i, spec, mask):
        ci, co, k, s, e, _, size = spec
        sd, p = self.sd, 'base._blocks.%d.' % i
        y = x
        if e != 1:
            y = swish(self.bn(F.conv2d(y, sd[p + '_expand_conv.weight']), p + '_bn0', 0.01, 1e-3))
        y = swish(self.bn(dwconv_same(y, sd[p + '_depthwise_conv.weight'], s, (size, size)), p + '_bn1', 0.01, 1e-3))
        y = squeeze_excite(y, sd[p + '_se_reduce.weight'], sd[p + '_se_reduce.bias'], sd[p + '_se_expand.weight'],
                           sd[p + '_se_expand.bias'])
        y = self.bn(F.conv2d(y, sd[p + '_project_conv.weight']), p + '_bn2', 0.01, 1e-3)
        if s == 1 and ci == co:
            if self.training and mask is not None:
                y = y * mask.view(-1, 1, 1, 1).to(y.dtype)
            y = y + x
        return y

    def forward(self, x, masks=None):
        sd = self.sd
        bl, _, _, size = blocks(self.variant)
        pt, pb = same_pads(size, 3, 2)
        x = F.conv2d(F.pad(x, (pt, pb, pt, pb)), sd['base._conv_stem.weight'], None, 2)
        x = swish(self.bn(x, 'base._bn0', 0.01, 1e-3))
        skip = {}
        sources = {v: k for k, v in SKIPS[self.variant].items()} if self.use_skip else {}
        for i, spec in enumerate(bl):
            x = self.block(x, i, spec, (masks or {}).get(i))
            if i in sources:
                skip[sources[i]] = x
        x = swish(self.bn(F.conv2d(x, sd['base._conv_head.weight']), 'base._bn1', 0.01, 1e-3))
        for i in range(3):
            x = F.conv_transpose2d(x, sd['deconv_layers.%d.weight' % (3 * i)], None, 2, 1)
            x = F.relu(self.bn(x, 'deconv_layers.%d' % (3 * i + 1), 0.1, 1e-5))
            lid = 3 * i + 2
            if lid in skip:
                s = F.conv2d(skip[lid], sd['skip_%d.0.weight' % lid], sd['skip_%d.0.bias' % lid])
                x = F.relu(self.bn(s, 'skip_%d.1' % lid, 0.1, 1e-5)) + x
        out = {}
        for h in self.heads:
            y = F.relu(F.conv2d(x, sd[h + '.0.weight'], sd[h + '.0.bias'], 1, 1))
            out[h] = F.conv2d(y, sd[h + '.2.weight'], sd[h + '.2.bias'])
        return out


def make_state(np_state, dtype):
    """numpy state -> tensors of `dtype` (integer buffers stay int64); parameters require a gradient"""
    sd = {}
    for k, v in np_state.items():
        t = torch.from_numpy(v.copy())
        if t.is_floating_point():
            t = t.to(dtype)
            if not k.endswith(('running_mean', 'running_var')):
                t.requires_grad_(True)
        sd[k] = t
    return sd
