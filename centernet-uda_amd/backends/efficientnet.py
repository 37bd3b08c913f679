"""EfficientNet CenterNet backend for MI355X (the reference's fourth backend; variants b0 .. b3).

Plugin contract of the reference (backends/efficientnet.py:203-223): `build(num_classes, variant='b0', num_keypoints=0,
pretrained=True, freeze_base=False, rotated_boxes=False, use_skip=False, **kwargs)` returns an nn.Module with
`.down_ratio == 4`, `.rotated_boxes`, `.variant` and `forward(x[B,3,H,W]) -> {'hm','wh','reg'[, 'kps']}` raw logits at
H/4.  Heads are registered in `sorted(heads)` order (:94) and emitted in `heads` insertion order (:145-148).

The trunk is `torch.hub.load('lukemelas/EfficientNet-PyTorch', 'efficientnet_<variant>')` (:53-56), a third-party
network the reference neither vendors nor pins by a test; its published architecture is restated here so that the
state_dict keys under `base.` are the ones that port produces:

    base._conv_stem, base._bn0      3x3 stride 2, 3 -> round_filters(32), SAME padding, BN, swish
    base._blocks.<i>                MBConvBlock (hip_runtime.nn), table (repeats, k, stride, expand, in, out), SE ratio 0.25:
                                    (1,3,1,1,32,16) (2,3,2,6,16,24) (2,5,2,6,24,40) (3,3,2,6,40,80) (3,5,1,6,80,112)
                                    (4,5,2,6,112,192) (1,3,1,6,192,320); widths through round_filters, repeats through
                                    round_repeats; variant (width, depth, nominal resolution): b0 (1.0,1.0,224)
                                    b1 (1.0,1.1,240) b2 (1.1,1.2,260) b3 (1.2,1.4,300)
    base._conv_head, base._bn1      1x1 -> round_filters(1280), BN, swish
    base._fc                        the classifier, unused but present (its keys are in every checkpoint)
    SAME padding is the static form: fixed per layer from the variant's nominal resolution followed through the strides.
    drop_connect_rate 0.2, scaled by idx / len(blocks) per block (:117-122); BN momentum 0.01, eps 1e-3.
    initialisation: convolutions normal(0, sqrt(2 / (k*k*out))), BN weight 1 / bias 0

What the reference owns, restated from its file: three up-sampling stages ConvTranspose2d 4x4/2 pad 1 (no bias) + BN(0.1)
+ ReLU to 256 channels (:163-200), optional skip branches `skip_<id>` = 1x1 convolution (bias) + BN + ReLU from trunk
blocks SKIP_MAPPINGS[variant] added after the stage whose ReLU has index <id> in `deconv_layers` (:8-29, :71-91,
:129-134), and per-head 3x3(256->256) + ReLU + 1x1 (:93-110, torch default init).  The `use_upsample` option (bilinear
x4 + stride-2 convolution instead of the transposed convolution, :176-185; no config sets it) is declined.  The stages,
the walk over them, the heads and the checkpoint lookup are backends/common.py's; this file is the trunk, the skip
branches and where they join.

All layers run on this repo's gfx950 kernels: 1x1 / 3x3 / transposed convolutions on the implicit-GEMM MFMA kernels,
the depthwise SAME convolution on the depthwise kernels of csrc/spatial.hip, swish, squeeze-and-excite, drop-connect
and the stem's zero-pad copy on csrc/mbconv.hip.
"""
import math

import torch
from torch import nn

from backends import common
from hip_runtime import nn as hnn
from hip_runtime import ops
from hip_runtime.fanout import fork

# key = deconv layer index, value = feature extractor block index (efficientnet.py:8-29; b7 is not built here)
SKIP_MAPPINGS = {
    "b0": {5: 4, 2: 10},
    "b1": {5: 7, 2: 15},
    "b2": {5: 7, 2: 15},
    "b3": {5: 7, 2: 17},
}
SKIP_MAPPINGS_REVERSED = {variant: {v: k for k, v in mapping.items()} for variant, mapping in SKIP_MAPPINGS.items()}

# (repeats, kernel, stride, expand ratio, in, out)
BLOCK_TABLE = ((1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
               (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320))
# variant -> (width coefficient, depth coefficient, nominal resolution)
VARIANTS = {'b0': (1.0, 1.0, 224), 'b1': (1.0, 1.1, 240), 'b2': (1.1, 1.2, 260), 'b3': (1.2, 1.4, 300)}
DROP_CONNECT_RATE = 0.2
# what the hub entry point downloads into the hub checkpoint cache
_PRETRAINED = {'b0': 'efficientnet-b0-355c32eb.pth', 'b1': 'efficientnet-b1-f1951068.pth',
               'b2': 'efficientnet-b2-8bb594d6.pth', 'b3': 'efficientnet-b3-5fb5a3c3.pth'}


def round_filters(filters, width):
    """channels scaled by the width coefficient, to the nearest multiple of 8 (at least 8, never below 90 % of the scaled
    value)"""
    scaled = filters * width
    new = max(8, int(scaled + 4) // 8 * 8)
    if new < 0.9 * scaled:
        new += 8
    return int(new)


def round_repeats(repeats, depth):
    return int(math.ceil(depth * repeats))


class EfficientNet(nn.Module):
    """The trunk, with the module names of the published PyTorch port."""

    def __init__(self, variant):
        super().__init__()
        width, depth, size = VARIANTS[variant]
        bn = lambda c: hnn.BatchNorm2d(c, momentum=0.01, eps=1e-3)
        stem = round_filters(32, width)
        # the stem's SAME padding (nothing on top / left for every variant built here) is a zero-pad copy in front of a
        # padding-0 convolution: the implicit-GEMM loaders keep their symmetric padding
        pt, pb = ops.same_padding(size, 3, 2)
        assert pt == 0, "stem padding of %s" % variant
        self.stem_padding = pb
        self._conv_stem = hnn.Conv2d(3, stem, 3, stride=2, padding=0, bias=False)
        self._bn0 = bn(stem)
        size = -(-size // 2)
        blocks = []
        for repeats, k, stride, expand, cin, cout in BLOCK_TABLE:
            cin, cout = round_filters(cin, width), round_filters(cout, width)
            for i in range(round_repeats(repeats, depth)):
                blocks.append(hnn.MBConvBlock(cin if i == 0 else cout, cout, k, stride if i == 0 else 1, expand,
                                              se_ratio=0.25, image_size=size))
                if i == 0:
                    size = -(-size // stride)
        self._blocks = nn.ModuleList(blocks)
        head = round_filters(1280, width)
        self._conv_head = hnn.Conv2d(blocks[-1].out_channels, head, 1, bias=False)
        self._bn1 = bn(head)
        self._fc = nn.Linear(head, 1000)
        self.drop_connect_rate = DROP_CONNECT_RATE
        common.kaiming_fan_out_((self._conv_stem, self._conv_head))

    def stem(self, x):
        x = ops.pad_right_bottom(x, self.stem_padding, self.stem_padding)
        return ops.swish(self._bn0(self._conv_stem(x)))

    def head(self, x):
        return ops.swish(self._bn1(self._conv_head(x)))

    def block_rate(self, idx):
        """the drop-connect rate of block idx (efficientnet.py:117-122)"""
        return self.drop_connect_rate * float(idx) / len(self._blocks)


class CenterEfficientNet(common.DeconvBackend):
    def __init__(self, variant, heads, pretrained, freeze_base=False, use_skip=False, rotated_boxes=False,
                 use_upsample=False, num_head_channels=256, num_deconv_channels=(256, 256, 256)):
        if use_upsample:
            raise NotImplementedError("CenterEfficientNet: use_upsample=True (bilinear up-sampling + stride-2 convolution "
                                      "instead of ConvTranspose2d) is not built here; no experiment config sets it")
        assert len(num_deconv_channels) == 3
        base = EfficientNet(variant)
        super().__init__(base, base._bn1.num_features, freeze_base, rotated_boxes,
                         deconv_channels=list(num_deconv_channels))
        self.use_skip = use_skip
        self.variant = variant
        self.use_upsample = False
        if pretrained:
            self._load_pretrained()
        if self.use_skip:
            for deconv_id, fe_id in SKIP_MAPPINGS[variant].items():
                in_channels = self.base._blocks[fe_id]._project_conv.out_channels
                out_channels = self.deconv_layers[deconv_id - 2].out_channels      # -2: conv, bn, relu
                setattr(self, "skip_%d" % deconv_id, nn.Sequential(
                    hnn.Conv2d(in_channels, out_channels, 1, padding=0), hnn.BatchNorm2d(out_channels), hnn.Slot()))
        self.add_heads(heads, head_conv=num_head_channels)

    def _load_pretrained(self):
        """the published port's ImageNet weights (efficientnet.py:53-56): its names are the trunk's, `_fc` included"""
        path = common.hub_checkpoint(_PRETRAINED[self.variant], 'efficientnet_%s' % self.variant)
        self.base.load_state_dict(torch.load(path, map_location='cpu'))

    def skip_branch(self, lid, feature):
        branch = getattr(self, "skip_%d" % lid)
        return branch[1](branch[0](feature), relu=True)

    def forward_to_deconv(self, x):
        base = self.base
        sources = SKIP_MAPPINGS_REVERSED[self.variant] if self.use_skip else {}
        skip = {}
        x = base.stem(x)
        for idx, block in enumerate(base._blocks):
            x = block(x, drop_connect_rate=base.block_rate(idx))
            if idx in sources:
                x, skip[sources[idx]] = fork(x, 2)          # the next block's input | the skip branch's
        return self.upsample(base.head(x), skip)      # ids 2 and 5: the branch joins after the stage's ReLU (:129-134)

    def forward(self, x):
        x = self.forward_to_deconv(x)
        return {head: getattr(self, head)(f) for head, f in zip(self.heads, fork(x, len(self.heads)))}


def build(num_classes, variant='b0', num_keypoints=0, pretrained=True, freeze_base=False, rotated_boxes=False,
          use_skip=False, **kwargs):
    if variant not in VARIANTS:
        raise NotImplementedError("EfficientNet variant %s is not implemented (built here: %s)"
                                  % (variant, ', '.join(sorted(VARIANTS))))
    heads = common.head_table(num_classes, num_keypoints, rotated_boxes)
    return CenterEfficientNet(variant, heads, pretrained=pretrained, freeze_base=freeze_base,
                              rotated_boxes=rotated_boxes, use_skip=use_skip, **kwargs)
