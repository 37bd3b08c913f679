"""MobileNetV2 CenterNet backend for MI355X.

Plugin contract of the reference (backends/mobilenetv2.py:168-186): `build(num_classes, num_keypoints=0,
pretrained=True, freeze_base=False, use_dcn=False, use_skip=False, rotated_boxes=False)` returns an nn.Module
with `.down_ratio == 4`, `.rotated_boxes` and `forward(x[B,3,H,W]) -> {'hm','wh','reg'[, 'kps']}` raw logits at
H/4.  Heads are registered in `sorted(heads)` order (mobilenetv2.py:75) and emitted in `heads` insertion order
(:115-117).

The trunk is `torch.hub.load('pytorch/vision:v0.6.0', 'mobilenet_v2').features` (mobilenetv2.py:31-36), a
third-party network the reference neither vendors nor pins by a test; its published architecture is restated
here so that the state_dict keys are the ones `mobilenet_v2.features` produces under the name `base`:

    base.0            ConvBNReLU(3, 32, 3x3 stride 2)           children 0 conv, 1 BN, 2 ReLU6
    base.1 .. base.17 InvertedResidual, settings (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2)
                      (6,96,3,1) (6,160,3,2) (6,320,1,1); `.conv` = [ConvBNReLU 1x1 expand (t != 1)],
                      ConvBNReLU 3x3 depthwise (stride), Conv2d 1x1 project, BN; residual iff stride 1 and in == out
    base.18           ConvBNReLU(320, 1280, 1x1)
    initialisation: kaiming_normal_(fan_out) for convolutions, BN weight 1 / bias 0

What the reference owns, restated from its file: three up-sampling stages `[DCN 3x3 + BN + ReLU]? +
ConvTranspose2d 4x4/2 pad 1 (no bias) + BN + ReLU` to 256 channels (:133-165; note that with `use_dcn` the first
DCN maps 1280 -> 256 and every ConvTranspose is 256 -> 256), optional 1x1 skip convolutions from trunk layers 13
and 6 added right after deconv-list entries 0 and 3 (:9-16, :66-72, :96-107 -- which only fits without `use_dcn`,
where those entries are the first two ConvTranspose layers; with both flags the reference fails on the shape
mismatch and so does this build), and per-head 3x3(256->64) + ReLU + 1x1 (:74-90, torch default init).  The stages, the walk over them, the heads and
the checkpoint lookup are backends/common.py's; this file is the trunk, the skip convolutions and where they join.

All layers run on this repo's gfx950 kernels: 1x1 / 3x3 convolutions on the implicit-GEMM MFMA kernels, the
depthwise 3x3 on `cnuda_dwconv2d_*` (the depthwise kernels of csrc/spatial.hip, which EfficientNet's SAME-padded
layers share), BN (+ residual) + ReLU6 in one kernel, DCN on the deformable kernels.
"""
import torch
from torch import nn

from backends import common
from hip_runtime import nn as hnn

# key = deconv layer index, value = feature extractor layer index (mobilenetv2.py:9-16)
SKIP_MAPPING = {3: 6, 0: 13}
SKIP_MAPPING_REVERSED = {v: k for k, v in SKIP_MAPPING.items()}
_SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
_PRETRAINED = 'mobilenet_v2-b0353104.pth'      # what torchvision 0.6 downloads into the hub checkpoint cache


class ConvBNReLU(nn.Sequential):
    """children '0' conv (dense or depthwise, no bias), '1' BN, '2' ReLU6 slot (fused into the BN kernel)"""

    def __init__(self, cin, cout, kernel_size=3, stride=1, groups=1):
        pad = (kernel_size - 1) // 2
        if groups == 1:
            conv = hnn.Conv2d(cin, cout, kernel_size, stride=stride, padding=pad, bias=False)
        elif groups == cin == cout:
            conv = hnn.DepthwiseConv2d(cin, kernel_size, stride=stride, padding=pad)
        else:
            raise NotImplementedError("grouped convolution other than depthwise")
        super().__init__(conv, hnn.BatchNorm2d(cout), hnn.Slot())
        self.out_channels = cout

    def forward(self, x):
        return self[1](self[0](x), relu=6)


class InvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        hidden = int(round(inp * expand_ratio))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand_ratio != 1:
            layers.append(ConvBNReLU(inp, hidden, kernel_size=1))
        layers += [ConvBNReLU(hidden, hidden, stride=stride, groups=hidden),
                   hnn.Conv2d(hidden, oup, 1, bias=False), hnn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        y = x
        for m in self.conv[:-2]:
            y = m(y)
        y = self.conv[-2](y)
        return self.conv[-1](y, residual=x if self.use_res_connect else None)      # BN + the residual add, no ReLU


def _features():
    layers = [ConvBNReLU(3, 32, stride=2)]
    cin = 32
    for t, c, n, s in _SETTINGS:
        for i in range(n):
            layers.append(InvertedResidual(cin, c, s if i == 0 else 1, t))
            cin = c
    layers.append(ConvBNReLU(cin, 1280, kernel_size=1))
    base = nn.Sequential(*layers)
    common.kaiming_fan_out_(base.modules())
    return base


class CenterMobileNetV2(common.DeconvBackend):
    def __init__(self, heads, pretrained, freeze_base=False, use_dcn=False, use_skip=False, rotated_boxes=False):
        super().__init__(_features(), 1280, freeze_base, rotated_boxes, use_dcn)
        self.use_skip = use_skip
        self.use_dcn = use_dcn
        if pretrained:
            self._load_pretrained()
        if self.use_skip:
            for deconv_id, fe_id in SKIP_MAPPING.items():
                in_channels = self.base[fe_id].conv[-2].out_channels
                out_channels = self.deconv_layers[deconv_id].out_channels
                setattr(self, "skip_%d" % deconv_id, hnn.Conv2d(in_channels, out_channels, 1, padding=0))
        self.add_heads(heads, head_conv=64)

    def _load_pretrained(self):
        """torchvision's ImageNet weights (mobilenetv2.py:31-34): the `features.` part, under the names of `base`"""
        tv = torch.load(common.hub_checkpoint(_PRETRAINED, 'mobilenet_v2'), map_location='cpu')
        self.base.load_state_dict({k[len('features.'):]: v for k, v in tv.items() if k.startswith('features.')})

    def skip_branch(self, lid, feature):
        return getattr(self, "skip_%d" % lid)(feature)

    def forward(self, x):
        skip = {}
        for lid, layer in enumerate(self.base):
            x = layer(x)
            if self.use_skip and lid in SKIP_MAPPING_REVERSED:
                skip[SKIP_MAPPING_REVERSED[lid]] = x
        x = self.upsample(x, skip)       # ids 0 and 3: the skip lands between the convolution and its BN (:103-107)
        return {head: getattr(self, head)(x) for head in self.heads}


def build(num_classes, num_keypoints=0, pretrained=True, freeze_base=False, use_dcn=False, use_skip=False,
          rotated_boxes=False):
    heads = common.head_table(num_classes, num_keypoints, rotated_boxes)
    return CenterMobileNetV2(heads, pretrained=pretrained, freeze_base=freeze_base, use_dcn=use_dcn,
                             use_skip=use_skip, rotated_boxes=rotated_boxes)
