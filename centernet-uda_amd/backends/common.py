"""What the CenterNet backends share.  The reference restates these pieces in each of backends/resnet.py,
mobilenetv2.py and efficientnet.py (and partly in dla.py); here each is written once:

    head_table         the ordered heads {'hm', 'wh', 'reg'[, 'kps']} every build() starts from
    make_head          3x3 + ReLU + final convolution of one head (hip_runtime.nn.Head)
    DeconvBackend      trunk -> three up-sampling stages [DCN 3x3 + BN + ReLU]? + ConvTranspose2d + BN + ReLU -> heads:
                       the attributes, the freeze, `deconv_layers`, the walk over it with its skip joins, the heads'
                       registration in sorted order
    hub_checkpoint     where a trunk's published ImageNet weights are looked for (there is no download in this build)
    kaiming_fan_out_   the trunks' convolution initialisation
    conv_to_bn, freeze
"""
import math
import os

import torch
from torch import nn

from hip_runtime import nn as hnn
from hip_runtime import ops
from libs.DCNv2.dcn_v2 import DCN

DECONV_CFG = {4: (4, 1, 0), 3: (3, 1, 1), 2: (2, 0, 0)}      # deconv kernel -> kernel, padding, output_padding


def head_table(num_classes, num_keypoints=0, rotated_boxes=False):
    heads = {'hm': num_classes, 'wh': 3 if rotated_boxes else 2, 'reg': 2}
    if num_keypoints > 0:
        heads['kps'] = num_keypoints * 2
    return heads


def make_head(cin, head_conv, classes, final_kernel=1):
    return hnn.Head(
        hnn.Conv2d(cin, head_conv, 3, padding=1, bias=True, act_slope=0.0),
        hnn.Slot(),      # index of the reference's nn.ReLU (fused into conv '0')
        hnn.Conv2d(head_conv, classes, final_kernel, padding=final_kernel // 2, bias=True))


def conv_to_bn(cin, cout, k, stride=1):
    return hnn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False, emit_stats=True)    # (every caller: conv -> BatchNorm)


def freeze(module):
    for p in module.parameters():
        p.requires_grad = False


def kaiming_fan_out_(modules):
    """kaiming_normal_(mode='fan_out', nonlinearity='relu') for the convolutions (dense or depthwise) among `modules`"""
    with torch.no_grad():
        for m in modules:
            if isinstance(m, (hnn.Conv2d, hnn.DepthwiseConv2d)):
                fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.normal_(0.0, math.sqrt(2.0 / fan_out))


def hub_checkpoint_path(filename):
    return os.path.join(torch.hub.get_dir(), 'checkpoints', filename)


def hub_checkpoint(filename, what):
    """The reference downloads a trunk's ImageNet weights through torch.hub.  There is no network path in this build:
    the file is taken from the hub checkpoint cache if present, otherwise this raises like a failed download does."""
    path = hub_checkpoint_path(filename)
    if not os.path.isfile(path):
        raise RuntimeError("%s pretrained=True: %s not found (no download in this build; place the published "
                           "checkpoint there or pass pretrained=False)" % (what, path))
    return path


def make_deconv_layers(inplanes, num_filters, num_kernels, use_dcn=False):
    """children: per stage [DCN 3x3, BatchNorm2d, ReLU slot]? + ConvTranspose2d /2 (no bias), BatchNorm2d, ReLU slot.
    With `use_dcn` the DCN maps inplanes -> planes and the ConvTranspose2d planes -> planes."""
    assert len(num_filters) == len(num_kernels)
    layers = []
    for planes, num_kernel in zip(num_filters, num_kernels):
        kernel, padding, output_padding = DECONV_CFG[num_kernel]
        if use_dcn:
            layers += [DCN(inplanes, planes, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1),
                       hnn.BatchNorm2d(planes, momentum=0.1), hnn.Slot()]
            inplanes = planes
        layers += [hnn.ConvTranspose2d(inplanes, planes, kernel, stride=2, padding=padding,
                                       output_padding=output_padding),
                   hnn.BatchNorm2d(planes, momentum=0.1), hnn.Slot()]
        inplanes = planes
    return nn.Sequential(*layers)


class DeconvBackend(nn.Module):
    """A trunk (`base`, already initialised or loaded) and the up-sampling neck on its `inplanes` channels.  The
    subclass registers its skip branches, then calls add_heads()."""

    def __init__(self, base, inplanes, freeze_base=False, rotated_boxes=False, use_dcn=False,
                 deconv_channels=(256, 256, 256)):
        super().__init__()
        self.deconv_with_bias = False
        self.down_ratio = 4
        self.rotated_boxes = rotated_boxes
        self.base = base
        if freeze_base:
            freeze(base)
        self.deconv_layers = make_deconv_layers(inplanes, deconv_channels, [4] * len(deconv_channels), use_dcn)
        self.inplanes = deconv_channels[-1]

    def add_heads(self, heads, head_conv):
        """registered in sorted order, emitted by forward() in the order of `heads`"""
        self.heads = heads
        for head in sorted(heads):
            setattr(self, head, make_head(self.inplanes, head_conv, heads[head]))

    def upsample(self, x, skip=()):
        """skip: {child index of deconv_layers: trunk feature}.  self.skip_branch(index, feature) is added to that
        child's output: at a convolution's index between it and its BatchNorm, at a ReLU slot's index after the stage.
        The branch is evaluated right where it joins."""
        d = self.deconv_layers
        for lid in range(0, len(d), 3):          # (conv-like, BN, ReLU) triples: BN + ReLU is one kernel
            x = d[lid](x)
            if lid in skip:
                x = ops.add(self.skip_branch(lid, skip[lid]), x)
            x = d[lid + 1](x, relu=True)
            if lid + 2 in skip:
                x = ops.add(self.skip_branch(lid + 2, skip[lid + 2]), x)
        return x
