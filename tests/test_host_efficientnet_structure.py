"""Host-side (no GPU) checks of the EfficientNet backend's module tree: state_dict names, order and shapes against the
oracle's list built from the published block table (tests/efficientnet_oracle.py), the width / depth rounding rules, the
static SAME padding, and the options this build declines."""
import inspect

import pytest
import torch

import efficientnet_oracle as eo


def test_state_dict_names_shapes_and_order_match_the_oracle():
    from backends import efficientnet
    model = efficientnet.build(6, 'b0', num_keypoints=4, pretrained=False, use_skip=True)
    want = eo.state_shapes('b0', {'hm': 6, 'wh': 2, 'reg': 2, 'kps': 8}, True)
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert [k for k, _ in got] == [k for k, _ in want]
    assert got == want
    assert len(model.base._blocks) == 16
    assert not hasattr(model.base._blocks[0], '_expand_conv') and 'base._blocks.0._bn0.weight' not in dict(got)
    assert hasattr(model.base._blocks[1], '_expand_conv')
    # skip sources: block 4 (40 channels, H/8) joins after the second stage, block 10 (112 channels, H/16) after the first
    assert dict(got)['skip_5.0.weight'] == (256, 40, 1, 1) and dict(got)['skip_2.0.weight'] == (256, 112, 1, 1)
    assert model.down_ratio == 4 and model.rotated_boxes is False and model.variant == 'b0'
    assert list(model.heads) == ['hm', 'wh', 'reg', 'kps']
    assert [n for n, _ in model.named_children()][-4:] == ['hm', 'kps', 'reg', 'wh']      # registered in sorted order
    for m in model.base.modules():
        if type(m).__name__ == 'BatchNorm2d':
            assert m.momentum == 0.01 and m.eps == 1e-3
    assert model.deconv_layers[1].momentum == 0.1 and model.deconv_layers[1].eps == 1e-5


@pytest.mark.parametrize('variant,n_blocks,head', [('b0', 16, 1280), ('b1', 23, 1280), ('b2', 23, 1408), ('b3', 26, 1536)])
def test_rounding_rules_give_the_published_depths_and_widths(variant, n_blocks, head):
    from backends import efficientnet
    model = efficientnet.build(2, variant, pretrained=False)
    assert len(model.base._blocks) == n_blocks
    assert model.base._conv_head.out_channels == model.base._bn1.num_features == head
    assert model.deconv_layers[0].weight.shape == (head, 256, 4, 4)
    want = eo.state_shapes(variant, {'hm': 2, 'wh': 2, 'reg': 2}, False)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    assert not any(k.startswith('skip_') for k in model.state_dict())


def test_round_filters_and_repeats():
    from backends.efficientnet import round_filters, round_repeats
    assert [round_filters(c, 1.0) for c in (32, 16, 24, 1280)] == [32, 16, 24, 1280]
    assert [round_filters(c, 1.1) for c in (32, 16, 24, 40, 320, 1280)] == [32, 16, 24, 48, 352, 1408]
    assert [round_filters(c, 1.2) for c in (32, 16, 24, 40, 80, 112, 192, 320)] == [40, 24, 32, 48, 96, 136, 232, 384]
    assert [round_repeats(r, 1.4) for r in (1, 2, 3, 4)] == [2, 3, 5, 6]
    assert [round_repeats(r, 1.1) for r in (1, 2, 3, 4)] == [2, 3, 4, 5]


def test_static_same_padding_follows_the_nominal_resolution():
    from backends import efficientnet
    from hip_runtime import ops
    assert ops.same_padding(224, 3, 2) == (0, 1) and ops.same_padding(112, 3, 1) == (1, 1)
    assert ops.same_padding(56, 5, 2) == (1, 2) and ops.same_padding(15, 5, 2) == (2, 2) and ops.same_padding(1, 3, 1) == (1, 1)
    for variant in ('b0', 'b1', 'b3'):
        model = efficientnet.build(2, variant, pretrained=False)
        specs = eo.blocks(variant)[0]
        for block, (_, _, k, s, _, _, size) in zip(model.base._blocks, specs):
            (pt, pb), (pl, pr) = eo.same_pads(size, k, s), eo.same_pads(size, k, s)
            assert block._depthwise_conv.static_padding == (pt, pl, pb, pr)
        assert model.base.stem_padding == 1
    # b1 at 240: the stride-2 5x5 block at a 15 x 15 nominal map pads 2 + 2, where an even map would pad 1 + 2
    b1 = efficientnet.build(2, 'b1', pretrained=False)
    assert [b._depthwise_conv.static_padding for b in b1.base._blocks if b.stride == 2 and b.kernel_size == 5] == \
        [(1, 1, 2, 2), (2, 2, 2, 2)]


def test_declined_options_and_signature():
    from backends import efficientnet
    sig = inspect.signature(efficientnet.build)
    assert list(sig.parameters) == ['num_classes', 'variant', 'num_keypoints', 'pretrained', 'freeze_base', 'rotated_boxes',
                                    'use_skip', 'kwargs']
    assert sig.parameters['variant'].default == 'b0' and sig.parameters['pretrained'].default is True
    with pytest.raises(NotImplementedError, match='use_upsample'):
        efficientnet.build(2, 'b0', pretrained=False, use_upsample=True)
    with pytest.raises(NotImplementedError, match='b5'):
        efficientnet.build(2, 'b5', pretrained=False)
    with pytest.raises(RuntimeError, match='not found'):              # no silent random init for pretrained=True
        efficientnet.build(2, 'b0')
    m = efficientnet.build(3, 'b0', num_keypoints=0, pretrained=False, freeze_base=True, rotated_boxes=True)
    assert m.state_dict()['wh.2.weight'].shape == (3, 256, 1, 1) and m.rotated_boxes is True
    assert not any(p.requires_grad for p in m.base.parameters())
    assert all(p.requires_grad for p in m.deconv_layers.parameters())
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))                                  # CPU tensors are refused


def test_drop_connect_rate_is_scaled_by_block_index():
    from backends import efficientnet
    base = efficientnet.build(2, 'b0', pretrained=False).base
    assert base.block_rate(0) == 0.0 and base.block_rate(8) == pytest.approx(0.1) and base.block_rate(15) == pytest.approx(0.1875)


def test_oracle_network_runs_on_the_product_state_dict():
    """the oracle is a function of the product's state dict: every key it reads exists, shapes fit, and the maps come out
    at H/4"""
    from backends import efficientnet
    model = efficientnet.build(6, 'b0', num_keypoints=4, pretrained=False, use_skip=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    net = eo.Net(sd, 'b0', model.heads, True)
    with torch.no_grad():
        out = net.forward(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)))
    assert {k: tuple(v.shape) for k, v in out.items()} == {'hm': (1, 6, 16, 16), 'wh': (1, 2, 16, 16), 'reg': (1, 2, 16, 16),
                                                           'kps': (1, 8, 16, 16)}
    assert list(out) == ['hm', 'wh', 'reg', 'kps'] and all(torch.isfinite(v).all() for v in out.values())
