"""Host-side (no GPU) checks of what the backends share (backends/common.py, uda.base.Model.forward_both): the head
table, the up-sampling neck's builder, the ImageNet checkpoint lookup with each deconv backend's key mapping, and the
one-pass / two-pass decision of the two-domain plugins."""
import os

import pytest
import torch


# ---------------------------------------------------------------------------
# head table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kps,rotated,want', [
    (0, False, {'hm': 5, 'wh': 2, 'reg': 2}), (0, True, {'hm': 5, 'wh': 3, 'reg': 2}),
    (4, False, {'hm': 5, 'wh': 2, 'reg': 2, 'kps': 8}), (4, True, {'hm': 5, 'wh': 3, 'reg': 2, 'kps': 8})])
def test_head_table(kps, rotated, want):
    from backends.common import head_table
    got = head_table(5, kps, rotated)
    assert got == want and list(got) == list(want)
    assert head_table(5, num_keypoints=kps, rotated_boxes=rotated) == want


def test_every_build_emits_the_head_table_in_its_order():
    from backends import dla, efficientnet, mobilenetv2, resnet
    from backends.common import head_table
    want = head_table(3, 2, True)
    models = [resnet.build(18, 3, num_keypoints=2, pretrained=False, rotated_boxes=True),
              mobilenetv2.build(3, num_keypoints=2, pretrained=False, rotated_boxes=True),
              efficientnet.build(3, 'b0', num_keypoints=2, pretrained=False, rotated_boxes=True),
              dla.build(3, num_keypoints=2, rotated_boxes=True)]
    for m in models:
        assert dict(m.heads) == want and list(m.heads) == ['hm', 'wh', 'reg', 'kps']      # what forward() walks
        assert m.wh[2].out_channels == 3 and m.kps[2].out_channels == 4
    for m in models[:3]:
        assert [n for n, _ in m.named_children()][-4:] == ['hm', 'kps', 'reg', 'wh']      # registered sorted
    assert [n for n, _ in models[3].named_children()][-4:] == ['hm', 'wh', 'reg', 'kps']  # DLA: insertion order


# ---------------------------------------------------------------------------
# the neck's builder
# ---------------------------------------------------------------------------
def _check_stage(conv, bn, slot, cin, cout, kernel, padding, output_padding):
    from hip_runtime import nn as hnn
    assert type(conv) is hnn.ConvTranspose2d and not hasattr(conv, 'bias')
    assert (conv.in_channels, conv.out_channels) == (cin, cout) and conv.weight.shape == (cin, cout, kernel, kernel)
    assert conv.kernel_size == (kernel, kernel) and conv.stride == (2, 2)
    assert conv.padding == (padding, padding) and conv.output_padding == (output_padding, output_padding)
    assert type(bn) is hnn.BatchNorm2d and bn.num_features == cout and bn.momentum == 0.1 and bn.eps == 1e-5
    assert type(slot) is hnn.Slot


def test_neck_builder_plain_form():
    from backends.common import make_deconv_layers
    d = make_deconv_layers(512, [256, 128, 64], [4, 3, 2])
    assert type(d) is torch.nn.Sequential and len(d) == 9
    _check_stage(d[0], d[1], d[2], 512, 256, 4, 1, 0)
    _check_stage(d[3], d[4], d[5], 256, 128, 3, 1, 1)       # the padding table's rows no backend uses
    _check_stage(d[6], d[7], d[8], 128, 64, 2, 0, 0)
    assert [k for k in d.state_dict() if k.endswith('weight')] == ['0.weight', '1.weight', '3.weight', '4.weight',
                                                                   '6.weight', '7.weight']
    with pytest.raises(AssertionError):
        make_deconv_layers(512, [256, 256], [4, 4, 4])
    with pytest.raises(KeyError):
        make_deconv_layers(512, [256], [5])


def test_neck_builder_dcn_form():
    from backends.common import make_deconv_layers
    from hip_runtime import nn as hnn
    from libs.DCNv2.dcn_v2 import DCN
    d = make_deconv_layers(1280, [256, 256, 256], [4, 4, 4], use_dcn=True)
    assert type(d) is torch.nn.Sequential and len(d) == 18
    for i in range(0, 18, 6):
        dcn, bn, slot = d[i], d[i + 1], d[i + 2]
        assert type(dcn) is DCN and dcn.weight.shape == (256, 1280 if i == 0 else 256, 3, 3)
        assert dcn.conv_offset_mask.weight.shape == (27, 1280 if i == 0 else 256, 3, 3)
        assert type(bn) is hnn.BatchNorm2d and bn.num_features == 256 and bn.momentum == 0.1
        assert type(slot) is hnn.Slot
        _check_stage(d[i + 3], d[i + 4], d[i + 5], 256, 256, 4, 1, 0)


# ---------------------------------------------------------------------------
# checkpoint lookup and each backend's key mapping
# ---------------------------------------------------------------------------
@pytest.fixture
def hub(tmp_path):
    old = torch.hub.get_dir()
    torch.hub.set_dir(str(tmp_path))
    os.makedirs(tmp_path / 'checkpoints')
    yield tmp_path / 'checkpoints'
    torch.hub.set_dir(old)


def test_hub_checkpoint_names_model_path_and_the_way_out(hub):
    from backends.common import hub_checkpoint
    with pytest.raises(RuntimeError) as e:
        hub_checkpoint('some-model-0123.pth', 'some_model')
    msg = str(e.value)
    assert 'some_model' in msg and str(hub / 'some-model-0123.pth') in msg and 'pretrained=False' in msg
    (hub / 'some-model-0123.pth').write_bytes(b'')
    assert hub_checkpoint('some-model-0123.pth', 'some_model') == str(hub / 'some-model-0123.pth')


def _random_base_state(model, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(v.shape, generator=g) + 0.5 if v.is_floating_point() else v.clone()
            for k, v in model.base.state_dict().items()}


def _check_loaded(build, path, published, base_state, drop):
    """build(pretrained=True) finds `published` at `path` and ends up with `base_state`; without the key `drop` it raises"""
    torch.save(published, path)
    got = build().state_dict()
    assert sorted(k for k in got if k.startswith('base.')) == sorted('base.' + k for k in base_state)
    for k, v in base_state.items():
        assert torch.equal(got['base.' + k], v), k
    assert drop in published
    torch.save({k: v for k, v in published.items() if k != drop}, path)
    with pytest.raises(RuntimeError, match='Missing key'):
        build()


def test_resnet_loads_torchvision_names(hub):
    from backends import resnet
    state = _random_base_state(resnet.build(18, 3, pretrained=False), 1)
    names = ['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4']
    published = {'%s.%s' % (names[int(k.split('.', 1)[0])], k.split('.', 1)[1]): v for k, v in state.items()}
    assert 'conv1.weight' in published and 'layer1.0.bn1.running_mean' in published
    assert 'layer4.0.downsample.0.weight' in published and len(published) == len(state)
    published['fc.weight'], published['fc.bias'] = torch.zeros(1000, 512), torch.zeros(1000)      # ignored
    _check_loaded(lambda: resnet.build(18, 3), hub / 'resnet18-5c106cde.pth', published, state,
                  'layer1.0.bn1.running_mean')


def test_mobilenetv2_loads_torchvision_names(hub):
    from backends import mobilenetv2
    state = _random_base_state(mobilenetv2.build(3, pretrained=False), 2)
    published = {'features.' + k: v for k, v in state.items()}
    assert 'features.0.0.weight' in published and 'features.18.1.running_var' in published
    published['classifier.1.weight'], published['classifier.1.bias'] = torch.zeros(1000, 1280), torch.zeros(1000)
    _check_loaded(lambda: mobilenetv2.build(3, use_skip=True), hub / 'mobilenet_v2-b0353104.pth', published, state,
                  'features.7.conv.1.0.weight')


def test_efficientnet_loads_the_published_names_unchanged(hub):
    from backends import efficientnet
    state = _random_base_state(efficientnet.build(3, 'b0', pretrained=False), 3)
    assert '_conv_stem.weight' in state and '_blocks.0._bn1.running_mean' in state and '_fc.weight' in state
    _check_loaded(lambda: efficientnet.build(3, 'b0'), hub / 'efficientnet-b0-355c32eb.pth', dict(state), state,
                  '_fc.bias')


# ---------------------------------------------------------------------------
# one pass over source | target, or two calls
# ---------------------------------------------------------------------------
class _TwoCalls:
    """a backend without forward_domains"""

    def __init__(self):
        self.calls = []

    def __call__(self, x):
        self.calls.append(('call', x))
        return {'hm': x}


class _OnePass(_TwoCalls):
    def forward_domains(self, source, target, target_grad_heads=None):
        self.calls.append(('domains', source, target, target_grad_heads))
        return {'hm': source}, {'hm': target}


@pytest.mark.parametrize('batch_domains', [True, False])
@pytest.mark.parametrize('offers', [True, False])
@pytest.mark.parametrize('same_shape', [True, False])
def test_forward_both(batch_domains, offers, same_shape):
    from uda.base import Model
    plugin = Model()
    plugin.batch_domains = batch_domains
    plugin.target_grad_heads = ('hm', 'wh')
    plugin.backend = _OnePass() if offers else _TwoCalls()
    data = {'input': torch.zeros(2, 3, 8, 8), 'target_domain_input': torch.ones(2 if same_shape else 1, 3, 8, 8)}
    src, tgt, batched = plugin.forward_both(data)
    assert batched is (batch_domains and offers and same_shape)
    assert src['hm'] is data['input'] and tgt['hm'] is data['target_domain_input']
    if batched:
        assert plugin.backend.calls == [('domains', data['input'], data['target_domain_input'], ('hm', 'wh'))]
    else:                                                    # the reference's sequence: source first
        assert [c[0] for c in plugin.backend.calls] == ['call', 'call']
        assert plugin.backend.calls[0][1] is data['input'] and plugin.backend.calls[1][1] is data['target_domain_input']
