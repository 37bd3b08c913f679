"""MI355X parity of the EfficientNet backend against the CPU oracle (tests/efficientnet_oracle.py): b0 with skip
connections and a keypoint head, B = 2 at 64 x 64 (all map sizes even: static and input-derived SAME padding agree).
The bounds are those of tests/test_gpu_mobilenetv2.py: as close to the fp64 result as the oracle's own fp32 run is, within
8x (16x for the scalar and the gradient checksums), never tighter than 1e-4; running statistics at 1e-4."""
import numpy as np
import pytest
import torch

import efficientnet_oracle as eo
import inputs as gin
from test_gpu_resnet import GRAD_FLOOR, _checksums, _close, _close_calibrated

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
HEADS = {'hm': 6, 'wh': 2, 'reg': 2, 'kps': 8}


def _cos_like(t):
    return torch.cos(torch.arange(t.numel(), dtype=torch.float32).reshape(t.shape) * 0.1)


@pytest.fixture(scope='module')
def case():
    """state, input and the oracle's results in fp32 and fp64, computed once"""
    state = gin.fill_state(dict(eo.state_shapes('b0', HEADS, True)))
    x = T(gin.image_batch(2, 64, 64, 83))
    ref = {}
    for name, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        sd = eo.make_state(state, dtype)
        net = eo.Net(sd, 'b0', HEADS, True)
        with torch.no_grad():
            ev = net.forward(x.to(dtype))
        net.training = True
        out = net.forward(x.to(dtype))
        scalar = sum((out[k] * _cos_like(out[k]).to(dtype)).sum() for k in out)
        scalar.backward()
        ref[name] = dict(eval={k: v.numpy() for k, v in ev.items()}, train={k: v.detach().numpy() for k, v in out.items()},
                         scalar=scalar.item(),
                         grads={k: _checksums(v.grad) for k, v in sd.items() if v.requires_grad and v.grad is not None},
                         buffers={k: v.detach().numpy() for k, v in sd.items() if not v.requires_grad})
    return state, x, ref


def _model(state, rate):
    from backends import efficientnet
    model = efficientnet.build(6, 'b0', num_keypoints=4, pretrained=False, use_skip=True)
    model.load_state_dict({k: T(v) for k, v in state.items()})
    model.base.drop_connect_rate = rate
    return model.to(DEV)


def test_efficientnet_b0_forward_backward_matches_oracle(case):
    state, x, ref = case
    r32, r64 = ref['f32'], ref['f64']
    model = _model(state, 0.0)
    model.eval()
    with torch.no_grad():
        out = model(x.to(DEV))
    assert list(out) == ['hm', 'wh', 'reg', 'kps']
    for k in out:
        noise = np.abs(r32['eval'][k] - r64['eval'][k]).max()
        print('eval %s: |gpu - f64| %.3e, oracle |f32 - f64| %.3e' % (k, np.abs(out[k].cpu().numpy() - r64['eval'][k]).max(), noise))
        _close_calibrated(out[k].cpu().numpy(), r32['eval'][k], r64['eval'][k], what='eval ' + k)
    model.train()
    out = model(x.to(DEV))
    for k in out:
        noise = np.abs(r32['train'][k] - r64['train'][k]).max()
        print('train %s: |gpu - f64| %.3e, oracle |f32 - f64| %.3e' % (
            k, np.abs(out[k].detach().cpu().numpy() - r64['train'][k]).max(), noise))
        _close_calibrated(out[k].detach().cpu().numpy(), r32['train'][k], r64['train'][k], what=k)
    scalar = sum((out[k] * _cos_like(out[k]).to(DEV)).sum() for k in out)
    scalar.backward()
    print('scalar: gpu %.6f f32 %.6f f64 %.6f' % (scalar.item(), r32['scalar'], r64['scalar']))
    _close_calibrated(scalar.item(), r32['scalar'], r64['scalar'], floor=2e-4, k=16.0, what='scalar')
    params = dict(model.named_parameters())
    assert sorted(r64['grads']) == sorted(n for n, p in params.items() if p.grad is not None)
    assert sorted(n for n, p in params.items() if p.grad is None) == ['base._fc.bias', 'base._fc.weight']
    worst = 0.0
    for n, w64 in r64['grads'].items():
        got, noise = _checksums(params[n].grad), np.abs(r32['grads'][n] - w64).max()
        bound = max(GRAD_FLOOR * max(1.0, w64[1]), 16 * noise)
        worst = max(worst, np.abs(got - w64).max() / bound)
        assert np.abs(got - w64).max() <= bound, (n, got, w64, noise)
    print('gradient checksums: worst error / bound %.3f' % worst)
    sd = model.state_dict()
    for n, want in r64['buffers'].items():
        if n.endswith('num_batches_tracked'):
            assert int(sd[n]) == int(want) == 1, n
        else:
            _close(sd[n].cpu().numpy(), want, 1e-4)


def _drop_connect_step(state, x):
    model = _model(state, 0.2)
    model.train()
    torch.manual_seed(1234)
    out = model(x.to(DEV))
    sum((out[k] * _cos_like(out[k]).to(DEV)).sum() for k in out).backward()
    torch.cuda.synchronize()
    return model, out


def test_drop_connect_step_is_finite_and_reproducible(case):
    state, x, ref = case
    (m1, o1), (m2, o2) = _drop_connect_step(state, x), _drop_connect_step(state, x)
    for k in o1:
        assert torch.isfinite(o1[k]).all() and torch.equal(o1[k], o2[k]), k
    # the masks did something: the training outputs differ from the run without drop-connect
    assert np.abs(o1['hm'].detach().cpu().numpy() - ref['f64']['train']['hm']).max() > 1e-3
    for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and torch.equal(p.grad, q.grad), n
    for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), n
    # eval mode ignores the rate
    m0 = _model(state, 0.0)
    m0.eval(), m1.eval()
    m1.load_state_dict(m0.state_dict())
    with torch.no_grad():
        a, b = m0(x.to(DEV)), m1(x.to(DEV))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_model_step_with_keypoint_loss(case):
    """uda.base.Model.step with this backend and DetectionLoss carrying the keypoint term (the keypoints.yaml pairing)"""
    from uda.base import Model
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    state = case[0]
    model = _model(state, 0.2)
    _, batch, weights = gin.kps_inputs('pairs_l1')                  # B = 2, 6 classes, 16 x 16 maps, 4 keypoints
    plugin = Model()
    plugin.backend = model
    plugin.device = torch.device(DEV)
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5)
    plugin.centernet_loss = DetectionLoss(**weights)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    data = {k: T(v) for k, v in batch.items()}
    data['input'] = T(gin.image_batch(2, 64, 64, 84))
    torch.manual_seed(5)
    before = model.base._blocks[3]._se_reduce.weight.detach().clone()
    out = plugin.step(data)
    src = out['source_domain']
    assert {k: tuple(v.shape) for k, v in src.items()} == {'hm': (2, 6, 16, 16), 'wh': (2, 2, 16, 16), 'reg': (2, 2, 16, 16),
                                                           'kps': (2, 8, 16, 16)}
    stats = out['stats']
    assert 'kp_loss' in stats, sorted(stats)
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    assert not torch.equal(before, model.base._blocks[3]._se_reduce.weight.detach())      # the optimizer moved the trunk


def test_b3_builds_and_runs():
    from backends import efficientnet
    model = efficientnet.build(6, 'b3', pretrained=False, use_skip=True).to(DEV)
    model.eval()
    with torch.no_grad():
        out = model(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV))
    assert {k: tuple(v.shape) for k, v in out.items()} == {'hm': (1, 6, 16, 16), 'wh': (1, 2, 16, 16), 'reg': (1, 2, 16, 16)}
    assert all(torch.isfinite(v).all() for v in out.values())
