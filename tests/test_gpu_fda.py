"""FDA on the MI355X: the batched HIP amplitude transfer (csrc/fda.hip) against the float64 oracle
(tests/fda_oracle.py), the eta-weighted entropy loss, and one step of the FDA plugin against the reference's literal
sequence."""
import ast
import time

import numpy as np
import pytest
import torch

import fda_oracle
import inputs as gin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(shape, generator=g)
    trg = torch.randn(shape, generator=g)
    return src, trg


CASES = [((2, 3, 64, 64), 0.1, 2e-5), ((2, 3, 96, 160), 0.05, 2e-5), ((1, 3, 512, 512), 0.01, 2e-5),
         ((1, 3, 60, 45), 0.1, 1e-4),          # odd W: 45 = 3^2 5 on Stockham, 60 = 4 3 5
         ((1, 3, 224, 224), 0.1, 1e-4)]        # 224 = 2^5 7: the direct DFT


@pytest.mark.parametrize('circular', [False, True], ids=['square', 'circular'])
@pytest.mark.parametrize('shape,L,tol', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_transfer_matches_the_oracle(shape, L, tol, circular):
    from utils.image import FDA_source_to_target, fda_low_freq_mask
    src, trg = _pair(shape, sum(shape))
    H, W = shape[-2:]
    mask = fda_low_freq_mask(H, W, L, circular)
    want = fda_oracle.fda_transfer(src, trg, mask)
    got = FDA_source_to_target(src.to(DEV), trg.to(DEV), L, circular)
    torch.cuda.synchronize()
    err = (got.cpu().double() - want).abs().max().item()
    moved = (want - src.double()).abs().max().item()
    print('fda %s %s L=%g: max err %.3g (oracle moves src by %.3g)' % ('circ' if circular else 'square', shape, L,
                                                                      err, moved))
    assert got.shape == src.shape and got.dtype == torch.float32
    assert moved >= 100 * tol, moved
    assert err <= tol, err


def test_zero_source_takes_the_target_amplitude_with_zero_phase():
    from utils.image import FDA_source_to_target, fda_low_freq_mask
    _, trg = _pair((2, 3, 32, 48), 3)
    src = torch.zeros_like(trg)
    want = fda_oracle.fda_transfer(src, trg, fda_low_freq_mask(32, 48, 0.2, False))
    assert want.abs().max().item() > 0.1               # (|T|, 0) on the corner bins: not zero
    got = FDA_source_to_target(src.to(DEV), trg.to(DEV), 0.2, False)
    assert (got.cpu().double() - want).abs().max().item() <= 2e-5


def test_square_L0_returns_src_and_two_calls_are_bit_identical():
    from utils.image import FDA_source_to_target
    src, trg = _pair((4, 3, 128, 160), 11)
    s, t = src.to(DEV), trg.to(DEV)
    got = FDA_source_to_target(s, t, 0.0, False)
    assert (got.cpu() - src).abs().max().item() <= 2e-5
    a = FDA_source_to_target(s, t, 0.1, True)
    b = FDA_source_to_target(s, t, 0.1, True)
    assert torch.equal(a, b)


def test_bad_inputs_raise():
    from utils.image import FDA_source_to_target
    src, trg = (t.to(DEV) for t in _pair((1, 3, 16, 16), 1))
    with pytest.raises(RuntimeError, match='differentiable'):
        FDA_source_to_target(src.clone().requires_grad_(True), trg, 0.1)
    with pytest.raises(ValueError, match='one shape'):
        FDA_source_to_target(src, trg[..., :8], 0.1)
    for L in (-0.1, 1.01):
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            FDA_source_to_target(src, trg, L)
    from hip_runtime import ops
    with pytest.raises(RuntimeError, match='4096'):
        big = torch.zeros(1, 1, 2, 8192, device=DEV)
        ops.fda_source_to_target(big, big, torch.zeros(2, 4097, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize('eta', [0.5, 1.0, 1.5])
@pytest.mark.parametrize('C,H,W', [(6, 16, 16), (80, 7, 9), (6, 13, 11)])
def test_entropy_eta_loss_matches_the_float64_oracle(eta, C, H, W):
    from losses.entropy import EntropyLoss
    g = torch.Generator().manual_seed(C * H + W)
    hm = torch.randn(2, C, H, W, generator=g) * 2
    want, want_grad = fda_oracle.entropy_eta_loss(hm, eta)
    x = hm.to(DEV).requires_grad_(True)
    loss, stats = EntropyLoss(eta=eta)({'hm': x}, None)
    assert stats['entropy_loss'] is loss
    loss.backward(torch.tensor(1.7, device=DEV))
    assert abs(loss.item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    gerr = (x.grad.cpu().double() - 1.7 * want_grad).abs().max().item()
    assert gerr <= 1e-4 * max(want_grad.abs().max().item(), 1e-6) * 1.7, gerr


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-30)


def _model(golden):
    from backends import dla
    shapes = dict(ast.literal_eval(str(golden('dla_axis')['shapes_json'])))
    model = dla.build(num_classes=6)
    model.load_state_dict({k: T(v) for k, v in gin.fill_state(shapes, 0.1).items()})
    return model.to(DEV)


def _batch(B, S):
    data = {k: T(v) for k, v in gin.detection_batch(B, 6, S // 4, S // 4, 8, (3, 2), 2, 81).items()}
    data['input'] = T(gin.image_batch(B, S, S, 82))
    data['target_domain_input'] = T(gin.image_batch(B, S, S, 83))
    return data


def test_fda_plugin_step(golden):
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    from losses.entropy import EntropyLoss
    from uda.fda import FDA
    from utils.image import FDA_source_to_target
    t0 = time.time()
    B, S, w, beta, eta = 2, 128, 0.3, 0.05, 1.5
    runs = []
    for batched in (True, False):
        model = _model(golden)
        plugin = FDA(w, beta, eta=eta, use_circular=True)
        plugin.batch_domains = batched
        plugin.backend, plugin.device = model, torch.device(DEV)
        plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
        plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
        plugin.init_done()
        plugin.to(DEV)
        plugin.set_phase(True)
        data = _batch(B, S)
        src0 = data['input'].clone()
        seen = []
        hook = model.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().clone()))
        out = plugin.step(data)
        hook.remove()
        assert torch.equal(data['input'].cpu(), src0)                     # the caller's batch is not replaced
        runs.append((out, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                     {n: p.detach().clone() for n, p in model.named_parameters()}, seen, data))
    (ob, gb, pb, seen_b, data), (os_, gs, ps, seen_s, _) = runs
    mixed = FDA_source_to_target(data['input'], data['target_domain_input'], beta, True)
    # what the backend saw in the reference's sequence: the mixed batch, then the target batch (the batched pass goes
    # through forward_domains and agrees with it below)
    assert torch.equal(seen_s[0], mixed) and torch.equal(seen_s[1], data['target_domain_input'])
    # the reference's stats: detection stats + entropy_loss + total_loss
    assert set(os_['stats']) == {'centernet_loss', 'hm_loss', 'wh_loss', 'off_loss', 'entropy_loss', 'total_loss'}
    assert list(ob['stats']) == list(os_['stats'])
    for k in os_['stats']:
        assert abs(float(ob['stats'][k]) - float(os_['stats'][k])) <= 1e-5 * max(abs(float(os_['stats'][k])), 1e-9), k
    assert sorted(gb) == sorted(gs)
    for n in gs:
        if n.endswith('.conv.bias') and 'ida' in n:
            continue
        assert _rel(gb[n], gs[n]) <= 2e-4, (n, _rel(gb[n], gs[n]))
    # the reference's literal sequence, composed by hand: fda -> backend(mixed) + detection loss,
    # entropy_weight * EntropyLoss(eta)(backend(trg)), two backward passes, one Adam step
    model = _model(golden)
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-5, weight_decay=1e-4)
    model.train(True)
    crit = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    opt.zero_grad()
    c_loss, _ = crit(model(mixed), data)
    e_loss, _ = EntropyLoss(eta)(model(data['target_domain_input']), data)
    e_loss = e_loss * w
    c_loss.backward()
    e_loss.backward()
    hand_grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    opt.step()
    assert abs(float(e_loss.detach()) - float(os_['stats']['entropy_loss'])) <= 1e-6 * abs(float(e_loss.detach()))
    # the DCN's data gradient accumulates with atomics: gradients agree up to summation order, and Adam's first step
    # (lr * g / (|g| + eps)) moves every parameter by ~lr whatever |g| is, so the parameters agree to well under lr
    # wherever the gradient is clear of that noise
    assert sorted(hand_grads) == sorted(gs)
    for n, p in model.named_parameters():
        if n.endswith('.conv.bias') and 'ida' in n:
            continue                                      # analytically zero (bias in front of a BatchNorm): noise
        assert _rel(hand_grads[n], gs[n]) <= 2e-4, (n, _rel(hand_grads[n], gs[n]))
        g = hand_grads[n].abs()
        sure = g > 1e-3 * g.max()                         # a noise-level gradient may flip sign: a +-lr step apart
        if sure.any():
            assert (p.detach() - ps[n])[sure].abs().max().item() <= 5e-6, n
    print('plugin step test: %.1f s' % (time.time() - t0))
