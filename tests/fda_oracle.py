"""float64 CPU restatement of FDA_source_to_target (utils/image.py:137-230) and of EntropyLoss(eta)
(losses/entropy.py:17-22), for the FDA tests.

The transfer follows the reference step by step: full fft2 of source and target, amplitude and phase, the target's
amplitude on the masked bins, recomposition amp * (cos pha, sin pha), and the reference's
torch.irfft(Z, 2, onesided=False, signal_sizes=(H, W)), which (torch 1.x) narrowed the last dimension to W//2+1
columns and ran a complex-to-real transform: today's torch.fft.irfft2(Z[..., :W//2+1], s=(H, W))."""
import math

import torch


def fda_transfer(src, trg, use_target_amp):
    """src, trg [B,C,H,W]; use_target_amp bool [H, W] (full spectrum) -> float64 [B,C,H,W]"""
    src, trg = src.double(), trg.double()
    H, W = src.shape[-2:]
    S, T = torch.fft.fft2(src), torch.fft.fft2(trg)
    amp_s, pha_s, amp_t = S.abs(), torch.atan2(S.imag, S.real), T.abs()
    m = torch.as_tensor(use_target_amp, dtype=torch.bool)
    amp = torch.where(m, amp_t, amp_s)
    Z = torch.complex(amp * torch.cos(pha_s), amp * torch.sin(pha_s))
    return torch.fft.irfft2(Z[..., :W // 2 + 1], s=(H, W))


def half_spectrum_inverse_direct(Z, H, W):
    """out(y,x) = 1/(HW) sum_{ky<H} sum_{kx<=W/2} c_kx Re(Z(ky,kx) e^{2 pi i (ky y/H + kx x/W)}),
    c = 1 for kx = 0 and (W even) kx = W/2, else 2.  Z: complex128 [..., H, W//2+1]."""
    ky = torch.arange(H, dtype=torch.float64)
    kx = torch.arange(W // 2 + 1, dtype=torch.float64)
    y = torch.arange(H, dtype=torch.float64)
    x = torch.arange(W, dtype=torch.float64)
    c = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64)
    c[0] = 1.0
    if W % 2 == 0:
        c[W // 2] = 1.0
    ey = torch.exp(2j * math.pi * torch.outer(y, ky) / H)            # [y, ky]
    ex = torch.exp(2j * math.pi * torch.outer(kx, x) / W) * c[:, None]   # [kx, x]
    return (ey @ Z.to(torch.complex128) @ ex).real / (H * W)


def entropy_eta_loss(hm, eta):
    """(loss, d loss / d hm) in float64, by autograd"""
    x = hm.detach().double().requires_grad_(True)
    v = torch.softmax(x, dim=1)
    C = x.shape[1]
    e = -(v * torch.log2(v + 1e-30)).sum(dim=1) / math.log2(C)
    loss = ((e ** 2 + 1e-30) ** eta).mean()
    loss.backward()
    return loss.detach(), x.grad
