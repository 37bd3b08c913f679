"""No-GPU checks of the FDA pieces: the oracle's half-spectrum inverse, the host-side masks (square corners; the
quarter ellipse of the circular mode) and the public signatures."""
import inspect

import numpy as np
import pytest
import torch

import fda_oracle


@pytest.mark.parametrize('H,W', [(12, 10), (9, 7), (8, 15), (6, 6)])
def test_oracle_inverse_is_the_c_weighted_half_spectrum_sum(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    Z = torch.complex(torch.randn(2, H, W // 2 + 1, generator=g, dtype=torch.float64),
                      torch.randn(2, H, W // 2 + 1, generator=g, dtype=torch.float64))   # not Hermitian
    got = torch.fft.irfft2(Z, s=(H, W))
    want = fda_oracle.half_spectrum_inverse_direct(Z, H, W)
    assert (got - want).abs().max().item() < 1e-12
    # ... which is not Re(ifft2) of the same bins: the narrowing matters
    full = torch.zeros(2, H, W, dtype=torch.complex128)
    full[..., :W // 2 + 1] = Z
    assert (torch.fft.ifft2(full).real - got).abs().max().item() > 1e-3


@pytest.mark.parametrize('H,W,L', [(64, 64, 0.1), (96, 160, 0.05), (10, 10, 0.0), (10, 10, 0.04), (8, 6, 0.5),
                                   (12, 7, 0.45), (33, 20, 0.2), (16, 16, 1.0)])
def test_square_mask_is_the_reference_slices(H, W, L):
    from utils.image import fda_low_freq_mask
    b = int(np.floor(np.amin((H, W)) * L))
    want = np.zeros((H, W), dtype=bool)
    want[0:b, 0:b] = True
    want[0:b, W - b:W] = True
    want[H - b:H, 0:b] = True
    want[H - b:H, W - b:W] = True
    if b == 0:                          # [h-0:h] is the empty slice, but [0:0] too: nothing moves
        want[:] = False
    got = fda_low_freq_mask(H, W, L, False)
    assert got.dtype == bool and got.shape == (H, W)
    assert np.array_equal(got, want)


def _pixels(img):
    return sorted((int(y), int(x)) for y, x in zip(*np.nonzero(img)))


def test_circular_mask_small_cases():
    from utils.image import filled_ellipse_at_origin, fda_low_freq_mask
    assert _pixels(filled_ellipse_at_origin(8, 8, (1, 1))) == [(0, 0), (0, 1), (1, 0)]
    assert _pixels(filled_ellipse_at_origin(8, 8, (2, 2))) == [(y, x) for y in range(3) for x in range(3) if x + y <= 2]
    assert _pixels(filled_ellipse_at_origin(8, 8, (0, 0))) == [(0, 0)]
    # cv2's first axis runs along x (columns): swapping the axes transposes the region
    a, b = filled_ellipse_at_origin(9, 9, (4, 1)), filled_ellipse_at_origin(9, 9, (1, 4))
    assert np.array_equal(a, b.T)
    assert a[0, 4] and not a[4, 0] and a[:, 0].sum() == 2
    # the mode's mask: axes (int(H L), int(W L)) -> x semi-axis int(H L); target amplitude OUTSIDE the ellipse
    m = fda_low_freq_mask(20, 10, 0.1, True)                 # axes (2, 1): x semi-axis 2, y semi-axis 1
    inside = ~m
    assert inside[0, 2] and not inside[2, 0] and inside.sum() < 10
    assert m[5, 5] and m[19, 0] and not m[0, 0]


def test_circular_mask_grows_with_the_axes_and_covers_a_quarter_disc():
    from utils.image import filled_ellipse_at_origin
    prev = 0
    for r in range(1, 30):
        e = filled_ellipse_at_origin(64, 64, (r, r))
        assert e[0, r] and e[r, 0] and not e[0, r + 2] and not e[r + 2, 0], r
        n = int(e.sum())
        assert n > prev and abs(n - np.pi * r * r / 4) < 3.5 * r + 3, (r, n)
        prev = n


def test_circular_mask_matches_cv2_when_available():
    cv2 = pytest.importorskip('cv2')
    from utils.image import filled_ellipse_at_origin
    for h, w, axes in [(512, 512, (5, 5)), (96, 160, (4, 8)), (64, 64, (6, 6)), (640, 640, (64, 64)), (30, 40, (2, 1))]:
        want = cv2.ellipse(np.zeros((h, w, 3), np.uint8), (0, 0), axes, 0, 0, 360, (255, 255, 255), -1)[..., 0] > 0
        assert np.array_equal(filled_ellipse_at_origin(h, w, axes), want), (h, w, axes)


def test_signatures_match_the_reference():
    from uda.fda import FDA
    from utils.image import FDA_source_to_target
    from uda.base import Model
    assert list(inspect.signature(FDA.__init__).parameters)[1:] == ['entropy_weight', 'beta', 'eta', 'use_circular']
    assert list(inspect.signature(FDA_source_to_target).parameters) == ['src_img', 'trg_img', 'L', 'use_circular']
    assert issubclass(FDA, Model)
    p = FDA(1e-3, 0.01)
    assert p.eta == 1.5 and p.use_circular is False and p.entropy_loss.eta == 1.5


def test_entropy_loss_takes_eta():
    from losses.entropy import EntropyLoss
    assert EntropyLoss(eta=1.5).eta == 1.5
    assert EntropyLoss().eta is None


def test_fda_refuses_cpu_tensors_and_bad_arguments_before_any_launch():
    from utils.image import FDA_source_to_target
    z = torch.zeros
    with pytest.raises(RuntimeError, match='MI355X only'):
        FDA_source_to_target(z(1, 3, 8, 8), z(1, 3, 8, 8), 0.1)
    with pytest.raises(ValueError, match='one shape'):
        FDA_source_to_target(z(1, 3, 8, 8), z(1, 3, 8, 6), 0.1)
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        FDA_source_to_target(z(1, 3, 8, 8), z(1, 3, 8, 8), 1.5)
    with pytest.raises(RuntimeError, match='differentiable'):
        FDA_source_to_target(z(1, 3, 8, 8).requires_grad_(True), z(1, 3, 8, 8), 0.1)


def test_fda_abi_entries():
    import hip_runtime as hr
    L = hr.lib()
    assert L.cnuda_fda_workspace_bytes(16, 3, 512, 512) == 2 * 16 * 3 * 512 * 257 * 8
    assert L.cnuda_fda_workspace_bytes(0, 3, 512, 512) == 0
    assert L.cnuda_fda_source_to_target(None, None, None, None, 1, 3, 8, 8, None, 0, None) == -1
    ws = hr.ctypes.c_void_p(1)
    src = hr.ctypes.c_void_p(1)
    assert L.cnuda_fda_source_to_target(src, src, src, src, 1, 1, 8, 8192, ws, 1 << 30, None) == -1
    assert b'4096' in L.cnuda_last_error()
    assert L.cnuda_entropy_eta_loss_forward(None, None, 1, 6, 16, 1.5, None, 0, None) == -1
