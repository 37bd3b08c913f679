"""MI355X: datasets.prepare_input against the numpy expression of datasets/coco.py:160-162, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN, STD = (0.3172, 0.52061, 0.4409), (0.2113, 0.30127, 0.1907)      # custom, not the defaults


def _numpy(images, mean, std):
    mean = np.array(mean, dtype=np.float32).reshape(1, 1, 3)
    std = np.array(std, dtype=np.float32).reshape(1, 1, 3)
    out = []
    for img in images:
        x = img.astype(np.float32) / 255.
        x = (x - mean) / std
        assert x.dtype == np.float32
        out.append(x.transpose(2, 0, 1))
    return np.stack(out)


def _images(B, H, W, seed):
    n = B * H * W * 3
    flat = np.arange(n, dtype=np.int64) % 256                           # every byte value, as far as the size allows
    return np.random.RandomState(seed).permutation(flat).astype(np.uint8).reshape(B, H, W, 3)


# (2, 3, 8): H*W a multiple of four -> float4 stores; (2, 5, 6): H*W = 30 -> scalar stores and a group of four pixels that
# straddles the two images; (3, 3, 3): 27 pixels, six groups and a tail of three; (1, 1, 1): the tail alone;
# (1, 4, 4100): 4100 groups, more than one workgroup
@pytest.mark.parametrize('shape', [(2, 3, 8), (2, 5, 6), (3, 3, 3), (1, 1, 1), (1, 4, 4100)])
def test_prepare_input_is_bit_identical_to_numpy(shape):
    from datasets import prepare_input
    B, H, W = shape
    img = _images(B, H, W, seed=H * W)
    if img.size >= 256:
        assert len(np.unique(img)) == 256
    got = prepare_input(torch.from_numpy(img).to(DEV), MEAN, STD)
    assert got.shape == (B, 3, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), _numpy(img, MEAN, STD))


def test_all_byte_values_with_the_default_statistics():
    from datasets import prepare_input
    from datasets.prepare import MEAN as M0, STD as S0
    img = np.stack([np.arange(256, dtype=np.uint8)] * 3, 1).reshape(1, 16, 16, 3)
    got = prepare_input(torch.from_numpy(img).to(DEV))
    np.testing.assert_array_equal(got.cpu().numpy(), _numpy(img, M0, S0))


def test_other_layouts_are_handled_or_refused():
    from datasets import prepare_input
    img = _images(2, 6, 8, seed=1)
    t = torch.from_numpy(img).to(DEV)
    # non-contiguous view (every second column) and a view that starts at an odd byte: both are copied first
    np.testing.assert_array_equal(prepare_input(t[:, :, ::2], MEAN, STD).cpu().numpy(), _numpy(img[:, :, ::2], MEAN, STD))
    flat = torch.zeros(t.numel() + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = t.reshape(-1)
    odd = flat[1:].view(2, 6, 8, 3)
    assert odd.data_ptr() % 4
    np.testing.assert_array_equal(prepare_input(odd, MEAN, STD).cpu().numpy(), _numpy(img, MEAN, STD))
    with pytest.raises(RuntimeError, match='uint8'):
        prepare_input(t.float(), MEAN, STD)
    with pytest.raises(RuntimeError, match=r'\[B, H, W, 3\]'):
        prepare_input(t.permute(0, 3, 1, 2).contiguous(), MEAN, STD)
    with pytest.raises(RuntimeError, match='three values'):
        prepare_input(t, (0.5, 0.5), STD)
    with pytest.raises(RuntimeError, match='MI355X only'):
        prepare_input(torch.from_numpy(img), MEAN, STD)
