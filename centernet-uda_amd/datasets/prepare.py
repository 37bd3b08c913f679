"""Input normalisation on the GPU.

`prepare_input(images, mean, std)` restates the two places where the reference's dataset turns the resized uint8
image into a network input (datasets/coco.py:160-162 and, for `target_domain_input`, 105-109):

    inp = ((img.astype(np.float32) / 255.) - mean) / std        # mean, std: float32 [1, 1, 3]
    inp = inp.transpose(2, 0, 1)

for a whole batch in one kernel (`cnuda_prepare_input`), so that the image crosses to the device as bytes, a quarter
of the fp32 tensor.  `images` is [B, H, W, 3] uint8 on the GPU; the result is [B, 3, H, W] float32 and bit-identical
to the numpy expression: every step is one float32 operation in the same order, with IEEE division.  Resizing and
augmentation come before it (datasets/augment.py); decoding stays on the host.
"""
import numpy as np
import torch

from hip_runtime import check, lib, ptr, require_gpu, stream

MEAN = (0.40789654, 0.44719302, 0.47026115)         # datasets/coco.py:27-28
STD = (0.28863828, 0.27408164, 0.27809835)


def _three(v, what):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size != 3:
        raise RuntimeError("prepare_input: %s must have three values, got %d" % (what, a.size))
    return [float(x) for x in a]                      # float32 values: the c_float conversion is exact


def prepare_input(images, mean=MEAN, std=STD, out=None):
    """`out`: a contiguous float32 [B, 3, H, W] tensor to fill instead of a new one (predict.py: the first half of the
    batch whose second half holds the mirrors)."""
    require_gpu(images)
    if images.dtype != torch.uint8:
        raise RuntimeError("prepare_input: images must be uint8, got %s" % images.dtype)
    if images.dim() != 4 or images.shape[3] != 3 or images.numel() == 0:
        raise RuntimeError("prepare_input: images must be a non-empty [B, H, W, 3], got %s" % (tuple(images.shape),))
    images = images.contiguous()
    if images.data_ptr() % 4:
        images = images.clone()                       # a byte-offset view: the kernel loads dwords
    B, H, W, _ = images.shape
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=images.device)
    elif tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != images.device:
        raise RuntimeError("prepare_input: out must be a contiguous float32 %s on %s, got %s %s"
                           % ((B, 3, H, W), images.device, out.dtype, tuple(out.shape)))
    check(lib().cnuda_prepare_input(ptr(images), ptr(out), B, H, W, *_three(mean, 'mean'), *_three(std, 'std'),
                                    stream()), 'prepare_input')
    return out
