"""MaxSquareLoss plugin (losses/max_square.py:6-14): -mean(softmax(hm)^2) / 2, and its image-wise class-balanced
form (Chen, Xue, Cai, "Domain Adaptation for Semantic Segmentation with Maximum Squares Loss", ICCV 2019)."""
import torch

from hip_runtime import ops


class MaxSquareLoss(torch.nn.Module):
    def forward(self, outputs, batch):
        loss = ops.max_square_loss(outputs['hm'])
        return loss, {'max_square_loss': loss}


class IWMaxSquareLoss(torch.nn.Module):
    """-sum(softmax(hm)^2 * w[argmax]) / (2 * batch * classes): every pixel weighs 1 / max(n^ratio * HW^(1 - ratio), 1),
    n the pixels of its image whose argmax (on the logits, lowest channel on a tie) is the pixel's own.  The published
    form is divided by 2 here, as MaxSquareLoss divides its own: ratio = 0 is MaxSquareLoss.  ratio = 0.2 is the
    paper's value."""

    def __init__(self, ratio=0.2):
        super().__init__()
        if not 0.0 <= float(ratio) <= 1.0:
            raise ValueError("IWMaxSquareLoss: ratio must be in [0, 1], got %r" % (ratio,))
        self.ratio = float(ratio)

    def forward(self, outputs, batch):
        loss = ops.iw_max_square_loss(outputs['hm'], self.ratio)
        return loss, {'iw_max_square_loss': loss}


class GuidanceLoss(torch.nn.Module):
    """The same paper's multi-level self-produced guidance: the low-level heat map `hm_low` learns the labels that it
    and the final `hm` agree on.  With p, q the class softmaxes of `hm` and `hm_low` and e = (p + q) / 2, a pixel whose
    max_c e exceeds `threshold` is guided towards a = argmax_c e (the lowest channel on a tie); the loss is the mean over
    the guided pixels of -log q_a, an exact 0 when there is none.  Labels and mask are constants: `hm` gets no gradient."""

    def __init__(self, threshold=0.95):
        super().__init__()
        if not 0.0 <= float(threshold) < 1.0:
            raise ValueError("GuidanceLoss: threshold must be in [0, 1), got %r" % (threshold,))
        self.threshold = float(threshold)

    def terms(self, outputs):
        """-> (loss, number of guided pixels in the batch), both device scalars"""
        return ops.guidance_loss(outputs['hm_low'], outputs['hm'], self.threshold, return_count=True)

    def forward(self, outputs, batch):
        loss, _ = self.terms(outputs)
        return loss, {'guidance_loss': loss}
