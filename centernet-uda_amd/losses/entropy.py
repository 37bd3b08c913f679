"""EntropyLoss plugin (losses/entropy.py:6-28): normalised softmax entropy of the
target-domain heat-map logits, one fused HIP reduction (forward) and one
elementwise kernel (backward).  With `eta` (the FDA plugin's form, :17-22): the
mean over pixels of (e^2 + 1e-30)^eta, e the per-pixel normalised entropy."""
import torch

from hip_runtime import ops


class EntropyLoss(torch.nn.Module):
    def __init__(self, eta=None):
        super().__init__()
        self.eta = eta

    def forward(self, outputs, batch):
        if self.eta is None:
            loss = ops.entropy_loss(outputs['hm'])
        else:
            loss = ops.entropy_eta_loss(outputs['hm'], self.eta)
        return loss, {'entropy_loss': loss}
