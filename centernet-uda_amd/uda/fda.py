"""Fourier domain adaptation plugin (uda/fda.py): the detection loss on the source batch with the target's
low-frequency amplitude (utils/image.FDA_source_to_target, one batched HIP transform), plus `entropy_weight` x
EntropyLoss(eta) of the target batch.  The weight is applied in place, so the logged `entropy_loss` is the weighted
value (Q4).  The step itself is uda.base.Model.step_with_target_term on a shallow copy of the batch whose `input` is
the mixed batch: the caller's `data["input"]` is not replaced, and with `batch_domains` (default) the mixed and the
target batch go through the backend as one pass; `batch_domains = False` is the reference's literal two forward /
two backward calls."""
from losses.entropy import EntropyLoss
from uda.base import Model
from utils.image import FDA_source_to_target


class FDA(Model):
    def __init__(self, entropy_weight, beta, eta=1.5, use_circular=False):
        super().__init__()
        self.entropy_loss = EntropyLoss(eta=eta)
        self.entropy_weight = entropy_weight
        self.beta = beta
        self.eta = eta
        self.use_circular = use_circular

    def _target_term(self, target_outputs, data):
        loss, stats = self.entropy_loss(target_outputs, data)
        loss *= self.entropy_weight           # in place: `stats` holds the same tensor
        return loss, stats

    def step(self, data, is_training=True):
        self._to_device(data)
        mixed = FDA_source_to_target(data["input"], data["target_domain_input"], self.beta, self.use_circular)
        return self.step_with_target_term(dict(data, input=mixed), is_training, self._target_term)
