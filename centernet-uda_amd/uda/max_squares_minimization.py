"""Max-squares UDA plugin (uda/max_squares_minimization.py:6-50): detection loss on the source batch plus
`max_squares_weight` x MaxSquareLoss of the target batch (weight applied in place, Q4).  The step itself is
uda.base.Model.step_with_target_term."""
import logging

import torch

from backends.common import make_head
from hip_runtime import ops
from hip_runtime import optim as hoptim
from losses.max_square import GuidanceLoss, IWMaxSquareLoss, MaxSquareLoss
from uda.base import Model
from utils import helper

log = logging.getLogger(__name__)


class MaxSquaresMinimization(Model):
    def __init__(self, max_squares_weight):
        super().__init__()
        self.max_squares_weight = max_squares_weight
        self.max_squares_loss = MaxSquareLoss()

    def _target_term(self, target_outputs, data):
        loss, stats = self.max_squares_loss(target_outputs, data)
        loss *= self.max_squares_weight       # in place: `stats` holds the same tensor
        return loss, stats

    def criterion(self, outputs, batch):
        """(source loss, weighted target loss, merged stats): the reference's method of this name (:11-20)"""
        det_loss, stats = self.centernet_loss(outputs["source_domain"], batch)
        uda_loss, uda_stats = self._target_term(outputs["target_domain"], batch)
        return det_loss, uda_loss, dict(stats, **uda_stats)

    def step(self, data, is_training=True):
        return self.step_with_target_term(data, is_training, self._target_term)


class IWMaxSquaresMinimization(MaxSquaresMinimization):
    """The same step with the paper's image-wise class-balanced weighting factor (losses.max_square.IWMaxSquareLoss):
    the statistic is `iw_max_square_loss`, weighted like its parent's."""

    def __init__(self, max_squares_weight, ratio=0.2):
        super().__init__(max_squares_weight)
        self.max_squares_loss = IWMaxSquareLoss(ratio)


class MultiLevelMaxSquaresMinimization(MaxSquaresMinimization):
    """Max-squares with the paper's multi-level self-produced guidance.  A second heat-map head,
    `hm_low`, reads the backend's low-level tap (DLASeg.features_with_low_level); it is the plugin's own module
    with its own optimizer, as ADVENT's discriminator is, and the backend's state_dict does not know it.

        total = detection loss (source)
              + aux_weight * focal(clamp(sigmoid(hm_low source)), batch['hm'])
              + max_squares_weight * MaxSquareLoss(hm target)
              + max_squares_weight * aux_weight * GuidanceLoss(threshold)(hm_low target | hm target)

    every weight applied in place on the logged tensor (Q4).  Statistics beside the parent's: aux_hm_loss, guidance_loss,
    guidance_pixels (guided pixels per image of this rank's batch, a device scalar).  With a data-parallel backend the
    guidance term divides by this rank's own number of guided pixels."""

    def __init__(self, max_squares_weight, aux_weight=0.1, threshold=0.95, optimizer=None):
        super().__init__(max_squares_weight)
        if not float(aux_weight) >= 0.0:
            raise ValueError("MultiLevelMaxSquaresMinimization: aux_weight must be >= 0, got %r" % (aux_weight,))
        self.aux_weight = float(aux_weight)
        self.guidance_loss = GuidanceLoss(threshold)        # (refuses a threshold outside [0, 1))
        self.optimizer_settings = optimizer
        self.low_level_head = None
        self.low_level_optimizer = None
        self.low_level_scheduler = None

    def init_done(self):
        backend = helper._unwrap(self.backend)
        channels = getattr(backend, 'low_level_channels', None)
        if channels is None:
            named = getattr(self.cfg.model.backend, 'name', None) if self.cfg is not None else None
            raise ValueError("MultiLevelMaxSquaresMinimization: backend %r (%s) has no low-level tap "
                             "(forward_low_level(x, head)); only the dla backend offers one"
                             % (named, type(backend).__name__))
        params = self.cfg.model.backend.params
        head_conv = params.get('head_conv', 256) if hasattr(params, 'get') else getattr(params, 'head_conv', 256)
        self.low_level_head = make_head(channels, head_conv, params.num_classes, 1)      # dla.build: final_kernel = 1
        with torch.no_grad():
            self.low_level_head[2].bias.fill_(-2.19)                                      # like `hm` (dla.py:485)
        opt = self.optimizer_settings
        if opt is None:
            self.low_level_optimizer = hoptim.Adam(self.low_level_head.parameters())
            return
        self.low_level_optimizer = hoptim.resolve(opt.name)(self.low_level_head.parameters(), **dict(opt.params))
        sched = opt.get('scheduler') if hasattr(opt, 'get') else getattr(opt, 'scheduler', None)
        if sched is not None:
            cls = getattr(torch.optim.lr_scheduler, sched.name)
            self.low_level_scheduler = cls(optimizer=self.low_level_optimizer, **dict(sched.params))

    def set_phase(self, is_training=True):
        super().set_phase(is_training)
        self.low_level_head.train(is_training)

    def to(self, device, parallel=False, global_normalizers=True):
        super().to(device, parallel, global_normalizers)
        self.low_level_head.to(device)
        if parallel:
            from hip_runtime.parallel import DataParallel
            self.low_level_head = DataParallel(self.low_level_head)

    def epoch_end(self):
        super().epoch_end()
        if self.low_level_scheduler is not None:
            self.low_level_scheduler.step()

    def forward_both(self, data):
        """uda.base.Model.forward_both with `hm_low` in both dictionaries."""
        source, target = data["input"], data["target_domain_input"]
        head = self.low_level_head
        if self.batch_domains and hasattr(self.backend, 'forward_domains') and source.shape == target.shape:
            return (*self.backend.forward_domains(source, target, target_grad_heads=self.target_grad_heads,
                                                  low_level_head=head), True)
        return self.backend.forward_low_level(source, head), self.backend.forward_low_level(target, head), False

    def step(self, data, is_training=True):
        self._to_device(data)
        head = self.low_level_head
        if is_training:
            self.optimizer.zero_grad()
            self.low_level_optimizer.zero_grad()
        src, tgt, batched = self.forward_both(data)
        outputs = {"source_domain": src, "target_domain": tgt}
        det_loss, stats = self.centernet_loss(src, data)
        aux_loss, _ = ops.focal_loss(src['hm_low'], data['hm'])       # sigmoid + clamp + focal, the detection loss's path
        aux_loss *= self.aux_weight
        ms_loss, ms_stats = self._target_term(tgt, data)
        guide_loss, guided = self.guidance_loss.terms(tgt)
        guide_loss *= self.max_squares_weight * self.aux_weight
        if is_training:
            if batched:
                (det_loss + aux_loss + ms_loss + guide_loss).backward()
            else:
                with self._defer_sync(), self._defer_sync(head):
                    (det_loss + aux_loss).backward()
                (ms_loss + guide_loss).backward()
            self._finish_backward(self.backend, head)
            self._optimizer_step()
            self.low_level_optimizer.step()
        stats = dict(stats, **ms_stats)
        stats["aux_hm_loss"] = aux_loss
        stats["guidance_loss"] = guide_loss
        stats["guidance_pixels"] = guided / float(tgt['hm'].shape[0])
        stats["total_loss"] = det_loss + aux_loss + ms_loss + guide_loss
        outputs["stats"] = self._detach_stats(stats)
        return outputs

    # -- checkpoints: the backend's entries as they are, the head (and its optimizer) beside them in the same file --------
    def save_model(self, path, epoch, with_optimizer=False):
        extra = {'low_level_head_state_dict': helper._unwrap(self.low_level_head).state_dict()}
        if with_optimizer:
            extra['low_level_head_optimizer'] = self.low_level_optimizer.state_dict()
            if self.low_level_scheduler is not None:
                extra['low_level_head_scheduler'] = self.low_level_scheduler.state_dict()
        helper.save_model(self.backend, path, epoch, self.optimizer if with_optimizer else None,
                          self.scheduler if with_optimizer else None, extra=extra)

    def load_model(self, path, resume=False):
        extra = {}
        epoch = helper.load_model(self.backend, self.optimizer, self.scheduler, path, resume, extra=extra)
        state = extra.get('low_level_head_state_dict')
        if state is not None:
            helper._unwrap(self.low_level_head).load_state_dict(state)
            if resume and 'low_level_head_optimizer' in extra:
                self.low_level_optimizer.load_state_dict(extra['low_level_head_optimizer'])
                if self.low_level_scheduler is not None and 'low_level_head_scheduler' in extra:
                    self.low_level_scheduler.load_state_dict(extra['low_level_head_scheduler'])
        elif extra.get('found'):
            log.warning("%s holds no low-level head: it keeps its initialisation", path)
        return epoch
