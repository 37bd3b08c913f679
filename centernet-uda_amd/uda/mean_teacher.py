"""Mean-teacher self-training ("Mean teacher"): a detection loss on TARGET images, against pseudo-labels from an
exponential-moving-average copy of the network.  No counterpart in the reference, whose UDA methods only regularise the
target-domain heat map.

A training step, with `n` EMA updates done so far:

  1. n < burn_in_steps: `Model.step` on the source batch; no teacher forward, no `pseudo_*` statistics.
  2. otherwise the teacher (eval mode, no tape) sees `target_domain_input`: sigmoid_clamp_ on `hm`, decode_detection
     (K = cfg.max_detections), hip_runtime.ops.pseudo_labels (per-class score thresholds, minimum extent, the mirror),
     datasets.targets.encode_targets -- a batch like the loader's, built on the device, nothing read back;
  3. the student's step is `step_with_target_term` over source | `student_view(target)` (the mirrored target with
     `mirror_student`; WeakStrongTeacher: the strong view of it), target term
     `pseudo_weight * centernet_loss(target outputs, pseudo batch)`; its statistics are logged under the loss's own names prefixed `pseudo_` (unweighted) plus `pseudo_boxes`, the mean number of pseudo-labels per image;
  4. right behind optimizer.step(): decay_t = min(decay, (1 + n) / (10 + n)), one cnuda_ema_update launch over the
     teacher's flat parameter buffer and every buffer, n += 1 -- during burn-in too.

DenseTeacher replaces 2 and the target term of 3: the teacher's heads stay dense (no decode, no pseudo-labels, no target
encoding), hip_runtime.ops.dense_select picks the top `ratio` of every image's positions and ops.dense_teacher_loss
regresses the student's `hm` and `wh` onto the teacher's there ("Dense teacher").

KeypointTeacher extends 2 for a model with a keypoint head: the decoded joints travel with their boxes through
pseudo_labels, the geometric view and encode_targets, and the detection loss adds its keypoint term on the target half
("Keypoint teacher").

The teacher is a copy of the unwrapped backend made in `to()`.  It is not a submodule of the backend (the backend's
state_dict, the optimizer and a data-parallel wrapper never see it); its trainable parameters are views of one flat
float32 buffer laid out like the student's arena, so that they are ONE segment of the update against
`arena.flat_param`; frozen parameters stay as copied."""
import copy

import torch

import hip_runtime as hr
from uda.base import Model
from utils import helper


def decay_at(decay, n):
    """The EMA decay of update number n (0-based): the warm-up (1 + n) / (10 + n) until it reaches `decay`."""
    return min(float(decay), (1.0 + n) / (10.0 + n))


class MeanTeacher(Model):
    target_grad_heads = ('hm', 'wh', 'reg')

    def __init__(self, pseudo_weight, decay=0.999, score_threshold=0.4, burn_in_steps=0, mirror_student=True,
                 min_size=2.0, evaluate_teacher=False):
        super().__init__()
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("MeanTeacher: decay=%r outside [0, 1)" % (decay,))
        if not float(pseudo_weight) >= 0.0:
            raise ValueError("MeanTeacher: pseudo_weight=%r is negative" % (pseudo_weight,))
        if int(burn_in_steps) < 0:
            raise ValueError("MeanTeacher: burn_in_steps=%r is negative" % (burn_in_steps,))
        self.pseudo_weight, self.decay = float(pseudo_weight), float(decay)
        self.score_threshold = (float(score_threshold) if isinstance(score_threshold, (int, float))
                                else [float(v) for v in score_threshold])
        self.burn_in_steps, self.mirror_student = int(burn_in_steps), bool(mirror_student)
        self.min_size, self.evaluate_teacher = float(min_size), bool(evaluate_teacher)
        self.teacher = None
        self.teacher_flat = None            # the teacher's trainable parameters, laid out like the student's arena
        self.teacher_updates = 0            # n
        self._pairs = None                  # (teacher trainable parameters, student's), in the student's order
        self._plan, self._plan_anchor = None, None
        self._thresholds = None
        self._pending = None                # a checkpoint's teacher entries, loaded before the teacher existed

    # -- set-up ------------------------------------------------------------------------
    def _model_params(self):
        return self.cfg.model.backend.params

    def _threshold_list(self):
        C = int(self._model_params().num_classes)
        if isinstance(self.score_threshold, list):
            if len(self.score_threshold) != C:
                raise ValueError("MeanTeacher: score_threshold lists %d values for num_classes=%d"
                                 % (len(self.score_threshold), C))
            return list(self.score_threshold)
        return [self.score_threshold] * C

    def init_done(self):
        if int(self._model_params().get('num_keypoints', 0) or 0) > 0:
            raise ValueError("MeanTeacher: num_keypoints=%r: keypoint pseudo-labels are not built; train a model "
                             "without the keypoint head" % (self._model_params().num_keypoints,))
        self._threshold_list()

    def _build_teacher(self):
        """A copy of the (unwrapped, already moved) backend whose storage is built here: the student's parameters may be
        views of an arena, and copy.deepcopy of a view clones the whole underlying buffer once per parameter."""
        from hip_runtime.arena import ParamArena
        student = helper._unwrap(self.backend)
        trainable = [p for p in student.parameters() if p.requires_grad]
        offsets, numel = ParamArena.layout(trainable)
        dev = trainable[0].device if trainable else next(student.parameters()).device
        self.teacher_flat = torch.zeros(numel, dtype=torch.float32, device=dev)
        memo, mine = {}, []
        with torch.no_grad():
            for p, o in zip(trainable, offsets):
                view = self.teacher_flat[o:o + p.numel()].view(p.shape)
                view.copy_(p)
                mine.append(torch.nn.Parameter(view, requires_grad=False))
                memo[id(p)] = mine[-1]
            for p in student.parameters():
                if id(p) not in memo:
                    memo[id(p)] = torch.nn.Parameter(p.detach().clone(), requires_grad=False)
            for b in student.buffers():
                memo[id(b)] = b.detach().clone()
        self.teacher = copy.deepcopy(student, memo).eval()
        assert all(not p.requires_grad for p in self.teacher.parameters())
        self._pairs = (mine, trainable)
        self._plan = None

    def to(self, device, parallel=False, global_normalizers=True):
        self.backend.to(device)
        self._build_teacher()
        self._thresholds = torch.tensor(self._threshold_list(), dtype=torch.float32, device=device)
        if self._pending is not None:
            self._apply_checkpoint(*self._pending)
            self._pending = None
        super().to(device, parallel, global_normalizers)

    # -- the EMA -----------------------------------------------------------------------
    def _student_flat(self, trainable):
        """The student's arena buffer, if the teacher's flat buffer is laid out like it (the optimizer's arena over
        the trainable parameters in module order); None: a stock optimizer, or groups in another order."""
        from hip_runtime.arena import _BY_PTR
        hit = _BY_PTR.get(trainable[0].data_ptr())
        arena = hit[0]() if hit is not None else None
        if arena is None or arena.numel != self.teacher_flat.numel() or len(arena.params) != len(trainable) \
                or any(a is not b for a, b in zip(arena.params, trainable)) or not arena.valid():
            return None
        return arena.flat_param

    def _ema_plan(self):
        mine, theirs = self._pairs
        anchor = theirs[0].data_ptr() if theirs else 0
        if self._plan is None or anchor != self._plan_anchor:
            from hip_runtime.ops import EmaPlan
            student = helper._unwrap(self.backend)
            flat = self._student_flat(theirs) if theirs else None
            if flat is not None:
                dst, src = [self.teacher_flat], [flat]
            else:                                       # the same launch, one segment per parameter
                dst, src = [p.data for p in mine], [p.data for p in theirs]
            dst += list(self.teacher.buffers())
            src += list(student.buffers())
            self._plan, self._plan_anchor = EmaPlan(dst, src), anchor
        return self._plan

    def _optimizer_step(self):
        # the optimizer's bump and the teacher's share ONE parameter epoch: the packed weights of both models are
        # carried by one refresh launch (two bumps in a row would strand both)
        with hr.single_param_epoch():
            self.optimizer.step()
            self._ema_plan().update(decay_at(self.decay, self.teacher_updates))
            hr.bump_param_epoch(self.teacher_flat)
        hr.bump_buffer_epoch()          # the teacher's running statistics moved: BatchNorm-folded copies are stale
        self.teacher_updates += 1

    # -- the step ----------------------------------------------------------------------
    def pseudo_batch(self, target_input):
        """The teacher's detections on `target_input` as a batch for the detection loss (+ 'kept')."""
        from datasets.targets import encode_targets
        from hip_runtime import ops
        rotated = bool(self._model_params().rotated_boxes)
        with torch.no_grad():
            heads = self.teacher(target_input)
            hm = ops.sigmoid_clamp_(heads['hm'])
            dets, joints = self.decode_teacher(hm, heads, rotated)
            H, W = hm.shape[2:]
            labels = ops.pseudo_labels(dets, self._thresholds, W, rotated=rotated, mirror=self.mirror_student,
                                       min_size=self.min_size, **joints)
            labels = self.view_labels(labels, target_input, H, W, rotated)
            batch = encode_targets(labels.get('boxes'), labels['classes'], labels['counts'], hm.shape[1], H, W,
                                   corners=labels.get('corners'), keypoints=labels.get('keypoints'),
                                   visibility=labels.get('visibility'))
        batch['kept'] = labels['kept']
        for name in ('dropped', 'joints'):
            if name in labels:
                batch[name] = labels[name]
        return batch

    def decode_teacher(self, hm, heads, rotated):
        """-> (the teacher's decoded detection table, further keyword arguments of `ops.pseudo_labels`: none here;
        KeypointTeacher: the decoded joints)."""
        from backends.decode import decode_detection
        return decode_detection(hm, heads['wh'], heads['reg'], K=self.cfg.max_detections, rotated=rotated), {}

    def view_labels(self, labels, target_input, map_h, map_w, rotated):
        """The teacher's pseudo-labels as the student's view shows them: here the labels themselves (`pseudo_labels`
        has mirrored them with `mirror_student`); GeometricTeacher: transformed and filtered."""
        return labels

    def student_view(self, target_input):
        """What the student sees of the target batch the teacher labelled: the mirror with `mirror_student` (the
        pseudo-labels are mirrored with it), else the batch itself.  Never writes `target_input`."""
        if self.mirror_student:
            from predict import mirror_input
            return mirror_input(target_input)
        return target_input

    def step(self, data, is_training=True):
        if not is_training:
            if not self.evaluate_teacher:
                return Model.step(self, data, False)
            student, self.backend = self.backend, self.teacher
            try:
                return Model.step(self, data, False)
            finally:
                self.backend = student
        if self.teacher_updates < self.burn_in_steps:
            return Model.step(self, data, True)
        self._to_device(data)
        pseudo = self.pseudo_batch(data['target_domain_input'])
        view = dict(data)                   # the caller's batch keeps its tensors
        view['target_domain_input'] = self.student_view(data['target_domain_input'])

        def target_term(target_outputs, _):
            # (a shallow copy: the loss rebinds `hm` to probabilities, the returned outputs keep the logits)
            loss, stats = self.centernet_loss(dict(target_outputs), pseudo)
            stats = {'pseudo_' + k: v for k, v in stats.items()}
            stats['pseudo_boxes'] = pseudo['kept']
            if 'dropped' in pseudo:
                stats['pseudo_dropped'] = pseudo['dropped']
            if 'joints' in pseudo:
                stats['pseudo_joints'] = pseudo['joints']
            return loss * self.pseudo_weight, stats
        return self.step_with_target_term(view, True, target_term)

    # -- checkpoints -------------------------------------------------------------------
    def _apply_checkpoint(self, state_dict, updates):
        with torch.no_grad():
            if state_dict is not None:
                self.teacher.load_state_dict(state_dict)
            else:                           # a checkpoint without a teacher: the freshly loaded student
                student = helper._unwrap(self.backend)
                for mine, theirs in ((self.teacher.parameters(), student.parameters()),
                                     (self.teacher.buffers(), student.buffers())):
                    for t, s in zip(mine, theirs):
                        t.copy_(s)
        if updates is not None:
            self.teacher_updates = int(updates)

    def load_model(self, path, resume=False):
        extra = {}
        epoch = helper.load_model(self.backend, self.optimizer, self.scheduler, path, resume, extra=extra)
        if extra.get('found'):
            found = (extra.get('teacher_state_dict'), extra.get('teacher_updates') if resume else None)
            if self.teacher is None:
                self._pending = found
            else:
                self._apply_checkpoint(*found)
        return epoch

    def save_model(self, path, epoch, with_optimizer=False):
        extra = {'teacher_state_dict': self.teacher.state_dict(), 'teacher_updates': self.teacher_updates}
        helper.save_model(self.backend, path, epoch, self.optimizer if with_optimizer else None,
                          self.scheduler if with_optimizer else None, extra=extra)


class WeakStrongTeacher(MeanTeacher):
    """MeanTeacher whose student trains on a STRONG view of the target batch ("Strong view"): the teacher labels
    `target_domain_input` as it is; the student sees its mirror (with `mirror_student`) through colour jitter, grayscale,
    gaussian blur and random erasing (datasets/strong_view.py, csrc/strongview.hip) -- photometric or occluding, so the
    teacher's boxes stay valid.  `strong_view`: the sampler's mapping (None: its defaults); the other arguments are
    MeanTeacher's.  Step n (= teacher_updates, which the checkpoint carries) draws from
    np.random.default_rng([cfg.seed, 0x57534B, n]) with fill counters n B .. n B + B - 1: a resumed run continues the
    same stream.  Burn-in, evaluation, checkpoints and statistics are the parent's."""

    def __init__(self, pseudo_weight, strong_view=None, **mean_teacher_arguments):
        super().__init__(pseudo_weight, **mean_teacher_arguments)
        from datasets.strong_view import StrongView
        self.strong_view = StrongView(strong_view)

    def student_view(self, target_input):
        return self.strengthen(super().student_view(target_input))

    def strengthen(self, x):
        """The strong view of `x` under the parameters of step n = teacher_updates; never writes `x`."""
        import numpy as np
        from datasets.strong_view import strong_view
        B, _, H, W = x.shape
        n = self.teacher_updates
        params = self.strong_view.sample(B, H, W, np.random.default_rng([int(self.cfg.seed), 0x57534B, n]),
                                         first_id=n * B)
        return strong_view(x, params, self.cfg.normalize.mean, self.cfg.normalize.std)


class GeometricTeacher(WeakStrongTeacher):
    """WeakStrongTeacher whose student also sees another GEOMETRY than the teacher labelled ("Geometric
    view"): per image a rotation, an isotropic change of scale and a shift about the image centre, drawn by
    datasets.geometric_view.GeometricView (`geometric_view`: its mapping; None: its defaults).  The teacher labels
    `target_domain_input` as it is.  The student sees ONE bilinear warp of it by the inverse of A . F (A: the image's
    similarity, F: the mirror with `mirror_student`, else the identity -- the mirror costs no launch of its own), then the
    parent's strong view.  The pseudo-labels go the parent's way up to `ops.pseudo_labels(mirror=...)`, then through
    `ops.transform_labels` with A at output-map resolution: a rotated-box model's corners are mapped point by point (any
    angle, no loss), an axis-aligned model gets the bounding box of the mapped corners; a label survives when at least
    `min_visible` of it lies inside the view and both extents reach `min_size`.  Statistics: the parent's, with
    `pseudo_boxes` counted after the filter, plus `pseudo_dropped` (labels removed per image).

    Step n (= teacher_updates) draws from np.random.default_rng([cfg.seed, 0x47454F, n]), a stream of its own: the strong
    view's draws at step n are WeakStrongTeacher's, and a resumed run continues both.  With every component null (or
    `p: 0`) the step is WeakStrongTeacher's bit for bit.  Burn-in, the EMA, checkpoints, evaluation and the keypoint
    refusal are the parent's."""

    def __init__(self, pseudo_weight, geometric_view=None, min_visible=0.5, strong_view=None, **mean_teacher_arguments):
        super().__init__(pseudo_weight, strong_view=strong_view, **mean_teacher_arguments)
        from datasets.geometric_view import GeometricView
        if isinstance(min_visible, bool) or not isinstance(min_visible, (int, float)) or not 0.0 < float(min_visible) <= 1.0:
            raise ValueError("GeometricTeacher: min_visible=%r outside (0, 1]" % (min_visible,))
        self.min_visible = float(min_visible)
        self.geometric_view = GeometricView(geometric_view)
        self._drawn = None                  # (key, record): the labels and the view of one step share one draw

    def geometry(self, target_input):
        """The GeometricViewParams of step n = teacher_updates for this batch: a function of (cfg.seed, n, the shape),
        drawn once per step."""
        import numpy as np
        B, _, H, W = target_input.shape
        key = (int(self.cfg.seed), self.teacher_updates, B, H, W)
        if self._drawn is None or self._drawn[0] != key:
            self._drawn = (key, self.geometric_view.sample(B, H, W, np.random.default_rng([key[0], 0x47454F, key[1]])))
        return self._drawn[1]

    def student_view(self, target_input):
        from datasets.geometric_view import warp_batch
        params = self.geometry(target_input)
        inverse = params.mirrored(target_input.shape[3])[1] if self.mirror_student else params.inverse
        return self.strengthen(warp_batch(target_input, inverse))

    def view_labels(self, labels, target_input, map_h, map_w, rotated):
        from hip_runtime import ops
        down_ratio = target_input.shape[3] / float(map_w)
        return ops.transform_labels(labels, self.geometry(target_input).forward_map(down_ratio), map_h, map_w,
                                    rotated=rotated, min_size=self.min_size, min_visible=self.min_visible)


class KeypointTeacher(GeometricTeacher):
    """GeometricTeacher for a model with a keypoint head ("Keypoint teacher"): the teacher's `kps` head is
    decoded with its boxes, and every pseudo-label carries its J joints through the score filter and the mirror
    (`ops.pseudo_labels(kps=...)`; with `mirror_student` the joints of `flip_pairs` -- [[left, right], ...], as
    predict.py --flip-pairs -- change places), through the geometric view (`ops.transform_labels`) and into
    `encode_targets(keypoints=, visibility=)`: the pseudo batch has `kps`, `gt_kps` and `kp_reg_mask`, and the detection
    loss (which must have its keypoint term: `kp_weight`) adds that term on the target half; the student's `kps` head
    records a tape there.  The teacher gives no confidence per joint: a joint is "visible" when it lies inside the
    student's map, and the joints never decide whether a label survives.  Statistics: the parent's, with
    `pseudo_kp_loss` among the `pseudo_` ones, plus `pseudo_joints` (visible joints per image).

    With every `geometric_view` component null the view is WeakStrongTeacher's.  Rotated-box models are allowed.  Burn-in,
    the EMA, checkpoints, evaluation and the two random streams are the parent's."""
    target_grad_heads = ('hm', 'wh', 'reg', 'kps')

    def __init__(self, pseudo_weight, flip_pairs=None, geometric_view=None, min_visible=0.5, strong_view=None,
                 **mean_teacher_arguments):
        super().__init__(pseudo_weight, geometric_view=geometric_view, min_visible=min_visible, strong_view=strong_view,
                         **mean_teacher_arguments)
        self.flip_pairs = None if flip_pairs is None else [tuple(pair) for pair in flip_pairs]
        self._flip_perm = None              # (host int32 [J], its device copy once moved)

    def init_done(self):
        from predict import flip_permutation
        params = self._model_params()
        J = int(params.get('num_keypoints', 0) or 0)
        if J <= 0:
            raise ValueError("KeypointTeacher: model.backend.params.num_keypoints=%r: there is no keypoint head to "
                             "teach; use uda.GeometricTeacher for this model" % (params.get('num_keypoints', 0),))
        try:
            self._flip_perm = (flip_permutation(self.flip_pairs, J), None)
        except ValueError as err:
            raise ValueError("KeypointTeacher: %s (num_keypoints=%d)" % (err, J)) from None
        if not getattr(self.centernet_loss, 'with_keypoints', False):
            raise ValueError("KeypointTeacher: the detection loss has no keypoint term: set "
                             "model.backend.loss.params.kp_weight")
        self._threshold_list()

    def decode_teacher(self, hm, heads, rotated):
        from backends.decode import decode_detection
        dets, kps = decode_detection(hm, heads['wh'], heads['reg'], kps=heads['kps'], K=self.cfg.max_detections,
                                     rotated=rotated)
        joints = {'kps': kps, 'map_height': hm.shape[2]}
        if self.mirror_student:
            host, dev = self._flip_perm
            if dev is None or dev.device != kps.device:
                dev = torch.from_numpy(host).to(kps.device)
                self._flip_perm = (host, dev)
            joints['flip_perm'] = dev
        return dets, joints


class DenseTeacher(WeakStrongTeacher):
    """The mean teacher without pseudo-boxes ("Dense teacher"; Dense Teacher, Zhou et al., ECCV 2022): the
    student regresses the teacher's heat map itself.  Per image the top `ratio` of the positions by the teacher's
    channel-max logit are selected, every tie included (hip_runtime.ops.dense_select); the target term is
    `pseudo_weight * (hm_weight * quality focal loss + wh_weight * score-weighted L1 of wh)` over that selection
    (ops.dense_teacher_loss; `reg` takes no part).  No score threshold, no decode, no target encoding.

    The step after burn-in: teacher forward (eval mode, no tape) on `target_domain_input`, dense_select, `student_view`
    (`strong_view=False`: the plain mirror / identity view; None or a mapping: WeakStrongTeacher's strong view), then
    `step_with_target_term`.  Statistics behind the source loss's: dense_loss, dense_hm_loss, dense_wh_loss,
    dense_positions (selected positions per image), dense_score (their mean teacher score).  With a data-parallel
    backend every rank normalises by its own selection.  The EMA, burn-in, checkpoints and evaluation are the parent's."""
    target_grad_heads = ('hm', 'wh')

    def __init__(self, pseudo_weight, ratio=0.01, hm_weight=1.0, wh_weight=0.1, strong_view=None, decay=0.999,
                 burn_in_steps=0, mirror_student=True, evaluate_teacher=False):
        super().__init__(pseudo_weight, strong_view=None if strong_view is False else strong_view, decay=decay,
                         burn_in_steps=burn_in_steps, mirror_student=mirror_student, evaluate_teacher=evaluate_teacher)
        if strong_view is False:
            self.strong_view = None
        if not 0.0 < float(ratio) <= 1.0:
            raise ValueError("DenseTeacher: ratio=%r outside (0, 1]" % (ratio,))
        for name, v in (('hm_weight', hm_weight), ('wh_weight', wh_weight)):
            if not float(v) >= 0.0:
                raise ValueError("DenseTeacher: %s=%r is negative" % (name, v))
        self.ratio, self.hm_weight, self.wh_weight = float(ratio), float(hm_weight), float(wh_weight)

    def init_done(self):
        params = self._model_params()
        if int(params.get('num_keypoints', 0) or 0) > 0:
            raise ValueError("DenseTeacher: model.backend.params.num_keypoints=%r: the dense loss has no keypoint term; "
                             "train a model without the keypoint head" % (params.num_keypoints,))
        if bool(params.get('rotated_boxes', False)):
            raise ValueError("DenseTeacher: model.backend.params.rotated_boxes is set: wh carries an angle channel "
                             "whose mirror is a sign flip, which the dense loss does not build")

    def student_view(self, target_input):
        if self.strong_view is None:
            return MeanTeacher.student_view(self, target_input)
        return super().student_view(target_input)

    @staticmethod
    def dense_stats(stats5, batch_size):
        """ops.dense_teacher_loss's five results as the step's statistics, in their logged order."""
        return {'dense_loss': stats5[0], 'dense_hm_loss': stats5[1], 'dense_wh_loss': stats5[2],
                'dense_positions': stats5[3] / batch_size, 'dense_score': stats5[4] / stats5[3].clamp(min=1.0)}

    def step(self, data, is_training=True):
        if not is_training or self.teacher_updates < self.burn_in_steps:
            return super().step(data, is_training)
        from hip_runtime import ops
        self._to_device(data)
        target = data['target_domain_input']
        with torch.no_grad():
            heads = self.teacher(target)
        teacher_hm, teacher_wh = heads['hm'], heads['wh']
        tau, count = ops.dense_select(teacher_hm, self.ratio)
        view = dict(data)                   # the caller's batch keeps its tensors
        view['target_domain_input'] = self.student_view(target)

        def target_term(target_outputs, _):
            loss, stats5 = ops.dense_teacher_loss(target_outputs['hm'], target_outputs['wh'], teacher_hm, teacher_wh,
                                                  tau, count, mirror=self.mirror_student, hm_weight=self.hm_weight,
                                                  wh_weight=self.wh_weight)
            return loss * self.pseudo_weight, self.dense_stats(stats5, teacher_hm.shape[0])
        return self.step_with_target_term(view, True, target_term)
