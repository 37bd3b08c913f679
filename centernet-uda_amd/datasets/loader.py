"""`DeviceLoader`: from a dataset of raw samples (datasets.coco / datasets.coco_merger) to the batch dict the step
consumes, every key on the device -- the place of `torch.utils.data.DataLoader` in the reference's driver
(train.py:30-63), with the work split differently:

host    decode (PIL) and pad into pinned buffers: threads of a `ThreadPoolExecutor(min(num_workers, 16))`, inline
        with num_workers = 0.  No worker PROCESSES: forking a process that has initialised HIP is fragile, and every
        worker would hold the GPU open.  PIL's decoders and numpy's copies release the interpreter lock.
        The random draws (target file, AugmentParams) are made by the consuming thread from
        `np.random.default_rng([seed, epoch, batch_index])`: a run is reproducible whatever num_workers is.
device  uploads and `datasets.build_batch` (augment, resize, normalise, encode), issued by the consuming thread on ONE
        side stream.  Batch k+1 is queued there before batch k is handed out; the consumer's stream waits on batch
        k's event.  The tensors handed out were allocated on the side stream, so each is marked as used by the
        consumer's stream (`record_stream`): the caching allocator will not recycle it under a kernel that may still
        read it.  The pinned staging buffers come from torch's host allocator, which holds a block back until the
        non-blocking copy that read it has completed.  `hip_runtime.workspace` is keyed by stream: the side stream has
        its own scratch.

The host half alone is `collate(batch_index)` (no GPU needed); `to_device(host_batch)` is the device half.
"""
import dataclasses
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .augment import AugmentParams, build_batch

MAX_THREADS = 16


def _members(dataset):
    return list(dataset.members) if hasattr(dataset, 'members') else [dataset]


def _locate(dataset, index):
    return dataset.locate(index) if hasattr(dataset, 'locate') else (dataset, index)


def merge_params(records, positions, B, seed, image_ids):
    """Per-member AugmentParams records, each for the batch positions `positions[i]`, -> one record of B images with
    the noise key `seed` and the noise counters `image_ids`."""
    first = records[0]
    out = {f: np.zeros((B,) + getattr(first, f).shape[1:], dtype=getattr(first, f).dtype)
           for f in ('sizes', 'color', 'taps', 'ntaps', 'forward', 'inverse', 'noise')}
    draws, applied = {}, {}
    for rec, pos in zip(records, positions):
        for f in out:
            out[f][pos] = getattr(rec, f)
        for k, v in rec.draws.items():
            draws.setdefault(k, np.full((B,) + v.shape[1:], np.nan))[pos] = v
        for k, v in rec.applied.items():
            applied.setdefault(k, np.zeros(B, dtype=bool))[pos] = v
    return AugmentParams(input_size=first.input_size, seed=int(seed), image_ids=np.asarray(image_ids, dtype=np.int64),
                         draws=draws, applied=applied, **out)


@dataclasses.dataclass
class HostBatch:
    """What `collate` leaves for the device half: CPU tensors (pinned when a GPU is present) and the two records."""
    images: torch.Tensor                    # [B, Hmax, Wmax, 3] uint8, image b in its top-left sizes[b] corner
    sizes: np.ndarray                       # [B, 2] int32 (h, w)
    geometry: torch.Tensor                  # boxes [B, M, 4] or corners [B, M, 4, 2], float64, zero padded
    classes: torch.Tensor                   # [B, M] int32
    counts: torch.Tensor                    # [B] int32
    areas: torch.Tensor                     # [B, M] float32, NaN where the annotation has none (and in the padding)
    ids: torch.Tensor                       # [B] int64, the samples' `id`
    indices: np.ndarray                     # [B] int64 dataset indices (= params.image_ids)
    params: AugmentParams
    keypoints: torch.Tensor = None          # [B, M, J, 2] float64
    visibility: torch.Tensor = None         # [B, M, J] int32
    target_images: torch.Tensor = None      # [B, Ht, Wt, 3] uint8
    target_sizes: np.ndarray = None
    target_params: AugmentParams = None


class DeviceLoader:
    def __init__(self, dataset, batch_size, shuffle, num_workers, device, seed, num_classes, num_keypoints,
                 rotated_boxes, down_ratio, mean, std, max_detections, keypoint_visibility=False):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("DeviceLoader: batch_size must be positive, got %r" % (batch_size,))
        self.shuffle = bool(shuffle)
        self.num_workers = max(0, int(num_workers))
        self.device = None if device is None else torch.device(device)
        self.seed = int(seed)
        self.num_classes, self.num_keypoints = int(num_classes), int(num_keypoints)
        self.rotated_boxes = bool(rotated_boxes)
        self.down_ratio = int(down_ratio)
        self.mean, self.std = tuple(mean), tuple(std)
        self.max_detections = int(max_detections)
        self.keypoint_visibility = bool(keypoint_visibility) and self.num_keypoints > 0
        self.epoch = 0
        sizes = sorted({tuple(m.input_size) for m in _members(dataset)})
        if len(sizes) != 1:
            raise ValueError("DeviceLoader: the member datasets have different input sizes %s; images of different "
                             "input sizes cannot share a batch -- give the members one input_size or load them "
                             "separately" % (sizes,))
        self.input_size = sizes[0]
        self._pin = self.device is not None and self.device.type == 'cuda' and torch.cuda.is_available()
        self._pool = ThreadPoolExecutor(min(self.num_workers, MAX_THREADS)) if self.num_workers > 0 else None
        self._side = None

    def __len__(self):
        return math.ceil(len(self.dataset) / self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    # -- host half ------------------------------------------------------------------------------------------------------
    def batch_indices(self, batch_index, epoch=None):
        epoch = self.epoch if epoch is None else int(epoch)
        n = len(self.dataset)
        order = np.random.default_rng([self.seed, epoch]).permutation(n) if self.shuffle else np.arange(n)
        return order[batch_index * self.batch_size:(batch_index + 1) * self.batch_size].astype(np.int64)

    def _map(self, fn, items):
        if self._pool is None:
            return [fn(*it) for it in items]
        return [f.result() for f in [self._pool.submit(fn, *it) for it in items]]

    def _start(self, batch_index, epoch):
        """Draw the target files and send the decoding off.  -> the state `_finish` completes."""
        indices = self.batch_indices(batch_index, epoch)
        rng = np.random.default_rng([self.seed, epoch, batch_index])
        choices = rng.random(len(indices))
        items = [(int(i), float(u)) for i, u in zip(indices, choices)]
        if self._pool is None:
            samples = None                                  # decoded in _finish: nothing runs ahead without threads
        else:
            samples = [self._pool.submit(self.dataset.get, *it) for it in items]
        return indices, rng, items, samples

    def _empty(self, shape, dtype, fill=0):
        t = torch.empty(shape, dtype=dtype, pin_memory=self._pin)
        t.fill_(fill)
        return t

    def _finish(self, state):
        indices, rng, items, samples = state
        if samples is None:
            samples = [self.dataset.get(*it) for it in items]
        else:
            samples = [f.result() for f in samples]
        B, M, J = len(samples), self.max_detections, self.num_keypoints
        sizes = np.array([s['image'].shape[:2] for s in samples], dtype=np.int32)
        images = self._empty((B, int(sizes[:, 0].max()), int(sizes[:, 1].max()), 3), torch.uint8)
        key = 'corners' if self.rotated_boxes else 'boxes'
        geometry = self._empty((B, M, 4, 2) if self.rotated_boxes else (B, M, 4), torch.float64)
        classes = self._empty((B, M), torch.int32)
        areas = self._empty((B, M), torch.float32, float('nan'))
        keypoints = self._empty((B, M, J, 2), torch.float64) if J else None
        visibility = self._empty((B, M, J), torch.int32) if J else None
        counts = np.zeros(B, dtype=np.int32)
        has_target = ['target_image' in s for s in samples]
        if any(has_target) and not all(has_target):
            raise ValueError("DeviceLoader: batch %s mixes samples with and without a target-domain image" % (indices,))
        target_images = target_sizes = None
        if all(has_target):
            target_sizes = np.array([s['target_image'].shape[:2] for s in samples], dtype=np.int32)
            target_images = self._empty((B, int(target_sizes[:, 0].max()), int(target_sizes[:, 1].max()), 3),
                                        torch.uint8)

        def pad(b, s):
            h, w = sizes[b]
            images.numpy()[b, :h, :w] = s['image']
            if target_images is not None:
                th, tw = target_sizes[b]
                target_images.numpy()[b, :th, :tw] = s['target_image']
            if key not in s:
                raise ValueError("DeviceLoader: rotated_boxes=%s but sample %d has no %r" % (self.rotated_boxes,
                                                                                               indices[b], key))
            m = min(len(s[key]), M)
            counts[b] = m
            geometry.numpy()[b, :m] = s[key][:m]
            classes.numpy()[b, :m] = s['classes'][:m]
            areas.numpy()[b, :m] = s['areas'][:m]
            if J:
                keypoints.numpy()[b, :m] = s['keypoints'][:m]
                visibility.numpy()[b, :m] = s['visibility'][:m]

        self._map(pad, list(enumerate(samples)))

        # the draws: one noise key per record, then member by member in the dataset's order
        seeds = rng.integers(0, 2 ** 64, size=2, dtype=np.uint64)
        owner = [_locate(self.dataset, int(i))[0] for i in indices]
        records, target_records, positions = [], [], []
        for member in _members(self.dataset):
            pos = np.array([b for b in range(B) if owner[b] is member], dtype=np.int64)
            if not len(pos):
                continue
            positions.append(pos)
            aug = getattr(member, 'augmenter', None)
            records.append(aug.sample(sizes[pos], self.input_size, rng) if aug is not None
                           else AugmentParams.identity(sizes[pos], self.input_size))
            if target_images is not None:
                aug_t = aug if getattr(member, 'augment_target_domain', False) else None
                target_records.append(aug_t.sample(target_sizes[pos], self.input_size, rng) if aug_t is not None
                                      else AugmentParams.identity(target_sizes[pos], self.input_size))
        params = merge_params(records, positions, B, seeds[0], indices)
        target_params = merge_params(target_records, positions, B, seeds[1], indices) if target_records else None
        ids = self._empty((B,), torch.int64)
        ids.numpy()[:] = [int(s['id']) for s in samples]
        counts_t = self._empty((B,), torch.int32)
        counts_t.numpy()[:] = counts
        return HostBatch(images=images, sizes=sizes, geometry=geometry, classes=classes, counts=counts_t, areas=areas,
                         ids=ids, indices=indices, params=params, keypoints=keypoints, visibility=visibility,
                         target_images=target_images, target_sizes=target_sizes, target_params=target_params)

    def collate(self, batch_index, epoch=None):
        """The host half for one batch of the current (or given) epoch."""
        epoch = self.epoch if epoch is None else int(epoch)
        return self._finish(self._start(batch_index, epoch))

    # -- device half ----------------------------------------------------------------------------------------------------
    def to_device(self, host):
        """Uploads and build_batch on the CURRENT stream -> the batch dict (the reference's keys plus `id`)."""
        up = lambda t: None if t is None else t.to(self.device, non_blocking=True)
        geometry, visibility = up(host.geometry), up(host.visibility)
        batch = build_batch(
            up(host.images), None if self.rotated_boxes else geometry, up(host.classes), up(host.counts),
            params=host.params, input_size=self.input_size, num_classes=self.num_classes, down_ratio=self.down_ratio,
            sizes=host.sizes, corners=geometry if self.rotated_boxes else None, keypoints=up(host.keypoints),
            visibility=visibility, areas=up(host.areas), mean=self.mean, std=self.std,
            target_images=up(host.target_images), target_sizes=host.target_sizes, target_params=host.target_params)
        batch['id'] = up(host.ids)
        if self.keypoint_visibility:
            batch['gt_kps_visibility'] = visibility          # [B, M, J] int32, COCO's v: evaluation/coco_keypoints.py
        return batch

    def _issue(self, host):
        with torch.cuda.stream(self._side):
            batch = self.to_device(host)
            ready = torch.cuda.Event()
            ready.record(self._side)
        return batch, ready

    def __iter__(self):
        if self.device is None or self.device.type != 'cuda':
            raise RuntimeError("DeviceLoader: iteration builds the batch on the MI355X; device=%r (the host half alone "
                               "is collate())" % (self.device,))
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        epoch, n = self.epoch, len(self)
        # decoding runs this many batches ahead of the one being handed out: the one queued on the device, and enough
        # more to keep every thread busy
        ahead = 2 + math.ceil(min(self.num_workers, MAX_THREADS) / self.batch_size)
        started = {}

        def host_batch(k):
            for j in range(k, min(k + ahead, n)):
                if j not in started:
                    started[j] = self._start(j, epoch)
            return self._finish(started.pop(k))

        queued = self._issue(host_batch(0)) if n else None
        for k in range(n):
            batch, ready = queued
            queued = self._issue(host_batch(k + 1)) if k + 1 < n else None
            consumer = torch.cuda.current_stream(self.device)
            consumer.wait_event(ready)
            for t in batch.values():
                t.record_stream(consumer)
            yield batch
