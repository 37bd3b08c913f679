"""The host half of datasets.loader.DeviceLoader (`collate`): padding, sizes and counts, and the random draws, which
must not depend on the number of decoding threads.  No GPU: the device half is tests/test_gpu_device_loader.py."""
import dataclasses

import numpy as np
import pytest
import torch

import coco_fixture as fx
from datasets.coco import Dataset
from datasets.coco_merger import Dataset as Merger
from datasets.loader import DeviceLoader

AUG = [{'Sometimes': {'p': 0.8, 'then_list': [{'AddToBrightness': {'add': [-50, 50]}},
                                               {'Affine': {'scale': [0.8, 1.3], 'translate_percent': [-0.2, 0.2]}},
                                               {'AdditiveGaussianNoise': {'scale': [0, 8]}}]}},
       {'Fliplr': {'p': 0.5}}]
AUG_B = [{'Flipud': {'p': 1.0}}, {'AddToHue': {'value': [10, 20]}}]


def _loader(dataset, num_workers=0, batch_size=2, shuffle=False, seed=42, **kw):
    args = dict(device=None, num_classes=3, num_keypoints=0, rotated_boxes=False, down_ratio=4,
                mean=(0.4, 0.4, 0.4), std=(0.3, 0.3, 0.3), max_detections=4)
    args.update(kw)
    return DeviceLoader(dataset, batch_size, shuffle, num_workers, seed=seed, **args)


def _dataset(tmp_path, count=5, name='train', **kw):
    folder, path = fx.write_dataset(tmp_path, count, name=name, boxes_per_image=kw.pop('boxes_per_image', 2),
                                    rotated=kw.get('rotated_boxes', False), keypoints=kw.get('num_keypoints', 0))
    return Dataset(folder, path, input_size=(32, 32), num_classes=3, max_detections=4, **kw)


def _same_record(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, dict):
            assert sorted(x) == sorted(y), f.name
            assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in x), f.name
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), f.name
        else:
            assert x == y, f.name


def _same_batch(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if x is None or y is None:
            assert x is None and y is None, f.name
        elif isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and np.array_equal(x.numpy(), y.numpy(), equal_nan=True), f.name
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), f.name
        else:
            _same_record(x, y)


def test_padding_sizes_counts_and_the_short_last_batch(tmp_path):
    ds = _dataset(tmp_path, boxes_per_image=5)                            # five boxes, max_detections four
    loader = _loader(ds)
    assert len(loader) == 3 and loader.dataset is ds
    assert [loader.batch_indices(k).tolist() for k in range(3)] == [[0, 1], [2, 3], [4]]
    h = loader.collate(0)
    assert h.images.dtype == torch.uint8 and tuple(h.images.shape) == (2, 40, 32, 3)      # max of 24 x 32 and 40 x 28
    assert h.sizes.tolist() == [[24, 32], [40, 28]] and h.sizes.dtype == np.int32
    img = h.images.numpy()
    assert np.array_equal(img[0, :24, :32], fx.pixels(24, 32, 0)) and not img[0, 24:].any()
    assert np.array_equal(img[1, :40, :28], fx.pixels(40, 28, 1)) and not img[1, :, 28:].any()
    assert h.counts.tolist() == [4, 0] and h.counts.dtype == torch.int32                  # truncated; image 1 has none
    raw = ds[0]
    assert tuple(h.geometry.shape) == (2, 4, 4) and h.geometry.dtype == torch.float64
    assert np.array_equal(h.geometry.numpy()[0], raw['boxes'].astype(np.float64)) and not h.geometry.numpy()[1].any()
    assert h.classes.numpy()[0].tolist() == raw['classes'].tolist() and h.classes.dtype == torch.int32
    assert np.array_equal(h.areas.numpy()[0], raw['areas']) and np.isnan(h.areas.numpy()[1]).all()
    assert h.ids.tolist() == [101, 102] and h.ids.dtype == torch.int64
    assert h.indices.tolist() == [0, 1] == h.params.image_ids.tolist()
    assert h.keypoints is None and h.visibility is None and h.target_images is None and h.target_params is None
    last = loader.collate(2)
    assert tuple(last.images.shape) == (1, 24, 32, 3) and last.ids.tolist() == [105] and last.counts.tolist() == [4]
    assert last.params.batch == 1 and last.indices.tolist() == [4]
    # no augmentation list: the resize-only record
    assert not h.params.color.any() and not h.params.noise.any() and h.params.ntaps.tolist() == [1, 1]
    assert h.params.forward[0].tolist() == [1.0, 0.0, 0.0, 0.0, 32 / 24, 0.0] and h.params.input_size == (32, 32)


def test_keypoints_and_corners_are_padded_too(tmp_path):
    ds = _dataset(tmp_path, rotated_boxes=True, num_keypoints=2)
    h = _loader(ds, rotated_boxes=True, num_keypoints=2).collate(0)
    raw = ds[0]
    assert tuple(h.geometry.shape) == (2, 4, 4, 2) and np.array_equal(h.geometry.numpy()[0, :2], raw['corners'])
    assert not h.geometry.numpy()[0, 2:].any() and h.counts.tolist() == [2, 0]
    assert tuple(h.keypoints.shape) == (2, 4, 2, 2) and np.array_equal(h.keypoints.numpy()[0, :2], raw['keypoints'])
    assert h.visibility.dtype == torch.int32 and h.visibility.numpy()[0, :2].tolist() == [[2, 1], [2, 1]]
    with pytest.raises(ValueError, match="rotated_boxes=False"):
        _loader(ds, rotated_boxes=False, num_keypoints=2).collate(0)


def test_the_draw_does_not_depend_on_the_number_of_threads_and_differs_between_epochs(tmp_path):
    glob = fx.write_target_images(tmp_path, 4)
    ds = _dataset(tmp_path, count=7, augmentation=AUG, target_domain_glob=glob, augment_target_domain=True)
    inline, threaded = _loader(ds, 0, shuffle=True), _loader(ds, 3, shuffle=True)
    for epoch in (1, 2):
        inline.set_epoch(epoch), threaded.set_epoch(epoch)
        for k in range(len(inline)):
            _same_batch(inline.collate(k), threaded.collate(k))
    # ... nor on the order in which the batches are asked for
    _same_batch(inline.collate(2, epoch=1), threaded.collate(2, epoch=1))
    a, b = inline.collate(0, epoch=1), inline.collate(0, epoch=2)
    assert a.params.seed != b.params.seed and not np.array_equal(a.params.forward, b.params.forward)
    assert sorted(sum((inline.batch_indices(k, 1).tolist() for k in range(4)), [])) == list(range(7))     # a permutation
    assert [inline.batch_indices(k, 1).tolist() for k in range(4)] != [inline.batch_indices(k, 2).tolist() for k in range(4)]
    other = _loader(ds, 0, shuffle=True, seed=43)
    assert other.collate(0, epoch=1).params.seed != a.params.seed
    # the target images: drawn, padded and -- under augment_target_domain -- with a record of their own
    assert a.target_images is not None and a.target_sizes.shape == (2, 2) and a.target_params.seed != a.params.seed
    assert a.target_params.batch == 2 and a.target_params.image_ids.tolist() == a.indices.tolist()
    assert 'Fliplr' in a.target_params.applied


def test_target_images_are_only_resized_without_augment_target_domain(tmp_path):
    glob = fx.write_target_images(tmp_path, 4)
    ds = _dataset(tmp_path, augmentation=AUG, target_domain_glob=glob)
    h = _loader(ds).collate(0, epoch=3)
    t = h.target_params
    assert t is not None and not t.applied and not t.draws and not t.color.any() and not t.noise.any()
    for b in range(2):
        th, tw = h.target_sizes[b]
        assert t.forward[b].tolist() == [32 / tw, 0.0, 0.0, 0.0, 32 / th, 0.0]
    assert h.params.applied                                             # the source images did draw


def test_merged_members_draw_from_their_own_lists(tmp_path):
    fa = fx.write_dataset(tmp_path, 3, name='a')
    fb = fx.write_dataset(tmp_path, 3, name='b', first_seed=50)
    fc = fx.write_dataset(tmp_path, 2, name='c', first_seed=70)
    members = [{'name': 'coco', 'params': {'image_folder': fa[0], 'annotation_file': fa[1], 'augmentation': AUG}},
               {'name': 'coco', 'params': {'image_folder': fb[0], 'annotation_file': fb[1], 'augmentation': AUG_B}},
               {'name': 'coco', 'params': {'image_folder': fc[0], 'annotation_file': fc[1]}}]
    merged = Merger(members, num_classes=3, max_detections=4, input_size=(32, 32))
    h = _loader(merged, batch_size=8).collate(0, epoch=1)               # one batch over all three members
    p = h.params
    assert p.batch == 8 and h.indices.tolist() == list(range(8))
    assert p.applied['Flipud'].tolist() == [False] * 3 + [True] * 3 + [False] * 2      # member b alone flips, always
    assert np.isnan(p.draws['AddToHue.value'][[0, 1, 2, 6, 7]]).all()
    assert ((p.draws['AddToHue.value'][3:6] >= 10) & (p.draws['AddToHue.value'][3:6] <= 20)).all()
    assert p.color[3:6, 1].all() and not p.color[[0, 1, 2, 6, 7], 1].any()
    assert not p.applied['Sometimes'][3:].any() and not p.applied['Fliplr'][3:].any()  # member a's list stays with a
    # member c has no list: resize only
    for b in (6, 7):
        hh, ww = h.sizes[b]
        assert p.forward[b].tolist() == [32 / ww, 0.0, 0.0, 0.0, 32 / hh, 0.0] and p.ntaps[b] == 1
    # Flipud composed with the resize: v -> 32 - v * 32 / h
    hh = h.sizes[3, 0]
    assert p.forward[3].tolist() == [32 / h.sizes[3, 1], 0.0, 0.0, 0.0, -32 / hh, 32.0]
    # a member with another input size cannot share a loader
    members[1]['params']['input_size'] = [64, 64]
    with pytest.raises(ValueError, match="different input sizes"):
        _loader(Merger(members, num_classes=3, max_detections=4, input_size=(32, 32)))


def test_iteration_needs_the_device(tmp_path):
    with pytest.raises(RuntimeError, match="collate"):
        iter(_loader(_dataset(tmp_path))).__next__()
