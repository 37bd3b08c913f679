"""datasets.loader.DeviceLoader on the GPU: five images of two sizes (24 x 32 and 40 x 28), input size 32 x 32, batch
size 2, shuffle off.  Every key of every batch must equal, bit for bit, `datasets.build_batch` called directly (on the
default stream) on the same samples with the same AugmentParams; batches that are held while later ones are produced
on the side stream must not change."""
import numpy as np
import pytest
import torch

import coco_fixture as fx
from datasets import build_batch
from datasets.coco import Dataset
from datasets.loader import DeviceLoader

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MEAN, STD = (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835)
AUG = [{'Sometimes': {'p': 0.9, 'then_list': [{'AddToBrightness': {'add': [-40, 40]}},
                                               {'Affine': {'scale': [0.8, 1.3], 'translate_percent': [-0.1, 0.1]}},
                                               {'AdditiveGaussianNoise': {'scale': [1, 6]}}]}},
       {'Fliplr': {'p': 0.5}}]
PLAIN_KEYS = ['gt_areas', 'gt_dets', 'hm', 'id', 'ind', 'input', 'reg', 'reg_mask', 'wh']


def _dataset(root, rotated=False, keypoints=0, **kw):
    folder, path = fx.write_dataset(root, 5, rotated=rotated, keypoints=keypoints)
    return Dataset(folder, path, input_size=(32, 32), num_classes=3, max_detections=6, rotated_boxes=rotated,
                   num_keypoints=keypoints, **kw)


def _loader(dataset, num_workers=0, rotated=False, keypoints=0):
    return DeviceLoader(dataset, batch_size=2, shuffle=False, num_workers=num_workers, device=DEV, seed=11,
                        num_classes=3, num_keypoints=keypoints, rotated_boxes=rotated, down_ratio=4, mean=MEAN,
                        std=STD, max_detections=6)


def _direct(loader, k):
    """build_batch on the default stream from the loader's own host batch, spelled out call by call"""
    h = loader.collate(k)
    geometry = h.geometry.to(DEV)
    up = lambda t: None if t is None else t.to(DEV)
    out = build_batch(h.images.to(DEV), None if loader.rotated_boxes else geometry, h.classes.to(DEV),
                      h.counts.to(DEV), params=h.params, input_size=(32, 32), num_classes=3, down_ratio=4,
                      sizes=h.sizes, corners=geometry if loader.rotated_boxes else None, keypoints=up(h.keypoints),
                      visibility=up(h.visibility), areas=h.areas.to(DEV), mean=MEAN, std=STD,
                      target_images=up(h.target_images), target_sizes=h.target_sizes, target_params=h.target_params)
    out['id'] = h.ids.to(DEV)
    return out


def _assert_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        assert got[key].device == DEV and got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key].view(torch.uint8) if got[key].dtype.is_floating_point else got[key],
                           want[key].view(torch.uint8) if want[key].dtype.is_floating_point else want[key]), (what, key)


@pytest.mark.parametrize('num_workers', [0, 3])
def test_batches_equal_build_batch_and_survive_being_held(tmp_path, num_workers):
    ds = _dataset(tmp_path, augmentation=AUG)
    loader = _loader(ds, num_workers)
    loader.set_epoch(2)
    assert len(loader) == 3
    it = iter(loader)
    first = next(it)
    held = {k: v.clone() for k, v in first.items()}
    rest = [next(it), next(it)]                         # batches 1 and 2 run on the side stream while 0 is held
    with pytest.raises(StopIteration):
        next(it)
    torch.cuda.synchronize()
    _assert_equal(first, held, 'batch 0 after batches 1 and 2')
    batches = [first] + rest
    assert [b['id'].tolist() for b in batches] == [[101, 102], [103, 104], [105]]
    assert all(b['id'].dtype == torch.int64 for b in batches) and batches[2]['input'].shape == (1, 3, 32, 32)
    for k, b in enumerate(batches):
        assert sorted(b) == PLAIN_KEYS
        _assert_equal(b, _direct(loader, k), 'batch %d' % k)
    assert first['hm'].shape == (2, 3, 8, 8) and first['wh'].shape == (2, 6, 2) and first['input'].dtype == torch.float32
    assert int(first['reg_mask'][1].sum()) == 0           # image 1 carries no annotation
    # the augmentation did something, and another epoch draws differently
    plain = _loader(_dataset(tmp_path / 'plain'), num_workers)
    same = next(iter(plain))
    assert not torch.equal(same['input'], first['input'])
    loader.set_epoch(3)
    assert not torch.equal(next(iter(loader))['input'], first['input'])
    # a second pass over the same epoch reproduces it
    loader.set_epoch(2)
    again = list(loader)
    for a, b in zip(again, batches):
        _assert_equal(a, b, 'second pass')


def test_resize_only_batch_against_numpy(tmp_path):
    """Without an augmentation list a 24 x 32 image only gets taller: the centre of box 0 lands where hand arithmetic
    puts it, and `id`, the order and the padding are as expected."""
    loader = _loader(_dataset(tmp_path))
    b = next(iter(loader))
    x, y, bw, bh = 1.5, 2.0, 32 / 3.0, 24 / 3.0           # coco_fixture.annotation(k=0) on a 24 x 32 image
    cx, cy = (x + bw / 2) / 4.0, (y + bh / 2) * (32 / 24) / 4.0
    assert int(b['ind'][0, 0]) == int(cy) * 8 + int(cx) and int(b['reg_mask'][0].sum()) == 2
    assert abs(float(b['wh'][0, 0, 0]) - bw / 4.0) < 1e-5 and abs(float(b['wh'][0, 0, 1]) - bh * (32 / 24) / 4.0) < 1e-5
    assert 'target_domain_input' not in b


def test_rotated_boxes_and_keypoints(tmp_path):
    ds = _dataset(tmp_path, rotated=True, keypoints=2, augmentation=AUG)
    loader = _loader(ds, rotated=True, keypoints=2)
    batches = list(loader)
    assert sorted(batches[0]) == sorted(PLAIN_KEYS + ['kps', 'gt_kps', 'kp_reg_mask'])
    assert batches[0]['wh'].shape == (2, 6, 3) and batches[0]['gt_dets'].shape == (2, 6, 7)
    assert batches[0]['kps'].shape == (2, 6, 4) and batches[2]['gt_kps'].shape == (1, 6, 2, 2)
    for k, b in enumerate(batches):
        _assert_equal(b, _direct(loader, k), 'batch %d' % k)


@pytest.mark.parametrize('augment_target', [False, True])
def test_target_images(tmp_path, augment_target):
    glob = fx.write_target_images(tmp_path, 4)
    ds = _dataset(tmp_path, augmentation=AUG, target_domain_glob=glob, augment_target_domain=augment_target)
    loader = _loader(ds)
    loader.set_epoch(1)
    batches = list(loader)
    for k, b in enumerate(batches):
        assert sorted(b) == sorted(PLAIN_KEYS + ['target_domain_input'])
        assert b['target_domain_input'].shape == b['input'].shape
        _assert_equal(b, _direct(loader, k), 'batch %d' % k)
    # resized only unless augment_target_domain: then it equals the plain normalised resize of the drawn files
    h = loader.collate(0)
    resized = build_batch(h.images.to(DEV), h.geometry.to(DEV), h.classes.to(DEV), h.counts.to(DEV), params=h.params,
                          input_size=(32, 32), num_classes=3, sizes=h.sizes, mean=MEAN, std=STD,
                          target_images=h.target_images.to(DEV), target_sizes=h.target_sizes)['target_domain_input']
    assert torch.equal(resized, batches[0]['target_domain_input']) != augment_target
    assert bool(h.target_params.applied) == augment_target
