"""datasets.coco.Dataset and datasets.coco_merger.Dataset on a dataset written into tmp_path.  The reference's classes
cannot be imported here (pycocotools, imgaug and cv2 are no dependencies), so every expectation is worked out by hand
from datasets/coco.py:76-113, 120-133, 264-279 and datasets/coco_merger.py:28-35 of the reference."""
import json
import os

import numpy as np
import pytest
from PIL import Image

import coco_fixture as fx
from datasets.coco import Dataset
from datasets.coco_merger import Dataset as Merger
from utils.box import get_annotation_with_angle, rotate_bbox
from utils.config import Config


def _write(root, images, annotations, categories=(1, 2, 3), name='ds'):
    """images: [(id, h, w)] -> (folder, annotation file); image k's pixels are fx.pixels(h, w, k)"""
    folder = os.path.join(str(root), name)
    os.makedirs(folder, exist_ok=True)
    recs = []
    for k, (img_id, h, w) in enumerate(images):
        fname = 'im%d.png' % k
        Image.fromarray(fx.pixels(h, w, k)).save(os.path.join(folder, fname))
        recs.append({'id': img_id, 'file_name': fname, 'height': h, 'width': w})
    path = os.path.join(folder, 'instances.json')
    with open(path, 'w') as f:
        json.dump({'images': recs, 'annotations': annotations,
                   'categories': [{'id': c, 'name': 'c%d' % c} for c in categories]}, f)
    return folder, path


IMAGES = [(7, 24, 32), (3, 40, 28), (5, 24, 32)]        # ids deliberately not sorted: file order counts
ANNS = [
    {'id': 11, 'image_id': 3, 'category_id': 2, 'bbox': [1.5, 2.0, 10.0, 20.25], 'area': 77.0},
    {'id': 12, 'image_id': 7, 'category_id': 3, 'bbox': [4, 5, 6, 7]},
    {'id': 13, 'image_id': 3, 'category_id': 1, 'bbox': [0.25, 0.5, 3.0, 4.0], 'keypoints': [1, 2, 2, 3.5, 4.5, 1]},
    {'id': 14, 'image_id': 3, 'category_id': 3, 'bbox': [2, 2, 2, 2], 'area': 4.0},
]


def test_order_length_decoding_and_the_plain_sample(tmp_path):
    folder, path = _write(tmp_path, IMAGES, ANNS)
    ds = Dataset(folder, path, num_classes=3)
    assert len(ds) == 3 and ds.images == [7, 3, 5]                       # file order, not sorted
    s = ds[1]                                                             # image id 3: annotations 11, 13, 14 in file order
    assert s['id'] == 3 and s['image'].dtype == np.uint8 and np.array_equal(s['image'], fx.pixels(40, 28, 1))
    assert s['boxes'].dtype == np.float32 and s['boxes'].shape == (3, 4)
    # xywh -> x1, y1, x2, y2 (datasets/coco.py:403-406)
    assert s['boxes'].tolist() == [[1.5, 2.0, 11.5, 22.25], [0.25, 0.5, 3.25, 4.5], [2.0, 2.0, 4.0, 4.0]]
    assert s['classes'].tolist() == [1, 0, 2] and s['classes'].dtype == np.int32      # category id - 1
    assert s['areas'].dtype == np.float32 and s['areas'][0] == 77.0 and np.isnan(s['areas'][1]) and s['areas'][2] == 4.0
    assert 'keypoints' not in s and 'visibility' not in s and 'corners' not in s and 'target_image' not in s
    s0, s2 = ds[0], ds[2]
    assert s0['id'] == 7 and s0['boxes'].tolist() == [[4.0, 5.0, 10.0, 12.0]] and np.isnan(s0['areas']).all()
    assert s2['id'] == 5 and s2['boxes'].shape == (0, 4) and s2['classes'].shape == (0,) and s2['areas'].shape == (0,)
    assert np.array_equal(s0['image'], fx.pixels(24, 32, 0)) and s2['image'].shape == (24, 32, 3)


def test_greyscale_and_palette_files_come_back_as_rgb(tmp_path):
    folder, path = _write(tmp_path, IMAGES[:1], [])
    grey = np.arange(24 * 32, dtype=np.uint8).reshape(24, 32)
    Image.fromarray(grey).save(os.path.join(folder, 'im0.png'))
    img = Dataset(folder, path, num_classes=3)[0]['image']
    assert img.shape == (24, 32, 3) and all(np.array_equal(img[..., c], grey) for c in range(3))


def test_truncation_at_max_detections(tmp_path):
    folder, path = _write(tmp_path, IMAGES, ANNS)
    s = Dataset(folder, path, num_classes=3, max_detections=2)[1]
    assert s['boxes'].shape == (2, 4) and s['classes'].tolist() == [1, 0] and s['areas'].shape == (2,)
    assert s['boxes'][1].tolist() == [0.25, 0.5, 3.25, 4.5]               # the FIRST two, in file order


def test_class_table_and_the_raise_for_a_category_outside_the_range(tmp_path):
    folder, path = _write(tmp_path, IMAGES, ANNS, categories=(1, 3))
    ds = Dataset(folder, path, num_classes=4)
    assert ds.cat_mapping == {1: 0, 2: 1, 3: 2, 4: 3}
    assert ds.classes == {0: {'id': 1, 'name': 'c1'}, 1: '', 2: {'id': 3, 'name': 'c3'}, 3: ''}
    two = Dataset(folder, path, num_classes=2)
    assert two[2]['classes'].shape == (0,)                                 # an image without annotations is fine
    with pytest.raises(ValueError, match=r"annotation 12 .* category_id 3 outside 1\.\.2"):
        two[0]
    with pytest.raises(ValueError, match="annotation 14"):                # 11 and 13 are in range, 14 is not
        two[1]
    bad = [dict(ANNS[1], category_id=0)]
    folder0, path0 = _write(tmp_path, IMAGES, bad, name='zero')
    with pytest.raises(ValueError, match="category_id 0 outside"):
        Dataset(folder0, path0, num_classes=3)[0]


def test_keypoints_zeros_where_missing_and_visibility(tmp_path):
    folder, path = _write(tmp_path, IMAGES, ANNS)
    s = Dataset(folder, path, num_classes=3, num_keypoints=2)[1]
    assert s['keypoints'].shape == (3, 2, 2) and s['visibility'].shape == (3, 2)
    assert s['keypoints'][1].tolist() == [[1.0, 2.0], [3.5, 4.5]] and s['visibility'][1].tolist() == [2, 1]
    for k in (0, 2):                                                       # no `keypoints`: zeros (coco.py:126-127)
        assert not s['keypoints'][k].any() and not s['visibility'][k].any()
    with pytest.raises(ValueError, match="annotation 13 has 6 keypoint values, expected 3 x 3"):
        Dataset(folder, path, num_classes=3, num_keypoints=3)[1]


def test_rotated_annotations_become_the_rotate_bbox_vertices(tmp_path):
    anns = [{'id': 1, 'image_id': 7, 'category_id': 1, 'bbox': [0, 0, 1, 1], 'rbbox': [16.0, 12.0, 10.0, 6.0, 30.0]},
            {'id': 2, 'image_id': 7, 'category_id': 2, 'bbox': [0, 0, 1, 1], 'rbbox': [10.0, 10.0, 4.0, 4.0, 90.0],
             'keypoints': [5, 6, 2]}]
    folder, path = _write(tmp_path, IMAGES, anns)
    s = Dataset(folder, path, num_classes=3, rotated_boxes=True, num_keypoints=1)[0]
    assert 'boxes' not in s and s['corners'].shape == (2, 4, 2) and s['corners'].dtype == np.float64
    for k, ann in enumerate(anns):
        want = np.asarray(rotate_bbox(*get_annotation_with_angle(ann)))
        assert np.array_equal(s['corners'][k], want)
    # the first by hand: w > h swaps the sides and turns 30 -> -60 degrees; half extents (3, 5); corners truncated
    c, sn = np.cos(np.radians(np.float32(-60))), np.sin(np.radians(np.float32(-60)))
    by_hand = [[16 + (-3 * c - (-5) * sn), 12 + (-3 * sn + (-5) * c)], [16 + (3 * c - (-5) * sn), 12 + (3 * sn + (-5) * c)],
               [16 + (3 * c - 5 * sn), 12 + (3 * sn + 5 * c)], [16 + (-3 * c - 5 * sn), 12 + (-3 * sn + 5 * c)]]
    assert s['corners'][0].tolist() == np.trunc(by_hand).tolist()
    assert s['keypoints'].tolist() == [[[0.0, 0.0]], [[5.0, 6.0]]] and s['visibility'].tolist() == [[0], [2]]
    assert s['classes'].tolist() == [0, 1]
    plain = [{'id': 1, 'image_id': 7, 'category_id': 1, 'bbox': [0, 0, 1, 1]}]
    folder2, path2 = _write(tmp_path, IMAGES, plain, name='plain')
    with pytest.raises(ValueError, match='rbbox'):
        Dataset(folder2, path2, num_classes=3, rotated_boxes=True)[0]


def test_string_ids_are_numbered_in_order_of_first_sight(tmp_path):
    images = [('zebra', 24, 32), ('apple', 40, 28), ('mango', 24, 32)]
    anns = [{'id': 1, 'image_id': 'apple', 'category_id': 1, 'bbox': [1, 1, 2, 2]}]
    folder, path = _write(tmp_path, images, anns)
    ds = Dataset(folder, path, num_classes=3)
    assert [ds[i]['id'] for i in (2, 0, 2, 1, 0)] == [1, 2, 1, 3, 2]
    assert ds[1]['boxes'].shape == (1, 4) and ds.string_id_mapping == {'mango': 1, 'zebra': 2, 'apple': 3}


def test_target_glob_as_string_list_and_none(tmp_path):
    folder, path = _write(tmp_path, IMAGES, ANNS)
    glob_a = fx.write_target_images(tmp_path, 3, name='ta', first_seed=100)
    glob_b = fx.write_target_images(tmp_path, 2, name='tb', first_seed=200)
    none = Dataset(folder, path, num_classes=3)
    assert none.target_domain_files == [] and 'target_image' not in none[0]
    one = Dataset(folder, path, num_classes=3, target_domain_glob=glob_a)
    assert [os.path.basename(p) for p in one.target_domain_files] == ['tgt_00.png', 'tgt_01.png', 'tgt_02.png']
    both = Dataset(folder, path, num_classes=3, target_domain_glob=[glob_a, glob_b])
    assert len(both.target_domain_files) == 5 and both.target_domain_files[:3] == one.target_domain_files
    assert Dataset(folder, path, num_classes=3, target_domain_glob=[]).target_domain_files == []
    # the choice: a number in [0, 1) picks the file; the image comes back decoded and unresized
    assert np.array_equal(both.get(0, 0.0)['target_image'], fx.pixels(24, 32, 100))
    assert np.array_equal(both.get(0, 0.39)['target_image'], fx.pixels(40, 28, 101))
    assert np.array_equal(both.get(0, 0.999)['target_image'], fx.pixels(40, 28, 201))
    # drawn uniformly when nobody chooses: all five files turn up
    np.random.seed(0)
    seen = {both[0]['target_image'].tobytes() for _ in range(60)}
    assert len(seen) == 5


def test_the_constructor_has_the_reference_signature():
    import inspect
    assert list(inspect.signature(Dataset.__init__).parameters)[1:] == [
        'image_folder', 'annotation_file', 'input_size', 'target_domain_glob', 'num_classes', 'num_keypoints',
        'rotated_boxes', 'mean', 'std', 'augmentation', 'augment_target_domain', 'max_detections', 'down_ratio']
    assert list(inspect.signature(Merger.__init__).parameters)[1:] == ['datasets', 'max_samples', 'defaults']


def test_merger_length_boundaries_and_per_member_overrides(tmp_path):
    fa, pa = _write(tmp_path, IMAGES, ANNS, name='a')                                       # 3 images
    fb, pb = _write(tmp_path, [(1, 40, 28), (2, 24, 32)], [], name='b')                     # 2 images
    fc, pc = _write(tmp_path, [(9, 24, 32)] * 1 + [(8, 40, 28)] * 1 + [(6, 24, 32), (4, 40, 28)], [], name='c')   # 4
    aug = [{'Fliplr': {'p': 1.0}}]
    spec = Config({'d': [
        {'name': 'coco', 'params': {'image_folder': fa, 'annotation_file': pa}},
        {'name': 'coco', 'params': {'image_folder': fb, 'annotation_file': pb, 'augmentation': aug,
                                    'input_size': [64, 48], 'max_detections': 7}},
        {'name': 'coco', 'params': {'image_folder': fc, 'annotation_file': pc, 'num_classes': 5}}]}).d
    m = Merger(spec, max_samples=None, num_classes=3, max_detections=20, input_size=(32, 32), augmentation=None)
    assert len(m) == 9 and m.intervals.tolist() == [3, 5, 9]
    a, b, c = m.members
    # first and last index of each member
    for index, member, local in [(0, a, 0), (2, a, 2), (3, b, 0), (4, b, 1), (5, c, 0), (8, c, 3)]:
        got, at = m.locate(index)
        assert got is member and at == local, index
        assert m[index]['id'] == member[local]['id']
    assert [m[i]['id'] for i in range(9)] == [7, 3, 5, 1, 2, 9, 8, 6, 4]
    assert m[4]['image'].shape == (24, 32, 3) and m[3]['image'].shape == (40, 28, 3)
    with pytest.raises(IndexError):
        m[9]
    with pytest.raises(IndexError):
        m[-1]
    # {**defaults, **member params}: the member wins, and keeps its own augmentation list and input size
    assert (a.input_size, a.max_detections, a.num_classes, a.augmentation) == ((32, 32), 20, 3, None)
    assert (b.input_size, b.max_detections, b.num_classes) == ((64, 48), 7, 3) and b.augmentation == aug
    assert b.augmenter is not None and a.augmenter is None and c.num_classes == 5 and c.input_size == (32, 32)
    assert m.classes == a.classes
