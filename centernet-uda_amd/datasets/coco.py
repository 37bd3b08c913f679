"""COCO-format detection dataset: the host half of the reference's `datasets.coco.Dataset` (datasets/coco.py:23-113).

The reference's `__getitem__` decodes, augments, resizes, normalises and encodes on the host.  Here it stops after
decoding: a sample is the RAW image and its annotations in source pixels, and `datasets.loader.DeviceLoader` pads a
batch of them, draws the augmentation and hands both to `datasets.build_batch` on the GPU.

The annotation file is indexed here (pycocotools is no dependency): images in file order, an image's annotations in
file order, categories by id -- what `COCO.getImgIds()`, `getAnnIds(imgIds=[i])` and `.cats` give the reference.
"""
import json
import logging
import threading
from glob import glob
from pathlib import Path

import numpy as np
from PIL import Image

from utils.box import get_annotation_with_angle, rotate_bbox

from .augment import Augmentation

log = logging.getLogger(__name__)


def load_rgb(path):
    """-> uint8 [H, W, 3], as the reference decodes (datasets/coco.py:83)."""
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


class Dataset:
    def __init__(
            self, image_folder, annotation_file, input_size=(512, 512),
            target_domain_glob=None, num_classes=80, num_keypoints=0,
            rotated_boxes=False, mean=(0.40789654, 0.44719302, 0.47026115),
            std=(0.28863828, 0.27408164, 0.27809835),
            augmentation=None, augment_target_domain=False, max_detections=150,
            down_ratio=4):
        self.image_folder = Path(image_folder)
        with open(annotation_file) as f:
            coco = json.load(f)
        self.imgs = {im['id']: im for im in coco.get('images', [])}
        self.cats = {c['id']: c for c in coco.get('categories', [])}
        self.anns = {i: [] for i in self.imgs}
        for ann in coco.get('annotations', []):
            self.anns.setdefault(ann['image_id'], []).append(ann)
        self.images = list(self.imgs)
        self.use_rotated_boxes = bool(rotated_boxes)
        self.max_detections = int(max_detections)
        self.down_ratio = down_ratio
        self.input_size = tuple(int(v) for v in input_size)
        assert len(self.input_size) == 2
        self.mean, self.std = tuple(mean), tuple(std)
        self.num_classes = int(num_classes)
        self.num_keypoints = int(num_keypoints)
        self.string_id_mapping = {}
        self._id_lock = threading.Lock()
        self.augment_target_domain = bool(augment_target_domain)
        self.cat_mapping = {v: i for i, v in enumerate(range(1, self.num_classes + 1))}
        self.classes = {y: self.cats[x] if x in self.cats else '' for x, y in self.cat_mapping.items()}

        if isinstance(target_domain_glob, str):
            patterns = [target_domain_glob]
        elif target_domain_glob is None:
            patterns = []
        else:
            patterns = list(target_domain_glob)
        self.target_domain_files = []
        for pattern in patterns:
            self.target_domain_files.extend(sorted(glob(pattern)))     # sorted: a run does not depend on the file system

        # the list as configured, and its parsed form; the draw itself is the loader's (one record per batch)
        self.augmentation = list(augmentation) if augmentation else None
        self.augmenter = Augmentation(self.augmentation) if self.augmentation else None
        log.info("found %d samples for target domain", len(self.target_domain_files))

    def __len__(self):
        return len(self.images)

    def _class_of(self, ann):
        cat = ann.get('category_id')
        if cat not in self.cat_mapping:
            raise ValueError("annotation %r of image %r has category_id %r outside 1..%d"
                             % (ann.get('id'), ann.get('image_id'), cat, self.num_classes))
        return self.cat_mapping[cat]

    def get(self, index, target_choice=None):
        """The raw sample `index`.  target_choice: a number in [0, 1) that picks the target-domain file (the loader
        draws it from the batch's generator); None draws it from numpy's global generator, as the reference does."""
        img_id = self.images[index]
        anns = self.anns[img_id]
        M = min(len(anns), self.max_detections)
        J = self.num_keypoints
        ret = {'image': load_rgb(self.image_folder / self.imgs[img_id]['file_name'])}
        if self.use_rotated_boxes:
            corners = np.zeros((M, 4, 2), dtype=np.float64)
            for k in range(M):
                corners[k] = np.asarray(rotate_bbox(*get_annotation_with_angle(anns[k])), dtype=np.float64)
            ret['corners'] = corners
        else:
            boxes = np.zeros((M, 4), dtype=np.float32)
            for k in range(M):
                x, y, w, h = anns[k]['bbox']
                boxes[k] = x, y, x + w, y + h
            ret['boxes'] = boxes
        ret['classes'] = np.array([self._class_of(anns[k]) for k in range(M)], dtype=np.int32)
        if J > 0:
            kps = np.zeros((M, J, 3), dtype=np.float64)
            for k in range(M):
                if 'keypoints' in anns[k]:
                    flat = np.asarray(anns[k]['keypoints'], dtype=np.float64)
                    if flat.size != 3 * J:
                        raise ValueError("annotation %r has %d keypoint values, expected 3 x %d"
                                         % (anns[k].get('id'), flat.size, J))
                    kps[k] = flat.reshape(J, 3)
            ret['keypoints'] = np.ascontiguousarray(kps[:, :, :2])
            ret['visibility'] = kps[:, :, 2].astype(np.int32)
        ret['areas'] = np.array([anns[k].get('area', np.nan) for k in range(M)], dtype=np.float32)

        if isinstance(img_id, str):                   # 1, 2, ... in order of first sight (datasets/coco.py:90-94)
            with self._id_lock:                       # samples are fetched from the loader's threads
                img_id = self.string_id_mapping.setdefault(img_id, 1 + len(self.string_id_mapping))
        ret['id'] = img_id

        if self.target_domain_files:
            u = np.random.random() if target_choice is None else float(target_choice)
            n = len(self.target_domain_files)
            ret['target_image'] = load_rgb(self.target_domain_files[min(int(u * n), n - 1)])
        return ret

    def __getitem__(self, index):
        return self.get(index)
