"""A tiny COCO-format dataset written with PIL and json (helper of the dataset, loader and driver tests): PNG images of
two sizes, alternating (24 x 32 and 40 x 28, height x width), with deterministic pixel content and hand-placed
annotations."""
import json
import os

import numpy as np
from PIL import Image

SIZES = [(24, 32), (40, 28)]                 # (height, width)


def pixels(h, w, seed):
    """A smooth colour ramp plus a seeded offset: survives PNG exactly, and no two images are equal."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 7 + seed * 13) % 256, (y * 5 + seed * 29) % 256, ((x + y) * 3 + seed * 41) % 256], 2)
    return img.astype(np.uint8)


def write_images(folder, count, prefix='img', first_seed=0):
    os.makedirs(folder, exist_ok=True)
    out = []
    for i in range(count):
        h, w = SIZES[i % 2]
        name = '%s_%02d.png' % (prefix, i)
        Image.fromarray(pixels(h, w, first_seed + i)).save(os.path.join(folder, name))
        out.append((name, h, w))
    return out


def annotation(ann_id, image_id, k, h, w, rotated=False, keypoints=0, with_area=True, category=None):
    """The k-th box of an image: a box of about a third of the frame, shifted with k, always inside the image."""
    bw, bh = max(4.0, w / 3.0 + k), max(4.0, h / 3.0 - k)
    x, y = 1.5 + 2.0 * k, 2.0 + 1.5 * k
    ann = {'id': ann_id, 'image_id': image_id, 'category_id': category if category is not None else 1 + (ann_id % 3),
           'bbox': [x, y, bw, bh], 'iscrowd': 0}
    if with_area:
        ann['area'] = bw * bh
    if rotated:
        ann['rbbox'] = [x + bw / 2, y + bh / 2, bw, bh, 15.0 * (k + 1)]
    if keypoints:
        ann['keypoints'] = [v for j in range(keypoints) for v in (x + j, y + 2 * j, 2 if j % 2 == 0 else 1)]
    return ann


def write_dataset(root, count, name='train', boxes_per_image=2, rotated=False, keypoints=0, first_seed=0,
                  categories=3):
    """-> (image_folder, annotation_file).  Image ids are 101, 102, ...; image i has `boxes_per_image` boxes, except
    image 1, which has none."""
    folder = os.path.join(str(root), name, 'images')
    files = write_images(folder, count, first_seed=first_seed)
    images, anns = [], []
    for i, (fname, h, w) in enumerate(files):
        images.append({'id': 101 + i, 'file_name': fname, 'height': h, 'width': w})
        for k in range(0 if i == 1 else boxes_per_image):
            anns.append(annotation(len(anns) + 1, 101 + i, k, h, w, rotated=rotated, keypoints=keypoints))
    cats = [{'id': c, 'name': 'class%d' % c, 'supercategory': 'thing'} for c in range(1, categories + 1)]
    path = os.path.join(str(root), name, 'instances.json')
    with open(path, 'w') as f:
        json.dump({'images': images, 'annotations': anns, 'categories': cats}, f)
    return folder, path


def write_target_images(root, count, name='target', first_seed=100):
    folder = os.path.join(str(root), name)
    write_images(folder, count, prefix='tgt', first_seed=first_seed)
    return os.path.join(folder, '*.png')
