"""Generate a COCO-format dataset for timing the training driver (profiles/driver_loop_cost.py): N source images of
640 x 480 with a few axis-aligned boxes each, N // 4 target-domain images and a small validation split, all PNG.
Nothing here is committed; the images are drawn from a seed.

    python profiles/make_driver_dataset.py OUT_DIR [--images 320] [--seed 0]
"""
import argparse
import json
import os

import numpy as np
from PIL import Image

W, H = 640, 480


def picture(rng, boxes):
    """A soft two-axis colour ramp with mild noise and one filled rectangle per box: decodes like a photo-sized PNG
    without being pure noise."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([x * rng.uniform(0.1, 0.4), y * rng.uniform(0.1, 0.5), (x + y) * rng.uniform(0.05, 0.2)], 2)
    img = base + rng.uniform(0, 60, 3).astype(np.float32) + rng.normal(0, 3, (H, W, 3)).astype(np.float32)
    for bx, by, bw, bh in boxes:
        img[int(by):int(by + bh), int(bx):int(bx + bw)] = rng.uniform(0, 255, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


def split(out, name, count, rng, classes, first_id):
    folder = os.path.join(out, name, 'images')
    os.makedirs(folder, exist_ok=True)
    images, anns = [], []
    for i in range(count):
        boxes = []
        for _ in range(int(rng.integers(1, 9))):
            bw, bh = rng.uniform(24, 200), rng.uniform(24, 200)
            boxes.append((float(rng.uniform(0, W - bw)), float(rng.uniform(0, H - bh)), float(bw), float(bh)))
        fname = '%s_%05d.png' % (name, i)
        Image.fromarray(picture(rng, boxes)).save(os.path.join(folder, fname), compress_level=3)
        images.append({'id': first_id + i, 'file_name': fname, 'width': W, 'height': H})
        for b in boxes:
            anns.append({'id': len(anns) + 1, 'image_id': first_id + i, 'category_id': int(rng.integers(1, classes + 1)),
                         'bbox': list(b), 'area': b[2] * b[3], 'iscrowd': 0})
    path = os.path.join(out, name, 'instances.json')
    with open(path, 'w') as f:
        json.dump({'images': images, 'annotations': anns,
                   'categories': [{'id': c, 'name': 'class%d' % c} for c in range(1, classes + 1)]}, f)
    return folder, path


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('out')
    ap.add_argument('--images', type=int, default=320)
    ap.add_argument('--classes', type=int, default=6)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    train = split(args.out, 'train', args.images, rng, args.classes, 1)
    val = split(args.out, 'val', 16, rng, args.classes, 100001)
    target = os.path.join(args.out, 'target')
    os.makedirs(target, exist_ok=True)
    for i in range(max(1, args.images // 4)):
        Image.fromarray(picture(rng, [])).save(os.path.join(target, 'target_%05d.png' % i), compress_level=3)
    print(json.dumps({'train': train, 'val': val, 'target_glob': os.path.join(target, '*.png')}))


if __name__ == '__main__':
    main()
