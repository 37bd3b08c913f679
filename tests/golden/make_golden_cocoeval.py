#!/usr/bin/env python
"""Generates the COCO-evaluation fixtures by IMPORTING the reference (read-only) in the build container; only recorded
results and a list of names are written, no reference source travels.

    CENTERNET_UDA_REFERENCE=<reference checkout> python tests/golden/make_golden_cocoeval.py

rotate_bbox.npz: `boxes` [512, 5] float32 (x, y, w, h, angle) and `verts` [512, 4, 2] int64, what the reference's
utils.box.rotate_bbox (numpy only) returns for each row given as float32 scalars.
cocoeval_keys.json: the 24 scalar names of evaluation.coco.Evaluator after its TensorBoard conversion (12 means, 12
per-class templates with `{}` for the class); the module is imported with stand-ins for cv2 and its helper imports,
none of which the name table touches."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

REF = os.environ['CENTERNET_UDA_REFERENCE']
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_rotate_bbox():
    box = _load('reference_box', 'utils/box.py')
    rng = np.random.RandomState(11)
    n = 512
    b = np.stack([rng.uniform(-60, 700, n), rng.uniform(-60, 700, n), rng.uniform(0.2, 300, n),
                  rng.uniform(0.2, 300, n), rng.uniform(-90, 90, n)], 1)
    b[::8, 4] = rng.choice([-90.0, 90.0, -45.0, 0.0, 45.0, 89.99], len(b[::8]))
    b[1::16, :2] = np.round(b[1::16, :2])            # centres on whole pixels: corners on the truncation boundary
    b[2::16, 2:4] = np.round(b[2::16, 2:4]) * 2
    b = b.astype(np.float32)
    verts = np.array([np.array(box.rotate_bbox(*row)) for row in b]).astype(np.int64)
    np.savez_compressed(os.path.join(HERE, 'rotate_bbox.npz'), boxes=b, verts=verts)
    print('rotate_bbox.npz', b.shape, verts.shape)


def make_keys():
    for name in ('cv2',):
        sys.modules.setdefault(name, types.ModuleType(name))
    utils = types.ModuleType('utils')
    helper = types.ModuleType('utils.helper')
    helper.RedirectOut = object
    boxm = types.ModuleType('utils.box')
    boxm.rotate_bbox = None
    utils.helper, utils.box = helper, boxm
    saved = {k: sys.modules.get(k) for k in ('utils', 'utils.helper', 'utils.box')}
    sys.modules.update({'utils': utils, 'utils.helper': helper, 'utils.box': boxm})
    try:
        coco = _load('reference_eval_coco', 'evaluation/coco.py')
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    table = getattr(coco.Evaluator, '_Evaluator__coco_key_mapping')
    names = []
    for v in table.values():
        for old, new in (('(', ''), (')', ''), (' ', '_'), ('@', '')):
            v = v.replace(old, new)
        names.append(v)
    assert len(names) == len(set(names)) == 24
    with open(os.path.join(HERE, 'cocoeval_keys.json'), 'w') as f:
        json.dump(names, f, indent=1)
        f.write('\n')
    print('cocoeval_keys.json', len(names))


if __name__ == '__main__':
    make_rotate_bbox()
    make_keys()
