"""No-GPU checks of the COCO evaluation (evaluation/coco.py, csrc/evalcoco.hip): the mask rule's rows have no holes,
`rotate_bbox` equals the reference's recorded results, the oracle (tests/cocoeval_oracle.py) is pinned by a hand-worked
case and by the tie / ignore rules, the evaluator's host half (grouping, accumulation, summary, names) agrees with the
oracle when fed the oracle's own matching bits, the closed-form rule of the kernels runs on the CPU under the sanitizers
and equals the Python rule, and the C surface rejects bad arguments without touching a device."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cocoeval_cases as cc
import cocoeval_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def sweep():
    from utils.box import rotate_bboxes
    boxes = co.sweep_boxes(4000, 0, 128)
    return boxes, rotate_bboxes(boxes)


def test_mask_rows_have_no_holes(sweep):
    """one (left, right) span per image row describes a mask only while no row of the rule has a gap"""
    _, verts = sweep
    holes = empty = 0
    for v in verts:
        m = co.quad_mask(v, 128, 128)
        holes += co.mask_rows(m)[2]
        empty += not m.any()
    print('holed rows %d, empty masks %d of %d' % (holes, empty, len(verts)))
    assert holes == 0
    assert empty <= len(verts) // 10


def test_rotate_bbox_equals_the_reference(golden):
    from utils.box import rotate_bbox, rotate_bboxes
    g = golden('rotate_bbox')
    boxes, want = g['boxes'], g['verts']
    assert boxes.dtype == np.float32 and len(boxes) >= 500 and (boxes[:, :2] < 0).any()
    assert set(np.float32([-90, 90])) <= set(boxes[:, 4])
    assert np.array_equal(rotate_bboxes(boxes), want)
    for b, w in zip(boxes, want):
        got = rotate_bbox(*b)
        assert len(got) == 4 and np.array_equal(np.array(got), w)
    # by hand: 20 x 10 about (50, 40), not rotated
    assert np.array(rotate_bbox(50.0, 40.0, 20.0, 10.0, 0.0)).tolist() == [[40, 35], [60, 35], [60, 45], [40, 45]]


def test_hand_worked_accumulation_on_the_oracle():
    o = co.OracleEvaluator()
    o.add_batch(**cc.hand_worked())
    r = o.evaluate()
    for name in ('mAP', 'mAP.50IOU', 'mAP.75IOU', 'mAP_medium'):
        assert abs(r['MSCOCO_Precision/' + name] - 0.8349835) < 1e-7
        assert abs(r['MSCOCO_Precision/' + name] - cc.HAND_AP) < 1e-9
    assert r['MSCOCO_Recall/mAR1'] == 0.5 and r['MSCOCO_Recall/mAR10'] == 1.0 and r['MSCOCO_Recall/mAR100'] == 1.0
    assert r['MSCOCO_Recall/mAR100_medium'] == 1.0
    for name in ('Precision/mAP_small', 'Precision/mAP_large', 'Recall/mAR100_small', 'Recall/mAR100_large'):
        assert np.isnan(r['MSCOCO_' + name])
    assert abs(r['MSCOCO_Class_0/Precision/AP'] - cc.HAND_AP) < 1e-9


def test_tie_and_ignore_rules_on_the_oracle():
    dt = [{'area': 2000.0, 'score': 0.9}]
    # equal IoU to two ground truths: the later one is matched
    gt = [{'area': 2000.0}, {'area': 2000.0}]
    r = co.evaluate_img(dt, gt, [[0.8, 0.8]], co.AREA_RANGES[0])
    assert [row[0] for row in r['match']] == [1] * 7 + [-1] * 3            # thresholds 0.5 .. 0.8 match, 0.85 .. do not
    # a non-ignored candidate wins over an ignored one of larger IoU ('medium' range: the 500-pixel one is ignored)
    gt = [{'area': 500.0}, {'area': 2000.0}]
    r = co.evaluate_img(dt, gt, [[0.9, 0.6]], co.AREA_RANGES[2])
    assert r['gt_ignore'] == [True, False]
    assert [row[0] for row in r['match']] == [1, 1, 1] + [0] * 6 + [-1]    # 0.5 .. 0.6: the non-ignored one; then the ignored
    assert [row[0] for row in r['dt_ignore']] == [False] * 3 + [True] * 6 + [False]
    # unmatched and outside the range: ignored
    r = co.evaluate_img([{'area': 100.0, 'score': 0.5}], gt, [[0.0, 0.0]], co.AREA_RANGES[2])
    assert all(row[0] for row in r['dt_ignore']) and not any(row[0] for row in r['matched'])


def _oracle_run(name):
    rotated, batches = cc.case(name)
    o = co.OracleEvaluator()
    o.use_rotated_boxes = rotated
    for b in batches:
        o.add_batch(**b)
    return o, o.evaluate()


@pytest.mark.parametrize('name', ['axis', 'many_dets', 'lonely'])
def test_host_half_of_the_evaluator_against_the_oracle(name):
    """evaluation.coco's grouping, accumulation, summary and names, fed the ORACLE's matching bits instead of the
    kernels' (the kernels' bits are held to the oracle's in tests/test_gpu_cocoeval.py)"""
    from evaluation import coco
    co.OracleEvaluator._known_ids.clear()
    o, want = _oracle_run(name)
    per_image = o.detail['per_image']
    _, batches = cc.case(name)
    det = {k: [] for k in ('image', 'cat', 'rank', 'score', 'bits')}
    gt = {'cat': [], 'ignore': []}
    labels, image_id = set(), 0
    for b in batches:
        det_src, gt_src, groups, keys, seen = coco.group_batch(b['pred_classes'], b['pred_scores'], b['gt_classes'], 0.1)
        labels |= seen
        assert groups[:, 1].max() <= 100
        pairs = 0
        for (d0, nd, g0, ng, p0), (i, c) in zip(groups, keys):
            e = per_image[(image_id + i + 1, c)]
            assert nd == len(e['dt']) and ng == len(e['gt'])
            assert [b['pred_scores'][i][j] for _, j in det_src[d0:d0 + nd]] == [d['score'] for d in e['dt']]
            assert p0 == pairs
            pairs += nd * ng
            bits = np.zeros((nd, 4), np.uint32)
            for a, r in enumerate(e['ranges']):
                for t in range(10):
                    bits[:, a] |= (np.array(r['matched'][t], dtype=np.uint32).reshape(-1) << t)
                    bits[:, a] |= (np.array(r['dt_ignore'][t], dtype=np.uint32).reshape(-1) << (16 + t))
            det['image'] += [image_id + i + 1] * nd
            det['cat'] += [c] * nd
            det['rank'] += list(range(nd))
            det['score'] += [d['score'] for d in e['dt']]
            det['bits'].append(bits)
            gt['cat'] += [c] * ng
            gt['ignore'].append(np.array([r['gt_ignore'] for r in e['ranges']], dtype=bool).reshape(4, ng).T)
        image_id += len(b['gt_ids'])
    det = {'image': np.array(det['image']), 'cat': np.array(det['cat']), 'rank': np.array(det['rank']),
           'score': np.array(det['score'], np.float32), 'bits': np.concatenate(det['bits'])}
    gt = {'cat': np.array(gt['cat']), 'ignore': np.concatenate(gt['ignore'])}
    cats = sorted(labels)
    precision, recall = coco.accumulate(cats, det, gt)
    assert np.array_equal(precision, o.detail['precision']) and np.array_equal(recall, o.detail['recall'])
    summaries = []
    for _, _, is_precision, iou_index, area_index, max_det in coco.SUMMARIES:
        per_class, mean = coco.summarize(precision, recall, is_precision, iou_index, area_index, max_det)
        per_label = np.full(max(cats) + 1, np.nan)
        per_label[cats] = per_class
        summaries.append((per_label, mean))
    got = coco.to_tensorboard(summaries, cats, True, None)
    assert set(got) == set(want)
    for k in want:
        assert np.isnan(got[k]) if np.isnan(want[k]) else abs(got[k] - want[k]) <= 1e-12, k


def test_metric_names():
    from evaluation import coco
    names = json.load(open(os.path.join(GOLDEN, 'cocoeval_keys.json')))
    assert len(names) == len(set(names)) == 24
    assert 'MSCOCO_Precision/mAP' in names and 'MSCOCO_Precision/mAP.50IOU' in names and 'MSCOCO_Recall/mAR100_small' in names
    means, templates = [n for n in names if '{}' not in n], [n for n in names if '{}' in n]
    summaries = [(np.arange(4.0), 0.5)] * 12
    classes = {1: {'name': 'car'}}
    # the evaluator's naming
    assert set(coco.to_tensorboard(summaries, [1, 3], False, classes)) == set(names)
    want = set(means) | {t.format(label) for t in templates for label in ('car', '3')}
    got = coco.to_tensorboard(summaries, [1, 3], True, classes)
    assert set(got) == want and got['MSCOCO_Class_car/Precision/AP'] == 1.0 and got['MSCOCO_Class_3/Recall/AR1'] == 3.0
    # the oracle's naming
    for per_class in (False, True):
        o = co.OracleEvaluator(per_class=per_class)
        o.classes = {0: {'name': 'car'}}
        o.add_batch(**cc.hand_worked())
        keys = set(o.evaluate())
        assert keys == (set(means) | {t.format('car') for t in templates} if per_class else set(names))


def test_evaluator_surface_and_no_cpu_fallback():
    import inspect
    import torch
    from evaluation.coco import Evaluator
    sig = inspect.signature(Evaluator.__init__)
    assert list(sig.parameters)[1:] == ['per_class', 'score_threshold']
    assert sig.parameters['per_class'].default is True and sig.parameters['score_threshold'].default == 0.1
    assert list(inspect.signature(Evaluator.add_batch).parameters)[1:] == [
        'pred_boxes', 'pred_classes', 'pred_scores', 'gt_boxes', 'gt_classes', 'gt_ids', 'gt_areas', 'image_shape',
        'pred_kps', 'gt_kps']
    assert callable(Evaluator.evaluate) and callable(Evaluator.reset)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='MI355X only'):
            Evaluator()


NEW_SYMBOLS = ('cnuda_eval_workspace_bytes', 'cnuda_eval_box_spans', 'cnuda_eval_iou_rotated', 'cnuda_eval_iou_axis',
               'cnuda_eval_match')


def test_new_symbols_in_header_signature_table_and_library():
    import ctypes
    import hip_runtime as hr
    text = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    L = hr.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(hr._Sig, name) and hasattr(L, name), name
    assert L.cnuda_abi_version() == hr.ABI_VERSION == 2
    assert L.cnuda_eval_workspace_bytes(300, 512) >= 300 * 512 * 8
    assert L.cnuda_eval_workspace_bytes(300, 0) == 0 and L.cnuda_eval_workspace_bytes(-1, 512) == 0
    # null pointers and bad sizes are rejected before anything touches the device
    assert L.cnuda_eval_box_spans(None, 10, 64, 96, None, None, None, 0, None) == -1
    assert b'null' in L.cnuda_last_error()
    assert L.cnuda_eval_box_spans(None, 10, 0, 96, None, None, None, 0, None) == -1
    assert b'height' in L.cnuda_last_error()
    assert L.cnuda_eval_box_spans(None, 10, 64, 9000, None, None, None, 0, None) == -1
    assert L.cnuda_eval_iou_rotated(None, 3, 10, 10, 100, None, None, 64, None, None, 0, None) == -1
    assert b'null' in L.cnuda_last_error()
    assert L.cnuda_eval_iou_axis(None, None, None, 3, 10, 10, 100, None, None) == -1
    assert b'null' in L.cnuda_last_error()
    assert L.cnuda_eval_iou_axis(None, None, None, 3, 10, 10, -1, None, None) == -1
    thr = (ctypes.c_double * 10)(*np.linspace(0.5, 0.95, 10))
    rng = (ctypes.c_double * 8)(0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10)
    assert L.cnuda_eval_match(None, None, 3, None, None, 10, 10, 100, thr, 10, rng, None, None, None) == -1
    assert b'null' in L.cnuda_last_error()
    assert L.cnuda_eval_match(None, None, 3, None, None, 10, 10, 100, None, 10, rng, None, None, None) == -1
    assert L.cnuda_eval_match(None, None, 3, None, None, 10, 10, 100, thr, 17, rng, None, None, None) == -1
    assert b'thresholds' in L.cnuda_last_error()


def test_closed_form_mask_rule_on_the_cpu_under_sanitizers(sweep, tmp_path):
    """csrc/evalcoco.cuh is what the kernels run: line steps and scanlines in closed form.  The stand-alone program
    (address + undefined-behaviour sanitizers on the host side) runs it lane by lane on the CPU, and its argument checks
    and workspace sizes; the spans must equal the Python rule's masks.  Boxes far outside the image reach the 64-bit
    arithmetic."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'evalcoco_host')
    subprocess.check_call([hipcc, '-O2', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-Xarch_host',
                           '-fsanitize=address,undefined', '-I', os.path.join(ROOT, 'centernet-uda_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'evalcoco_host.cpp'), '-o', exe])
    from utils.box import rotate_bboxes
    _, verts = sweep
    far = rotate_bboxes(np.float32([[30000, -20000, 90000, 80000, 33], [-40000, 50, 100000, 30, -3], [50, 40000, 70, 90000, 88],
                                    [48, 32, 100000, 100000, 45], [48, 32, 100000, 3, 12.5], [-30000, -30000, 100000, 2, -45]]))
    for H, W, v in ((64, 96, np.concatenate([verts[:600], far])), (128, 128, verts[600:1400])):
        v = v.astype(np.int32)
        v.tofile(str(tmp_path / 'verts.bin'))
        subprocess.check_call([exe, str(tmp_path / 'verts.bin'), str(len(v)), str(H), str(W), str(tmp_path / 'spans.bin')])
        got = np.fromfile(str(tmp_path / 'spans.bin'), dtype=np.int32).reshape(len(v), H, 2)
        filled = 0
        for i in range(len(v)):
            left, right, holes = co.mask_rows(co.quad_mask(v[i], H, W))
            assert holes == 0
            assert np.array_equal(left, got[i, :, 0]) and np.array_equal(right, got[i, :, 1]), (i, v[i].tolist())
            filled += int((right >= left).any())
        assert filled > len(v) // 3


def test_mask_rule_against_cv2_fillpoly(sweep):
    cv2 = pytest.importorskip('cv2')
    _, verts = sweep
    differing = 0
    for v in verts[:1000]:
        want = np.zeros((128, 128), np.uint8)
        cv2.fillPoly(want, [v.astype(np.int32).reshape(1, -1, 2)], color=(1,))
        differing += not np.array_equal(want > 0, co.quad_mask(v, 128, 128))
    assert differing == 0


def test_whole_results_against_pycocotools():
    pytest.importorskip('pycocotools')
    import pycocotools.coco
    import pycocotools.cocoeval
    co.OracleEvaluator._known_ids.clear()
    o, _ = _oracle_run('axis')
    per_image = o.detail['per_image']
    cats = sorted({c for _, c in per_image})
    gt_coco, dt_coco = pycocotools.coco.COCO(), pycocotools.coco.COCO()
    images = [{'id': i} for i in sorted({i for i, _ in per_image})]
    gts, dts = [], []
    for (img, c), e in per_image.items():
        for g in e['gt']:
            gts.append({'image_id': img, 'category_id': c, 'bbox': [float(v) for v in g['bbox']], 'area': float(g['area']),
                        'iscrowd': False, 'id': len(gts) + 1})
        for d in e['dt']:
            dts.append({'image_id': img, 'category_id': c, 'bbox': [float(v) for v in d['bbox']], 'area': float(d['area']),
                        'iscrowd': False, 'id': len(dts) + 1, 'score': float(d['score'])})
    for coco_obj, annos in ((gt_coco, gts), (dt_coco, dts)):
        coco_obj.dataset = {'categories': [{'id': c} for c in cats], 'annotations': annos, 'images': images}
        coco_obj.createIndex()
    ev = pycocotools.cocoeval.COCOeval(gt_coco, dt_coco, 'bbox')
    ev.evaluate()
    ev.accumulate()
    assert np.allclose(ev.eval['precision'], o.detail['precision'], atol=1e-12)
    assert np.allclose(ev.eval['recall'], o.detail['recall'], atol=1e-12)
