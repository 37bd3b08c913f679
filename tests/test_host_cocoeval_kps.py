"""No-GPU checks of the COCO keypoint evaluation (evaluation/coco_keypoints.py, csrc/evalcoco.hip): the oracle
(tests/cocoeval_kps_oracle.py) is pinned by cases worked by hand and by the ignore rule and the cut to 20, the
evaluator's host half (grouping, accumulation and summary with the limits (20,), names) agrees with the oracle when fed
the oracle's own matching bits, and the C surface has the two symbols and rejects bad arguments without a device."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import cocoeval_kps_cases as kc
import cocoeval_kps_oracle as ko
import cocoeval_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG2 = (0.05, 0.1)

MEANS = ['MSCOCO_Keypoints_Precision/mAP', 'MSCOCO_Keypoints_Precision/mAP.50IOU', 'MSCOCO_Keypoints_Precision/mAP.75IOU',
         'MSCOCO_Keypoints_Precision/mAP_medium', 'MSCOCO_Keypoints_Precision/mAP_large',
         'MSCOCO_Keypoints_Recall/mAR20', 'MSCOCO_Keypoints_Recall/mAR20.50IOU', 'MSCOCO_Keypoints_Recall/mAR20.75IOU',
         'MSCOCO_Keypoints_Recall/mAR20_medium', 'MSCOCO_Keypoints_Recall/mAR20_large']
PER_CLASS = ['MSCOCO_Keypoints_Class_{}/Precision/AP', 'MSCOCO_Keypoints_Class_{}/Precision/AP.50IOU',
             'MSCOCO_Keypoints_Class_{}/Precision/AP.75IOU', 'MSCOCO_Keypoints_Class_{}/Precision/mAP_medium',
             'MSCOCO_Keypoints_Class_{}/Precision/mAP_large', 'MSCOCO_Keypoints_Class_{}/Recall/AR20',
             'MSCOCO_Keypoints_Class_{}/Recall/AR20.50IOU', 'MSCOCO_Keypoints_Class_{}/Recall/AR20.75IOU',
             'MSCOCO_Keypoints_Class_{}/Recall/AR20_medium', 'MSCOCO_Keypoints_Class_{}/Recall/AR20_large']

# (ground truth (x, y, v) x 2, detection (x, y) x 2, box, OKS): J = 2, sigma = (0.05, 0.1), area 100.  var = (0.01, 0.04),
# so a distance of 1 at joint 0 and of 2 at joint 1 both give e = 0.5
HAND = [
    ([(10, 10, 2), (20, 10, 1)], [(11, 10), (20, 12)], (0, 0, 1, 1), math.exp(-0.5)),
    ([(10, 10, 2), (0, 0, 0)], [(11, 10), (99, 99)], (0, 0, 1, 1), math.exp(-0.5)),         # the unlabelled joint does not count
    ([(10, 10, 2), (20, 10, 2)], [(13, 10), (20, 10)], (0, 0, 1, 1), (math.exp(-4.5) + 1) / 2),
    ([(10, 10, 0), (20, 10, 0)], [(0, 30), (29.5, 0.5)], (10, 10, 10, 10), 1.0),           # inside [0, 30]^2
    ([(10, 10, 0), (20, 10, 0)], [(31, 10), (15, 15)], (10, 10, 10, 10), (math.exp(-0.5) + 1) / 2),
]


def _oks(gt, det, box):
    g = np.float32(gt)
    return ko.oks(np.float32(det), g[:, :2], g[:, 2], 100.0, np.float32(box), SIG2)


def test_hand_worked_similarities():
    assert abs(HAND[0][3] - 0.6065306597126334) < 1e-16 and abs(HAND[2][3] - 0.5055544982691211) < 1e-16
    for gt, det, box, want in HAND:
        # (2 sigma)^2 and the quotients round: a few units in the last place of e, fewer of exp(-e)
        assert abs(_oks(gt, det, box) - want) <= 1e-15, (gt, det)
    assert _oks(*HAND[3][:3]) == 1.0


def test_hand_worked_match_between_two_thresholds():
    gt, det, box, want = HAND[2]
    g = np.float32(gt)
    r = ko.evaluate_img([{'area': 0.0, 'score': 0.9}], [{'area': 100.0, 'ignore': False}], [[_oks(gt, det, box)]],
                        co.AREA_RANGES[0])
    assert 0.50 < want < 0.55 and g.shape == (2, 3)
    assert [row[0] for row in r['matched']] == [True] + [False] * 9          # matched at 0.50 and not at 0.55


def _two_objects(flagged_score, labelled_score):
    """one image, one class: a ground truth without a labelled joint and one with both, each with an exact detection"""
    gt = np.float32([[[50, 50, 0], [60, 60, 0]], [[200, 200, 2], [220, 210, 2]]])
    det = np.float32([[[52, 52], [58, 61]], [[200, 200], [220, 210]]])
    return {'pred_boxes': np.float32([[[40, 40, 70, 70], [190, 190, 230, 220]]]), 'pred_classes': np.zeros((1, 2), np.int32),
            'pred_scores': np.float32([[flagged_score, labelled_score]]), 'pred_kps': det[None],
            'gt_boxes': [np.float32([[40, 40, 70, 70], [190, 190, 230, 220]])], 'gt_classes': [np.zeros(2, np.int32)],
            'gt_ids': [np.int64(7100)], 'gt_areas': [np.float32([900, 1200])], 'gt_kps': [gt], 'image_shape': (3, 256, 256)}


def test_ground_truth_without_a_labelled_joint_is_ignored():
    o = ko.OracleKeypointEvaluator(sigmas=SIG2)
    o.add_batch(**_two_objects(0.9, 0.8))                 # the detection on the ignored ground truth scores higher
    r = o.evaluate()
    e = o.detail['per_image'][(co.OracleEvaluator._known_ids.index(7100) + 1, 0)]
    assert [g['ignore'] for g in e['gt']] == [True, False] and e['ious'][0][0] == 1.0
    for rng in e['ranges']:
        assert rng['gt_ignore'][0] is True
    everything = e['ranges'][0]
    assert all(row == [True, True] for row in everything['matched'])
    assert all(row == [True, False] for row in everything['dt_ignore'])          # neither true nor false positive
    # as a false positive ahead of the true one it would halve the precision
    # (precision is tp / (tp + fp + 2^-52): one unit in the last place below 1)
    assert abs(r['MSCOCO_Keypoints_Precision/mAP'] - 1.0) < 1e-15 and r['MSCOCO_Keypoints_Recall/mAR20'] == 1.0
    assert abs(r['MSCOCO_Keypoints_Precision/mAP_medium'] - 1.0) < 1e-15
    assert np.isnan(r['MSCOCO_Keypoints_Precision/mAP_large'])


def test_a_group_of_25_detections_is_cut_to_20():
    from evaluation import coco, coco_keypoints
    o = ko.OracleKeypointEvaluator(sigmas=kc.SIGMAS3)
    batch = kc.case(3)[1]
    o.add_batch(**batch)
    o.evaluate()
    first = co.OracleEvaluator._known_ids.index(int(batch['gt_ids'][0])) + 1
    e = o.detail['per_image'][(first, 0)]
    assert int((batch['pred_scores'][0] >= np.float32(0.1)).sum()) == 25
    assert len(e['dt']) == 20 and len(e['gt']) == 70 and len(e['ranges'][0]['matched'][0]) == 20
    assert [d['score'] for d in e['dt']] == sorted((d['score'] for d in e['dt']), reverse=True)
    assert coco_keypoints.MAX_DETECTIONS == (20,) and coco.MAX_DETECTIONS == (1, 10, 100)
    groups = coco.group_batch(batch['pred_classes'], batch['pred_scores'], batch['gt_classes'], 0.1, 20)[2]
    assert groups[0].tolist() == [0, 20, 0, 70, 0] and groups[1].tolist() == [20, 20, 70, 120, 1400]
    assert coco.group_batch(batch['pred_classes'], batch['pred_scores'], batch['gt_classes'], 0.1)[2][0, 1] == 25


@pytest.mark.parametrize('J', [3, 17])
def test_the_seeded_cases_keep_away_from_thresholds_and_ties(J):
    """what lets tests/test_gpu_cocoeval_kps.py ask for equal match bits: no similarity within 1e-9 of a threshold, no
    two candidates of a detection closer than that unless equal; and the cases are what their description says"""
    o = ko.OracleKeypointEvaluator(sigmas=None if J == 17 else kc.SIGMAS3)
    for b in kc.case(J):
        o.add_batch(**b)
    o.evaluate()
    values, flagged, matched_to_flagged = [], 0, 0
    for e in o.detail['per_image'].values():
        flagged += sum(g['ignore'] for g in e['gt'])
        for d, row in enumerate(e['ious']):
            row = np.array(row)
            values += row.tolist()
            cand = np.sort(row[row >= 0.5])
            gaps = np.diff(cand)
            assert not ((gaps > 0) & (gaps < 1e-9)).any()
            for t in range(10):
                m = e['ranges'][0]['match'][t][d]
                matched_to_flagged += m > -1 and e['gt'][m]['ignore']
    values = np.array(values)
    assert np.abs(values[:, None] - co.IOU_THRS[None, :]).min() > 1e-9
    assert len(values) > 3000 and flagged >= 15 and matched_to_flagged > 0
    hist = np.histogram(values, bins=[0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0 + 1e-9])[0]
    print(J, len(values), hist.tolist())
    assert (hist > 20).all()                                     # spread over (0, 1)
    assert (values == 1.0).any()                                 # inside the doubled box of an unlabelled ground truth


def test_host_half_of_the_evaluator_against_the_oracle():
    """evaluation.coco's accumulate / summarize / to_tensorboard with the limits (20,) and the keypoint table, fed the
    oracle's matching bits"""
    from evaluation import coco, coco_keypoints as ck
    co.OracleEvaluator._known_ids.clear()
    o = ko.OracleKeypointEvaluator(sigmas=kc.SIGMAS3)
    batches = kc.case(3)
    for b in batches:
        o.add_batch(**b)
    want = o.evaluate()
    per_image = o.detail['per_image']
    det = {k: [] for k in ('image', 'cat', 'rank', 'score', 'bits')}
    gt = {'cat': [], 'ignore': []}
    labels, image_id = set(), 0
    for b in batches:
        det_src, gt_src, groups, keys, seen = coco.group_batch(b['pred_classes'], b['pred_scores'], b['gt_classes'], 0.1, 20)
        labels |= seen
        for (d0, nd, g0, ng, p0), (i, c) in zip(groups, keys):
            e = per_image[(image_id + i + 1, c)]
            assert nd == len(e['dt']) and ng == len(e['gt'])
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
    precision, recall = coco.accumulate(cats, det, gt, ck.MAX_DETECTIONS)
    assert precision.shape == (10, 101, len(cats), 4, 1)
    assert np.array_equal(precision, o.detail['precision']) and np.array_equal(recall, o.detail['recall'])
    summaries = []
    for _, _, is_precision, iou_index, area_index, max_det in ck.SUMMARIES:
        per_class, mean = coco.summarize(precision, recall, is_precision, iou_index, area_index, max_det, ck.MAX_DETECTIONS)
        per_label = np.full(max(cats) + 1, np.nan)
        per_label[cats] = per_class
        summaries.append((per_label, mean))
    got = coco.to_tensorboard(summaries, cats, True, None, ck.SUMMARIES)
    assert set(got) == set(want)
    finite = 0
    for k in want:
        assert np.isnan(got[k]) if np.isnan(want[k]) else abs(got[k] - want[k]) <= 1e-12, k
        finite += not np.isnan(want[k])
    assert finite >= 20 and 0 < want['MSCOCO_Keypoints_Precision/mAP'] < 1


def test_metric_names():
    from evaluation import coco, coco_keypoints as ck
    assert [s[0] for s in ck.SUMMARIES] == MEANS and [s[1] for s in ck.SUMMARIES] == PER_CLASS
    assert all(s[5] == 20 for s in ck.SUMMARIES) and {s[4] for s in ck.SUMMARIES} == {0, 2, 3}      # all, medium, large
    summaries = [(np.arange(4.0), 0.5)] * 10
    classes = {1: {'name': 'person'}}
    assert set(coco.to_tensorboard(summaries, [1, 3], False, classes, ck.SUMMARIES)) == set(MEANS) | set(PER_CLASS)
    got = coco.to_tensorboard(summaries, [1, 3], True, classes, ck.SUMMARIES)
    assert set(got) == set(MEANS) | {t.format(label) for t in PER_CLASS for label in ('person', '3')}
    assert got['MSCOCO_Keypoints_Class_person/Precision/AP'] == 1.0 and got['MSCOCO_Keypoints_Class_3/Recall/AR20'] == 3.0
    for per_class in (False, True):
        o = ko.OracleKeypointEvaluator(per_class=per_class, sigmas=SIG2)
        o.classes = {0: {'name': 'person'}}
        o.add_batch(**_two_objects(0.9, 0.8))
        keys = set(o.evaluate())
        assert keys == (set(MEANS) | {t.format('person') for t in PER_CLASS} if per_class else set(MEANS) | set(PER_CLASS))
    # the box evaluator's table and defaults are what they were
    assert len(coco.SUMMARIES) == 12 and coco.accumulate.__defaults__ == (coco.MAX_DETECTIONS,)
    assert coco.summarize.__defaults__ == (coco.MAX_DETECTIONS,) and coco.to_tensorboard.__defaults__ == (coco.SUMMARIES,)


def test_evaluator_surface_and_no_cpu_fallback():
    import torch
    from evaluation import coco
    from evaluation.coco_keypoints import COCO_PERSON_SIGMAS, Evaluator
    sig = inspect.signature(Evaluator.__init__)
    assert list(sig.parameters)[1:] == ['per_class', 'score_threshold', 'sigmas']
    assert sig.parameters['per_class'].default is True and sig.parameters['score_threshold'].default == 0.1
    assert sig.parameters['sigmas'].default is None
    assert list(inspect.signature(Evaluator.add_batch).parameters) == list(inspect.signature(coco.Evaluator.add_batch).parameters)
    assert callable(Evaluator.evaluate) and callable(Evaluator.reset)
    assert COCO_PERSON_SIGMAS == kc.PERSON and ko.COCO_PERSON_SIGMAS.tolist() == list(kc.PERSON)
    for bad in ([], [0.1, 0.0], [0.1, -1.0], [0.1] * 65):
        with pytest.raises(ValueError, match='sigmas'):
            Evaluator(sigmas=bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='MI355X only'):
            Evaluator()


def test_loader_and_driver_surface():
    from datasets.loader import DeviceLoader
    import train
    p = inspect.signature(DeviceLoader.__init__).parameters
    assert p['keypoint_visibility'].default is False and list(p)[-1] == 'keypoint_visibility'
    wants = train.wants_keypoint_visibility
    assert wants({'coco': None, 'coco_keypoints': {'per_class': True}}, 17) is True
    assert wants({'coco': {'per_class': True}}, 17) is False and wants({'coco': None}, 0) is False
    with pytest.raises(ValueError, match='num_keypoints'):
        wants({'coco': None, 'coco_keypoints': None}, 0)


KEYPOINT_OVERRIDES = ['model.backend.params.num_keypoints=17', 'model.backend.loss.params.kp_weight=1.0',
                      'evaluation={coco: {per_class: True}, coco_keypoints: {per_class: True}}']


def test_the_documented_overrides_compose_and_bind():
    """README's keypoint run: three overrides on any experiment (an experiment file of its own is not shipped)"""
    from importlib import import_module
    import train
    from utils.config import load_config
    cfg = load_config(os.path.join(ROOT, 'centernet-uda_amd', 'configs'), ['experiment=dla_baseline'] + KEYPOINT_OVERRIDES)
    assert cfg.model.backend.params.num_keypoints == 17 and cfg.model.backend.loss.params.kp_weight == 1.0
    assert list(cfg.evaluation.keys()) == ['coco', 'coco_keypoints']
    for e in cfg.evaluation:
        params = {'score_threshold': cfg.score_threshold, **(cfg.evaluation[e] or {})}
        inspect.signature(import_module('evaluation.%s' % e).Evaluator).bind(**params)
    assert train.wants_keypoint_visibility(cfg.evaluation, cfg.model.backend.params.num_keypoints) is True
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for o in KEYPOINT_OVERRIDES:
        assert o in readme, o


NEW_SYMBOLS = ('cnuda_eval_oks', 'cnuda_eval_match_flagged')


def test_new_symbols_in_header_signature_table_library_and_notes():
    import ctypes
    import hip_runtime as hr
    text = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    notes = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    L = hr.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(hr._Sig, name) and hasattr(L, name), name
        assert '`%s`' % name in notes, name
    assert L.cnuda_abi_version() == hr.ABI_VERSION == 2
    # null pointers and bad sizes are rejected before anything touches the device
    oks = lambda J, pairs=100: L.cnuda_eval_oks(None, None, None, None, None, None, J, None, 3, 10, 10, pairs, None, None,
                                                None, None)
    assert oks(17) == -1 and b'null' in L.cnuda_last_error()
    for J in (0, 65, -1):
        assert oks(J) == -1
        assert b'J = %d' % J in L.cnuda_last_error(), L.cnuda_last_error()
    assert oks(17, -1) == -1 and b'negative' in L.cnuda_last_error()
    assert L.cnuda_eval_oks(None, None, None, None, None, None, 64, None, 0, 0, 0, 0, None, None, None, None) == 0
    thr = (ctypes.c_double * 10)(*np.linspace(0.5, 0.95, 10))
    rng = (ctypes.c_double * 8)(0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10)
    flagged = lambda t, n, r: L.cnuda_eval_match_flagged(None, None, 3, None, None, None, 10, 10, 100, t, n, r, None, None,
                                                         None)
    assert flagged(thr, 10, rng) == -1 and b'null' in L.cnuda_last_error()
    assert b'cnuda_eval_match_flagged' in L.cnuda_last_error()
    assert flagged(None, 10, rng) == -1
    assert flagged(thr, 17, rng) == -1 and b'thresholds' in L.cnuda_last_error()


def test_whole_results_against_pycocotools():
    pytest.importorskip('pycocotools')
    import pycocotools.coco
    import pycocotools.cocoeval
    co.OracleEvaluator._known_ids.clear()
    o = ko.OracleKeypointEvaluator()
    for b in kc.case(17):
        o.add_batch(**b)
    o.evaluate()
    per_image = o.detail['per_image']
    cats = sorted({c for _, c in per_image})
    gt_coco, dt_coco = pycocotools.coco.COCO(), pycocotools.coco.COCO()
    images = [{'id': i} for i in sorted({i for i, _ in per_image})]
    gts, dts = [], []
    triples = lambda k, v: [float(x) for row in np.concatenate([k, np.asarray(v, np.float32)[:, None]], 1) for x in row]
    for (img, c), e in per_image.items():
        for g in e['gt']:
            gts.append({'image_id': img, 'category_id': c, 'bbox': [float(v) for v in g['bbox']], 'area': float(g['area']),
                        'iscrowd': 0, 'id': len(gts) + 1, 'keypoints': triples(g['kps'], g['vis']),
                        'num_keypoints': int((g['vis'] > 0).sum())})
        for d in e['dt']:
            dts.append({'image_id': img, 'category_id': c, 'area': float(d['area']), 'iscrowd': 0, 'id': len(dts) + 1,
                        'score': float(d['score']), 'keypoints': triples(d['kps'], np.ones(len(d['kps'])))})
    for coco_obj, annos in ((gt_coco, gts), (dt_coco, dts)):
        coco_obj.dataset = {'categories': [{'id': c} for c in cats], 'annotations': annos, 'images': images}
        coco_obj.createIndex()
    ev = pycocotools.cocoeval.COCOeval(gt_coco, dt_coco, 'keypoints')
    ev.evaluate()
    ev.accumulate()
    assert np.allclose(ev.eval['precision'], o.detail['precision'], atol=1e-12)
    assert np.allclose(ev.eval['recall'], o.detail['recall'], atol=1e-12)
