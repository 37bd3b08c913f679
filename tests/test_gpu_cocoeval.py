"""evaluation.coco.Evaluator and the kernels of csrc/evalcoco.hip on the GPU against the independent oracle
(tests/cocoeval_oracle.py): row spans and areas of the box masks, pair IoU bit for bit in float64, matching bits, and
every returned scalar within 1e-12 (the integers underneath are equal; what remains are sums of at most a few thousand
doubles in [0, 1]).  Inputs: tests/cocoeval_cases.py."""
import numpy as np
import pytest
import torch

import cocoeval_cases as cc
import cocoeval_oracle as co

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _fresh_ids():
    from evaluation.coco import Evaluator
    Evaluator._known_ids.clear()
    co.OracleEvaluator._known_ids.clear()


def _both(name, **kw):
    """the case through the Evaluator and the oracle -> (per-batch device results on the host, scalars, oracle, scalars)"""
    from evaluation.coco import Evaluator
    _fresh_ids()
    rotated, batches = cc.case(name)
    ev, o = Evaluator(**kw), co.OracleEvaluator(**kw)
    ev.use_rotated_boxes = o.use_rotated_boxes = rotated
    ev._keep_intermediates = True
    for b in batches:
        ev.add_batch(**b)
        o.add_batch(**b)
    seen = []
    for rec in ev._batches:
        seen.append({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()})
    return seen, ev.evaluate(), o, o.evaluate()


_RUNS = {}


@pytest.fixture
def run():
    def get(name):
        if name not in _RUNS:
            _RUNS[name] = _both(name)
        return _RUNS[name]
    return get


def _groups_of(seen, o, batches):
    """yields (batch record, group row, oracle entry of that (image, category))"""
    first = 0
    for rec, b in zip(seen, batches):
        for grp, (i, c) in zip(rec['groups'], rec['keys']):
            yield rec, grp, o.detail['per_image'][(first + i + 1, int(c))]
        first += len(b['gt_ids'])


def test_spans_and_areas_equal_the_oracle_masks():
    """the sweep's first 600 boxes on 64 x 96, wholly or partly outside included"""
    import hip_runtime as hr
    from utils.box import rotate_bboxes
    H, W, n = 64, 96, 600
    verts = rotate_bboxes(co.sweep_boxes(4000, 0, 128)[:n])
    L = hr.lib()
    d_verts = torch.from_numpy(verts.astype(np.int32)).to(DEV)
    rows = torch.full((n, 2), -7, dtype=torch.int32, device=DEV)
    area = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    nbytes = L.cnuda_eval_workspace_bytes(n, H)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    hr.check(L.cnuda_eval_box_spans(hr.ptr(d_verts), n, H, W, hr.ptr(rows), hr.ptr(area), hr.ptr(ws), nbytes, hr.stream()))
    spans = ws[:n * H * 8].view(torch.int32).view(n, H, 2).cpu().numpy()
    rows, area = rows.cpu().numpy(), area.cpu().numpy()
    filled = 0
    for i in range(n):
        m = co.quad_mask(verts[i], H, W)
        left, right, holes = co.mask_rows(m)
        assert holes == 0
        assert np.array_equal(spans[i, :, 0], left) and np.array_equal(spans[i, :, 1], right), (i, verts[i].tolist())
        assert area[i] == m.sum()
        nz = np.flatnonzero(m.any(1))
        assert rows[i].tolist() == ([nz[0], nz[-1]] if len(nz) else [0, -1])
        filled += bool(len(nz))
    assert n // 3 < filled < n


@pytest.mark.parametrize('name', ['rotated', 'axis', 'many_gts', 'areas'])
def test_pair_iou_is_bit_equal(run, name):
    seen, _, o, _ = run(name)
    pairs = positive = 0
    for rec, (d0, nd, g0, ng, p0), e in _groups_of(seen, o, cc.case(name)[1]):
        assert nd == len(e['dt']) and ng == len(e['gt'])
        want = np.array(e['ious'], dtype=np.float64).reshape(nd, ng)
        got = rec['iou'][p0:p0 + nd * ng].reshape(nd, ng)
        assert np.array_equal(got, want), (name, d0, g0)
        pairs += nd * ng
        positive += int((want > 0).sum())
        if nd:
            assert np.array_equal(rec['det_area'][d0:d0 + nd], np.array([float(d['area']) for d in e['dt']]))
    assert pairs > 500 and 0 < positive < pairs          # touching and disjoint pairs (IoU exactly 0) beside overlapping ones


@pytest.mark.parametrize('name', cc.CASES)
def test_matching_bits_equal_the_oracle(run, name):
    seen, _, o, _ = run(name)
    max_nd = max_ng = 0
    for rec, (d0, nd, g0, ng, p0), e in _groups_of(seen, o, cc.case(name)[1]):
        max_nd, max_ng = max(max_nd, nd), max(max_ng, ng)
        for a, r in enumerate(e['ranges']):
            bits = rec['det_bits'][d0:d0 + nd, a].astype(np.int64) & 0xffffffff
            for t in range(10):
                assert ((bits >> t) & 1).tolist() == [int(v) for v in r['matched'][t]], (name, a, t)
                assert ((bits >> (16 + t)) & 1).tolist() == [int(v) for v in r['dt_ignore'][t]], (name, a, t)
            assert (bits >> 26 == 0).all() and ((bits >> 10) & 63 == 0).all()
            assert rec['gt_ignore'][g0:g0 + ng, a].tolist() == [int(v) for v in r['gt_ignore']]
    if name == 'many_dets':
        assert max_nd == 100                 # 130 detections of one class, cut
    if name == 'many_gts':
        assert max_ng == 70                  # a lane owns two ground truths
    if name == 'lonely':
        kinds = {(nd > 0, ng > 0) for rec in seen for _, nd, _, ng, _ in rec['groups']}
        assert kinds == {(True, False), (False, True), (True, True)}
    if name == 'areas':
        ig = np.concatenate([rec['gt_ignore'][:rec['ngt']] for rec in seen])
        assert not ig[:, 0].any() and all(0 < ig[:, a].sum() < len(ig) for a in (1, 2, 3))


@pytest.mark.parametrize('name', cc.CASES)
def test_end_to_end_scalars(run, name):
    _, got, _, want = run(name)
    assert set(got) == set(want) and len(got) >= 24
    finite = 0
    for k, w in want.items():
        print('%-44s %.17g %.17g' % (k, got[k], w))
        if np.isnan(w):
            assert np.isnan(got[k]), k
        else:
            assert abs(got[k] - w) <= 1e-12, (k, got[k], w)
            finite += 1
    assert finite >= 12


def test_hand_worked_case_and_key_sets():
    import json
    import os
    from evaluation.coco import Evaluator
    _fresh_ids()
    names = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cocoeval_keys.json')))
    ev = Evaluator()
    ev.num_workers = 4
    ev.classes = {0: {'name': 'car'}}
    ev.add_batch(**cc.hand_worked())
    r = ev.evaluate()
    assert set(r) == {n.format('car') for n in names}
    for name in ('mAP', 'mAP.50IOU', 'mAP.75IOU', 'mAP_medium'):
        assert abs(r['MSCOCO_Precision/' + name] - cc.HAND_AP) < 1e-9
    assert abs(r['MSCOCO_Class_car/Precision/AP'] - 0.8349835) < 1e-7
    assert r['MSCOCO_Recall/mAR1'] == 0.5 and r['MSCOCO_Recall/mAR10'] == 1.0 and r['MSCOCO_Recall/mAR100'] == 1.0
    assert r['MSCOCO_Recall/mAR100_medium'] == 1.0 and r['MSCOCO_Precision/mAP_medium'] == r['MSCOCO_Precision/mAP']
    for name in ('Precision/mAP_small', 'Precision/mAP_large', 'Recall/mAR100_small', 'Recall/mAR100_large'):
        assert np.isnan(r['MSCOCO_' + name])
    ev = Evaluator(per_class=False)
    ev.add_batch(**cc.hand_worked())
    r = ev.evaluate()
    assert set(r) == set(names) and r['MSCOCO_Class_{}/Precision/AP'].shape == (1,)


@pytest.mark.parametrize('name', ['axis', 'rotated'])
def test_evaluate_resets_and_repeats_bit_for_bit(name):
    from evaluation.coco import Evaluator
    _fresh_ids()
    rotated, batches = cc.case(name)
    ev = Evaluator()
    ev.use_rotated_boxes = rotated
    results = []
    for _ in range(2):
        for b in batches:
            ev.add_batch(**b)
        results.append(ev.evaluate())          # evaluate() resets: the same ids may come again
        ev.reset()
    assert set(results[0]) == set(results[1])
    for k, v in results[0].items():
        assert v == results[1][k] or (np.isnan(v) and np.isnan(results[1][k])), k


def test_score_threshold_and_repeated_id():
    from evaluation.coco import Evaluator
    _fresh_ids()
    _, batches = cc.case('axis')
    b = batches[0]
    scores = b['pred_scores']
    assert (scores < 0.3).any() and (scores >= 0.3).any() and (scores == np.float32(0.1)).any()
    ev = Evaluator(score_threshold=0.3)
    ev.add_batch(**b)
    assert ev._batches[0]['nd'] == int((scores >= np.float32(0.3)).sum())
    assert ev._batches[0]['det_score'].min() >= np.float32(0.3)
    got = ev.evaluate()
    o = co.OracleEvaluator(score_threshold=0.3)
    o.add_batch(**b)
    want = o.evaluate()
    for k, w in want.items():
        assert np.isnan(got[k]) if np.isnan(w) else abs(got[k] - w) <= 1e-12, k
    ev = Evaluator()                               # 0.1: a score of exactly 0.1 stays
    ev.add_batch(**b)
    assert ev._batches[0]['nd'] == int((scores >= np.float32(0.1)).sum())
    with pytest.raises(ValueError, match='already added'):
        ev.add_batch(**b)
    ev.reset()
    ev.add_batch(**b)                              # after reset() the id is free again
    dup = dict(batches[1])
    dup['gt_ids'] = [dup['gt_ids'][0]] * len(dup['gt_ids'])
    with pytest.raises(ValueError, match='already added'):
        ev.add_batch(**dup)
