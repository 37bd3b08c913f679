"""evaluation.coco_keypoints.Evaluator and its kernels (csrc/evalcoco.hip: cnuda_eval_oks, cnuda_eval_match_flagged) on
the GPU against the independent oracle (tests/cocoeval_kps_oracle.py), and the visibility flag from the loader to
`get_detections`.  Inputs: tests/cocoeval_kps_cases.py, J = 3 and J = 17.

Pair similarity: at most 1e-13 from the oracle's.  Both sides do the same float64 operations in the same order without
contraction; they can differ only in exp, at most about one unit in the last place on each side, over terms in (0, 1]
that are averaged: a few 1e-16, times about 100 for the two math libraries.  Areas, flags and match bits: equal.
Scalars: within 1e-12 (the integers underneath are equal; what remains are sums of a few thousand doubles in [0, 1])."""
import types

import numpy as np
import pytest
import torch

import cocoeval_kps_cases as kc
import cocoeval_kps_oracle as ko
import cocoeval_oracle as co

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _fresh_ids():
    from evaluation.coco import Evaluator
    Evaluator._known_ids.clear()
    co.OracleEvaluator._known_ids.clear()


def _sigmas(J):
    return None if J == 17 else kc.SIGMAS3


def _both(J, per_class=True):
    from evaluation.coco_keypoints import Evaluator
    _fresh_ids()
    batches = kc.case(J)
    ev, o = Evaluator(per_class=per_class, sigmas=_sigmas(J)), ko.OracleKeypointEvaluator(per_class=per_class, sigmas=_sigmas(J))
    ev._keep_intermediates = True
    for b in batches:
        ev.add_batch(**b)
        o.add_batch(**b)
    seen = [{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()} for rec in ev._batches]
    return seen, ev.evaluate(), o, o.evaluate()


_RUNS = {}


@pytest.fixture
def run():
    def get(J):
        if J not in _RUNS:
            _RUNS[J] = _both(J)          # computed once, shared, left unchanged
        return _RUNS[J]
    return get


def _groups_of(seen, o, batches):
    first = 0
    for rec, b in zip(seen, batches):
        for grp, (i, c) in zip(rec['groups'], rec['keys']):
            yield rec, grp, o.detail['per_image'][(first + i + 1, int(c))]
        first += len(b['gt_ids'])


@pytest.mark.parametrize('J', [3, 17])
def test_pair_similarity_areas_and_flags(run, J):
    seen, _, o, _ = run(J)
    pairs, worst, shapes, flagged = 0, 0.0, set(), 0
    for rec, (d0, nd, g0, ng, p0), e in _groups_of(seen, o, kc.case(J)):
        assert nd == len(e['dt']) and ng == len(e['gt'])
        shapes.add((nd, ng))
        want = np.array(e['ious'], dtype=np.float64).reshape(nd, ng)
        got = rec['iou'][p0:p0 + nd * ng].reshape(nd, ng)
        if nd and ng:
            worst = max(worst, float(np.abs(got - want).max()))
        pairs += nd * ng
        assert np.array_equal(rec['det_area'][d0:d0 + nd], np.array([d['area'] for d in e['dt']], dtype=np.float64))
        assert rec['gt_flags'][g0:g0 + ng].tolist() == [int(g['ignore']) for g in e['gt']]
        assert np.array_equal(rec['gt_area'][g0:g0 + ng], np.array([g['area'] for g in e['gt']], dtype=np.float64))
        flagged += sum(g['ignore'] for g in e['gt'])
    print('J = %d: %d pairs, largest |OKS - oracle| = %.3g' % (J, pairs, worst))
    assert worst <= 1e-13
    assert pairs > 3000 and flagged >= 15
    assert (20, 70) in shapes and (20, 120) in shapes                    # the cut; the grid-stride loop (2400 pairs)
    assert any(nd == 0 and ng > 0 for nd, ng in shapes) and any(nd > 0 and ng == 0 for nd, ng in shapes)


@pytest.mark.parametrize('J', [3, 17])
def test_matching_bits_equal_the_oracle(run, J):
    seen, _, o, _ = run(J)
    # the precondition, on the oracle alone: no similarity within 1e-9 of a threshold, no near-tie among the candidates
    for e in o.detail['per_image'].values():
        for row in e['ious']:
            row = np.array(row, dtype=np.float64)
            if len(row):
                assert np.abs(row[:, None] - co.IOU_THRS[None, :]).min() > 1e-9
            gaps = np.diff(np.sort(row[row >= 0.5]))
            assert not ((gaps > 0) & (gaps < 1e-9)).any()
    ignored_matches = 0
    for rec, (d0, nd, g0, ng, p0), e in _groups_of(seen, o, kc.case(J)):
        for a, r in enumerate(e['ranges']):
            bits = rec['det_bits'][d0:d0 + nd, a].astype(np.int64) & 0xffffffff
            for t in range(10):
                assert ((bits >> t) & 1).tolist() == [int(v) for v in r['matched'][t]], (J, a, t)
                assert ((bits >> (16 + t)) & 1).tolist() == [int(v) for v in r['dt_ignore'][t]], (J, a, t)
            assert (bits >> 26 == 0).all() and ((bits >> 10) & 63 == 0).all()
            assert rec['gt_ignore'][g0:g0 + ng, a].tolist() == [int(v) for v in r['gt_ignore']]
            # a flagged ground truth is ignored in every range
            assert all(rec['gt_ignore'][g0 + j, a] == 1 for j, g in enumerate(e['gt']) if g['ignore'])
        r = e['ranges'][0]
        ignored_matches += sum(m > -1 and e['gt'][m]['ignore'] for row in r['match'] for m in row)
    assert ignored_matches > 0               # detections matched to a ground truth without a labelled joint


@pytest.mark.parametrize('per_class', [True, False])
@pytest.mark.parametrize('J', [3, 17])
def test_end_to_end_scalars(run, J, per_class):
    _, got, _, want = run(J) if per_class else _both(J, per_class=False)[0:4]
    assert set(got) == set(want) and len(got) >= 20
    finite = 0
    for k, w in want.items():
        g = np.asarray(got[k], dtype=np.float64)
        w = np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape, k
        print('%-52s %s %s' % (k, g, w))
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        assert (np.abs(g - w)[~np.isnan(w)] <= 1e-12).all(), (k, g, w)
        finite += int((~np.isnan(w)).sum())
    assert finite >= 20


def test_evaluate_resets_and_repeats_bit_for_bit():
    from evaluation.coco_keypoints import Evaluator
    _fresh_ids()
    batches = kc.case(3)
    ev = Evaluator(sigmas=kc.SIGMAS3)
    results = []
    for _ in range(2):
        for b in batches:
            ev.add_batch(**b)
        results.append(ev.evaluate())          # evaluate() resets: the same ids may come again
        assert not ev._batches and not ev.ids
    assert set(results[0]) == set(results[1])
    for k, v in results[0].items():
        assert v == results[1][k] or (np.isnan(v) and np.isnan(results[1][k])), k


def test_two_column_ground_truth_means_every_joint_labelled():
    from evaluation.coco_keypoints import Evaluator
    _fresh_ids()
    out = []
    for form in (kc.two_columns, kc.all_visible):
        ev = Evaluator(sigmas=kc.SIGMAS3)
        for b in kc.case(3):
            ev.add_batch(**form(b))
        out.append(ev.evaluate())
    assert set(out[0]) == set(out[1])
    for k, v in out[0].items():
        assert v == out[1][k] or (np.isnan(v) and np.isnan(out[1][k])), k
    assert 0 < out[0]['MSCOCO_Keypoints_Precision/mAP'] < 1


def test_the_box_evaluator_beside_it_is_unchanged_by_the_third_column():
    from evaluation.coco import Evaluator
    _fresh_ids()
    out = []
    for form in (lambda b: b, kc.two_columns):
        ev = Evaluator()
        for b in kc.case(3):
            ev.add_batch(**form(b))
        out.append(ev.evaluate())
    assert set(out[0]) == set(out[1]) and len(out[0]) >= 24
    for k, v in out[0].items():
        assert v == out[1][k] or (np.isnan(v) and np.isnan(out[1][k])), k


def test_arguments_the_evaluator_refuses():
    from evaluation.coco_keypoints import Evaluator
    _fresh_ids()
    b = kc.case(3)[0]
    with pytest.raises(ValueError, match='pred_kps and gt_kps'):
        Evaluator(sigmas=kc.SIGMAS3).add_batch(**{k: v for k, v in b.items() if k not in ('pred_kps', 'gt_kps')})
    with pytest.raises(ValueError, match='pred_kps and gt_kps'):
        Evaluator(sigmas=kc.SIGMAS3).add_batch(**{k: v for k, v in b.items() if k != 'gt_kps'})
    with pytest.raises(ValueError, match='J = 3'):
        Evaluator().add_batch(**b)                            # no sigmas: only for the 17 person joints
    with pytest.raises(ValueError, match='2 sigmas for J = 3'):
        Evaluator(sigmas=[0.1, 0.1]).add_batch(**b)
    ev = Evaluator(sigmas=kc.SIGMAS3)
    ev.add_batch(**b)                                         # none of the refused calls took the image ids
    with pytest.raises(ValueError, match='already added'):
        ev.add_batch(**b)


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def test_visibility_from_the_loader_to_get_detections(tmp_path):
    import coco_fixture as fx
    import uda.base as ub
    from datasets.coco import Dataset
    from datasets.loader import DeviceLoader
    folder, path = fx.write_dataset(tmp_path, 5, keypoints=2)
    ds = Dataset(folder, path, input_size=(32, 32), num_classes=3, max_detections=6, rotated_boxes=False, num_keypoints=2)
    kw = dict(batch_size=2, shuffle=False, num_workers=0, device=DEV, seed=11, num_classes=3, num_keypoints=2,
              rotated_boxes=False, down_ratio=4, mean=(0.4, 0.4, 0.4), std=(0.3, 0.3, 0.3), max_detections=6)
    plain, flagged = next(iter(DeviceLoader(ds, **kw))), next(iter(DeviceLoader(ds, keypoint_visibility=True, **kw)))
    assert sorted(flagged) == sorted(list(plain) + ['gt_kps_visibility'])
    for k in plain:
        assert torch.equal(plain[k], flagged[k]), k
    v = flagged['gt_kps_visibility']
    assert v.shape == (2, 6, 2) and v.dtype == torch.int32 and v.device == DEV
    counts = flagged['reg_mask'].sum(1).tolist()
    assert counts[0] == 2
    assert v[0, :2].tolist() == [[2, 1], [2, 1]] and int(v[0, 2:].abs().sum()) == 0      # the fixture's v: 2, 1
    # without keypoints the flag asks for nothing
    ds0 = Dataset(folder, path, input_size=(32, 32), num_classes=3, max_detections=6, rotated_boxes=False, num_keypoints=0)
    none = next(iter(DeviceLoader(ds0, keypoint_visibility=True, **dict(kw, num_keypoints=0))))
    assert 'gt_kps_visibility' not in none and 'gt_kps' not in none

    m = ub.Model()
    m.cfg = _ns(max_detections=5, model=_ns(backend=_ns(params=_ns(rotated_boxes=False))))
    m.backend = _ns(down_ratio=4)
    g = torch.Generator().manual_seed(3)
    heads = {'hm': torch.rand(2, 3, 8, 8, generator=g), 'wh': torch.rand(2, 2, 8, 8, generator=g) * 4,
             'reg': torch.rand(2, 2, 8, 8, generator=g), 'kps': torch.randn(2, 4, 8, 8, generator=g)}
    outputs = lambda: {'source_domain': {k: t.to(DEV).clone() for k, t in heads.items()}}
    with_v = m.get_detections(outputs(), {k: t.clone() for k, t in flagged.items()})
    without = m.get_detections(outputs(), {k: t.clone() for k, t in plain.items()})
    assert sorted(with_v) == sorted(without)
    for k in without:
        if k != 'gt_kps':
            for a, b in zip(with_v[k], without[k]):
                assert np.array_equal(np.asarray(a), np.asarray(b)), k
    for i, n in enumerate(counts):
        assert without['gt_kps'][i].shape == (n, 2, 2) and with_v['gt_kps'][i].shape == (n, 2, 3)
        assert with_v['gt_kps'][i].dtype == without['gt_kps'][i].dtype
        assert np.array_equal(with_v['gt_kps'][i][:, :, :2], without['gt_kps'][i])
        assert with_v['gt_kps'][i][:, :, 2].tolist() == [[2, 1]] * n
    assert with_v['pred_kps'].shape == (2, 5, 2, 2)
    # both evaluators take the dictionary as the driver hands it over
    from evaluation.coco import Evaluator as Boxes
    from evaluation.coco_keypoints import Evaluator as Joints
    _fresh_ids()
    scalars = {}
    for ev in (Boxes(), Joints(sigmas=[0.05, 0.08])):
        ev.add_batch(image_shape=flagged['input'].shape[1:], **with_v)
        scalars.update(ev.evaluate())
    assert 'MSCOCO_Precision/mAP' in scalars and 'MSCOCO_Keypoints_Precision/mAP' in scalars
    # the previews read the first two columns
    from utils.visualize import Visualizer
    vis = Visualizer({c: {'name': str(c)} for c in range(3)}, 0.2, (0.4, 0.4, 0.4), (0.3, 0.3, 0.3))
    a = vis.visualize_batch(flagged['input'], with_v)
    b = vis.visualize_batch(plain['input'], without)
    assert torch.equal(a, b)
