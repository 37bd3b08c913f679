"""MI355X: the rotated-box IoU (csrc/polyiou.cuh) through its three entries against the restatements of
tests/polyiou_oracle.py -- `ops.rotated_iou` and the evaluator's pair IoUs and areas bit for bit in float64, the rotated
soft-NMS merge with boxes and classes exact and scores to one float32 unit in the last place (the one difference the
kernel may show is a last bit of a double `exp`), the predictor with `soft_nms='polygon'` at two scales against the
same steps taken by hand, and the evaluator's scalars with `rotated_iou = 'polygon'` against the matching of
tests/cocoeval_oracle.py fed with the restatement's IoUs."""
import numpy as np
import pytest
import torch

import cocoeval_oracle as co
import polyiou_oracle as pio
import predict_oracle as po

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
G = lambda a: T(a).to(DEV)
N = lambda t: t.detach().cpu().numpy()


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def assert_one_ulp(got, want64, what=''):
    """got (float32) equals the float64 oracle rounded to float32, within one float32 unit in the last place (the rule
    of tests/test_gpu_predict.py for the axis-aligned merge)."""
    got, want = np.asarray(got), np.asarray(want64).astype(F)
    assert got.dtype == F and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
    assert not bad.any(), (what, got[bad][:4], want[bad][:4])


def square(x, y, side):
    return F([[x, y], [x + side, y], [x + side, y + side], [x, y + side]])


DIAMOND = F([[2, -1], [5, 2], [2, 5], [-1, 2]])


# ---------------------------------------------------------------------------------------------------------------------
# ops.rotated_iou
# ---------------------------------------------------------------------------------------------------------------------
def test_rotated_iou_hand_cases_are_the_restatements_bits():
    from hip_runtime import ops
    nan = square(0, 0, 4)
    nan[1, 0] = np.nan
    a = np.stack([np.stack([square(0, 0, 4), square(1, 1, 2), square(0, 0, 4)[::-1], F([[0, 0], [1, 1], [2, 2], [3, 3]]), nan]),
                  np.stack([square(0, 0, 4), square(2, 0, 4), square(4, 4, 4), DIAMOND, DIAMOND[::-1]])])
    b = np.stack([np.stack([square(0, 0, 4), DIAMOND, square(2, 0, 4)]),
                  np.stack([square(0, 0, 4), square(4, 0, 4), DIAMOND[::-1]])])
    assert a.shape == (2, 5, 4, 2) and b.shape == (2, 3, 4, 2)
    iou, area_a, area_b = (N(t) for t in ops.rotated_iou(G(a), G(b), return_areas=True))
    assert iou.dtype == np.float64 and iou.shape == (2, 5, 3) and area_a.shape == (2, 5) and area_b.shape == (2, 3)
    for i in range(2):
        want = pio.pairs(a[i], b[i])
        assert same_bits(iou[i], want[0]) and same_bits(area_a[i], want[1]) and same_bits(area_b[i], want[2])
    # the answers worked by hand
    assert iou[0, 0].tolist() == [1.0, 0.7, 1 / 3]             # identical squares, the octagon, shifted by half a side
    assert iou[0, 1, 0] == 0.25 and same_bits(iou[0, 2], iou[0, 0])      # 2-square in a 4-square; reversed winding
    assert not iou[0, 3].any() and not iou[0, 4].any()         # four collinear points; a NaN vertex
    assert iou[1, 0].tolist() == [1.0, 0.0, 0.7] and iou[1, 1, 0] == 1 / 3       # sharing an edge: 0
    assert iou[1, 2].tolist() == [0.0, 0.0, 0.0]               # sharing a corner, sharing an edge, apart
    assert same_bits(iou[1, 3], iou[1, 4])                     # the same pair with reversed winding: the same bits
    assert area_a[0].tolist() == [16.0, 4.0, 16.0, 0.0, 0.0] and area_b[0].tolist() == [16.0, 18.0, 16.0]
    assert same_bits(N(ops.rotated_iou(G(a), G(b))), iou)      # without the areas
    empty = ops.rotated_iou(G(a), torch.zeros((2, 0, 4, 2), device=DEV), return_areas=True)
    assert tuple(empty[0].shape) == (2, 5, 0) and same_bits(N(empty[1]), area_a) and tuple(empty[2].shape) == (2, 0)
    with pytest.raises(RuntimeError, match='rotated_iou'):
        ops.rotated_iou(G(a), G(b[:1]))


def test_rotated_iou_random_boxes_across_a_wave_and_a_workgroup():
    from hip_runtime import ops
    rng = np.random.default_rng(41)

    def boxes(n):
        c = rng.uniform(20, 140, (n, 2))
        return np.stack([pio.rotated_box(c[i, 0], c[i, 1], rng.uniform(3, 60), rng.uniform(3, 60), rng.uniform(-90, 90))
                         for i in range(n)])
    a, b = boxes(70), boxes(67)
    b[5], b[6] = a[3], a[4][::-1]                              # identical, and identical with the other winding
    want = pio.pairs(a, b)
    assert 0.1 < (want[0] > 0).mean() < 0.9 and want[0][3, 5] == 1.0 and want[0][4, 6] == 1.0
    first = [N(t) for t in ops.rotated_iou(G(a[None]), G(b[None]), return_areas=True)]
    again = [N(t) for t in ops.rotated_iou(G(a[None]), G(b[None]), return_areas=True)]
    for got, twice, w in zip(first, again, want):
        assert same_bits(got[0], w) and same_bits(twice, got)


# ---------------------------------------------------------------------------------------------------------------------
# the rotated soft-NMS merge
# ---------------------------------------------------------------------------------------------------------------------
B_NMS, C_NMS, N_NMS, K_NMS = 2, 3, 300, 20
NCAND = np.array([260, 300], np.int32)
THR_NMS = 0.95


def soft_nms_inputs():
    """Two images of 300 candidates: objects seen five times each as jittered rotated boxes; class 0 has more than 64
    members; five disjoint boxes of class 2 carry one score bit for bit; one candidate's class is outside [0, C)."""
    rng = np.random.default_rng([2025, 3])
    quads = np.zeros((B_NMS, N_NMS, 4, 2), F)
    scores = np.zeros((B_NMS, N_NMS), F)
    classes = np.zeros((B_NMS, N_NMS), np.int32)
    for b in range(B_NMS):
        objects = N_NMS // 5
        cx, cy = rng.uniform(30, 610, objects), rng.uniform(30, 450, objects)
        w, h, ang = rng.uniform(6, 40, objects), rng.uniform(20, 90, objects), rng.uniform(-90, 90, objects)
        k = 0
        for o in range(objects):
            for _ in range(5):
                j = rng.uniform(-1, 1, 5) * (1.5, 1.5, 1.0, 2.0, 4.0)
                quads[b, k] = pio.rotated_box(cx[o] + j[0], cy[o] + j[1], w[o] + j[2], h[o] + j[3], ang[o] + j[4])
                k += 1
        obj_class = np.where(np.arange(objects) < 24, 0, np.where(np.arange(objects) < 43, 1, 2))      # 120 / 95 / 85
        classes[b] = np.repeat(obj_class, 5)
        scores[b] = rng.uniform(0.02, 1.0, N_NMS).astype(F)
        order = rng.permutation(N_NMS)
        quads[b], scores[b], classes[b] = quads[b][order], scores[b][order], classes[b][order]
    ties = np.flatnonzero(classes[0] == 2)[:5]
    for n, i in enumerate(ties):                               # far from everything: they never decay
        quads[0, i] = square(2000 + 10 * n, 2000, 8)
        scores[0, i] = F(0.625)
    classes[0, 17] = 7
    classes[1, 250] = -1
    kps = rng.uniform(0, 640, (B_NMS, N_NMS, 2, 2)).astype(F)
    return quads, scores, classes, kps


@pytest.fixture(scope='module')
def soft_nms_case():
    """-> inputs and, computed once, the oracle's result per (image, candidates in use)"""
    quads, scores, classes, kps = soft_nms_inputs()
    want = {}
    for b, n in ((0, int(NCAND[0])), (1, int(NCAND[1]))):
        want[b] = pio.soft_nms_image(quads[b, :n], scores[b, :n], classes[b, :n], C_NMS, K_NMS, THR_NMS, kps=kps[b, :n])
        want['all', b] = pio.soft_nms_image(quads[b, :n], scores[b, :n], classes[b, :n], C_NMS, N_NMS, 0.1, kps=kps[b, :n])
    return quads, scores, classes, kps, want


def test_soft_nms_inputs_meet_the_condition_of_the_one_ulp_rule(soft_nms_case):
    """On the oracle alone: any two live scores of an arg-max round are more than 1e-6 apart, relative, or equal bit
    for bit (and then the candidate index decides); the stop and the final order have the same room.  With that a
    last-bit difference of `exp` cannot reorder anything."""
    _, _, classes, _, want = soft_nms_case
    for b in (0, 1):
        m = want[b]['margins']
        print(b, m, want[b]['kept'])
        assert m['gap'] > 1e-6 and m['stop'] > 1e-6 and m['order'] > 1e-6, m
        assert want[b]['kept'] > K_NMS and len(want[b]['index']) == K_NMS
    assert want[0]['margins']['ties'] >= 4                     # the five equal scores of class 2
    assert (classes[0, :NCAND[0]] == 0).sum() > 64 and (classes[0] == 7).sum() == 1


def check_image(got, b, want, K, J):
    n = len(want['index'])
    assert n == min(want['kept'], K)
    assert same_bits(got['boxes'][b, :n], want['boxes']) and same_bits(got['classes'][b, :n], want['classes'])
    if J:
        assert same_bits(got['kps'][b, :n], want['kps']) and not got['kps'][b, n:].any()
    assert_one_ulp(got['scores'][b, :n], want['scores'], 'scores')
    assert int(got['counts'][b]) == want['count']
    assert not got['boxes'][b, n:].any() and not got['scores'][b, n:].any() and (got['classes'][b, n:] == -1).all()


@pytest.mark.parametrize('J', [0, 2])
def test_soft_nms_merge_rotated_equals_the_oracle(soft_nms_case, J):
    import predict
    quads, scores, classes, kps, want = soft_nms_case
    d_kps = G(kps) if J else None
    got = {k: N(v) for k, v in predict.soft_nms_merge_rotated(G(quads), G(scores), G(classes), d_kps, C_NMS, K_NMS, THR_NMS,
                                                              ncand=G(NCAND)).items()}
    assert got['boxes'].shape == (B_NMS, K_NMS, 4, 2) and ('kps' in got) == bool(J)
    check_image(got, 0, want[0], K_NMS, J)                     # cut short by ncand: rows 260.. are never candidates
    check_image(got, 1, want[1], K_NMS, J)
    assert 0 < want[0]['count'] < K_NMS or 0 < want[1]['count'] < K_NMS
    # an image without candidates beside a full one
    none = {k: N(v) for k, v in predict.soft_nms_merge_rotated(G(quads), G(scores), G(classes), d_kps, C_NMS, K_NMS, THR_NMS,
                                                               ncand=G(np.array([0, 300], np.int32))).items()}
    assert none['counts'][0] == 0 and not none['scores'][0].any() and (none['classes'][0] == -1).all()
    assert not none['boxes'][0].any()
    check_image(none, 1, want[1], K_NMS, J)
    # every emitted candidate kept (max_detections = N): the decayed scores and the whole order, not only the best 20
    full = {k: N(v) for k, v in predict.soft_nms_merge_rotated(G(quads), G(scores), G(classes), d_kps, C_NMS, N_NMS, 0.1,
                                                               ncand=G(NCAND)).items()}
    for b in (0, 1):
        assert K_NMS < want['all', b]['kept'] < N_NMS
        check_image(full, b, want['all', b], N_NMS, J)
    if not J:
        with pytest.raises(RuntimeError, match='2048'):
            predict.soft_nms_merge_rotated(torch.zeros((1, 2049, 4, 2), device=DEV), torch.zeros((1, 2049), device=DEV),
                                           torch.zeros((1, 2049), dtype=torch.int32, device=DEV), None, 3, 4, 0.5)
        with pytest.raises(RuntimeError, match=r'\[B, N, 4, 2\]'):
            predict.soft_nms_merge_rotated(G(quads.reshape(B_NMS, N_NMS, 8)), G(scores), G(classes), None, 3, 4, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the predictor: a rotated model at two scales
# ---------------------------------------------------------------------------------------------------------------------
K = 20
IMAGE_SIZES = np.array([[50, 70], [64, 64]], dtype=np.int32)


@pytest.fixture(scope='module')
def backend():
    from backends import resnet
    torch.manual_seed(3)
    return resnet.build(18, num_classes=6, num_keypoints=3, pretrained=False, rotated_boxes=True).to(DEV).eval()


@pytest.fixture(scope='module')
def images():
    rng = np.random.default_rng(21)
    batch = np.zeros((2, 64, 70, 3), np.uint8)
    for b, (h, w) in enumerate(IMAGE_SIZES):
        batch[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return G(batch)


def candidates_by_hand(p, images, size, flip):
    """One scale by hand: the forward (with the mirror pass merged by the numpy oracle when `flip`), the decode, and
    predict.project_detections into source pixels."""
    import predict
    from backends.decode import decode_detection
    from datasets import AugmentParams, augment_images, prepare_input
    from hip_runtime import ops
    params = AugmentParams.identity(IMAGE_SIZES, size)
    x = prepare_input(augment_images(images, params))
    if flip:
        heads = p.model.heads(torch.cat([x, x.flip(-1)]))
        raw = {k: N(v) for k, v in heads.items()}
        prob = N(ops.sigmoid_clamp_(heads['hm'].clone()))
        merged = po.tta_merge(prob, raw['wh'], raw['reg'], raw['kps'], perm=[2, 1, 0])
        hm, wh, reg, kps = (G(merged[k]) for k in ('hm', 'wh', 'reg', 'kps'))
    else:
        heads = p.model.heads(x)
        hm, wh, reg, kps = ops.sigmoid_clamp_(heads['hm'].clone()), heads['wh'], heads['reg'], heads['kps']
    dets, kps = decode_detection(hm, wh, reg, kps=kps, K=K, rotated=True)
    assert tuple(dets.shape) == (2, K, 7)
    return predict.project_detections(dets, kps, G(predict.inverse_matrices(params)), G(IMAGE_SIZES), 0.1, rotated=True,
                                      scale=p.down_ratio)


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_rotated_predictor_with_two_scales_is_the_polygon_merge_of_both_candidate_sets(backend, images, flip):
    import predict
    p = predict.Predictor(backend, (64, 64), max_detections=K, rotated=True, scales=(1.0, 1.5), soft_nms='polygon',
                          flip=flip, flip_pairs=((0, 2),) if flip else None)
    assert p.sizes == [(64, 64), (96, 96)] and p.soft_nms and p.rotated
    out = {k: N(v) for k, v in p(images, IMAGE_SIZES).items()}
    assert out['boxes'].shape == (2, K, 4, 2) and out['kps'].shape == (2, K, 3, 2)
    cand = [candidates_by_hand(p, images, size, flip) for size in p.sizes]
    for b in range(2):
        cat = lambda key: np.concatenate([N(c[key])[b] for c in cand])            # scale-major, then decode rank
        want = pio.soft_nms_image(cat('boxes'), cat('scores'), cat('classes'), 6, K, 0.1, kps=cat('kps'))
        m = want['margins']
        # a random-initialised model scores every cell near 0.5, one float32 step apart: the guard is sized for what
        # can differ between the kernel and numpy, a few units in the last place of a double (tests/test_gpu_predict.py)
        assert m['gap'] > 1e-12 and m['order'] > 1e-12 and m['stop'] > 1e-6, m
        check_image(out, b, want, K, 3)
    one = predict.Predictor(backend, (64, 64), max_detections=K, rotated=True, soft_nms='polygon', flip=flip,
                            flip_pairs=((0, 2),) if flip else None)(images, IMAGE_SIZES)
    assert tuple(one['boxes'].shape) == (2, K, 4, 2)                               # one scale alone is accepted too
    w = pio.soft_nms_image(N(cand[0]['boxes'])[0], N(cand[0]['scores'])[0], N(cand[0]['classes'])[0], 6, K, 0.1)
    assert same_bits(N(one['boxes'])[0, :len(w['index'])], w['boxes'])


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator: rotated_iou = 'polygon'
# ---------------------------------------------------------------------------------------------------------------------
SHAPE = (3, 120, 160)


def eval_batches():
    """Two batches of two images, 12 detections and 5 ground truths each, (cx, cy, w, h, angle) float32, three classes:
    half of the detections are jittered ground truths; image 0 has a thin 3 x 40 box at 30 degrees as ground truth and
    as a slightly shifted detection, and a detection identical to a ground truth."""
    rng = np.random.default_rng(8)
    batches, gid = [], 100
    for _ in range(2):
        pb, pc, ps, gb, gc, ga, ids = [], [], [], [], [], [], []
        for i in range(2):
            gt = np.concatenate([rng.uniform(15, 145, (5, 1)), rng.uniform(15, 105, (5, 1)), rng.uniform(6, 40, (5, 1)),
                                 rng.uniform(10, 60, (5, 1)), rng.uniform(-90, 90, (5, 1))], 1)
            gcls = rng.integers(0, 3, 5)
            if not batches and i == 0:
                gt[0] = (80.3, 60.7, 3, 40, 30)
            src = rng.integers(0, 5, 12)
            det = gt[src] + rng.normal(0, 1, (12, 5)) * (2, 2, 2, 3, 6)
            dcls = gcls[src].copy()
            fresh = rng.uniform(size=12) < 0.4
            det[fresh, :2] = rng.uniform(15, 105, (int(fresh.sum()), 2))
            dcls[fresh] = rng.integers(0, 3, int(fresh.sum()))
            det[:, 2:4] = np.abs(det[:, 2:4]) + 1
            if not batches and i == 0:
                det[0], dcls[0] = (80.9, 60.2, 3, 40, 30), gcls[0]
                det[1], dcls[1] = gt[1], gcls[1]
            pb.append(det.astype(F)), pc.append(dcls.astype(np.int32)), ps.append(rng.uniform(0.05, 1, 12).astype(F))
            gb.append(gt.astype(F)), gc.append(gcls.astype(np.int32)), ga.append((gt[:, 2] * gt[:, 3]).astype(F))
            ids.append(np.int64(gid))
            gid += 1
        batches.append({'pred_boxes': np.stack(pb), 'pred_classes': np.stack(pc), 'pred_scores': np.stack(ps),
                        'gt_boxes': gb, 'gt_classes': gc, 'gt_ids': ids, 'gt_areas': ga, 'image_shape': SHAPE})
    return batches


class PolygonOracle(co.OracleEvaluator):
    """tests/cocoeval_oracle.py's evaluator -- its grouping, matching, accumulation and summary -- with the annotations
    of the rotated mode measured by the restatement: polygon areas, polygon pair IoUs (detection = subject)."""

    def _anno(self, box, label, image_id, score, area, shape):
        from utils.box import rotate_bboxes_float
        quad = rotate_bboxes_float(np.asarray(box, F)[None, :5])[0]
        a = {'image_id': image_id, 'category_id': int(label), 'quad': quad, 'area': pio.quad_area(quad)}
        if score is not None:
            a['score'] = score
        return a

    def per_image(self):
        out = {}
        for key in sorted(set(self.dts) | set(self.gts)):
            dt, gt = self.dts.get(key, []), self.gts.get(key, [])
            order = np.argsort([-d['score'] for d in dt], kind='mergesort')
            dt = [dt[i] for i in order][:co.MAX_DETS[-1]]
            ious = [[pio.quad_iou(d['quad'], g['quad'])[0] for g in gt] for d in dt]
            out[key] = {'dt': dt, 'gt': gt, 'ious': ious,
                        'ranges': [co.evaluate_img(dt, gt, ious, rng) for rng in co.AREA_RANGES]}
        return out


def run_evaluator(mode, oracle):
    from evaluation.coco import Evaluator
    Evaluator._known_ids.clear()
    co.OracleEvaluator._known_ids.clear()
    batches = eval_batches()
    ev = Evaluator()
    ev.use_rotated_boxes = oracle.use_rotated_boxes = True
    ev.rotated_iou = mode
    ev._keep_intermediates = True
    for b in batches:
        ev.add_batch(**b)
        oracle.add_batch(**b)
    seen = [{k: (N(v) if torch.is_tensor(v) else v) for k, v in rec.items()} for rec in ev._batches]
    return batches, seen, ev.evaluate(), oracle, oracle.evaluate()


def assert_scalars(got, want):
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


def test_evaluator_polygon_mode_bits_and_scalars():
    batches, seen, got, o, want = run_evaluator('polygon', PolygonOracle())
    first = pairs = positive = 0
    thin = identical = False
    for rec, b in zip(seen, batches):
        for (d0, nd, g0, ng, p0), (i, c) in zip(rec['groups'], rec['keys']):
            e = o.detail['per_image'][(first + i + 1, int(c))]
            assert nd == len(e['dt']) and ng == len(e['gt'])
            w = np.array(e['ious'], dtype=np.float64).reshape(nd, ng)
            assert same_bits(rec['iou'][p0:p0 + nd * ng].reshape(nd, ng), w), (first, i, c)
            assert same_bits(rec['det_area'][d0:d0 + nd], np.array([d['area'] for d in e['dt']], dtype=np.float64))
            assert same_bits(rec['gt_area'][g0:g0 + ng], np.array([g['area'] for g in e['gt']], dtype=np.float64))
            pairs, positive = pairs + nd * ng, positive + int((w > 0).sum())
            identical = identical or bool((w == 1.0).any())
            thin = thin or any(abs(g['area'] - 120.0) < 1e-3 for g in e['gt'])
        first += len(b['gt_ids'])
    assert pairs >= 40 and 0 < positive < pairs and thin and identical
    assert_scalars(got, want)


def test_evaluator_mask_mode_is_untouched_and_other_values_are_refused():
    """the same detections with `rotated_iou = 'mask'` (the default): the rasterised path, against the oracle it has
    always been held to, and with other pair IoUs than the polygon path"""
    from evaluation.coco import Evaluator
    assert Evaluator().rotated_iou == 'mask'
    _, seen_mask, got, _, want = run_evaluator('mask', co.OracleEvaluator())
    assert_scalars(got, want)
    _, seen_poly, _, _, _ = run_evaluator('polygon', PolygonOracle())
    assert seen_mask[0]['iou'].shape == seen_poly[0]['iou'].shape and not same_bits(seen_mask[0]['iou'], seen_poly[0]['iou'])
    assert np.array_equal(seen_mask[0]['det_area'], np.round(seen_mask[0]['det_area']))           # pixel counts
    ev = Evaluator()
    ev.use_rotated_boxes, ev.rotated_iou = True, 'exact'
    with pytest.raises(ValueError, match='rotated_iou'):
        ev.add_batch(**eval_batches()[0])
    assert not ev.ids and not ev._batches
