"""MI355X: prediction over images (predict.py, csrc/predict.hip) against the numpy oracle of tests/predict_oracle.py:
the mirror merge bit for bit, the projection and the soft-NMS merge to one float32 unit in the last place (the kernels
work in double like the oracle; a last-bit difference of a double sin, cos, exp or product can move a float32 rounding
by one unit and no more), and the whole path -- plain, mirrored, two scales, the command line -- against the same
steps taken by hand."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import coco_fixture as fx
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
    """got (float32) equals the float64 oracle rounded to float32, within one float32 unit in the last place."""
    got, want = np.asarray(got), np.asarray(want64).astype(F)
    assert got.dtype == F and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
    assert not bad.any(), (what, got[bad][:4], want[bad][:4])


# ---------------------------------------------------------------------------------------------------------------------
# mirror and merge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wh_ch', [2, 3], ids=['axis', 'rotated'])
@pytest.mark.parametrize('W', [7, 65])
def test_mirror_and_merge_are_bit_exact(W, wh_ch):
    import predict
    from hip_runtime import ops
    B, C, H, J = 2, 3, 5, 3
    rng = np.random.default_rng([11, W, wh_ch])
    x = rng.normal(0, 1, (B, 3, H, W)).astype(F)
    assert same_bits(N(predict.mirror_input(G(x))), x[..., ::-1])
    into = torch.full((2 * B, 3, H, W), 7.0, device=DEV)
    into[:B] = G(x)
    predict.mirror_input(into[:B], out=into[B:])
    assert same_bits(N(into), np.concatenate([x, x[..., ::-1]]))
    hm = rng.normal(0, 3, (2 * B, C, H, W)).astype(F)
    hm[0, 0, 0, :2] = (-20.0, 20.0)                     # both clamps
    wh = rng.uniform(-2, 30, (2 * B, wh_ch, H, W)).astype(F)
    reg = rng.uniform(0, 1, (2 * B, 2, H, W)).astype(F)
    kps = rng.normal(0, 9, (2 * B, 2 * J, H, W)).astype(F)
    perm = predict.flip_permutation(((0, 2),), J)
    prob = N(ops.sigmoid_clamp_(G(hm)))                 # (in place on its own copy of the logits)
    assert prob.min() == F(1e-4) and prob.max() == F(1.0) - F(1e-4)
    got = predict.tta_merge({'hm': G(hm), 'wh': G(wh), 'reg': G(reg), 'kps': G(kps)}, G(perm))
    want = po.tta_merge(prob, wh, reg, kps, perm)
    assert sorted(got) == ['hm', 'kps', 'reg', 'wh']
    for k in want:
        assert same_bits(N(got[k]), want[k]), k
    # no keypoint head, no permutation: the identity
    got = predict.tta_merge({'hm': G(hm), 'wh': G(wh), 'reg': G(reg)})
    assert sorted(got) == ['hm', 'reg', 'wh'] and all(same_bits(N(got[k]), want[k]) for k in got)
    got = predict.tta_merge({'hm': G(hm), 'wh': G(wh), 'reg': G(reg), 'kps': G(kps)})
    assert same_bits(N(got['kps']), po.tta_merge(prob, wh, reg, kps)['kps'])


# ---------------------------------------------------------------------------------------------------------------------
# projection
# ---------------------------------------------------------------------------------------------------------------------
THR = 0.3
SIZES = np.array([[48, 64], [60, 40]], dtype=np.int32)
MATRIX = np.array([[1.37, 0.0, 0.0, 0.0, 0.77, 0.0],              # diagonal
                   [0.9, 0.35, -3.2, -0.2, 1.1, 4.7]])            # sheared


@pytest.mark.parametrize('rotated', [False, True], ids=['axis', 'rotated'])
def test_projection_matches_the_float64_oracle(rotated):
    import predict
    B, K, J = 2, 5, 2
    rng = np.random.default_rng(5)
    if rotated:
        geo = F([[20.5, 18.25, 9.5, 14.75], [2.5, 30.1, 12.3, 40.9], [220.1, 300.2, 20.3, 30.4],
                 [31.0, 7.0, 5.0, 9.0], [12.0, 12.0, 3.5, 3.5]])
        angle = F([[33.3], [-71.2], [90.0], [0.0], [-180.0]])
        geo = np.concatenate([geo, angle], 1)
    else:
        geo = F([[10.5, 8.25, 30.75, 20.5],             # inside
                 [-5.5, 12.1, 18.3, 70.9],              # straddles the border
                 [200.1, 300.2, 240.3, 330.4],          # outside
                 [31.0, 7.0, 36.0, 16.0], [12.0, 12.0, 15.5, 15.5]])
    scores = F([[0.9, 0.6, F(THR), 0.2, 0.1],           # one score equals the threshold: kept
                [0.29, 0.2, 0.1, 0.05, 0.01]])          # nothing above it
    classes = F([[3, 0, 5, 1, 1], [2, 2, 0, 4, 1]])
    dets = np.concatenate([np.stack([geo, geo[::-1]]), scores[..., None], classes[..., None]], 2).astype(F)
    kps = rng.uniform(-10, 80, (B, K, J, 2)).astype(F)
    want = po.project(dets, kps, MATRIX, SIZES, THR, rotated)
    assert want['counts'].tolist() == [3, 0]
    got = predict.project_detections(G(dets), G(kps), G(MATRIX), G(SIZES), THR, rotated)
    assert N(got['counts']).tolist() == [3, 0] and got['counts'].dtype == torch.int32
    assert same_bits(N(got['classes']), want['classes']) and same_bits(N(got['scores']), want['scores'])
    assert tuple(got['boxes'].shape) == ((B, K, 4, 2) if rotated else (B, K, 4))
    assert_one_ulp(N(got['boxes']), want['boxes'], 'boxes')
    assert_one_ulp(N(got['kps']), want['kps'], 'kps')
    if not rotated:
        b = N(got['boxes'])
        assert b[0, 2].tolist() == [64, 48, 64, 48]      # outside: collapses onto the corner (w, h)
        assert b[0, 1, 0] == 0.0 and b[0, 1, 3] == 48.0
    # without keypoints, and through the one-copy buffer
    bare = predict.project_detections(G(dets), None, G(MATRIX), G(SIZES), THR, rotated)
    assert 'kps' not in bare and same_bits(N(bare['boxes']), N(got['boxes']))
    back = predict.unpack_result(N(got['packed']), B, K, J, rotated)
    assert all(same_bits(back[k], N(got[k])) for k in ('boxes', 'scores', 'classes', 'counts', 'kps'))


# ---------------------------------------------------------------------------------------------------------------------
# soft-NMS merge
# ---------------------------------------------------------------------------------------------------------------------
def clustered(seed, groups=6, width=64, height=48):
    rng = np.random.default_rng([2024, seed])
    W, H, Gn = width, height, groups
    cx, cy = rng.uniform(8, W - 8, Gn), rng.uniform(8, H - 8, Gn)
    w, h = rng.uniform(6, 24, Gn), rng.uniform(6, 24, Gn)
    base = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    boxes = (base[:, None] + rng.uniform(-0.5, 0.5, (Gn, 5, 4))).reshape(-1, 4).astype(np.float32)
    scores = rng.uniform(0.02, 1.0, 5 * Gn).astype(np.float32)
    return boxes, scores


def assert_margins(m, ties=0):
    """Guards, asserted on the oracle alone: with them a last-bit difference cannot flip a decision."""
    assert m['gap'] > 1e-6 and m['stop'] > 1e-6 and m['order'] > 1e-6 and m['ties'] == ties, m


def check_image(got, b, want, K):
    n = len(want['index'])
    assert n == min(want['kept'], K)
    assert same_bits(got['boxes'][b, :n], want['boxes']) and same_bits(got['classes'][b, :n], want['classes'])
    if 'kps' in want:
        assert same_bits(got['kps'][b, :n], want['kps'])
        assert not got['kps'][b, n:].any()
    assert_one_ulp(got['scores'][b, :n], want['scores'], 'scores')
    assert int(got['counts'][b]) == want['count']
    assert not got['boxes'][b, n:].any() and not got['scores'][b, n:].any() and (got['classes'][b, n:] == -1).all()


def test_soft_nms_on_the_clustered_recipe():
    import predict
    B, Nc, K, J = 5, 30, 30, 2
    rng = np.random.default_rng(77)
    boxes, scores = map(np.stack, zip(*[clustered(seed) for seed in range(B)]))
    kps = rng.uniform(0, 64, (B, Nc, J, 2)).astype(F)
    classes = np.zeros((B, Nc), np.int32)
    want = [po.soft_nms_image(boxes[b], scores[b], classes[b], 1, K, 0.1, kps=kps[b]) for b in range(B)]
    for w in want:
        assert_margins(w['margins'])
    assert [w['kept'] for w in want] == [23, 24, 22, 22, 23]
    got = {k: N(v) for k, v in predict.soft_nms_merge(G(boxes), G(scores), G(classes), G(kps), 1, K, 0.1).items()}
    for b in range(B):
        check_image(got, b, want[b], K)


def test_soft_nms_edge_cases():
    """130 candidates of one class (more than two waves), one candidate of a class, exact ties, max_detections below the
    kept count, two images with different N (what lies past an image's count is never read as a candidate), N = 0."""
    import predict
    C, K, stride = 3, 40, 160
    boxes, scores, classes, ncand, want0, want1 = edge_case_inputs(C, K, stride)
    got = {k: N(v) for k, v in predict.soft_nms_merge(G(boxes), G(scores), G(classes), None, C, K, 0.5,
                                                      ncand=G(ncand)).items()}
    check_image(got, 0, want0, K)
    check_image(got, 1, want1, K)
    tied = [i for i in range(K) if got['classes'][0, i] == 2]
    assert [got['boxes'][0, i, 0] for i in tied] == [0.0, 10.0, 20.0, 30.0, 40.0]       # lower candidate index first
    # an image without candidates, by count and by shape
    none = {k: N(v) for k, v in predict.soft_nms_merge(G(boxes), G(scores), G(classes), None, C, K, 0.5,
                                                       ncand=G(np.array([0, 30], np.int32))).items()}
    assert none['counts'][0] == 0 and not none['scores'][0].any() and (none['classes'][0] == -1).all()
    check_image(none, 1, want1, K)
    empty = predict.soft_nms_merge(torch.zeros((1, 0, 4), device=DEV), torch.zeros((1, 0), device=DEV),
                                   torch.zeros((1, 0), dtype=torch.int32, device=DEV), None, C, 4, 0.5)
    assert N(empty['counts']).tolist() == [0] and (N(empty['classes']) == -1).all() and not N(empty['boxes']).any()
    with pytest.raises(RuntimeError, match='2048'):
        predict.soft_nms_merge(torch.zeros((1, 2049, 4), device=DEV), torch.zeros((1, 2049), device=DEV),
                               torch.zeros((1, 2049), dtype=torch.int32, device=DEV), None, C, 4, 0.5)


def edge_case_inputs(C, K, stride):
    """-> boxes, scores, classes [2, stride, ...], ncand, and the oracle's result per image (margins asserted)."""
    big_boxes, big_scores = clustered(9, groups=26, width=160, height=120)            # 130, class 0
    one_box, one_score = F([[3, 3, 9, 9]]), F([0.4321])                               # class 1
    tie_boxes = F([[10 * i, 200, 10 * i + 8, 208] for i in range(5)])                 # class 2: disjoint, equal scores
    tie_scores = np.full(5, 0.625, F)
    boxes0 = np.concatenate([big_boxes[:70], tie_boxes[:2], one_box, big_boxes[70:], tie_boxes[2:]])
    scores0 = np.concatenate([big_scores[:70], tie_scores[:2], one_score, big_scores[70:], tie_scores[2:]])
    classes0 = np.concatenate([np.zeros(70), np.full(2, 2), [1], np.zeros(60), np.full(3, 2)]).astype(np.int32)
    n0 = len(scores0)
    assert n0 == 136
    boxes1, scores1 = clustered(0)
    boxes = np.zeros((2, stride, 4), F)
    scores = np.full((2, stride), 0.99, F)              # past the counts: would win every round if it were read
    classes = np.zeros((2, stride), np.int32)
    boxes[:, :] = F([1, 1, 50, 50])
    boxes[0, :n0], scores[0, :n0], classes[0, :n0] = boxes0, scores0, classes0
    boxes[1, :30], scores[1, :30], classes[1, :30] = boxes1, scores1, 1
    classes[1, 7] = 3                                   # a class outside [0, C): ignored
    ncand = np.array([n0, 30], np.int32)
    want0 = po.soft_nms_image(boxes0, scores0, classes0, C, K, 0.5)
    # ties: five equal scores in class 2, nothing decays (disjoint): the index decides in four rounds
    assert_margins(want0['margins'], ties=4)
    assert want0['kept'] > K and len(want0['index']) == K
    keep1 = np.arange(30) != 7
    want1 = po.soft_nms_image(boxes1[keep1], scores1[keep1], np.ones(29, int), C, K, 0.5)
    assert_margins(want1['margins'])
    assert want1['kept'] < K
    return boxes, scores, classes, ncand, want0, want1


# ---------------------------------------------------------------------------------------------------------------------
# the whole path
# ---------------------------------------------------------------------------------------------------------------------
K = 20
IMAGE_SIZES = np.array([[50, 70], [64, 64]], dtype=np.int32)


@pytest.fixture(scope='module')
def backend():
    from backends import resnet
    torch.manual_seed(3)
    return resnet.build(18, num_classes=6, num_keypoints=3, pretrained=False).to(DEV).eval()


@pytest.fixture(scope='module')
def images():
    rng = np.random.default_rng(21)
    batch = np.zeros((2, 64, 70, 3), np.uint8)
    for b, (h, w) in enumerate(IMAGE_SIZES):
        batch[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return G(batch)


def prepared(images, size):
    from datasets import AugmentParams, augment_images, prepare_input
    params = AugmentParams.identity(IMAGE_SIZES, size)
    return params, prepare_input(augment_images(images, params))


def by_hand(backend, images, size, threshold=0.1):
    """export.CenterNet on the prepared input (input pixels), projected by the oracle."""
    import predict
    from export import CenterNet
    params, x = prepared(images, size)
    boxes, scores, classes, kps = CenterNet(backend, K).eval()(x)
    dets = np.concatenate([N(boxes), N(scores)[..., None], N(classes)[..., None]], 2).astype(F)
    return dets, N(kps), predict.inverse_matrices(params), po.project(dets, N(kps), predict.inverse_matrices(params),
                                                                     IMAGE_SIZES, threshold)


def check_projected(out, want):
    assert same_bits(N(out['scores']), want['scores']) and same_bits(N(out['classes']), want['classes'])
    assert same_bits(N(out['counts']), want['counts'])
    assert_one_ulp(N(out['boxes']), want['boxes'], 'boxes')
    assert_one_ulp(N(out['kps']), want['kps'], 'kps')


def test_predictor_without_options_is_the_export_wrapper_projected(backend, images):
    import predict
    p = predict.Predictor(backend, (64, 64), max_detections=K)
    assert not p.flip and not p.soft_nms and p.num_keypoints == 3 and p.num_classes == 6
    out = p(images, IMAGE_SIZES)
    want = by_hand(backend, images, (64, 64))[3]
    assert tuple(out['boxes'].shape) == (2, K, 4) and tuple(out['kps'].shape) == (2, K, 3, 2)
    check_projected(out, want)
    assert (N(out['boxes'])[0, :, 2] <= 70).all() and (N(out['boxes'])[0, :, 3] <= 50).all()
    # a threshold between the scores: counts is the prefix
    s = N(out['scores'])
    mid = float(s[0, K // 2])
    cut = predict.Predictor(backend, (64, 64), max_detections=K, score_threshold=mid)(images, IMAGE_SIZES)
    assert N(cut['counts']).tolist() == [(s[b] >= F(mid)).sum() for b in range(2)] and N(cut['counts'])[0] >= K // 2 + 1


def test_predictor_with_flip_is_the_merged_double_batch(backend, images):
    import predict
    from backends.decode import decode_detection
    from hip_runtime import ops
    p = predict.Predictor(backend, (64, 64), max_detections=K, flip=True, flip_pairs=((0, 2),))
    out = p(images, IMAGE_SIZES)
    params, x = prepared(images, (64, 64))
    heads = p.model.heads(torch.cat([x, x.flip(-1)]))
    assert heads['hm'].shape[0] == 4
    raw = {k: N(v) for k, v in heads.items()}
    prob = N(ops.sigmoid_clamp_(heads['hm'].clone()))
    merged = po.tta_merge(prob, raw['wh'], raw['reg'], raw['kps'], perm=[2, 1, 0])
    dets, kps = decode_detection(G(merged['hm']), G(merged['wh']), G(merged['reg']), kps=G(merged['kps']), K=K)
    dets, kps = N(dets), N(kps) * F(backend.down_ratio)
    dets[:, :, :4] *= F(backend.down_ratio)
    want = po.project(dets, kps, predict.inverse_matrices(params), IMAGE_SIZES, 0.1)
    check_projected(out, want)
    plain = predict.Predictor(backend, (64, 64), max_detections=K)(images, IMAGE_SIZES)
    assert not same_bits(N(plain['scores']), N(out['scores']))          # the mirror pass really changed the maps


def test_predictor_with_two_scales_is_soft_nms_over_both_candidate_sets(backend, images):
    import predict
    p = predict.Predictor(backend, (64, 64), max_detections=K, scales=(1.0, 1.5))
    assert p.sizes == [(64, 64), (96, 96)] and p.soft_nms
    out = {k: N(v) for k, v in p(images, IMAGE_SIZES).items()}
    cand = []
    for size in p.sizes:
        dets, kps, matrix, _ = by_hand(backend, images, size)
        cand.append(predict.project_detections(G(dets), G(kps), G(matrix), G(IMAGE_SIZES), 0.1))
    for b in range(2):
        cat = lambda key: np.concatenate([N(c[key])[b] for c in cand])            # scale-major, then decode rank
        want = po.soft_nms_image(cat('boxes'), cat('scores'), cat('classes'), 6, K, 0.1, kps=cat('kps'))
        m = want['margins']
        # a random-initialised model scores every cell near 0.5, one float32 step apart: the guard is sized for what
        # can differ between the kernel and numpy, a few units in the last place of a double
        assert m['gap'] > 1e-12 and m['order'] > 1e-12 and m['stop'] > 1e-6, m
        check_image(out, b, want, K)


def test_command_line_writes_the_records_of_predict_files(tmp_path, backend):
    import export
    import predict
    from utils.helper import save_model
    run = tmp_path / 'run'
    (run / '.hydra').mkdir(parents=True)
    spec = {'name': 'resnet', 'params': {'num_layers': 18, 'num_classes': 6, 'num_keypoints': 3, 'rotated_boxes': False,
                                         'pretrained': False}}
    cfg = {'model': {'backend': spec}, 'datasets': {'validation': {'params': {'input_size': [64, 64]}}},
           'normalize': {'mean': list(predict.MEAN), 'std': list(predict.STD)}, 'max_detections': K,
           'score_threshold': 0.1, 'batch_size': 3, 'num_workers': 2, 'gpu': 0}
    (run / '.hydra' / 'config.yaml').write_text(yaml.safe_dump(cfg))
    save_model(backend, run / 'model_last.pth', epoch=1)
    files = fx.write_images(str(tmp_path / 'pictures'), 4)
    out = tmp_path / 'results.json'
    summary = predict.main([str(run), str(tmp_path / 'pictures'), '--out', str(out), '--flip', '--flip-pairs', '0-2'])
    assert summary['images'] == 4 and summary['images_per_second'] > 0
    written = json.loads(out.read_text())
    assert written and {d['image_id'] for d in written} == {1, 2, 3, 4} and len(written[0]['keypoints']) == 9
    again = export.build_model(run, spec, True, K).to(DEV).eval()
    p = predict.Predictor(again, (64, 64), max_detections=K, flip=True, flip_pairs=((0, 2),))
    paths = predict.expand_files([str(tmp_path / 'pictures')])
    assert [os.path.basename(f) for f in paths] == sorted(name for name, _, _ in files)
    records = list(predict.predict_files(p, paths, batch_size=3, num_workers=0, device=torch.device(DEV)))
    assert [r['file'] for r in records] == paths and [r['index'] for r in records] == [0, 1, 2, 3]
    assert all(r['boxes'].shape == (len(r['scores']), 4) and r['kps'].shape == (len(r['scores']), 3, 2) for r in records)
    assert predict.coco_results(records) == written
