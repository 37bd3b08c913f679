"""MI355X: the keypoint and rotated modes of datasets.encode_targets against tests/targets_modes_oracle.py, the round
trip through decode_detection, and the encoded batch as DetectionLoss input.

One shape for every case: B = 3, C = 3, map 24 x 40 (H != W), M = 8, J = 5, counts (0, 5, 8)."""
import functools

import numpy as np
import pytest
import torch

import targets_modes_oracle as tmo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, C, H, W, M, J = 3, 3, 24, 40, 8, 5
COUNTS = (0, 5, 8)
SEED = 172                                                              # chosen on the oracle alone: check_inputs
MODES = {'keypoints': (False, True), 'rotated': (True, False), 'rotated_keypoints': (True, True)}
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def _corners(cx, cy, w, h, angle):
    t = np.radians(angle)
    c, s = np.cos(t), np.sin(t)
    half = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]])
    return np.array([cx, cy]) + half @ np.array([[c, s], [-s, c]])


@functools.lru_cache(maxsize=None)
def inputs(seed=SEED):
    """Rotated rectangles (some reach over the map's edge and are clipped into general quadrilaterals), their
    axis-aligned boxes, classes, keypoints around the map (y between H and W included), visibility 0 / 1 / 2, areas."""
    rs = np.random.RandomState(seed)
    corners, boxes = np.zeros((B, M, 4, 2)), np.zeros((B, M, 4))
    classes = rs.randint(0, C, (B, M)).astype(np.int32)
    for b in range(B):
        for k in range(M):
            cx, cy = rs.uniform(1, W - 2), rs.uniform(1, H - 2)
            w = rs.uniform(2, 7)
            h = w + rs.uniform(1.5, 9)
            corners[b, k] = _corners(cx, cy, w, h, rs.uniform(-90, 90))
            boxes[b, k] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    # image 2: slots 0 and 1 are one class and three cells apart (overlapping gaussians); slot 3 is degenerate in both
    # modes (every point left of the map: clipped onto x = 0, and a box of no width) in the middle of the list
    corners[2, 1] = corners[2, 0] + (3.0, 0.0)
    boxes[2, 1] = boxes[2, 0] + (3.0, 0.0, 3.0, 0.0)
    classes[2, 1] = classes[2, 0]
    corners[2, 3] = [(-5, 3), (-2, 10), (-8, 20), (-1, 15)]
    boxes[2, 3] = (-6.0, 3.0, -1.0, 20.0)
    keypoints = rs.uniform(-3, W + 3, (B, M, J, 2))
    visibility = rs.randint(0, 3, (B, M, J)).astype(np.int32)
    areas = np.full((B, M), np.nan, np.float32)
    areas[1, 2], areas[2, 5] = 77.25, 31.5                              # the others have no "area"
    return dict(corners=corners, boxes=boxes, classes=classes, keypoints=keypoints, visibility=visibility, areas=areas)


@functools.lru_cache(maxsize=None)
def oracle(mode, seed=SEED):
    rot, kp = MODES[mode]
    d = inputs(seed)
    per_image = []
    for b in range(B):
        n = COUNTS[b]
        per_image.append(tmo.encode_targets_modes(
            d['classes'][b, :n], C, H, W, M, corners=d['corners'][b, :n] if rot else None,
            boxes=None if rot else d['boxes'][b, :n], keypoints=d['keypoints'][b, :n] if kp else None,
            visibility=d['visibility'][b, :n] if kp else None, areas=d['areas'][b, :n]))
    out = {k: np.stack([im[k] for im in per_image]) for k in per_image[0] if not k.startswith('_')}
    return out, [im['_radius_args'] for im in per_image]


def _encode(mode):
    from datasets import encode_targets
    rot, kp = MODES[mode]
    d = inputs()
    g = lambda k: T(d[k]).to(DEV)
    return encode_targets(None if rot else g('boxes'), g('classes'), torch.tensor(COUNTS, dtype=torch.int32, device=DEV),
                          C, H, W, corners=g('corners') if rot else None, keypoints=g('keypoints') if kp else None,
                          visibility=g('visibility') if kp else None, areas=g('areas'))


@pytest.fixture(scope='module')
def encoded():
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = _encode(mode)
        return {k: v.clone() for k, v in cache[mode].items()}
    return get


def _angle_diff(a, b):
    return np.abs((a.astype(np.float64) - b + 90.0) % 180.0 - 90.0)


@pytest.mark.parametrize('mode', sorted(MODES))
def test_inputs_keep_clear_of_tie_breaks(mode):
    """Judged on the oracle alone: a centre next to an integer, w next to h or a radius argument next to an integer
    could turn a last-bit difference into another cell, a swapped pair of sides or another radius."""
    check_inputs(mode, SEED)


def check_inputs(mode, seed):
    want, radius_args = oracle(mode, seed)
    valid = want['reg_mask'].astype(bool)
    np.testing.assert_array_equal(valid.sum(1), [0, 5, 7])              # the degenerate slot of image 2 is skipped
    assert not valid[2, 3] and valid[2, 4:].all()
    reg = want['reg'][valid]
    assert reg.min() >= 0.01 and reg.max() <= 0.99
    assert np.abs(want['wh'][valid][:, 0] - want['wh'][valid][:, 1]).min() >= 1e-3
    for img in radius_args:
        for h, w in img.values():
            assert min(abs(h - round(h)), abs(w - round(w))) >= 1e-3
    for b in range(B):                                                  # the round trip needs one object per cell
        assert len(set(want['ind'][b][valid[b]])) == valid[b].sum()
    assert want['ind'][2, 1] - want['ind'][2, 0] == 3 and want['gt_dets'][2, 0, -1] == want['gt_dets'][2, 1, -1]
    if 'kp_reg_mask' in want:
        m = want['kp_reg_mask'][valid]
        assert 0 < m.sum() < m.size
        ys = inputs(seed)['keypoints'][..., 1][valid]
        assert ((ys >= H) & (ys < W)).any()                             # the y-against-width rule is exercised


@pytest.mark.parametrize('mode', sorted(MODES))
def test_modes_match_the_oracle(encoded, mode):
    rot, kp = MODES[mode]
    want, _ = oracle(mode)
    out = encoded(mode)
    assert out['reg_mask'].dtype == torch.uint8 and out['ind'].dtype == torch.int64
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert sorted(got) == sorted(want)
    assert got['wh'].shape == (B, M, 3 if rot else 2) and got['gt_dets'].shape == (B, M, 7 if rot else 6)
    for key in ('reg_mask', 'ind') + (('kp_reg_mask',) if kp else ()):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for key in ('wh', 'reg', 'gt_dets', 'gt_areas') + (('kps', 'gt_kps') if kp else ()):
        g, w = got[key].copy(), want[key].copy()
        if rot and key in ('wh', 'gt_dets'):                            # the angle is a direction: modulo 180
            col = 2 if key == 'wh' else 4
            err = _angle_diff(g[..., col], w[..., col])
            print(mode, key, 'angle max error', err.max())
            assert err.max() <= 1e-4
            g[..., col] = w[..., col] = 0
        print(mode, key, 'max error', np.abs(g - w).max())
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-4, err_msg=key)
    print(mode, 'hm max error', np.abs(got['hm'] - want['hm']).max())
    np.testing.assert_allclose(got['hm'], want['hm'], rtol=0, atol=1.2e-7)
    assert np.array_equal(got['hm'] == 1.0, want['hm'] == 1.0)
    # areas: the given ones are taken as they are, NaN falls back to w * h
    assert got['gt_areas'][1, 2] == np.float32(77.25) and got['gt_areas'][2, 5] == np.float32(31.5)
    assert not np.isnan(got['gt_areas']).any()
    # the skipped object's rows are zero
    for key in got:
        if key != 'hm':
            assert not got[key][2, 3].any(), key


def test_two_runs_are_bit_identical(encoded):
    first = encoded('rotated_keypoints')
    again = _encode('rotated_keypoints')
    for k in first:
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k


def test_round_trip_through_decode(encoded):
    """Scatter wh, reg and kps into maps at ind, decode with the encoded heat map: the detections with score 1 are the
    valid objects.  Decode adds the sub-pixel centre xs = x + reg to the keypoint offsets (backends/decode.py:69-74,
    the reference's own arithmetic), and the encoder stores offsets from the INTEGER centre (coco.py:221-222), so the
    decoded keypoints are gt_kps + reg of their object, not gt_kps: max |decoded - gt_kps| over this batch equals
    max(reg) (0.987), while decoded - reg matches gt_kps within the 1e-4 asserted below."""
    from backends.decode import decode_detection
    out = encoded('rotated_keypoints')
    ind, valid = out['ind'], out['reg_mask'].bool()

    def scatter(rows):
        ch = rows.shape[2]
        m = torch.zeros((B, ch, H * W), dtype=torch.float32, device=DEV)
        for b in range(B):
            m[b][:, ind[b][valid[b]]] = rows[b][valid[b]].t()
        return m.view(B, ch, H, W)

    dets, kps = decode_detection(out['hm'], scatter(out['wh']), scatter(out['reg']), kps=scatter(out['kps']), K=M,
                                 rotated=True)
    dets, kps = dets.cpu().numpy(), kps.cpu().numpy()
    gt, gt_kps, reg = out['gt_dets'].cpu().numpy(), out['gt_kps'].cpu().numpy(), out['reg'].cpu().numpy()
    valid, ind = valid.cpu().numpy(), ind.cpu().numpy()
    assert dets.shape == (B, M, 7) and kps.shape == (B, M, J, 2)
    worst = worst_kp = literal = 0.0
    for b in range(B):
        found = {}
        for k in range(M):
            if dets[b, k, 5] == 1.0:
                found[(int(dets[b, k, 6]), int(dets[b, k, 1]) * W + int(dets[b, k, 0]))] = k
        assert len(found) == valid[b].sum()
        for k in np.nonzero(valid[b])[0]:
            d = found[(int(gt[b, k, 6]), int(ind[b, k]))]
            worst = max(worst, np.abs(dets[b, d][[0, 1, 2, 3, 5, 6]] - gt[b, k][[0, 1, 2, 3, 5, 6]]).max())
            worst_kp = max(worst_kp, np.abs(kps[b, d] - reg[b, k] - gt_kps[b, k]).max())
            literal = max(literal, np.abs(kps[b, d] - gt_kps[b, k]).max())
    print('round trip: boxes', worst, 'keypoints minus reg', worst_kp, 'keypoints as decoded', literal, 'max reg', reg.max())
    assert worst <= 1e-4
    assert worst_kp <= 1e-4


def test_encoded_batch_feeds_the_periodic_keypoint_loss(encoded):
    from losses.centernet import DetectionLoss
    batch = encoded('rotated_keypoints')
    g = torch.Generator().manual_seed(0)
    pred = {k: torch.randn(B, ch, H, W, generator=g).to(DEV).requires_grad_() for k, ch in
            (('hm', C), ('wh', 3), ('reg', 2), ('kps', 2 * J))}
    crit = DetectionLoss(1.0, 0.1, 1.0, kp_weight=1.0, kp_indices=[[0, 1], [1, 2]], periodic=True)
    leaves = dict(pred)                                                 # the loss swaps its clamped sigmoid into pred['hm']
    loss, stats = crit(pred, batch)
    loss.backward()
    assert torch.isfinite(loss.detach()) and float(stats['hm_loss']) > 0
    for k, p in leaves.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    assert leaves['kps'].grad.abs().sum() > 0 and leaves['wh'].grad.abs().sum() > 0


def test_refusals():
    from datasets import encode_targets
    d = inputs()
    g = lambda k: T(d[k]).to(DEV)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='not both'):
        encode_targets(g('boxes'), g('classes'), counts, C, H, W, corners=g('corners'))
    with pytest.raises(RuntimeError, match='together'):
        encode_targets(g('boxes'), g('classes'), counts, C, H, W, keypoints=g('keypoints'))
    with pytest.raises(RuntimeError, match='together'):
        encode_targets(None, g('classes'), counts, C, H, W, corners=g('corners'), visibility=g('visibility'))
    with pytest.raises(RuntimeError, match='corners must be'):
        encode_targets(None, g('classes'), counts, C, H, W, corners=g('corners').reshape(B, M, 8))
    with pytest.raises(RuntimeError, match='do not match'):
        encode_targets(None, g('classes')[:, :-1], counts, C, H, W, corners=g('corners'))
    with pytest.raises(RuntimeError, match='keypoints must be'):
        encode_targets(None, g('classes'), counts, C, H, W, corners=g('corners'), keypoints=g('keypoints')[:, 1:],
                       visibility=g('visibility'))
    with pytest.raises(RuntimeError, match='visibility'):
        encode_targets(None, g('classes'), counts, C, H, W, corners=g('corners'), keypoints=g('keypoints'),
                       visibility=g('visibility')[..., :-1])
    with pytest.raises(RuntimeError, match='areas must be'):
        encode_targets(g('boxes'), g('classes'), counts, C, H, W, areas=g('areas')[:1])
    with pytest.raises(RuntimeError, match='MI355X only'):
        encode_targets(None, g('classes'), counts, C, H, W, corners=T(d['corners']))
    with pytest.raises(RuntimeError, match='MI355X only'):
        encode_targets(g('boxes'), g('classes'), counts, C, H, W, keypoints=g('keypoints'),
                       visibility=T(d['visibility']))


def test_positional_call_is_unchanged_and_counts_are_clamped():
    """The plain call and boxes with keyword arguments are one route: the same single encoder kernel, the same bytes;
    a count above M is clamped; cnuda_encode_targets called directly gives those bytes too."""
    import hip_runtime as hr
    from datasets import encode_targets
    d = inputs()
    g = lambda k: T(d[k]).to(DEV)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    with hr.launch_log() as log:
        plain = encode_targets(g('boxes'), g('classes'), counts, C, H, W)
    nan = torch.full((B, M), float('nan'), device=DEV)
    with hr.launch_log() as log_modes:
        modes = encode_targets(g('boxes'), g('classes'), counts, C, H, W, areas=nan)
        over = encode_targets(g('boxes'), g('classes'), counts + torch.tensor([0, 0, 5], dtype=torch.int32, device=DEV),
                              C, H, W, areas=nan)
    assert len(log.names) == 1 and 'encode_targets_kernel<false>' in log.names[0], log.names
    assert log_modes.names == log.names and log.counts[log.names[0]] == 1 and log_modes.counts[log.names[0]] == 2
    for k in plain:
        assert torch.equal(plain[k], modes[k]) and torch.equal(plain[k], over[k]), k
    order = ('hm', 'reg_mask', 'ind', 'wh', 'reg', 'gt_dets', 'gt_areas')
    assert sorted(plain) == sorted(order)
    raw = {k: torch.full_like(v, 7) for k, v in plain.items()}                  # every output is fully overwritten
    boxes, classes = g('boxes'), g('classes')                                  # float64 / int32, contiguous
    hr.check(hr.lib().cnuda_encode_targets(hr.ptr(boxes), hr.ptr(classes), hr.ptr(counts), *(hr.ptr(raw[k]) for k in order),
                                           B, C, H, W, M, hr.stream()), 'encode_targets')
    for k in plain:
        assert torch.equal(plain[k], raw[k]), k
