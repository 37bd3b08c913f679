"""MI355X: cnuda_render_detections and the Visualizer on top of it against tests/visualize_oracle.py (pinned by hand in
tests/test_host_visualize.py), byte for byte.  The shapes are the smallest that reach every path of the kernel: the
tile is 64 x 16 output pixels, a thread holds four columns; W % 4 == 0 selects 16-byte loads, W % 2 == 0 dword stores."""
import types

import numpy as np
import pytest
import torch

import visualize_oracle as vo
from utils import visualize as uv

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN, STD = (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835)
KERNEL = 'render_detections_kernel'


def _input(B, H, W, seed):
    """normalised values whose pixels span below 0 to above 255: (-2 * 0.28 + 0.41) < 0, (2.6 * 0.27 + 0.45) > 1"""
    return np.random.RandomState(seed).uniform(-2.0, 2.6, (B, 3, H, W)).astype(np.float32)


def _atlas(seed=3, G=6, gh=7, gw=5):
    """random coverage with whole glyph rows of 0 and of 255; neither side of the cell is a multiple of four"""
    a = np.random.RandomState(seed).randint(0, 256, (G, gh, gw)).astype(np.uint8)
    a[:, 0, :], a[:, 1, :] = 0, 255
    return a


def _render(x, index, first, prims, atlas=None):
    """one launch through utils.visualize.render, checked to be the new kernel -> numpy"""
    import hip_runtime as hr
    with hr.launch_log() as log:
        got = uv.render(torch.from_numpy(x).to(DEV), index, first, prims, MEAN, STD,
                        None if atlas is None else torch.from_numpy(atlas).to(DEV))
    assert [n for n in log.names if KERNEL in n] and sum(log.counts.values()) == 1, log.counts
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
    assert got.shape == (len(index), 3, x.shape[2], 2 * x.shape[3])
    return got.cpu().numpy()


def _check(x, index, first, prims, atlas=None):
    got = _render(x, index, first, prims, atlas)
    want = vo.paint(x, index, first, prims, MEAN, STD, atlas)
    np.testing.assert_array_equal(got, want)
    return got


def _scene(H, W, count, seed, G):
    """`count` primitives of every kind on both panels, in and around the panel"""
    rng = np.random.RandomState(seed)
    recs = []
    for k in range(count):
        kind, panel = k % 4, int(rng.randint(2))
        color = tuple(int(v) for v in rng.randint(0, 256, 3))
        alpha = float(rng.choice([0.25, 0.5, 0.7, 1.0]))
        x1, y1 = int(rng.randint(-6, W)), int(rng.randint(-6, H))
        x2, y2 = x1 + int(rng.randint(0, W // 2 + 4)), y1 + int(rng.randint(0, H // 2 + 4))
        if kind == vo.QUAD:
            geometry = (x1, y1, x2, y1 + int(rng.randint(-3, 4)), x2 + int(rng.randint(-3, 4)), y2, x1, y2)
            recs.append(vo.rec(kind, panel, color, alpha, int(rng.randint(1, 4)), geometry))
        elif kind == vo.GLYPH:
            recs.append(vo.rec(kind, panel, color, alpha, int(rng.randint(G)), (x1, y1)))
        else:
            recs.append(vo.rec(kind, panel, color, alpha, int(rng.randint(1, 4)), (x1, y1, x2, y2)))
    return np.stack(recs)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the oracle
# ---------------------------------------------------------------------------------------------------------------------
# 19 x 21: output width 42 -> byte stores, scalar loads, a two-pixel tail, one tile across.  40 x 70: 140 columns -> dword
# stores, scalar loads, 3 x 3 tiles and a seam inside a tile.  33 x 68: 16-byte loads and dword stores, 3 x 3 tiles.
@pytest.mark.parametrize('H,W', [(19, 21), (40, 70), (33, 68)])
def test_every_kind_on_both_panels(H, W):
    atlas = _atlas()
    x = _input(2, H, W, seed=H)
    prims = _scene(H, W, 40, seed=W, G=len(atlas))
    got = _check(x, [0, 1], [0, 23, 40], prims, atlas)
    base = vo.paint(x, [0, 1], [0, 0, 0], prims[:0], MEAN, STD)
    assert (got != base).mean() > 0.2                               # the scene really covered the picture


def test_base_pixel_clamps_below_0_and_above_255():
    x = _input(1, 5, 9, seed=1)
    x[0, :, 0, :4] = np.float32([-5.0, -1.47, 2.2, 9.0])            # far below, just below, just above, far above
    got = _check(x, [0], [0, 0], np.zeros((0, 16), np.int32))
    assert got[0, :, 0, 0].tolist() == [0, 0, 0] and got[0, :, 0, 3].tolist() == [255, 255, 255]
    assert got[0, 0, 0, 1] == 0 and got[0, 0, 0, 2] == 255          # (-1.47 * .2886 + .4079) < 0;  (2.2 * .2886 + .4079) > 1
    assert np.array_equal(got[0, :, :, :9], got[0, :, :, 9:])       # both panels hold the same base picture
    assert len(np.unique(got)) > 50                                 # and ordinary values in between survive


def test_per_image_lists_and_index():
    H, W = 18, 22
    x = _input(3, H, W, seed=2)
    atlas = _atlas()
    prims = _scene(H, W, 7, seed=5, G=len(atlas))
    first_full = _check(x, [2, 0], [0, 7, 7], prims, atlas)                      # image 0 has no primitives
    base = vo.paint(x, [2, 0], [0, 0, 0], prims[:0], MEAN, STD)
    assert np.array_equal(first_full[1], base[1]) and not np.array_equal(first_full[0], base[0])
    _check(x, [2, 0], [0, 2, 7], prims, atlas)
    _check(x, [2, 0], [0, 0, 7], prims, atlas)                                   # the first list is the empty one
    _check(x, [1, 1, 2], [0, 3, 3, 7], prims, atlas)                             # one image twice, different lists


def test_nothing_leaks_across_the_panel_seam():
    H, W = 12, 21
    x = _input(1, H, W, seed=4)
    prims = np.stack([vo.rec(vo.RING, 0, (255, 0, 0), 1.0, 2, (W - 6, 5, W - 1, 9)),     # grows to column W: cut there
                      vo.rec(vo.FILL, 1, (0, 0, 255), 1.0, 0, (-3, 2, 0, 9)),           # ground truth, column 0 only
                      vo.rec(vo.QUAD, 0, (0, 255, 0), 1.0, 2, (W - 1, 0, W + 4, 0, W + 4, 1, W - 1, 1))])
    got = _check(x, [0], [0, 3], prims)
    base = vo.paint(x, [0], [0, 0], prims[:0], MEAN, STD)
    assert np.array_equal(got[0, :, :, W + 1:], base[0, :, :, W + 1:])            # right panel: only its column 0 changed
    assert (got[0, :, 2:10, W] == np.uint8([[0], [0], [255]])).all()
    assert np.array_equal(got[0, :, 10:, W], base[0, :, 10:, W]) and np.array_equal(got[0, :, :2, W], base[0, :, :2, W])
    assert (got[0, :, 4:11, W - 1] == np.uint8([[255], [0], [0]])).all()          # left panel's last column: the ring
    assert got[0, :, 0, W - 1].tolist() == [0, 255, 0]                            # ... and the outline's visible end
    assert np.array_equal(got[0, :, :, :W - 7], base[0, :, :, :W - 7])


def test_primitives_partly_and_wholly_outside():
    H, W = 20, 37
    x = _input(1, H, W, seed=6)
    prims = np.stack([vo.rec(vo.FILL, 0, (9, 200, 30), 0.5, 0, (-20, -20, 4, 3)),
                      vo.rec(vo.FILL, 1, (9, 200, 30), 0.5, 0, (W - 3, H - 2, W + 50, H + 50)),
                      vo.rec(vo.RING, 0, (250, 20, 30), 0.5, 3, (1, 1, W - 2, H - 2)),        # the outermost frame is outside
                      vo.rec(vo.RING, 1, (250, 20, 30), 0.5, 2, (-30000, -30000, 30000, 30000)),
                      vo.rec(vo.FILL, 0, (1, 2, 3), 1.0, 0, (-9, 5, -1, 9)),                  # wholly left of the panel
                      vo.rec(vo.FILL, 1, (1, 2, 3), 1.0, 0, (W, 5, W + 9, 9)),                # wholly right of it
                      vo.rec(vo.FILL, 0, (1, 2, 3), 1.0, 0, (3, H, 9, H + 5)),                # below
                      vo.rec(vo.FILL, 0, (1, 2, 3), 1.0, 0, (9, 9, 3, 3)),                    # x1 > x2: empty
                      vo.rec(vo.QUAD, 1, (0, 0, 0), 1.0, 2, (-10, -10, 15, 12, 60, 30, -32768, 32767)),
                      vo.rec(vo.QUAD, 0, (0, 0, 0), 1.0, 2, (-40, -40, -20, -40, -20, -30, -40, -30)),
                      vo.rec(vo.GLYPH, 0, (255, 255, 255), 1.0, 2, (-2, -3)),
                      vo.rec(vo.GLYPH, 1, (255, 255, 255), 1.0, 9, (4, 4)),                   # no such glyph: skipped
                      vo.rec(7, 0, (255, 255, 255), 1.0, 0, (0, 0, 9, 9)),                    # no such kind ...
                      vo.rec(vo.FILL, 2, (255, 255, 255), 1.0, 0, (0, 0, 9, 9))])             # ... or panel: skipped
    oracle_ok = prims[:12]                           # the oracle raises on the last two, the kernel skips them
    got = _render(x, [0], [0, len(prims)], prims, _atlas())
    np.testing.assert_array_equal(got, vo.paint(x, [0], [0, 12], oracle_ok, MEAN, STD, _atlas()))


def test_more_primitives_than_one_chunk_keep_their_order():
    CHUNK = uv.CHUNK
    H, W = 24, 40                                                    # 80 columns: two tiles across, two down
    count = CHUNK + 37
    x = _input(2, H, W, seed=7)
    rng = np.random.RandomState(8)
    recs = []
    for k in range(count):
        if CHUNK - 4 <= k < CHUNK + 4:               # translucent, overlapping, on both sides of the boundary
            color = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)][k % 4]
            recs.append(vo.rec(vo.FILL, k % 2, color, 0.5, 0, (10 + (k - CHUNK), 4, 34 + (k - CHUNK), 19)))
        else:
            x1, y1 = int(rng.randint(-2, W)), int(rng.randint(-2, H))
            recs.append(vo.rec(vo.FILL, int(rng.randint(2)), tuple(int(v) for v in rng.randint(0, 256, 3)), 0.5, 0,
                               (x1, y1, x1 + int(rng.randint(4)), y1 + int(rng.randint(4)))))
    prims = np.stack(recs)
    forward = vo.paint(x, [1], [0, count], prims, MEAN, STD)
    backward = vo.paint(x, [1], [0, count], prims[::-1], MEAN, STD)
    assert (forward[0, :, 4:20, 10:34] != backward[0, :, 4:20, 10:34]).any()       # the order shows in the oracle itself
    assert (forward[0, :, 4:20, W + 10:W + 34] != backward[0, :, 4:20, W + 10:W + 34]).any()
    np.testing.assert_array_equal(_render(x, [1], [0, count], prims), forward)
    np.testing.assert_array_equal(_render(x, [1], [0, count], prims[::-1].copy()), backward)
    # the long list behind a short one: the range does not start on a chunk boundary
    both = np.concatenate([prims[:5], prims])
    _check(x, [0, 1], [0, 5, 5 + count], both)


def test_quads_at_0_33_90_degrees_and_a_point():
    from utils.box import rotate_bbox
    H, W = 40, 70
    x = _input(1, H, W, seed=9)
    recs = []
    for k, (angle, t) in enumerate([(0, 2), (33, 2), (90, 2), (33, 3), (33, 1)]):
        box = np.float32([20 + 9 * k, 20, 18, 30, angle])
        verts = np.asarray(rotate_bbox(*box)).reshape(-1)
        recs.append(vo.rec(vo.QUAD, k % 2, (250 - 40 * k, 30 * k, 128), 1.0 if k < 3 else 0.5, t, verts))
    recs.append(vo.rec(vo.QUAD, 0, (255, 255, 255), 1.0, 2, (63, 15) * 4))       # a point on a tile corner
    recs.append(vo.rec(vo.QUAD, 1, (255, 255, 255), 1.0, 3, (5, 5) * 4))
    recs.append(vo.rec(vo.QUAD, 1, (0, 0, 0), 1.0, 0, (9, 9) * 4))               # t = 0: the point itself (d = 0)
    got = _check(x, [0], [0, len(recs)], np.stack(recs))
    assert got[0, :, 15, 63].tolist() == [255] * 3 and got[0, :, 14, 63].tolist() == [255] * 3
    assert got[0, :, 4:7, W + 4:W + 7].min() == 255 and got[0, :, 9, W + 9].tolist() == [0, 0, 0]


def test_glyphs_from_a_synthetic_atlas():
    H, W = 40, 70
    atlas = _atlas()                                                 # cells of 5 x 7
    x = _input(1, H, W, seed=10)
    prims = np.stack([vo.rec(vo.GLYPH, 0, (255, 255, 255), 0.0, 0, (3, 3)),          # the record's alpha is ignored
                      vo.rec(vo.GLYPH, 0, (0, 0, 0), 1.0, 1, (W - 2, 20)),           # straddles the panel's right edge
                      vo.rec(vo.GLYPH, 1, (255, 0, 0), 1.0, 2, (-3, H - 3)),         # and the left / bottom edge
                      vo.rec(vo.GLYPH, 0, (0, 255, 0), 1.0, 3, (62, 13)),            # straddles the tile corner (64, 16)
                      vo.rec(vo.GLYPH, 1, (0, 0, 255), 1.0, 4, (126 - W, 29)),       # the same in the right panel
                      vo.rec(vo.FILL, 0, (10, 20, 30), 0.5, 0, (60, 10, 69, 22)),    # a bar over text over a bar
                      vo.rec(vo.GLYPH, 0, (255, 255, 0), 1.0, 5, (63, 12)),
                      vo.rec(vo.GLYPH, 1, (255, 255, 0), 1.0, 5, (0, -6))])          # only its last row shows
    got = _check(x, [0], [0, len(prims)], prims, atlas)
    assert got[0, :, 4, 3:8].tolist() == [[255] * 5] * 3             # row 1 of every glyph has full coverage: opaque ink
    base = vo.paint(x, [0], [0, 0], prims[:0], MEAN, STD)
    assert np.array_equal(got[0, :, 3, 3:8], base[0, :, 3, 3:8])     # row 0 has none: the picture shows through


def test_two_runs_are_bit_identical():
    H, W = 40, 70
    atlas = _atlas()
    x = torch.from_numpy(_input(2, H, W, seed=11)).to(DEV)
    prims = _scene(H, W, 300, seed=12, G=len(atlas))
    import hip_runtime as hr
    d_atlas = torch.from_numpy(atlas).to(DEV)
    with hr.launch_log() as log:
        a = uv.render(x, [1, 0], [0, 290, 300], prims, MEAN, STD, d_atlas)
        b = uv.render(x, [1, 0], [0, 290, 300], prims, MEAN, STD, d_atlas)
    assert [n for n in log.names if KERNEL in n] and sum(log.counts.values()) == 2
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# Visualizer and TensorboardLogger end to end
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = {0: {'name': 'car'}, 1: {'name': 'person'}, 2: ''}
COLORS = [[255, 0, 0], [250, 250, 0], [0, 0, 90]]


def _visualizer():
    vis = uv.Visualizer(CLASSES, 0.3, MEAN, STD, font_size=10, alpha=0.5, colors=COLORS)
    rng = np.random.RandomState(13)
    vis.set_atlas(rng.randint(0, 256, (95, 9, 6)).astype(np.uint8), rng.randint(3, 7, 95))     # not PIL's: synthetic
    return vis


def _detections(B, H, W, rotated, keypoints, seed):
    """shaped like uda.Model.get_detections' result: predictions [B, K, .] arrays, ground truth per-image lists"""
    rng = np.random.RandomState(seed)
    K, cols = 6, 5 if rotated else 4

    def boxes(n):
        if rotated:
            return np.stack([rng.uniform(5, W - 5, n), rng.uniform(15, H - 5, n), rng.uniform(4, 14, n),
                             rng.uniform(10, 24, n), rng.uniform(-90, 90, n)], 1).astype(np.float32)
        x1, y1 = rng.uniform(-4, W - 8, n), rng.uniform(10, H - 8, n)
        return np.stack([x1, y1, x1 + rng.uniform(3, 45, n), y1 + rng.uniform(3, 20, n)], 1).astype(np.float32)

    counts = [(3 * b + 2) % 5 for b in range(B)]                   # 2, 0, 3, ...: one image without ground truth
    out = {'pred_boxes': np.stack([boxes(K) for _ in range(B)]),
           'pred_classes': rng.randint(0, 3, (B, K)).astype(np.int32),
           'pred_scores': rng.uniform(0.1, 1.0, (B, K)).astype(np.float32),
           'gt_boxes': [boxes(n).reshape(n, cols) for n in counts],
           'gt_classes': [rng.randint(0, 3, n).astype(np.int32) for n in counts]}
    if keypoints:
        out['pred_kps'] = rng.uniform(-2, W + 2, (B, K, 3, 2)).astype(np.float32)
        out['gt_kps'] = [rng.uniform(0, H, (n, 3, 2)).astype(np.float32) for n in counts]
    return out


@pytest.mark.parametrize('mode', ['boxes+keypoints', 'boxes', 'rotated'])
def test_visualize_batch_equals_the_oracle_on_its_own_primitives(mode):
    import hip_runtime as hr
    B, H, W = 3, 40, 70
    vis = _visualizer()
    x = _input(B, H, W, seed=14)
    d_x = torch.from_numpy(x).to(DEV)
    dets = _detections(B, H, W, mode == 'rotated', mode == 'boxes+keypoints', seed=15)
    index = [2, 0, 1]
    with hr.launch_log() as log:
        got = vis.visualize_batch(d_x, dets, index)
    assert [n for n in log.names if KERNEL in n] and sum(log.counts.values()) == 1, log.counts     # one launch
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, 3, H, 2 * W)
    lists = [vis.build_primitives(dets['pred_boxes'][i], dets['pred_classes'][i], dets['pred_scores'][i],
                                  dets['gt_boxes'][i], dets['gt_classes'][i],
                                  dets['gt_kps'][i] if 'gt_kps' in dets else None,
                                  dets['pred_kps'][i] if 'pred_kps' in dets else None) for i in index]
    kinds = np.concatenate(lists)[:, 0]
    assert (kinds == vo.GLYPH).sum() > 20 and (kinds == (vo.QUAD if mode == 'rotated' else vo.RING)).sum() >= 5
    first = np.concatenate([[0], np.cumsum([len(p) for p in lists])])
    want = vo.paint(x, index, first, np.concatenate(lists), MEAN, STD, vis.atlas)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    # the reference's call for one image is row i of the batch form
    i = 2
    with hr.launch_log() as log:
        one = vis.visualize_detections(d_x[i].permute(1, 2, 0), dets['pred_boxes'][i], dets['pred_classes'][i],
                                       dets['pred_scores'][i], dets['gt_boxes'][i], dets['gt_classes'][i],
                                       dets['gt_kps'][i] if 'gt_kps' in dets else None,
                                       dets['pred_kps'][i] if 'pred_kps' in dets else None)
    assert [n for n in log.names if KERNEL in n]
    assert one.shape == (3, H, 2 * W) and torch.equal(one, got[index.index(i)])
    # all images, in batch order, when no indices are given
    assert torch.equal(vis.visualize_batch(d_x, dets)[[2, 0, 1]], got)


def test_default_atlas_renders_text():
    """PIL's font is not part of the correctness chain; this only shows that the default atlas reaches the kernel"""
    import hip_runtime as hr
    vis = uv.Visualizer(CLASSES, 0.3, MEAN, STD, colors=COLORS)
    H, W = 40, 70
    x = _input(1, H, W, seed=16)
    args = (np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
            np.float32([[2, 22, 66, 38]]), np.int32([1]))
    with hr.launch_log() as log:
        got = vis.visualize_detections(torch.from_numpy(x[0].transpose(1, 2, 0).copy()).to(DEV), *args)
    assert [n for n in log.names if KERNEL in n]
    prims = vis.build_primitives(*args)
    want = vo.paint(x, [0], [0, len(prims)], prims, MEAN, STD, vis.atlas if vis.atlas.size else None)
    np.testing.assert_array_equal(got.cpu().numpy(), want[0])
    if vis.atlas.size:
        assert (prims[:, 0] == vo.GLYPH).sum() == len('person')


class _Recorder:
    def __init__(self):
        self.images = []

    def add_image(self, name, image, step):
        self.images.append((name, image, step))


def test_logger_logs_exactly_num_visualizations_images_across_two_calls():
    import hip_runtime as hr
    from utils.tensorboard import TensorboardLogger
    B, H, W = 2, 19, 21
    cfg = types.SimpleNamespace(tensorboard=types.SimpleNamespace(score_threshold=0.3, font_size=10, alpha=0.5,
                                                                  num_visualizations=3),
                                normalize=types.SimpleNamespace(mean=list(MEAN), std=list(STD)))
    writer = _Recorder()
    logger = TensorboardLogger(cfg, CLASSES, writer=writer)
    x = _input(B, H, W, seed=17)
    batch = {'input': torch.from_numpy(x).to(DEV), 'id': torch.tensor([41, 42])}
    dets = _detections(B, H, W, False, True, seed=18)
    with hr.launch_log() as log:
        logger.log_detections(batch, dets, 1, 'validation')
        logger.log_detections(batch, dets, 2, 'validation')
        logger.log_detections(batch, dets, 3, 'validation')
    assert [n for n in log.names if KERNEL in n] and sum(log.counts.values()) == 2      # one launch per logging call
    assert [(n, s) for n, _, s in writer.images] == [('validation/detection_41', 1), ('validation/detection_42', 1),
                                                     ('validation/detection_41', 2)]
    want = logger.visualizer.visualize_batch(batch['input'], dets).cpu().numpy()
    for (_, image, _), row in zip(writer.images, (0, 1, 0)):
        assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.shape == (3, H, 2 * W)
        assert np.array_equal(image, want[row])
    logger.reset()
    logger.log_detections(batch, dets, 4, 'test')
    assert len(writer.images) == 5 and writer.images[-1][0] == 'test/detection_42'
