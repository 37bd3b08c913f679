"""No-GPU checks of the preview path: tests/visualize_oracle.py pinned by pictures worked out by hand, the record list
`Visualizer.build_primitives` makes, `TensorboardLogger`'s counter and tags with a recording writer and a stub
renderer, the file writer, and the C call's argument checks."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import visualize_oracle as vo
from utils import visualize as uv
from utils.tensorboard import FileWriter, TensorboardLogger
from utils.visualize import Visualizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _picture(rows):
    """rows of '.' and '#' -> the set of (x, y) marked '#'"""
    return {(x, y) for y, row in enumerate(rows) for x, ch in enumerate(row) if ch == '#'}


def _covered(r, H, W, atlas=None):
    ys, xs, _ = vo.pixel_set(r, H, W, atlas)
    return set(zip(xs.tolist(), ys.tolist()))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, pinned by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_ring_of_an_8x8_box_is_two_frames_growing_outward():
    want = _picture(['..............',
                     '..............',
                     '..##########..',
                     '..##########..',
                     '..##......##..',
                     '..##......##..',
                     '..##......##..',
                     '..##......##..',
                     '..##......##..',
                     '..##......##..',
                     '..##########..',
                     '..##########..',
                     '..............',
                     '..............'])
    assert len(want) == 64
    assert _covered(vo.rec(vo.RING, 0, (1, 2, 3), 0.5, 2, (3, 3, 10, 10)), 14, 14) == want
    # t = 1 is the box's own frame; t = 0 is nothing
    frame = _covered(vo.rec(vo.RING, 0, (1, 2, 3), 0.5, 1, (3, 3, 10, 10)), 14, 14)
    assert frame == {(x, y) for x in range(3, 11) for y in range(3, 11) if x in (3, 10) or y in (3, 10)}
    assert _covered(vo.rec(vo.RING, 0, (1, 2, 3), 0.5, 0, (3, 3, 10, 10)), 14, 14) == set()


def test_oracle_blend_rounds_ties_to_even():
    # 10 + 0.5 * (15 - 10) = 12.5 -> 12;  11 + 0.5 * (16 - 11) = 13.5 -> 14;  0 + 0.5 * 255 = 127.5 -> 128
    assert vo.blend(np.uint8([10, 11, 0]), 0.5, 15).tolist()[:1] == [12]
    assert vo.blend(np.uint8([11]), 0.5, 16).tolist() == [14]
    assert vo.blend(np.uint8([0]), 0.5, 255).tolist() == [128]
    # no tie: 200 + 0.25 * (0 - 200) = 150;  alpha 1 is the colour, alpha 0 the pixel
    assert vo.blend(np.uint8([200]), 0.25, 0).tolist() == [150]
    assert vo.blend(np.uint8([7, 250]), 1.0, 99).tolist() == [99, 99]
    assert vo.blend(np.uint8([7, 250]), 0.0, 99).tolist() == [7, 250]


def test_oracle_base_pixel_clamps_and_truncates():
    x = np.float32([[[-3.0, 0.0, 0.999, 1.0, 5.0]]] * 3)                    # [3, 1, 5], mean 0, std 1: v = x * 255
    got = vo.base_pixels(x, (0, 0, 0), (1, 1, 1))
    assert got[0, :, 0].tolist() == [0, 0, 254, 255, 255]                   # 0.999 * 255 = 254.7 truncates


def test_oracle_quad_edge_at_45_degrees():
    # the segment (2, 2) - (6, 6) walked there and back, t = 2: every pixel within distance 1 of it.  Along the edge that
    # is |x - y| <= 1 (0.71) but not 2 (1.41); beyond an end only the end point's 4-neighbours remain.
    want = _picture(['.........',
                     '..#......',
                     '.###.....',
                     '..###....',
                     '...###...',
                     '....###..',
                     '.....###.',
                     '......#..',
                     '.........'])
    assert len(want) == 17
    assert _covered(vo.rec(vo.QUAD, 0, (9, 9, 9), 1.0, 2, (2, 2, 6, 6, 6, 6, 2, 2)), 9, 9) == want


def test_oracle_degenerate_quad_is_the_disc_around_its_point():
    point = (5, 5) * 4
    assert _covered(vo.rec(vo.QUAD, 0, (9, 9, 9), 1.0, 2, point), 11, 11) == {(5, 5), (4, 5), (6, 5), (5, 4), (5, 6)}
    # t = 3: d^2 <= 2.25 -> the 3 x 3 block;  t = 1: d^2 <= 0.25 -> the point alone
    assert _covered(vo.rec(vo.QUAD, 0, (9, 9, 9), 1.0, 3, point), 11, 11) == {(x, y) for x in (4, 5, 6) for y in (4, 5, 6)}
    assert _covered(vo.rec(vo.QUAD, 0, (9, 9, 9), 1.0, 1, point), 11, 11) == {(5, 5)}


def test_oracle_paints_in_list_order_and_keeps_panels_apart():
    x = np.zeros((1, 3, 4, 5), np.float32)
    prims = np.stack([vo.rec(vo.FILL, 0, (200, 0, 0), 0.5, 0, (1, 1, 3, 2)),
                      vo.rec(vo.FILL, 0, (0, 100, 0), 0.5, 0, (3, 0, 9, 1)),      # runs off the panel's right edge
                      vo.rec(vo.FILL, 1, (0, 0, 255), 1.0, 0, (-4, 3, 0, 3))])     # and this one off the left
    got = vo.paint(x, [0], [0, 3], prims, (0, 0, 0), (1, 1, 1))
    assert got.shape == (1, 3, 4, 10)
    assert got[0, :, 1, 3].tolist() == [50, 50, 0]             # red 0 -> 100, then green over it: 100 -> 50, 0 -> 50
    assert got[0, :, 1, 2].tolist() == [100, 0, 0] and got[0, :, 0, 4].tolist() == [0, 50, 0]
    assert got[0, :, 0, 5:].max() == 0 and got[0, :, 1, 5:].max() == 0          # nothing crossed the seam
    assert got[0, :, 3, 5].tolist() == [0, 0, 255] and got[0, :, 3, 4].tolist() == [0, 0, 0]
    swapped = vo.paint(x, [0], [0, 3], prims[[1, 0, 2]], (0, 0, 0), (1, 1, 1))
    assert swapped[0, :, 1, 3].tolist() == [100, 25, 0]


# ---------------------------------------------------------------------------------------------------------------------
# build_primitives
# ---------------------------------------------------------------------------------------------------------------------
CLASSES = {0: {'name': 'ab'}, 1: {'name': 'c'}, 2: ''}
COLORS = [[255, 0, 0], [250, 250, 0], [0, 0, 90]]           # luminance 76 (white ink), 221 (black ink), 10 (white ink)
GW, GH = 5, 7


def _visualizer(**kw):
    vis = Visualizer(CLASSES, 0.3, (0.4, 0.4, 0.4), (0.2, 0.2, 0.2), font_size=10, alpha=0.5, colors=COLORS, **kw)
    cover = np.random.RandomState(0).randint(0, 256, (95, GH, GW)).astype(np.uint8)
    vis.set_atlas(cover, np.full(95, 4, np.int32))          # every glyph advances 4, the cell is 5 wide
    return vis


def _fields(r):
    return (int(r[0]), int(r[1]), (int(r[2]) & 255, (int(r[2]) >> 8) & 255, (int(r[2]) >> 16) & 255),
            float(np.array([r[3]], np.int32).view(np.float32)[0]), int(r[4]), [int(v) for v in r[5:13]])


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    defines = dict(re.findall(r'#define (CNUDA_RENDER_\w+) (\d+)', text))
    assert int(defines['CNUDA_RENDER_RECORD']) == uv.RECORD == vo.RECORD
    assert int(defines['CNUDA_RENDER_CHUNK']) == uv.CHUNK
    assert [int(defines['CNUDA_RENDER_' + k]) for k in ('RING', 'FILL', 'QUAD', 'GLYPH')] == \
        [uv.RING, uv.FILL, uv.QUAD, uv.GLYPH] == [vo.RING, vo.FILL, vo.QUAD, vo.GLYPH]


def test_axis_aligned_records_order_counts_and_threshold():
    vis = _visualizer()
    pred_boxes = np.float32([[10.4, 20.5, 50.6, 40.5], [0, 0, 5, 5], [60, 30, 100, 70]])
    prims = vis.build_primitives(pred_boxes, np.int32([0, 1, 2]), np.float32([0.87, 0.29, 0.3]),
                                 np.float32([[12, 22, 52, 42]]), np.int32([1]))
    assert prims.dtype == np.int32 and prims.shape[1] == uv.RECORD
    f = [_fields(r) for r in prims]
    # prediction 0: "ab: 0.87" = 8 glyphs; prediction 1 is below the threshold; prediction 2 (score == threshold stays):
    # "2: 0.30" = 7 glyphs;  ground truth: "c" = 1 glyph
    assert [k[0] for k in f] == [uv.RING, uv.FILL] + [uv.GLYPH] * 8 + [uv.RING, uv.FILL] + [uv.GLYPH] * 7 + \
        [uv.RING, uv.FILL, uv.GLYPH]
    assert [k[1] for k in f] == [0] * 19 + [1] * 3
    # np.rint: 10.4 -> 10, 20.5 -> 20 (half to even), 50.6 -> 51, 40.5 -> 40
    assert f[0] == (uv.RING, 0, (255, 0, 0), 0.5, 2, [10, 20, 51, 40, 0, 0, 0, 0])
    assert f[1] == (uv.FILL, 0, (255, 0, 0), 0.5, 0, [10, 6, 51, 19, 0, 0, 0, 0])         # height = font_size + 4 = 14
    text = 'ab: 0.87'
    for k, ch in enumerate(text):
        assert f[2 + k] == (uv.GLYPH, 0, (255, 255, 255), 1.0, ord(ch) - 32, [12 + 4 * k, 8, 0, 0, 0, 0, 0, 0])
    assert f[10][2] == (0, 0, 90) and f[12][2] == (255, 255, 255) and f[12][4] == ord('2') - 32   # '' -> the id
    assert f[19] == (uv.RING, 1, (250, 250, 0), 0.5, 2, [12, 22, 52, 42, 0, 0, 0, 0])
    assert f[21] == (uv.GLYPH, 1, (0, 0, 0), 1.0, ord('c') - 32, [14, 10, 0, 0, 0, 0, 0, 0])   # bright colour: black ink


def test_reversed_boxes_are_normalised_and_glyphs_stop_at_x2():
    vis = _visualizer()
    prims = vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                 np.float32([[30, 40, 18, 12]]), np.int32([0]))
    f = [_fields(r) for r in prims]
    assert f[0][5][:4] == [18, 12, 30, 40] and f[1][5][:4] == [18, -2, 30, 11]
    # "ab" from x = 20: cell 20..24 fits, cell 24..28 fits (28 <= 30)
    assert [k[0] for k in f] == [uv.RING, uv.FILL, uv.GLYPH, uv.GLYPH]
    # box 18..26: the first cell 20..24 fits, the second, 24..28, would pass x2 = 26 and is dropped
    prims = vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                 np.float32([[18, 12, 26, 40]]), np.int32([0]))
    assert [int(r[0]) for r in prims] == [uv.RING, uv.FILL, uv.GLYPH]
    # box 18..23: no cell fits, the bar stays
    prims = vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                 np.float32([[18, 12, 23, 40]]), np.int32([0]))
    assert [int(r[0]) for r in prims] == [uv.RING, uv.FILL]


def test_five_column_mode_is_selected_by_gt_boxes():
    vis = _visualizer()
    gt = np.float32([[40, 30, 20, 10, 0], [40, 30, 20, 10, 90]])
    pred = np.float32([[50, 50, 10, 30, 33]])
    prims = vis.build_primitives(pred, np.int32([1]), np.float32([0.5]), gt, np.int32([0, 0]))
    f = [_fields(r) for r in prims]
    quads = [k for k in f if k[0] == uv.QUAD]
    assert len(quads) == 3 and not any(k[0] == uv.RING for k in f)
    assert all(k[3] == 1.0 and k[4] == 2 for k in quads)                           # opaque, thickness 2
    assert quads[1][5] == [30, 25, 50, 25, 50, 35, 30, 35]                         # 0 degrees: the box itself
    from utils.box import rotate_bbox
    assert quads[0][5] == [int(v) for v in np.asarray(rotate_bbox(*pred[0])).reshape(-1)]
    # the label sits on the vertices' bounding box
    xs, ys = quads[2][5][0::2], quads[2][5][1::2]
    bar = f[f.index(quads[2]) + 1]
    assert bar[0] == uv.FILL and bar[5][:4] == [min(xs), min(ys) - 14, max(xs), min(ys) - 1] and bar[3] == 0.5
    # four columns of ground truth select the axis-aligned mode even when the predictions carry five
    prims = vis.build_primitives(pred, np.int32([1]), np.float32([0.5]), gt[:, :4], np.int32([0, 0]))
    assert not any(int(r[0]) == uv.QUAD for r in prims)


def test_keypoints_follow_the_boxes_of_their_panel():
    vis = _visualizer()
    gt_kps = np.float32([[[5.5, 6.5], [9, 9]]])                                    # [1, 2, 2]
    pred_kps = np.float32([[[1, 2, 0.9], [3, 4, 0.8]], [[7, 7, 0.1], [8, 8, 0.1]]])   # [2, 2, 3]: two columns are used
    prims = vis.build_primitives(np.float32([[0, 20, 30, 40], [0, 20, 30, 40]]), np.int32([2, 2]),
                                 np.float32([0.9, 0.1]), np.float32([[0, 20, 3, 40]]), np.int32([2]), gt_kps, pred_kps)
    f = [_fields(r) for r in prims]
    kinds = [(k[1], k[0]) for k in f]
    n_pred_glyphs = len('2: 0.90')
    assert kinds == [(0, uv.RING), (0, uv.FILL)] + [(0, uv.GLYPH)] * n_pred_glyphs + [(0, uv.FILL)] * 2 + \
        [(1, uv.RING), (1, uv.FILL)] + [(1, uv.FILL)] * 2                          # the gt box 0..3 has room for no glyph
    kp = f[2 + n_pred_glyphs]
    assert kp == (uv.FILL, 0, (0, 255, 255), 0.5, 0, [0, 1, 2, 3, 0, 0, 0, 0])     # 3 x 3 around (1, 2)
    assert f[-2][5][:4] == [5, 5, 7, 7]                                            # rint(5.5) = 6, rint(6.5) = 6
    # without pred_kps nothing is drawn, as in the reference
    prims = vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                 np.float32([[0, 20, 3, 40]]), np.int32([2]), gt_kps, None)
    assert len(prims) == 2


def test_unknown_class_raises_and_empty_lists_are_empty():
    vis = _visualizer()
    with pytest.raises(ValueError, match='palette'):
        vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                             np.float32([[0, 0, 5, 5]]), np.int32([3]))
    with pytest.raises(ValueError, match='palette'):
        vis.build_primitives(np.float32([[0, 0, 5, 5]]), np.int32([-1]), np.float32([0.9]),
                             np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    empty = vis.build_primitives(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                 np.zeros((0, 4), np.float32), np.zeros(0, np.int32))
    assert empty.shape == (0, uv.RECORD) and empty.dtype == np.int32


def test_coordinates_are_clamped_to_16_bits():
    r = uv.record(uv.FILL, 1, (1, 2, 3), 2.0, 0, (-10 ** 6, -32769, 32768, 10 ** 9))
    assert _fields(r) == (uv.FILL, 1, (1, 2, 3), 1.0, 0, [-32768, -32768, 32767, 32767, 0, 0, 0, 0])
    assert np.array_equal(uv.record(uv.RING, 0, (4, 5, 6), 0.25, 2, (1, 2, 3, 4)),
                          vo.rec(vo.RING, 0, (4, 5, 6), 0.25, 2, (1, 2, 3, 4)))


def test_palette_and_default_atlas():
    assert np.array_equal(_visualizer().cmap, np.uint8(COLORS))
    vis = Visualizer([{'name': 'a'}] * 5, 0.3, (0, 0, 0), (1, 1, 1))
    assert vis.cmap.shape == (5, 3) and vis.cmap.dtype == np.uint8 and len({tuple(c) for c in vis.cmap}) == 5
    try:
        import matplotlib
        cm = matplotlib.colormaps['gist_rainbow']
        assert vis.cmap.tolist() == [[int(y * 255.0) for y in cm(1.0 * x / 5)[:3]] for x in range(5)]
    except ImportError:
        assert vis.cmap[0].tolist() == [255, 0, 0]
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert vis.atlas.shape[0] == 0
        return
    G, gh, gw = vis.atlas.shape
    assert G == 95 and gh >= 8 and gw >= 4 and vis.atlas.dtype == np.uint8
    assert vis.atlas[0].max() == 0 and vis.atlas[ord('W') - 32].max() == 255          # the space is empty, a letter is inked
    assert vis.advances.shape == (95,) and vis.advances.min() >= 1 and vis.advances.max() <= gw


# ---------------------------------------------------------------------------------------------------------------------
# TensorboardLogger
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.images, self.scalars = [], []

    def add_image(self, name, image, step):
        self.images.append((name, np.asarray(image).copy(), step))

    def add_scalar(self, name, value, step):
        self.scalars.append((name, value, step))


class _StubRenderer:
    """stands in for the Visualizer: records what it was asked for, returns image k filled with k"""

    def __init__(self):
        self.calls = []

    def visualize_batch(self, input, detections, indices=None):
        indices = list(indices)
        self.calls.append(indices)
        return torch.stack([torch.full((3, 2, 4), i, dtype=torch.uint8) for i in indices])


def _config(num):
    return types.SimpleNamespace(tensorboard=types.SimpleNamespace(score_threshold=0.3, font_size=10, alpha=0.5,
                                                                   num_visualizations=num),
                                 normalize=types.SimpleNamespace(mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2]))


def test_logger_counter_tags_and_reset():
    writer = _Recorder()
    logger = TensorboardLogger(_config(5), CLASSES, writer=writer)
    assert logger.classes is CLASSES and logger.log_callback is None and logger.summary_writer is writer
    assert logger.visualizer.score_threshold == 0.3 and logger.visualizer.font_size == 10
    stub = logger.visualizer = _StubRenderer()
    batch = {'input': torch.zeros(3, 3, 2, 2), 'id': torch.tensor([17, 4, 99])}
    logger.log_detections(batch, {}, 7, 'validation')
    logger.log_detections(batch, {}, 8, 'validation')           # only two are left: only two are rendered
    logger.log_detections(batch, {}, 9, 'validation')           # nothing is left: nothing is rendered
    assert stub.calls == [[0, 1, 2], [0, 1]]
    assert [(n, s) for n, _, s in writer.images] == [
        ('validation/detection_17', 7), ('validation/detection_4', 7), ('validation/detection_99', 7),
        ('validation/detection_17', 8), ('validation/detection_4', 8)]
    assert [int(im[0, 0, 0]) for _, im, _ in writer.images] == [0, 1, 2, 0, 1]
    assert all(im.shape == (3, 2, 4) and im.dtype == np.uint8 for _, im, _ in writer.images)
    logger.reset()
    logger.log_detections({'input': torch.zeros(1, 3, 2, 2), 'id': [5]}, {}, 10, 'test')
    assert stub.calls[-1] == [0] and writer.images[-1][0] == 'test/detection_5' and len(writer.images) == 6
    logger.log_stat('loss', 0.25, 3)
    logger.log_image('picture', np.zeros((3, 1, 1), np.uint8), 4)
    assert writer.scalars == [('loss', 0.25, 3)] and writer.images[-1][0] == 'picture'


def test_file_writer_appends_scalars_and_writes_ppm(tmp_path):
    w = FileWriter(str(tmp_path / 'logs'))
    w.add_scalar('train/loss', 1.5, 1)
    w.add_scalar('train/loss', np.float32(0.5), 2)
    lines = (tmp_path / 'logs' / 'scalars.jsonl').read_text().splitlines()
    assert len(lines) == 2 and '"step": 2' in lines[1] and '0.5' in lines[1]
    image = np.arange(3 * 2 * 5, dtype=np.uint8).reshape(3, 2, 5)
    w.add_image('validation/detection_7', image, 12)
    raw = (tmp_path / 'logs' / 'validation' / 'detection_7' / '00000012.ppm').read_bytes()
    assert raw.startswith(b'P6\n5 2\n255\n')
    assert np.array_equal(np.frombuffer(raw[len(b'P6\n5 2\n255\n'):], np.uint8).reshape(2, 5, 3), image.transpose(1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------------
# the C call and the Python entry refuse bad arguments without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_c_call_rejects_null_pointers_and_oversized_images():
    import hip_runtime as hr
    L = hr.lib()
    m = [0.4] * 3 + [0.2] * 3
    assert L.cnuda_render_detections(None, None, None, None, None, None, 1, 1, 8, 8, 0, 0, 0, 0, *m, None) == -1
    assert b'null pointer' in L.cnuda_last_error()
    buf = (ctypes.c_int * 64)()                                  # host memory: the checks run before anything reads it
    p = ctypes.addressof(buf)
    assert L.cnuda_render_detections(p, p, None, p, None, None, 1, 1, 8, 8, 0, 0, 0, 0, *m, None) == -1   # out is null
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 1, 8193, 8, 0, 0, 0, 0, *m, None) == -1
    assert b'8192' in L.cnuda_last_error()
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 1, 8, 8193, 0, 0, 0, 0, *m, None) == -1
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 0, 8, 8, 0, 0, 0, 0, *m, None) == -1     # n = 0
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 1, 0, 8, 0, 0, 0, 0, *m, None) == -1     # H = 0
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 1, 8, 8, 3, 0, 0, 0, *m, None) == -1     # N > 0, no prims
    assert L.cnuda_render_detections(p, p, None, p, None, p, 1, 1, 8, 8, 0, 2, 7, 5, *m, None) == -1     # G > 0, no atlas
    assert b'atlas' in L.cnuda_last_error()


def test_cpu_tensors_raise():
    vis = _visualizer()
    dets = {'pred_boxes': np.zeros((1, 0, 4), np.float32), 'pred_classes': np.zeros((1, 0), np.int32),
            'pred_scores': np.zeros((1, 0), np.float32), 'gt_boxes': [np.zeros((0, 4), np.float32)],
            'gt_classes': [np.zeros(0, np.int32)]}
    with pytest.raises(RuntimeError, match='MI355X only'):
        vis.visualize_batch(torch.zeros(1, 3, 4, 4), dets)
    with pytest.raises(RuntimeError, match='MI355X only'):
        vis.visualize_detections(torch.zeros(4, 4, 3), dets['pred_boxes'][0], dets['pred_classes'][0],
                                 dets['pred_scores'][0], dets['gt_boxes'][0], dets['gt_classes'][0])
    with pytest.raises(RuntimeError, match='MI355X only'):
        uv.render(torch.zeros(1, 3, 4, 4), [0], [0, 0], np.zeros((0, 16), np.int32), (0, 0, 0), (1, 1, 1))
