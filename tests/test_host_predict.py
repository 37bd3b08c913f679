"""Prediction without a GPU: the numpy oracle of the three kernels pinned by hand-worked cases, the host-side rules of
predict.py (scale sizes, refusals, file lists, the COCO results file, the command line), and the new C entry points'
argument checks."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import yaml
from PIL import Image

import predict_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ('cnuda_mirror_input', 'cnuda_tta_merge', 'cnuda_project_detections', 'cnuda_predict_workspace_bytes',
               'cnuda_soft_nms_merge')


def clustered(seed):
    """The clustered recipe: six objects seen five times each, one class."""
    rng = np.random.default_rng([2024, seed])
    W, H, G = 64, 48, 6
    cx, cy = rng.uniform(8, W - 8, G), rng.uniform(8, H - 8, G)
    w, h = rng.uniform(6, 24, G), rng.uniform(6, 24, G)
    base = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    boxes = (base[:, None] + rng.uniform(-0.5, 0.5, (G, 5, 4))).reshape(-1, 4).astype(np.float32)
    scores = rng.uniform(0.02, 1.0, 30).astype(np.float32)
    return boxes, scores


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_soft_nms_two_identical_boxes_decay_by_e_minus_two():
    boxes = F([[2, 3, 10, 9], [2, 3, 10, 9]])
    out = po.soft_nms_image(boxes, F([0.9, 0.5]), [0, 0], 1, 10, 0.0)
    assert out['index'].tolist() == [0, 1]
    assert out['scores'][0] == float(F(0.9))
    assert out['scores'][1] == float(F(0.5)) * math.exp(-2.0)          # iou 1: exp(-1 / 0.5)


def test_soft_nms_disjoint_boxes_keep_their_scores_and_touching_is_no_overlap():
    boxes = F([[0, 0, 4, 4], [4, 0, 8, 4], [20, 20, 30, 30]])
    out = po.soft_nms_image(boxes, F([0.3, 0.8, 0.5]), [0, 0, 0], 1, 10, 0.0)
    assert out['index'].tolist() == [1, 2, 0]
    assert out['scores'].tolist() == [float(F(0.8)), float(F(0.5)), float(F(0.3))]
    assert po.iou([0, 0, 4, 4], [2, 0, 6, 4]) == 8.0 / 24.0                # no '+ 1' in the areas
    assert po.iou([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0                      # empty union


def test_soft_nms_tie_goes_to_the_lower_index():
    boxes = F([[0, 0, 4, 4], [10, 10, 14, 14], [20, 20, 24, 24]])
    out = po.soft_nms_image(boxes, F([0.5, 0.7, 0.5]), [0, 0, 0], 1, 10, 0.0)
    assert out['index'].tolist() == [1, 0, 2] and out['margins']['ties'] == 1


def test_soft_nms_class_loop_stops_below_the_floor():
    # the duplicate decays to 0.005 e^-2 = 6.8e-4 < 1e-3 and is dropped; a score below the floor never enters
    boxes = F([[0, 0, 8, 8], [0, 0, 8, 8], [20, 20, 24, 24]])
    out = po.soft_nms_image(boxes, F([0.9, 0.005, 0.0009]), [0, 0, 0], 1, 10, 0.0)
    assert out['index'].tolist() == [0] and out['kept'] == 1
    out = po.soft_nms_image(boxes, F([0.9, 0.008, 0.0009]), [0, 0, 0], 1, 10, 0.0)       # 0.008 e^-2 = 1.08e-3 stays
    assert out['index'].tolist() == [0, 1]


def test_soft_nms_cross_class_order_cut_and_count():
    boxes = F([[0, 0, 4, 4], [0, 0, 4, 4], [10, 10, 14, 14], [10, 10, 14, 14], [30, 30, 34, 34]])
    scores = F([0.5, 0.5, 0.9, 0.25, 0.5])
    classes = [2, 0, 1, 3, 0]                           # identical boxes in different classes do not touch each other
    out = po.soft_nms_image(boxes, scores, classes, 4, 10, 0.5)
    # score descending, then class ascending, then index ascending: 0.9 | 0.5: class 0 (1, 4), class 2 (0) | 0.25
    assert out['index'].tolist() == [2, 1, 4, 0, 3] and out['classes'].tolist() == [1, 0, 0, 2, 3]
    assert out['count'] == 4 and out['kept'] == 5        # a score equal to the threshold is kept
    cut = po.soft_nms_image(boxes, scores, classes, 4, 3, 0.5)
    assert cut['index'].tolist() == [2, 1, 4] and cut['count'] == 3 and cut['kept'] == 5
    kps = np.arange(5 * 2 * 2, dtype=F).reshape(5, 2, 2)
    assert np.array_equal(po.soft_nms_image(boxes, scores, classes, 4, 3, 0.5, kps=kps)['kps'], kps[[2, 1, 4]])


def test_clustered_recipe_keeps_what_the_issue_measured_with_room_to_spare():
    kept, gap, stop = [], [], []
    for seed in range(5):
        boxes, scores = clustered(seed)
        out = po.soft_nms_image(boxes, scores, np.zeros(30, int), 1, 30, 0.1)
        kept.append(out['kept'])
        gap.append(out['margins']['gap'])
        stop.append(out['margins']['stop'])
        assert out['margins']['ties'] == 0
    assert kept == [23, 24, 22, 22, 23]
    assert min(gap) > 1e-6 and min(stop) > 1e-6
    assert min(gap) == pytest.approx(9.7e-4, rel=0.05) and min(stop) == pytest.approx(0.049, rel=0.05)


def test_mirror_merge_of_an_odd_width_map_and_the_keypoint_rule():
    assert po.mirror(np.arange(5)).tolist() == [4, 3, 2, 1, 0]          # the middle column stays
    prob = np.zeros((2, 1, 1, 3), F)
    prob[0, 0, 0], prob[1, 0, 0] = [0.2, 0.4, 0.6], [0.8, 0.5, 0.1]
    wh = np.zeros((2, 3, 1, 3), F)
    wh[0, :, 0], wh[1, :, 0] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]], [[10, 20, 30], [40, 50, 60], [70, 80, 90]]
    reg = np.stack([np.full((2, 1, 3), 1, F), np.full((2, 1, 3), 2, F)])
    kps = np.zeros((2, 4, 1, 3), F)                     # J = 2: channels x0, y0, x1, y1
    kps[0, :, 0] = [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]]
    kps[1, :, 0] = [[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]]
    out = po.tta_merge(prob, wh, reg, kps, perm=[1, 0])
    assert np.array_equal(out['hm'][0, 0, 0], F(0.5) * (F([0.2, 0.4, 0.6]) + F([0.1, 0.5, 0.8])))
    assert out['wh'][0, :, 0].tolist() == [[15.5, 11, 6.5], [32, 27.5, 23], [7, 8, 9]]      # the angle is not averaged
    assert np.array_equal(out['reg'], reg[:1])
    # x_0 = (x_0 - M x'_1) / 2, y_0 = (y_0 + M y'_1) / 2, and joint 1 takes the mirrored pass's joint 0
    assert out['kps'][0, :, 0].tolist() == [[-44.5, -39.5, -34.5], [61, 56, 51], [-13.5, -8.5, -3.5], [32, 27, 22]]
    same = po.tta_merge(prob, wh, reg, kps)
    assert same['kps'][0, 0, 0].tolist() == [-14.5, -9.5, -4.5] and 'kps' not in po.tta_merge(prob, wh, reg)


def test_projection_bounds_the_four_corners_clips_and_keeps_a_score_at_the_threshold():
    thr = 0.3
    dets = F([[[2, 1, 6, 3, 0.9, 2], [-4, 2, 5, 30, F(thr), 0], [40, 50, 44, 60, 0.2, 1]]])
    shear = [[1.0, 0.5, 1.0, 0.25, 2.0, -1.0]]         # X = x + y/2 + 1, Y = x/4 + 2y - 1: every corner matters
    out = po.project(dets, None, shear, [[20, 10]], thr)
    # corners (2,1) (6,1) (6,3) (2,3) -> X 3.5, 7.5, 8.5, 4.5; Y 1.5, 2.5, 6.5, 5.5
    assert out['boxes'][0, 0].tolist() == [3.5, 1.5, 8.5, 6.5]
    # corners (-4,2) (5,2) (5,30) (-4,30) -> X -2, 7, 21, 12; Y 2, 4.25, 60.25, 58 -> clipped to w = 10, h = 20
    assert out['boxes'][0, 1].tolist() == [0.0, 2.0, 10.0, 20.0]
    assert out['boxes'][0, 2].tolist() == [10.0, 20.0, 10.0, 20.0]        # outside: collapses onto the border
    assert out['counts'].tolist() == [2] and out['classes'].tolist() == [[2, 0, 1]]
    assert po.project(dets, None, shear, [[20, 10]], np.nextafter(F(thr), F(1)))['counts'].tolist() == [1]
    kps = F([[[[2, 1]], [[-4, 30]], [[0, 0]]]])
    assert po.project(dets, kps, shear, [[20, 10]], thr)['kps'][0, :, 0].tolist() == [[3.5, 1.5], [12, 58], [1, -1]]
    # scale: the geometry (not the score) is multiplied first
    assert po.project(dets, None, [[1, 0, 0, 0, 1, 0]], [[100, 100]], thr, scale=4.0)['boxes'][0, 0].tolist() == [8, 4, 24, 12]


def test_projection_of_a_rotated_box_follows_rotate_bboxes_without_truncation():
    from utils.box import rotate_bboxes
    dets = F([[[10, 20, 4, 8, 90, 0.5, 0], [7.5, 3.25, 3, 5, -30, 0.4, 1]]])
    out = po.project(dets, None, [[1, 0, 0, 0, 1, 0]], [[5, 5]], 0.0, rotated=True)
    np.testing.assert_allclose(out['boxes'][0, 0], [[14, 18], [14, 22], [6, 22], [6, 18]], atol=1e-12)   # not clipped
    # a box in general position (no coordinate near an integer): truncated, it is rotate_bboxes' polygon
    assert np.array_equal(np.trunc(out['boxes'][0, 1]).astype(int), rotate_bboxes(dets[0, 1:, :5].astype(np.float64))[0])
    moved = po.project(dets, None, [[2, 0, 1, 0, 3, -1]], [[5, 5]], 0.0, rotated=True)
    np.testing.assert_allclose(moved['boxes'][0, 0], [[29, 53], [29, 65], [13, 65], [13, 53]], atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# predict.py on the host
# ---------------------------------------------------------------------------------------------------------------------
class Backend:
    down_ratio = 4

    def __init__(self, J=0):
        self.heads = {'hm': 6, 'wh': 2, 'reg': 2, **({'kps': 2 * J} if J else {})}


def test_scale_size_rule():
    import predict
    assert [predict.scale_size(512, s) for s in (0.5, 0.75, 1.0, 1.25, 1.5)] == [256, 384, 512, 640, 768]
    assert predict.scale_size(64, 0.1) == 64 and predict.scale_size(512, 0.1) == 64       # the floor
    assert predict.scale_size(80, 1.0) == 96 and predict.scale_size(79, 1.0) == 64        # 2.5 rounds up, 2.47 down
    p = predict.Predictor(Backend(), (64, 96), scales=(1.0, 1.5), max_detections=20)
    assert p.sizes == [(64, 96), (96, 160)] and p.soft_nms is True
    assert predict.Predictor(Backend(), (64, 64), max_detections=20).soft_nms is False
    assert predict.Predictor(Backend(), (64, 64), max_detections=20, soft_nms=True).soft_nms is True


def test_every_refusal_names_its_argument_and_needs_no_gpu():
    import predict
    P = predict.Predictor
    with pytest.raises(ValueError, match='scales.*rotated'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, scales=(1.0, 1.5))
    with pytest.raises(ValueError, match='soft_nms.*rotated'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, soft_nms=True)
    for bad in ((), (1.0, 0.0), (-1.0,), (float('nan'),)):
        with pytest.raises(ValueError, match='scales'):
            P(Backend(), (64, 64), max_detections=20, scales=bad)
    for bad in (((0, 3),), ((0, 0),), ((0, 1), (1, 2)), ((0, 1, 2),), ((-1, 1),)):
        with pytest.raises(ValueError, match='flip_pairs'):
            P(Backend(J=3), (64, 64), max_detections=20, flip_pairs=bad)
    with pytest.raises(ValueError, match='flip_pairs'):
        P(Backend(), (64, 64), max_detections=20, flip_pairs=((0, 1),))                  # no keypoint head: J = 0
    with pytest.raises(ValueError, match='max_detections'):
        P(Backend(), (64, 64), max_detections=257)                                       # the map has 16 x 16 cells
    with pytest.raises(ValueError, match='max_detections'):
        P(Backend(), (128, 128), max_detections=300, scales=(0.5, 1.0))                  # the smallest scale decides
    assert P(Backend(), (64, 64), max_detections=256).max_detections == 256
    assert P(Backend(J=3), (64, 64), max_detections=20, flip_pairs=((0, 2),)).perm.tolist() == [2, 1, 0]
    assert P(Backend(J=3), (64, 64), max_detections=20).perm.tolist() == [0, 1, 2]


def test_file_lists_expand_directories_and_globs_and_come_back_sorted(tmp_path):
    import predict
    for name in ('b.png', 'a.JPG', 'c.txt', 'sub/d.png', 'z.jpeg'):
        (tmp_path / name).parent.mkdir(exist_ok=True)
        (tmp_path / name).write_bytes(b'')
    t = str(tmp_path)
    want = [os.path.join(t, n) for n in ('a.JPG', 'b.png', 'z.jpeg')]
    assert predict.expand_files([t]) == want                                             # images only, not recursive
    assert predict.expand_files([os.path.join(t, 'z.jpeg'), os.path.join(t, '*.png'), os.path.join(t, 'b.png')]) \
        == [os.path.join(t, 'b.png'), os.path.join(t, 'z.jpeg')]                         # sorted, no repeats
    assert predict.expand_files(os.path.join(t, 'sub')) == [os.path.join(t, 'sub', 'd.png')]
    assert predict.expand_files([os.path.join(t, 'c.txt')]) == [os.path.join(t, 'c.txt')]   # a named file is taken
    with pytest.raises(FileNotFoundError, match='nothing'):
        predict.expand_files([os.path.join(t, '*.gif')])


def test_write_coco_results(tmp_path):
    import predict
    axis = [{'file': '/x/one.png', 'index': 0, 'size': (10, 20), 'boxes': F([[1, 2, 4, 8], [0, 0, 5, 5]]),
             'scores': F([0.75, 0.5]), 'classes': np.int32([0, 4]), 'kps': None},
            {'file': '/x/two.png', 'index': 1, 'size': (10, 20), 'boxes': np.zeros((0, 4), F), 'scores': np.zeros(0, F),
             'classes': np.zeros(0, np.int32), 'kps': None},
            {'file': '/x/three.png', 'index': 2, 'size': (10, 20), 'boxes': F([[2, 2, 3, 3]]), 'scores': F([0.25]),
             'classes': np.int32([1]), 'kps': F([[[1, 2], [3, 4]]])}]
    path = tmp_path / 'r.json'
    got = predict.write_coco_results(axis, path)
    assert json.loads(path.read_text()) == got == [
        {'image_id': 1, 'category_id': 1, 'bbox': [1.0, 2.0, 3.0, 6.0], 'score': 0.75},
        {'image_id': 1, 'category_id': 5, 'bbox': [0.0, 0.0, 5.0, 5.0], 'score': 0.5},
        {'image_id': 3, 'category_id': 2, 'bbox': [2.0, 2.0, 1.0, 1.0], 'score': 0.25,
         'keypoints': [1.0, 2.0, 1.0, 3.0, 4.0, 1.0]}]
    ann = tmp_path / 'ann.json'
    ann.write_text(json.dumps({'images': [{'id': 70, 'file_name': 'three.png'}, {'id': 50, 'file_name': 'one.png'},
                                          {'id': 60, 'file_name': 'two.png'}]}))
    ids = predict.image_ids_from_annotations(ann)
    assert [d['image_id'] for d in predict.write_coco_results(axis, path, image_ids=ids)] == [50, 50, 70]
    with pytest.raises(KeyError, match='two.png'):        # even an image without detections must be a known one
        predict.write_coco_results(axis, path, image_ids={'one.png': 1})
    rotated = [{'file': 'r.png', 'index': 4, 'size': (9, 9), 'boxes': F([[[1, 5], [4, 1], [8, 4], [5, 8]]]),
                'scores': F([0.5]), 'classes': np.int32([2]), 'kps': None}]
    assert predict.write_coco_results(rotated, path) == [
        {'image_id': 5, 'category_id': 3, 'segmentation': [[1.0, 5.0, 4.0, 1.0, 8.0, 4.0, 5.0, 8.0]],
         'bbox': [1.0, 1.0, 7.0, 7.0], 'score': 0.5}]


def test_command_line_against_a_written_run_config(tmp_path):
    import predict
    run = tmp_path / 'run'
    (run / '.hydra').mkdir(parents=True)
    cfg = {'model': {'backend': {'name': 'resnet', 'params': {'num_layers': 18, 'num_classes': 3, 'num_keypoints': 0,
                                                              'rotated_boxes': True, 'pretrained': False}}},
           'datasets': {'training': {'params': {'input_size': [256, 256]}},
                        'validation': {'params': {'input_size': [128, 96]}}},
           'normalize': {'mean': [0.1, 0.2, 0.3], 'std': [0.4, 0.5, 0.6]},
           'max_detections': 20, 'score_threshold': 0.25, 'batch_size': 4, 'num_workers': 3, 'gpu': [2]}
    (run / '.hydra' / 'config.yaml').write_text(yaml.safe_dump(cfg))
    s = predict.settings_from_run(predict.parse_args([str(run), 'a.png']))
    assert s['backend'] == cfg['model']['backend'] and s['use_last'] and s['gpu'] == 2
    assert (s['batch_size'], s['num_workers']) == (4, 3)
    assert s['predictor'] == {'input_size': (128, 96), 'max_detections': 20, 'score_threshold': 0.25, 'rotated': True,
                              'mean': (0.1, 0.2, 0.3), 'std': (0.4, 0.5, 0.6), 'flip': False, 'scales': (1.0,),
                              'soft_nms': None, 'flip_pairs': None}
    args = predict.parse_args([str(run), 'a.png', 'dir', '--out', 'o.json', '--best', '--flip', '--scales', '0.75,1,1.25',
                               '--soft-nms', '--score-threshold', '0.5', '--batch-size', '2', '--num-workers', '0',
                               '--gpu', '1', '--annotation-file', 'ann.json', '--flip-pairs', '1-2,3-4'])
    assert args.inputs == ['a.png', 'dir'] and args.out == 'o.json' and args.annotation_file == 'ann.json'
    s = predict.settings_from_run(args)
    assert not s['use_last'] and s['gpu'] == 1 and (s['batch_size'], s['num_workers']) == (2, 0)
    p = s['predictor']
    assert p['flip'] and p['scales'] == (0.75, 1.0, 1.25) and p['soft_nms'] is True and p['score_threshold'] == 0.5
    assert p['flip_pairs'] == ((1, 2), (3, 4))
    with pytest.raises(SystemExit):
        predict.parse_args([str(run), 'a.png', '--scales', 'big'])
    with pytest.raises(FileNotFoundError, match='config.yaml'):
        predict.settings_from_run(predict.parse_args([str(tmp_path), 'a.png']))
    # the driver's own defaults carry every key the tool reads
    from utils.config import load_config, to_plain
    (run / '.hydra' / 'config.yaml').write_text(yaml.safe_dump(to_plain(load_config(
        os.path.join(ROOT, 'centernet-uda_amd', 'configs'), []))))
    d = predict.settings_from_run(predict.parse_args([str(run), 'a.png']))
    assert d['backend']['name'] == 'dla' and d['predictor']['input_size'] == (512, 512)
    assert d['predictor']['max_detections'] == 150 and d['batch_size'] == 16


def test_inverse_matrices_invert_the_resize():
    import predict
    from datasets import AugmentParams
    params = AugmentParams.identity([[50, 70], [64, 64]], (96, 64))
    inv = predict.inverse_matrices(params)
    assert inv.dtype == np.float64 and inv.shape == (2, 6)
    np.testing.assert_allclose(inv[0], [70 / 96, 0, 0, 0, 50 / 64, 0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(inv[1], [64 / 96, 0, 0, 0, 1, 0], rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signature_table_library_and_integration_notes():
    import hip_runtime as hr
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read(), flags=re.S)
    notes = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib = ctypes.CDLL(hr.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert hasattr(hr._Sig, name) and hasattr(lib, name), name
        assert name in notes, name
    assert hr.lib().cnuda_abi_version() == hr.ABI_VERSION == 2


def test_bad_arguments_return_minus_one_with_a_message_and_touch_no_device():
    import hip_runtime as hr
    L = hr.lib()
    err = lambda: L.cnuda_last_error().decode()
    assert L.cnuda_mirror_input(None, None, 6, 5, 7, None) == -1 and 'null pointer' in err()
    assert L.cnuda_tta_merge(*[None] * 9, 2, 3, 2, 0, 5, 7, None) == -1 and 'cnuda_tta_merge' in err()
    assert L.cnuda_project_detections(*[None] * 9, 2, 5, 0, 0, 1.0, 0.1, 5, 0, None) == -1
    assert 'cnuda_project_detections' in err()
    assert L.cnuda_soft_nms_merge(*[None] * 10, 1, 8, 1, 0, 4, 0.1, None, 0, None) == -1 and 'null pointer' in err()
    # host addresses stand in for device pointers: every check below fails before anything is launched
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    limit = 2048
    assert L.cnuda_predict_workspace_bytes(2, 1200) >= 2 * 1200 * 8 and L.cnuda_predict_workspace_bytes(1, limit) > 0
    assert L.cnuda_predict_workspace_bytes(1, limit + 1) == 0 and str(limit) in err()
    assert L.cnuda_soft_nms_merge(*[p] * 3, None, None, *[p] * 3, None, p, 1, limit + 1, 1, 0, 4, 0.1, p, 1 << 30,
                                  None) == -1
    assert 'exceed' in err() and str(limit) in err()
    need = L.cnuda_predict_workspace_bytes(1, 8)
    assert L.cnuda_soft_nms_merge(*[p] * 3, None, None, *[p] * 3, None, p, 1, 8, 1, 0, 4, 0.1, p, need - 1, None) == -1
    assert 'workspace too small' in err()
    assert L.cnuda_project_detections(p, None, p, p, p, p, p, None, p, 2, 5, 0, 0, 1.0, 0.1, 4, 0, None) == -1
    assert 'output rows' in err()
    assert L.cnuda_tta_merge(p, p, None, None, None, p, p, None, None, 2, 3, 4, 0, 5, 7, None) == -1 and 'channels' in err()
    assert L.cnuda_mirror_input(p, p, 1, 2, 2, None) == -1 and 'overlap' in err()
