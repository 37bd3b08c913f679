"""The rotated-box IoU without a GPU: the float64 restatement (tests/polyiou_oracle.py) against exact rational
arithmetic and against answers worked by hand, the device function itself (csrc/polyiou.cuh) run on the CPU by a
stand-alone program under the sanitizers and compared bit for bit, the new C entry points' argument checks, the
predictor's and the command line's rules for `soft_nms='polygon'`, and `rotate_bboxes_float`."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import yaml

import polyiou_oracle as pio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ('cnuda_quad_iou_pairs', 'cnuda_eval_iou_quads', 'cnuda_soft_nms_merge_rotated')
# Required, not measured: well under half a float32 unit at 1 (3e-8) -- scores leave the kernels as float32.
# The case set below gives a worst error of 9.3e-11 ("Rotated IoU").
IOU_ERROR_BOUND = 1e-9


def square(x, y, side):
    return F([[x, y], [x + side, y], [x + side, y + side], [x, y + side]])


DIAMOND = F([[2, -1], [5, 2], [2, 5], [-1, 2]])          # |x - 2| + |y - 2| <= 3


def hand_cases():
    """[(name, a, b, exact IoU)]"""
    nan = square(0, 0, 4)
    nan[1, 0] = np.nan
    inf = square(0, 0, 4)
    inf[2, 1] = np.inf
    return [
        ('identical squares', square(0, 0, 4), square(0, 0, 4), Fraction(1)),
        ('shifted by half a side', square(0, 0, 4), square(2, 0, 4), Fraction(1, 3)),
        ('sharing an edge', square(0, 0, 4), square(4, 0, 4), Fraction(0)),
        ('sharing a corner', square(0, 0, 4), square(4, 4, 4), Fraction(0)),
        ('2-square inside a 4-square', square(1, 1, 2), square(0, 0, 4), Fraction(1, 4)),
        ('4-square around a 2-square', square(0, 0, 4), square(1, 1, 2), Fraction(1, 4)),
        ('square against diamond: an octagon', square(0, 0, 4), DIAMOND, Fraction(14, 20)),
        ('the octagon, both windings reversed', square(0, 0, 4)[::-1], DIAMOND[::-1], Fraction(14, 20)),
        ('the octagon, one winding reversed', square(0, 0, 4), DIAMOND[::-1], Fraction(14, 20)),
        ('four collinear points', F([[0, 0], [1, 1], [2, 2], [3, 3]]), square(0, 0, 4), Fraction(0)),
        ('a NaN vertex', nan, square(0, 0, 4), Fraction(0)),
        ('an infinite vertex in the clipper', square(0, 0, 4), inf, Fraction(0)),
    ]


@pytest.fixture(scope='module')
def cases():
    return pio.case_set(4000)


def test_hand_answers_are_exact():
    for name, a, b, want in hand_cases():
        got = pio.quad_iou(a, b)[0]
        assert isinstance(got, float) and got == float(want), (name, got, want)
        assert pio.quad_iou(a, b, Fraction)[0] == want, name
    octagon = pio.quad_iou(square(0, 0, 4), DIAMOND)
    assert octagon == (0.7, 16.0, 18.0) and pio.intersection_size(square(0, 0, 4), DIAMOND) == 8
    again = pio.quad_iou(square(0, 0, 4)[::-1], DIAMOND[::-1])
    assert np.float64(octagon[0]).tobytes() == np.float64(again[0]).tobytes() and again[1:] == (16.0, 18.0)
    assert pio.quad_iou(hand_cases()[10][1], square(0, 0, 4)) == (0.0, 0.0, 0.0)          # non-finite: areas are 0 too


def test_restatement_against_exact_arithmetic(cases):
    a, b = cases
    worst, sizes, reversed_pairs = Fraction(0), set(), 0
    for i in range(len(a)):
        got = pio.quad_iou(a[i], b[i])[0]
        exact = pio.quad_iou(a[i], b[i], Fraction)[0]
        assert 0.0 <= got <= 1.0
        worst = max(worst, abs(Fraction(got) - exact))
        sizes.add(pio.intersection_size(a[i], b[i]))
        reversed_pairs += pio.quad_iou(a[i], b[i])[1] > 0 and _signed(a[i]) * _signed(b[i]) < 0
    print('worst |float64 - exact| over %d pairs: %.3g' % (len(a), float(worst)))
    assert float(worst) <= IOU_ERROR_BOUND
    assert sizes == set(range(9))                          # every intersection size from 0 to 8 vertices
    assert reversed_pairs >= len(a) // 6                   # one pair in five has one winding reversed
    assert np.abs(a).max() <= 4096 + 1 and np.abs(b).max() <= 4096 + 600


def _signed(q):
    x, y = q[:, 0].astype(np.float64), q[:, 1].astype(np.float64)
    return float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def test_device_function_on_the_cpu_equals_the_restatement_bit_for_bit(cases, tmp_path):
    """csrc/polyiou.cuh is what the kernels run.  The stand-alone program (address + undefined-behaviour sanitizers on
    the host side) calls it pair by pair on the CPU; IoU and both areas must be the restatement's bits."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    exe = str(tmp_path / 'polyiou_host')
    subprocess.check_call([hipcc, '-O2', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-Xarch_host',
                           '-fsanitize=address,undefined', '-I', os.path.join(ROOT, 'centernet-uda_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'polyiou_host.cpp'), '-o', exe])
    hand = hand_cases()
    bow = F([[0, 0], [4, 4], [4, 0], [0, 4]])              # self-crossing: unspecified, but finite and inside [0, 1]
    dart = F([[0, 0], [4, 0], [1, 1], [0, 4]])             # not convex
    odd = [(bow, square(0, 0, 4)), (square(0, 0, 4), bow), (bow, F([[1, 0], [3, 4], [3, 0], [1, 4]])),
           (dart, dart), (dart, square(0, 0, 4)), (square(0, 0, 4) * F(1e30), DIAMOND * F(1e30))]
    a = np.concatenate([cases[0], np.stack([h[1] for h in hand]), np.stack([o[0] for o in odd])])
    b = np.concatenate([cases[1], np.stack([h[2] for h in hand]), np.stack([o[1] for o in odd])])
    a.tofile(str(tmp_path / 'a.bin'))
    b.tofile(str(tmp_path / 'b.bin'))
    subprocess.check_call([exe, str(tmp_path / 'a.bin'), str(tmp_path / 'b.bin'), str(len(a)), str(tmp_path / 'out.bin')])
    got = np.fromfile(str(tmp_path / 'out.bin'), dtype=np.float64).reshape(len(a), 4)
    want = np.array([pio.quad_iou(a[i], b[i]) for i in range(len(a))], dtype=np.float64)
    assert got[:, :3].tobytes() == want.tobytes(), np.flatnonzero((got[:, :3] != want).any(1))[:8]
    alone = np.array([pio.quad_iou(q, square(0, 0, 1))[1] for q in a], dtype=np.float64)     # beside a finite partner
    assert got[:, 3].tobytes() == alone.tobytes()                                      # quad_area: what the entries report
    assert np.isfinite(got).all() and (got[:, 0] >= 0).all() and (got[:, 0] <= 1).all()


def test_rotated_soft_nms_oracle_by_hand():
    q = np.stack([square(0, 0, 4), square(0, 0, 4)[::-1], square(20, 20, 4)])
    out = pio.soft_nms_image(q, F([0.9, 0.5, 0.25]), [0, 0, 0], 1, 10, 0.0)
    assert out['index'].tolist() == [0, 2, 1]
    assert out['scores'].tolist() == [float(F(0.9)), 0.25, float(F(0.5)) * float(np.exp(-2.0))]    # iou 1: exp(-1 / 0.5)
    assert out['boxes'].shape == (3, 4, 2) and np.array_equal(out['boxes'][2], q[1])               # rows are copied as given
    tied = pio.soft_nms_image(np.stack([square(10 * i, 0, 4) for i in range(3)]), F([0.5, 0.7, 0.5]), [0, 0, 0], 1, 10, 0.0)
    assert tied['index'].tolist() == [1, 0, 2] and tied['margins']['ties'] >= 1


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
    # host addresses stand in for device pointers: every check below fails before anything is launched
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert L.cnuda_quad_iou_pairs(None, None, None, None, None, 2, 5, 3, None) == -1
    assert 'cnuda_quad_iou_pairs' in err() and 'null pointer' in err()
    assert L.cnuda_quad_iou_pairs(p, p, None, None, None, 2, 5, 3, None) == -1 and 'null pointer' in err()
    assert L.cnuda_quad_iou_pairs(p, p, p, None, None, 0, 5, 3, None) == -1 and 'bad sizes' in err()
    assert L.cnuda_quad_iou_pairs(p, p, p, None, None, 1, -1, 3, None) == -1 and 'bad sizes' in err()
    assert L.cnuda_quad_iou_pairs(None, None, None, None, None, 3, 0, 0, None) == 0           # nothing to do
    assert L.cnuda_eval_iou_quads(None, None, 3, 10, 10, 100, None, None, None) == -1
    assert 'cnuda_eval_iou_quads' in err() and 'null pointer' in err()
    assert L.cnuda_eval_iou_quads(p, None, 3, 10, 10, 100, p, p, None) == -1 and 'null pointer' in err()
    assert L.cnuda_eval_iou_quads(p, p, 3, 10, 10, -1, p, p, None) == -1 and 'negative' in err()
    assert L.cnuda_eval_iou_quads(p, p, -1, 10, 10, 100, p, p, None) == -1 and 'negative' in err()
    assert L.cnuda_eval_iou_quads(None, None, 0, 0, 0, 0, None, None, None) == 0              # no box at all
    assert L.cnuda_soft_nms_merge_rotated(*[None] * 10, 1, 8, 1, 0, 4, 0.1, None, 0, None) == -1
    assert 'cnuda_soft_nms_merge_rotated' in err() and 'null pointer' in err()
    limit = 2048
    assert L.cnuda_soft_nms_merge_rotated(*[p] * 3, None, None, *[p] * 3, None, p, 1, limit + 1, 1, 0, 4, 0.1, p, 1 << 30,
                                          None) == -1
    assert 'exceed' in err() and str(limit) in err()
    need = L.cnuda_predict_workspace_bytes(1, 8)
    assert L.cnuda_soft_nms_merge_rotated(*[p] * 3, None, None, *[p] * 3, None, p, 1, 8, 1, 0, 4, 0.1, p, need - 1,
                                          None) == -1
    assert 'workspace too small' in err()
    assert L.cnuda_soft_nms_merge_rotated(*[p] * 3, None, None, *[p] * 3, p, p, 1, 8, 1, 0, 4, 0.1, p, need, None) == -1
    assert 'kps' in err()
    assert L.cnuda_soft_nms_merge_rotated(*[p] * 3, None, None, *[p] * 3, None, p, 1, 8, 0, 0, 4, 0.1, p, need, None) == -1
    assert 'bad sizes' in err()


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    import predict
    from hip_runtime import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.rotated_iou(z(1, 2, 4, 2), z(1, 3, 4, 2))
    with pytest.raises(RuntimeError, match='MI355X only'):
        predict.soft_nms_merge_rotated(z(1, 5, 4, 2), z(1, 5), z(1, 5, dtype=torch.int32), None, 3, 4, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# predict.py: the argument rules, on the stub backend of tests/test_host_predict.py
# ---------------------------------------------------------------------------------------------------------------------
class Backend:
    down_ratio = 4

    def __init__(self, J=0):
        self.heads = {'hm': 6, 'wh': 3, 'reg': 2, **({'kps': 2 * J} if J else {})}


def test_predictor_takes_polygon_soft_nms_for_rotated_models_only():
    import predict
    P = predict.Predictor
    one = P(Backend(), (64, 64), max_detections=20, rotated=True, soft_nms='polygon')
    assert one.soft_nms is True and one.rotated and one.sizes == [(64, 64)]
    two = P(Backend(J=3), (64, 96), max_detections=20, rotated=True, soft_nms='polygon', scales=(1.0, 1.5), flip=True,
            flip_pairs=((0, 2),))
    assert two.soft_nms is True and two.sizes == [(64, 96), (96, 160)] and two.perm.tolist() == [2, 1, 0]
    # every refusal of a rotated model stays exactly as it was
    with pytest.raises(ValueError, match='scales.*rotated'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, scales=(1.0, 1.5))
    with pytest.raises(ValueError, match='scales.*rotated'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, scales=(1.0, 1.5), soft_nms=True)
    with pytest.raises(ValueError, match='soft_nms.*rotated'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, soft_nms=True)
    assert P(Backend(), (64, 64), max_detections=20, rotated=True).soft_nms is False
    assert P(Backend(), (64, 64), max_detections=20, rotated=True, soft_nms=False).soft_nms is False
    with pytest.raises(ValueError, match='soft_nms'):
        P(Backend(), (64, 64), max_detections=20, soft_nms='polygon')                     # an axis-aligned model
    with pytest.raises(ValueError, match='soft_nms'):
        P(Backend(), (64, 64), max_detections=20, scales=(1.0, 1.5), soft_nms='polygon')
    with pytest.raises(ValueError, match='soft_nms'):
        P(Backend(), (64, 64), max_detections=20, rotated=True, soft_nms='mask')
    with pytest.raises(ValueError, match='candidates'):                                   # the candidate limit holds
        P(Backend(), (512, 512), max_detections=1100, rotated=True, soft_nms='polygon', scales=(1.0, 1.25))


def test_polygon_nms_flag(tmp_path):
    import predict
    run = tmp_path / 'run'
    (run / '.hydra').mkdir(parents=True)
    cfg = {'model': {'backend': {'name': 'resnet', 'params': {'num_layers': 18, 'num_classes': 3, 'num_keypoints': 0,
                                                              'rotated_boxes': True, 'pretrained': False}}},
           'datasets': {'validation': {'params': {'input_size': [128, 96]}}},
           'max_detections': 20, 'score_threshold': 0.25, 'batch_size': 4, 'num_workers': 3, 'gpu': 0}
    (run / '.hydra' / 'config.yaml').write_text(yaml.safe_dump(cfg))
    plain = predict.settings_from_run(predict.parse_args([str(run), 'a.png']))['predictor']
    assert plain['soft_nms'] is None and plain['rotated'] is True
    args = predict.parse_args([str(run), 'a.png', '--polygon-nms', '--scales', '1,1.5'])
    assert args.polygon_nms is True
    p = predict.settings_from_run(args)['predictor']
    assert p['soft_nms'] == 'polygon' and p['scales'] == (1.0, 1.5)
    assert set(p) == set(plain)                                                           # the dict gains no key
    assert predict.settings_from_run(predict.parse_args([str(run), 'a.png', '--soft-nms']))['predictor']['soft_nms'] is True
    built = predict.Predictor(Backend(), p.pop('input_size'), **p)
    assert built.soft_nms is True and built.sizes == [(128, 96), (192, 160)]


# ---------------------------------------------------------------------------------------------------------------------
# the vertices the evaluator measures
# ---------------------------------------------------------------------------------------------------------------------
def test_rotate_bboxes_float_is_rotate_bboxes_without_truncation():
    from utils.box import rotate_bboxes, rotate_bboxes_float
    # centres on the half-pixel grid the extents ask for, angles of 0 and +-90 degrees: every corner is an integer up
    # to the 1e-16 of cos(90 deg), which the single float32 rounding removes
    boxes = F([[10, 20, 4, 8, 0], [10, 20, 4, 8, 90], [5, 5, 4, 4, -90], [30.5, 12, 7, 2, 0], [100, 50, 20, 6, 0],
               [12.5, 30, 7, 2, 0]])
    got = rotate_bboxes_float(boxes)
    assert got.dtype == np.float32 and got.shape == (6, 4, 2)
    assert np.array_equal(got, np.round(got))
    assert np.array_equal(got.astype(np.int64), rotate_bboxes(boxes.astype(np.float64)))
    assert got[1].tolist() == [[14, 18], [14, 22], [6, 22], [6, 18]]                      # the corner order, turned
    # in general position: the same polygon before truncation, float64 arithmetic on the float32 values
    gen = F([[7.5, 3.25, 3, 5, -30], [640.3, 200.7, 3, 40, 30]])
    want = []
    for x, y, w, h, ang in gen.astype(np.float64):
        r = np.radians(ang)
        want.append([[x + (ox * np.cos(r) - oy * np.sin(r)), y + (ox * np.sin(r) + oy * np.cos(r))]
                     for ox, oy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))])
    assert np.array_equal(rotate_bboxes_float(gen), np.asarray(want).astype(F))
    assert np.array_equal(np.trunc(rotate_bboxes_float(gen)).astype(np.int64), rotate_bboxes(gen.astype(np.float64)))
    assert rotate_bboxes_float(np.zeros((0, 5), F)).shape == (0, 4, 2)
    with pytest.raises(ValueError, match='rotate_bboxes_float'):
        rotate_bboxes_float(np.zeros((3, 4), F))


def test_evaluator_mode_names():
    from evaluation import coco
    assert coco.ROTATED_IOU_MODES == ('mask', 'polygon')
