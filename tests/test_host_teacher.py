"""Mean teacher without a GPU: the numpy oracle of tests/teacher_oracle.py pinned by hand-worked cases, the decay
schedule, how the driver resolves `uda.MeanTeacher`, and every refusal."""
import os

import numpy as np
import pytest

import teacher_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'centernet-uda_amd', 'configs')
OVERRIDE = 'model.uda={MeanTeacher: {pseudo_weight: 1.0, score_threshold: 0.4, burn_in_steps: 2000}}'
F = np.float32


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(num_classes=3, num_keypoints=0, rotated=False):
    return Cfg(max_detections=20, model=Cfg(backend=Cfg(params=Cfg(
        rotated_boxes=rotated, num_classes=num_classes, num_keypoints=num_keypoints))))


# -- the oracle, by hand ---------------------------------------------------------------------------------------------
def test_oracle_filter_threshold_class_and_nan_by_hand():
    """C = 2, thresholds (0.5, 0.25).  Row 0 sits exactly on its class threshold (kept), row 1 below its own, row 2 names
    class C (dropped), row 3 has a NaN corner (dropped), row 4 a fractional class (dropped), row 5 is kept: the
    survivors are rows 0 and 5, in that order."""
    dets = F([[[1, 2, 5, 6, 0.5, 0],
               [1, 2, 5, 6, 0.2, 1],
               [1, 2, 5, 6, 0.9, 2],
               [1, np.nan, 5, 6, 0.9, 0],
               [1, 2, 5, 6, 0.9, 0.5],
               [0, 1, 3, 4, 0.25, 1]]])
    out = to.pseudo_labels(dets, F([0.5, 0.25]), 8)
    assert out['counts'].tolist() == [2] and out['kept'] == F(2.0) and out['kept'].dtype == np.float32
    assert out['classes'].tolist() == [[0, 1, 0, 0, 0, 0]] and out['classes'].dtype == np.int32
    assert out['boxes'].dtype == np.float64
    assert out['boxes'][0].tolist() == [[1, 2, 5, 6], [0, 1, 3, 4], [0] * 4, [0] * 4, [0] * 4, [0] * 4]
    # negative class, infinite score is fine (it is a score), infinite geometry is not
    dets = F([[[1, 2, 5, 6, 0.9, -1], [1, 2, 5, 6, np.inf, 0], [1, 2, np.inf, 6, 0.9, 0], [1, 2, 5, 6, np.nan, 0]]])
    out = to.pseudo_labels(dets, F([0.5]), 8)
    assert out['counts'].tolist() == [1] and out['boxes'][0, 0].tolist() == [1, 2, 5, 6]


def test_oracle_mirror_and_min_size_by_hand():
    dets = F([[[1, 2, 5, 6, 0.9, 0]]])
    out = to.pseudo_labels(dets, F([0.1]), 8, mirror=True)
    assert out['boxes'][0, 0].tolist() == [3, 2, 7, 6]
    # extents 4 x 4: kept at min_size 4 (equality keeps), dropped just above; one short side is enough to drop
    assert to.pseudo_labels(dets, F([0.1]), 8, min_size=4.0)['counts'].tolist() == [1]
    assert to.pseudo_labels(dets, F([0.1]), 8, min_size=np.nextafter(F(4), F(5)))['counts'].tolist() == [0]
    thin = F([[[1, 2, 5, 3, 0.9, 0]]])
    assert to.pseudo_labels(thin, F([0.1]), 8, min_size=2.0)['counts'].tolist() == [0]
    assert to.pseudo_labels(thin, F([0.1]), 8, min_size=1.0)['counts'].tolist() == [1]
    # kept is the mean over images: 1 survivor in 2 images
    two = F([[[1, 2, 5, 6, 0.9, 0]], [[1, 2, 5, 6, 0.0, 0]]])
    out = to.pseudo_labels(two, F([0.1]), 8)
    assert out['counts'].tolist() == [1, 0] and out['kept'] == F(0.5)


def test_oracle_rotated_box_at_ninety_degrees_by_hand():
    """Centre (3, 2), w = 4, h = 2, 90 degrees: cos = 0, sin = 1, a vertex offset (ox, oy) lands at (-oy, ox): the vertices
    (-2,-1), (2,-1), (2,1), (-2,1) become (1,-2), (1,2), (-1,2), (-1,-2), i.e. (4,0), (4,4), (2,4), (2,0).  Mirrored at
    W = 8: x -> 8 - x, the vertex order stays: (4,0), (4,4), (6,4), (6,0)."""
    dets = F([[[3, 2, 4, 2, 90, 0.9, 0]]])
    out = to.pseudo_labels(dets, F([0.1]), 8, rotated=True)
    assert out['corners'].shape == (1, 1, 4, 2) and out['counts'].tolist() == [1]
    assert np.abs(out['corners'][0, 0] - [[4, 0], [4, 4], [2, 4], [2, 0]]).max() < 1e-12
    out = to.pseudo_labels(dets, F([0.1]), 8, rotated=True, mirror=True)
    assert np.abs(out['corners'][0, 0] - [[4, 0], [4, 4], [6, 4], [6, 0]]).max() < 1e-12
    # the extents of a rotated row are its w and h columns; a NaN angle drops it
    assert to.pseudo_labels(dets, F([0.1]), 8, rotated=True, min_size=2.0)['counts'].tolist() == [1]
    assert to.pseudo_labels(dets, F([0.1]), 8, rotated=True, min_size=2.5)['counts'].tolist() == [0]
    dets[0, 0, 4] = np.nan
    assert to.pseudo_labels(dets, F([0.1]), 8, rotated=True)['counts'].tolist() == [0]


def test_oracle_ema_is_two_rounded_products_and_a_rounded_sum():
    t, s = F([1.0, 3.0, -2.5]), F([2.0, 1.0, 0.5])
    assert to.ema(t, s, 0.5).tolist() == [1.5, 2.0, -1.0]
    assert to.ema(t, s, 0.0).tolist() == s.tolist()
    d = F(0.999)
    omd = F(1) - d
    want = [float(F(F(a * d) + F(b * omd))) for a, b in zip(t, s)]
    assert to.ema(t, s, 0.999).tolist() == want and to.ema(t, s, 0.999).dtype == np.float32
    assert omd != F(0.001)                                    # float32(1) - float32(0.999), not float32(0.001)


def test_decay_schedule():
    from uda.mean_teacher import decay_at
    for fn in (to.decay_t, decay_at):
        assert fn(0.999, 0) == 0.1
        assert fn(0.999, 1) == 2.0 / 11.0
        assert fn(0.999, 90) == 0.91
        assert fn(0.999, 10 ** 6) == 0.999
        assert fn(0.05, 0) == 0.05


# -- the driver's view ------------------------------------------------------------------------------------------------
def test_the_driver_resolves_mean_teacher_from_the_readme_override():
    import train
    import uda
    from utils.config import load_config
    cls = train.resolve_plugin('MeanTeacher')
    assert cls is uda.MeanTeacher and issubclass(cls, uda.Model) and 'MeanTeacher' in dir(uda)
    cfg = load_config(CONFIGS, ['experiment=dla_baseline', OVERRIDE,
                                'datasets.training.params.target_domain_glob=[/data/target/images/*.jpg]'])
    got, args = train.plugin_from_config(cfg.model.uda)
    assert got is cls and args == {'pseudo_weight': 1.0, 'score_threshold': 0.4, 'burn_in_steps': 2000}
    plugin = got(**args)
    assert (plugin.pseudo_weight, plugin.decay, plugin.score_threshold, plugin.burn_in_steps, plugin.mirror_student,
            plugin.min_size, plugin.evaluate_teacher) == (1.0, 0.999, 0.4, 2000, True, 2.0, False)
    assert plugin.target_grad_heads == ('hm', 'wh', 'reg')
    plugin.cfg = cfg
    plugin.init_done()                                        # dla_baseline: no keypoints, any class count
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert OVERRIDE in readme


def test_signature():
    import inspect
    import uda
    params = inspect.signature(uda.MeanTeacher.__init__).parameters
    assert list(params)[1:] == ['pseudo_weight', 'decay', 'score_threshold', 'burn_in_steps', 'mirror_student', 'min_size',
                                'evaluate_teacher']
    assert [params[k].default for k in list(params)[2:]] == [0.999, 0.4, 0, True, 2.0, False]


def test_refusals_name_the_argument():
    import uda
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='decay'):
            uda.MeanTeacher(1.0, decay=bad)
    uda.MeanTeacher(1.0, decay=0.0)
    with pytest.raises(ValueError, match='pseudo_weight'):
        uda.MeanTeacher(-1e-3)
    uda.MeanTeacher(0.0)
    plugin = uda.MeanTeacher(1.0, score_threshold=[0.3, 0.4])
    plugin.cfg = _cfg(num_classes=3)
    with pytest.raises(ValueError, match='score_threshold'):
        plugin.init_done()
    plugin.cfg = _cfg(num_classes=2)
    plugin.init_done()
    assert plugin._threshold_list() == [0.3, 0.4]
    plugin = uda.MeanTeacher(1.0)
    plugin.cfg = _cfg(num_keypoints=4)
    with pytest.raises(ValueError, match='num_keypoints'):
        plugin.init_done()
    plugin.cfg = _cfg(num_classes=5)
    plugin.init_done()
    assert plugin._threshold_list() == [0.4] * 5


# -- host-side plumbing -------------------------------------------------------------------------------------------------
def test_segment_table_layout_and_block_prefix():
    from hip_runtime import ops
    table, blocks = ops.ema_segment_table([(1000, 2000, 0, 0), (16, 32, 1, 0), (64, 128, 4096, 0), (256, 512, 4097, 0),
                                           (7, 9, 8, 1)])
    assert table.dtype.itemsize == 32 and blocks == 1 + 1 + 2 + 1
    assert table['block0'].tolist() == [0, 1, 2, 4] and table['kind'].tolist() == [0, 0, 0, 1]
    assert table['count'].tolist() == [1, 4096, 4097, 8] and table['dst'].tolist() == [16, 64, 256, 7]
    assert ops.ema_segment_table([])[1] == 0


def test_one_bump_carries_several_buffers_and_deferred_bumps_end_as_one():
    import torch
    import hip_runtime as hr
    a, b = torch.zeros(4), torch.zeros(4)
    e = hr._PARAM_EPOCH
    hr.bump_param_epoch()
    hr.bump_param_epoch(a)
    hr.bump_param_epoch([a, b])
    hr.bump_param_epoch((a,))
    hr.bump_param_epoch([])
    assert hr._PARAM_EPOCH == e + 5
    with hr.single_param_epoch():
        hr.bump_param_epoch(a)
        hr.bump_param_epoch(b)
        hr.bump_param_epoch()
        assert hr._PARAM_EPOCH == e + 5
    assert hr._PARAM_EPOCH == e + 6
    with hr.single_param_epoch():
        pass
    assert hr._PARAM_EPOCH == e + 6
    with pytest.raises(RuntimeError, match='nest'):
        with hr.single_param_epoch():
            with hr.single_param_epoch():
                pass
    assert hr._HELD is None
    with pytest.raises(RuntimeError, match='MI355X only'):
        hr.ops.EmaPlan([a], [b])
    with pytest.raises(RuntimeError, match='MI355X only'):
        hr.ops.pseudo_labels(torch.zeros(1, 2, 6), torch.zeros(1), 8)


def test_teacher_is_a_separate_copy_on_one_flat_buffer_and_checkpoints_round_trip(tmp_path):
    """Everything about the teacher that needs no kernel: built in to(), equal to the student, not part of its state_dict,
    frozen, unknown to the optimizer, its trainable parameters views of one buffer with the arena's layout, fresh pack
    tokens; save_model / load_model in the driver's order (load before to) and afterwards."""
    import torch
    import uda
    from backends import resnet
    from hip_runtime import optim
    from hip_runtime.arena import ParamArena
    from uda.base import Model

    def make(seed):
        torch.manual_seed(seed)
        p = uda.MeanTeacher(1.0, score_threshold=[0.3, 0.4, 0.5])
        p.cfg, p.device = _cfg(), torch.device('cpu')
        p.backend = resnet.build(18, num_classes=3, pretrained=False)
        p.optimizer = optim.Adam([q for q in p.backend.parameters() if q.requires_grad], lr=1e-3)
        p.init_done()
        return p
    p = make(0)
    p.optimizer.zero_grad()                    # the student's parameters become views of the arena first
    keys = list(p.backend.state_dict())
    p.to('cpu')
    t, m = p.teacher, p.backend
    assert list(m.state_dict()) == keys and not t.training and m.training
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr()
               for a, b in zip(m.state_dict().values(), t.state_dict().values()))
    mine = {id(q) for q in t.parameters()}
    assert all(not q.requires_grad for q in t.parameters())
    assert not any(id(q) in mine for g in p.optimizer.param_groups for q in g['params'])
    arena = p.optimizer._ensure()
    assert ParamArena.layout(arena.params) == (arena.offsets, arena.numel)
    assert p.teacher_flat.numel() == arena.numel
    for q, o in zip(t.parameters(), arena.offsets):
        assert q.data_ptr() == p.teacher_flat.data_ptr() + 4 * o
    assert p._student_flat(p._pairs[1]) is arena.flat_param
    tokens = lambda mod: {int(x._pack_token) for x in mod.modules() if hasattr(x, '_pack_token')}
    assert tokens(m) and tokens(m).isdisjoint(tokens(t)) and len(tokens(m)) == len(tokens(t))
    # checkpoints
    with torch.no_grad():
        p.teacher_flat.mul_(0.5)
        next(t.buffers()).add_(1.0)
    p.teacher_updates = 7
    path = str(tmp_path / 'model_last.pth')
    p.save_model(path, 3, True)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ck) == ['epoch', 'optimizer', 'state_dict', 'teacher_state_dict', 'teacher_updates']
    assert list(ck['state_dict']) == keys and ck['teacher_updates'] == 7

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    q = make(1)
    assert q.load_model(path, True) == 4       # the driver's order: load, then to()
    q.to('cpu')
    assert q.teacher_updates == 7 and same(q.teacher, t) and same(q.backend, m) and not same(q.teacher, q.backend)
    q = make(2)
    q.to('cpu')
    assert q.load_model(path, False) == 0      # pretrained: the teacher's weights, not its update count
    assert q.teacher_updates == 0 and same(q.teacher, t) and same(q.backend, m)
    # a checkpoint of the plain plugin: the teacher starts as the loaded student
    base = Model()
    base.backend, base.optimizer = m, None
    plain = str(tmp_path / 'plain.pth')
    base.save_model(plain, 5)
    assert sorted(torch.load(plain, map_location='cpu', weights_only=False)) == ['epoch', 'state_dict']
    for after_to in (False, True):
        q = make(3)
        if after_to:
            q.to('cpu')
        q.load_model(plain, True)
        if not after_to:
            q.to('cpu')
        assert same(q.teacher, m) and same(q.backend, m) and q.teacher_updates == 0


def test_predict_teacher_flag_selects_the_entry_and_names_the_file_when_it_is_absent(tmp_path):
    import torch
    import export
    import predict
    from backends import resnet
    args = predict.parse_args(['run', 'a.png', '--teacher'])
    assert args.teacher and not predict.parse_args(['run', 'a.png']).teacher
    spec = {'name': 'resnet', 'params': {'num_layers': 18, 'num_classes': 2, 'pretrained': False}}
    torch.manual_seed(4)
    a, b = resnet.build(18, num_classes=2, pretrained=False), resnet.build(18, num_classes=2, pretrained=False)
    torch.save({'epoch': 1, 'state_dict': a.state_dict(), 'teacher_state_dict': b.state_dict(), 'teacher_updates': 3},
               tmp_path / 'model_last.pth')
    got = export.build_model(str(tmp_path), spec, True, 10, state_key='teacher_state_dict')
    assert all(torch.equal(x, y) for x, y in zip(got.state_dict().values(), b.state_dict().values()))
    got = export.build_model(str(tmp_path), spec, True, 10)
    assert all(torch.equal(x, y) for x, y in zip(got.state_dict().values(), a.state_dict().values()))
    torch.save({'epoch': 1, 'state_dict': a.state_dict()}, tmp_path / 'model_last.pth')
    with pytest.raises(KeyError, match='model_last.pth'):
        export.build_model(str(tmp_path), spec, True, 10, state_key='teacher_state_dict')
