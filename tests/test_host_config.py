"""Config composition (utils/config.py) and the config schema: every experiment file of the reference
(tests/golden/ref_configs: verbatim copies, settings only) and of this project (centernet-uda_amd/configs), composed
with its defaults, must resolve and bind everything the driver looks up -- without building anything on a device."""
import glob
import inspect
import os
from importlib import import_module

import pytest
import torch
import yaml

from utils.config import Config, load_config, merge, run_dir, to_plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, 'tests', 'golden', 'ref_configs')
OWN = os.path.join(ROOT, 'centernet-uda_amd', 'configs')


def _experiments(config_dir):
    return sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(config_dir, 'experiment', '*.yaml')))


CASES = [(REF, n) for n in _experiments(REF)] + [(OWN, n) for n in _experiments(OWN)]


def test_the_fixture_and_the_project_both_have_their_files():
    assert len(_experiments(REF)) == 12 and os.path.isfile(os.path.join(REF, 'defaults.yaml'))
    assert len(_experiments(OWN)) == 5 and os.path.isfile(os.path.join(OWN, 'defaults.yaml'))


def _bind(callable_, *args, **kwargs):
    try:
        inspect.signature(callable_).bind(*args, **kwargs)
    except TypeError as e:
        raise AssertionError("%s does not take %s: %s" % (getattr(callable_, '__qualname__', callable_),
                                                           sorted(kwargs), e)) from None


def _check_dataset(spec, defaults, merged_member=False):
    from datasets import Augmentation
    cls = import_module('datasets.%s' % spec.name).Dataset
    params = {**defaults, **spec.params} if merged_member else {**spec.params, **defaults}
    _bind(cls, **params)
    if spec.name == 'coco_merger':
        member_defaults = {k: v for k, v in params.items() if k not in ('datasets', 'max_samples')}
        assert len(params['datasets']) >= 1
        for member in params['datasets']:
            _check_dataset(member, member_defaults, merged_member=True)
    elif params.get('augmentation'):
        Augmentation(params['augmentation'])            # parses the whole list; raises on anything unsupported


@pytest.mark.parametrize('config_dir,name', CASES, ids=['%s-%s' % ('ref' if d == REF else 'own', n) for d, n in CASES])
def test_everything_the_driver_looks_up_resolves_and_binds(config_dir, name):
    import train
    from hip_runtime import optim
    cfg = load_config(config_dir, ['experiment=%s' % name])
    backend = cfg.model.backend
    _bind(import_module('backends.%s' % backend.name).build, **backend.params)
    module, cls = backend.loss.name.rsplit('.', 1)
    _bind(getattr(import_module('losses.%s' % module), cls), **backend.loss.params)
    plugin, plugin_args = train.plugin_from_config(cfg.model.uda)         # the class and arguments the driver will use
    _bind(plugin, **plugin_args)
    if cfg.model.uda is not None:
        key = list(cfg.model.uda.keys())[0]
        assert plugin is train.resolve_plugin(key)
    else:
        assert plugin is import_module('uda.base').Model and plugin_args == {}
    _bind(optim.resolve(cfg.optimizer.name), [], **cfg.optimizer.params)
    if cfg.optimizer.scheduler is not None:
        _bind(getattr(torch.optim.lr_scheduler, cfg.optimizer.scheduler.name),
              **{'optimizer': None, **cfg.optimizer.scheduler.params})
    if cfg.model.uda is not None and 'optimizer' in (cfg.model.uda[key] or {}):     # the plugin's own optimizer block
        block = cfg.model.uda[key].optimizer
        _bind(optim.resolve(block.name), [], **dict(block.params))
        assert block.get('scheduler') is None or hasattr(torch.optim.lr_scheduler, block.scheduler.name)
    defaults = {'max_detections': cfg.max_detections, 'down_ratio': 4,
                'rotated_boxes': backend.params.rotated_boxes, 'num_classes': backend.params.num_classes,
                'num_keypoints': backend.params.num_keypoints, 'mean': cfg.normalize.mean, 'std': cfg.normalize.std}
    assert 'training' in cfg.datasets and 'validation' in cfg.datasets
    for split in cfg.datasets:
        _check_dataset(cfg.datasets[split], defaults)
    assert len(cfg.evaluation) >= 1
    for e in cfg.evaluation:
        _bind(import_module('evaluation.%s' % e).Evaluator,
              **{'score_threshold': cfg.score_threshold, **(cfg.evaluation[e] or {})})
    # what the logger and the plugins read (utils/tensorboard.py, uda/base.py get_detections)
    for k in ('score_threshold', 'font_size', 'alpha', 'num_visualizations'):
        assert k in cfg.tensorboard
    assert isinstance(cfg.model.backend.params.rotated_boxes, bool) and cfg.max_detections > 0
    assert cfg.save_best_metric.mode in ('min', 'max')
    assert run_dir(cfg) == './outputs/%s/' % cfg.experiment
    assert yaml.safe_load(yaml.safe_dump(to_plain(cfg))) == to_plain(cfg)


def test_fda_resolves_although_the_package_does_not_register_it():
    import train
    import uda
    with pytest.raises(AttributeError):
        uda.FDA
    assert train.resolve_plugin('FDA') is import_module('uda.fda').FDA
    with pytest.raises(AttributeError):
        train.resolve_plugin('NoSuchPlugin')


def test_the_old_spelling_of_the_advent_weight_is_read_as_the_new_one(caplog):
    """The reference's `adversarial_entropy_minimization.yaml` says `entropy_weight` where the plugin (the reference's
    own too: tests/test_host_abi.py pins the signature) takes `adversarial_weight`; the sibling `..._dla.yaml` gives the
    same 0.0001 under the current name.  Only that plugin, only that key, and only when the new name is absent."""
    import logging
    import train
    old = load_config(REF, ['experiment=adversarial_entropy_minimization']).model.uda
    new = load_config(REF, ['experiment=adversarial_entropy_minimization_dla']).model.uda
    assert list(old.AdversarialEntropyMinimization.keys()) == ['entropy_weight']
    with caplog.at_level(logging.WARNING, logger='uda'):
        cls, args = train.plugin_from_config(old)
    assert args == {'adversarial_weight': 0.0001} and 'entropy_weight' in caplog.text
    assert cls is train.plugin_from_config(new)[0]
    assert train.plugin_from_config(new)[1]['adversarial_weight'] == args['adversarial_weight']
    assert to_plain(old) == {'AdversarialEntropyMinimization': {'entropy_weight': 0.0001}}        # the config is not edited
    both = Config({'AdversarialEntropyMinimization': {'entropy_weight': 1.0, 'adversarial_weight': 2.0}})
    assert train.plugin_from_config(both)[1] == {'entropy_weight': 1.0, 'adversarial_weight': 2.0}     # still a TypeError
    with pytest.raises(TypeError):
        inspect.signature(train.plugin_from_config(both)[0]).bind(**train.plugin_from_config(both)[1])
    other = Config({'EntropyMinimization': {'adversarial_weight': 1.0}})
    assert train.plugin_from_config(other)[1] == {'adversarial_weight': 1.0}                      # no other plugin is touched
    assert train.plugin_from_config(None) == (import_module('uda.base').Model, {})


# -- merge semantics -------------------------------------------------------------------------------------------------
def _write(tmp_path, defaults, **experiments):
    (tmp_path / 'experiment').mkdir(parents=True)
    (tmp_path / 'defaults.yaml').write_text(defaults)
    for name, text in experiments.items():
        (tmp_path / 'experiment' / (name + '.yaml')).write_text(text)
    return str(tmp_path)


DEFAULTS = """
experiment: default
pretrained: /weights/start.pth
model:
  uda:
    EntropyMinimization:
      entropy_weight: 0.1
datasets:
  validation:
    name: coco
    params:
      image_folder: /val/images
      annotation_file: /val/instances.json
      input_size: [800, 800]
      target_domain_glob:
        - /a/*.png
        - /b/*.jpg
optimizer:
  name: Adam
  params:
    lr: 0.00005
gpu: 0
resume:
hydra:
  run:
    dir: ./outputs/${experiment}/
"""


def test_a_null_clears_a_mapping_lists_replace_and_a_partial_override_keeps_the_rest(tmp_path):
    d = _write(tmp_path, DEFAULTS, exp="""
experiment: mine
pretrained:
model:
  uda:
datasets:
  validation:
    params:
      input_size: [512, 384]
      target_domain_glob:
        - /c/*.png
""")
    base = load_config(d, [])
    assert base.experiment == 'default' and base.model.uda.EntropyMinimization.entropy_weight == 0.1
    cfg = load_config(d, ['experiment=exp'])
    assert cfg.experiment == 'mine'
    assert cfg.pretrained is None and cfg.model.uda is None                       # null clears
    p = cfg.datasets.validation.params
    assert p.input_size == [512, 384] and p.target_domain_glob == ['/c/*.png']    # lists replace
    assert p.image_folder == '/val/images' and p.annotation_file == '/val/instances.json'    # the rest stays
    assert cfg.datasets.validation.name == 'coco' and cfg.optimizer.params.lr == 0.00005
    assert merge({'a': {'b': 1, 'c': [1, 2]}, 'd': 3}, {'a': {'c': [9]}, 'd': None}) == {'a': {'b': 1, 'c': [9]},
                                                                                         'd': None}


def test_an_experiment_file_that_does_not_name_itself_takes_the_override_as_its_name(tmp_path):
    d = _write(tmp_path, DEFAULTS, quiet="gpu: 1\n")
    cfg = load_config(d, ['experiment=quiet'])
    assert cfg.experiment == 'quiet' and cfg.gpu == 1 and run_dir(cfg) == './outputs/quiet/'


def test_anchors_and_aliases_are_resolved(tmp_path):
    d = _write(tmp_path, DEFAULTS, al="""
datasets:
  training:
    name: coco_merger
    params:
      datasets:
        - name: coco
          params:
            target_domain_glob: &tgt
              - /t/*.png
        - name: coco
          params:
            target_domain_glob: *tgt
""")
    members = load_config(d, ['experiment=al']).datasets.training.params.datasets
    assert members[0].params.target_domain_glob == members[1].params.target_domain_glob == ['/t/*.png']


def test_override_parsing(tmp_path):
    d = _write(tmp_path, DEFAULTS)
    cfg = load_config(d, ['gpu=[0]', 'resume=null', 'optimizer.params.lr=1e-4', 'optimizer.params.weight_decay=0.01',
                          'pretrained=', 'model.backend.name=resnet', 'test_only=true', 'epochs=3'])
    assert cfg.gpu == [0] and cfg.resume is None and cfg.pretrained is None
    assert cfg.optimizer.params.lr == 1e-4 and isinstance(cfg.optimizer.params.lr, float)
    assert cfg.optimizer.params.weight_decay == 0.01 and cfg.optimizer.name == 'Adam'
    assert cfg.model.backend.name == 'resnet' and cfg.test_only is True and cfg.epochs == 3
    with pytest.raises(ValueError, match='key.path=value'):
        load_config(d, ['justaword'])
    # overrides are applied after the experiment file, wherever they stand on the command line
    _write(tmp_path / 'second', DEFAULTS, e="gpu: 3\n")
    assert load_config(str(tmp_path / 'second'), ['gpu=5', 'experiment=e']).gpu == 5


def test_the_run_directory_substitutes_the_experiment_and_has_a_default(tmp_path):
    d = _write(tmp_path, DEFAULTS)
    assert run_dir(load_config(d, [])) == './outputs/default/'
    assert run_dir(load_config(d, ['hydra.run.dir=/runs/${experiment}/x'])) == '/runs/default/x'
    cfg = load_config(d, ['hydra=null'])
    assert run_dir(cfg) == './outputs/default/'


def test_an_unknown_interpolation_raises_and_names_it(tmp_path):
    d = _write(tmp_path, DEFAULTS)
    with pytest.raises(NotImplementedError, match=r'\$\{now:%Y\}'):
        load_config(d, ['hydra.run.dir=./outputs/${experiment}/${now:%Y}'])
    with pytest.raises(NotImplementedError, match=r'\$\{seed\}'):
        load_config(d, ['optimizer.name=${seed}'])
    with pytest.raises(NotImplementedError, match=r'\$\{experiment\}'):       # understood in hydra.run.dir only
        load_config(d, ['pretrained=/w/${experiment}.pth'])


def test_the_mapping_type(tmp_path):
    cfg = Config({'a': {'b': 1, 'params': {'lr': 0.1, 'betas': [0.9, 0.99]}}, 'l': [{'x': 1}, 2], 'n': None})
    assert cfg.a.b == cfg['a']['b'] == 1 and 'a' in cfg and 'zz' not in cfg and 'b' in cfg.a
    assert list(cfg.keys()) == ['a', 'l', 'n'] == list(cfg) and len(cfg) == 3
    assert dict(cfg.a.params.items()) == {'lr': 0.1, 'betas': [0.9, 0.99]}
    assert (lambda **kw: kw)(**cfg.a.params) == {'lr': 0.1, 'betas': [0.9, 0.99]}
    assert {**cfg.a.params, 'lr': 1} == {'lr': 1, 'betas': [0.9, 0.99]}
    assert cfg.l[0].x == 1 and cfg.n is None and cfg.get('zz', 7) == 7 and cfg.a.get('b') == 1
    assert to_plain(cfg) == {'a': {'b': 1, 'params': {'lr': 0.1, 'betas': [0.9, 0.99]}}, 'l': [{'x': 1}, 2], 'n': None}
    assert type(to_plain(cfg)['a']) is dict and type(to_plain(cfg)['l'][0]) is dict
    with pytest.raises(AttributeError, match='zz'):
        cfg.zz
    with pytest.raises(KeyError):
        cfg['zz']
    # a dumped config loads again as the same tree
    path = tmp_path / 'config.yaml'
    path.write_text(yaml.safe_dump(to_plain(cfg)))
    assert to_plain(load_config(str(path), [])) == to_plain(cfg)


def test_the_existing_readers_of_cfg_work_on_it():
    """utils/tensorboard.py:62-67 and uda/base.py:154-157 read attributes; the ADVENT plugin reads `name`, `params`
    and `scheduler` of its own optimizer block (uda/adversarial_entropy_minimization.py init_done)."""
    cfg = load_config(REF, ['experiment=adversarial_entropy_minimization_dla'])
    t = cfg.tensorboard
    assert (t.score_threshold, t.font_size, t.alpha, t.num_visualizations) == (0.2, 12, 0.7, 50)
    assert len(cfg.normalize.mean) == 3 and bool(cfg.model.backend.params.rotated_boxes) is False
    opt = cfg.model.uda.AdversarialEntropyMinimization.optimizer
    assert opt.name == 'Adam' and dict(opt.params) == {'lr': 0.001, 'weight_decay': 0.0001}
    assert (opt.get('scheduler') if hasattr(opt, 'get') else getattr(opt, 'scheduler', None)) is None
