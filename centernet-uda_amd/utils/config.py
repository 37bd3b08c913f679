"""Config composition for the training driver, on PyYAML alone.

The reference composes its config with hydra (train.py:70: `configs/defaults.yaml`, then `experiment=<name>` pulls
`configs/experiment/<name>.yaml` over it, then `a.b.c=value` overrides from the command line) and hands the driver an
omegaconf tree.  Neither library is a dependency here; what the driver needs of them is small:

    cfg = load_config('configs', ['experiment=entropy_minimization', 'optimizer.params.lr=1e-4', 'gpu=[0]'])
    cfg.model.backend.name, cfg['epochs'], 'test' in cfg.datasets, {**cfg.datasets.training.params}
    run_dir(cfg)                # hydra.run.dir with ${experiment} substituted
    to_plain(cfg)               # dicts and lists again, for yaml.safe_dump

Merge rule (what the reference's experiment files rely on): mappings merge key by key; lists, scalars and null
REPLACE -- `uda:` or `pretrained:` left empty in an experiment file clears the default, a partly given
`validation.params` keeps the remaining keys.  YAML anchors and aliases are resolved by `yaml.safe_load`
before the merge.  Interpolation is not implemented: `${experiment}` inside `hydra.run.dir` is the one place a
`${...}` is understood; any other raises NotImplementedError naming it.
"""
import os
import re
from collections.abc import Mapping

import yaml

DEFAULT_RUN_DIR = './outputs/${experiment}/'
_INTERPOLATION = re.compile(r'\$\{[^}]*\}')


class Config(Mapping):
    """A read-mostly mapping with attribute access.  Nested mappings are Configs, lists are plain lists (of Configs
    where they hold mappings).  It is a `collections.abc.Mapping`: `in`, `keys()`, `items()`, iteration, `len`,
    `.get` and `**cfg` work as on a dict."""
    __slots__ = ('_data',)

    def __init__(self, data=None):
        object.__setattr__(self, '_data', {k: _wrap(v) for k, v in dict(data or {}).items()})

    def __getitem__(self, key):
        return self._data[key]

    def __iter__(self):
        return iter(self._data)

    def __len__(self):
        return len(self._data)

    def __getattr__(self, name):
        try:
            return object.__getattribute__(self, '_data')[name]
        except KeyError:
            raise AttributeError("config has no key %r (keys: %s)" % (name, ', '.join(map(str, self._data)))) from None

    def __setattr__(self, name, value):
        self._data[name] = _wrap(value)

    __setitem__ = __setattr__

    def __repr__(self):
        return 'Config(%r)' % (to_plain(self),)

    def __getstate__(self):
        return to_plain(self)

    def __setstate__(self, state):
        object.__setattr__(self, '_data', {k: _wrap(v) for k, v in state.items()})


def _wrap(v):
    if isinstance(v, Config):
        return v
    if isinstance(v, Mapping):
        return Config(v)
    if isinstance(v, (list, tuple)):
        return [_wrap(x) for x in v]
    return v


def to_plain(v):
    """Config tree -> dicts, lists and scalars (what yaml.safe_dump takes)."""
    if isinstance(v, Mapping):
        return {k: to_plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [to_plain(x) for x in v]
    return v


def merge(base, over):
    """Deep merge of plain trees: mappings key by key, anything else (lists, scalars, None) replaces."""
    if isinstance(base, dict) and isinstance(over, dict):
        out = dict(base)
        for k, v in over.items():
            out[k] = merge(base[k], v) if k in base else v
        return out
    return over


def _load(path):
    if not os.path.isfile(path):
        raise FileNotFoundError("config file %s not found" % path)
    with open(path) as f:
        tree = yaml.safe_load(f)
    if tree is None:
        return {}
    if not isinstance(tree, dict):
        raise ValueError("%s: the top level must be a mapping, got %s" % (path, type(tree).__name__))
    return tree


_EXPONENT_FLOAT = re.compile(r'^[-+]?\d+[eE][-+]?\d+$')


def _parse_value(text):
    """The right side of an override, by yaml.safe_load.  YAML 1.1 reads a float only where it sees a dot, so `1e-4`
    comes back as a string; on a command line it can only mean the number, and it is converted."""
    value = yaml.safe_load(text) if text.strip() else None
    if isinstance(value, str) and _EXPONENT_FLOAT.match(value):
        return float(value)
    return value


def _set_path(tree, path, value):
    keys = path.split('.')
    node = tree
    for k in keys[:-1]:
        if not isinstance(node.get(k), dict):
            node[k] = {}
        node = node[k]
    node[keys[-1]] = value


def _check_interpolations(tree, where=''):
    if isinstance(tree, dict):
        for k, v in tree.items():
            _check_interpolations(v, '%s.%s' % (where, k) if where else str(k))
    elif isinstance(tree, list):
        for i, v in enumerate(tree):
            _check_interpolations(v, '%s[%d]' % (where, i))
    elif isinstance(tree, str):
        for m in _INTERPOLATION.findall(tree):
            if not (where == 'hydra.run.dir' and m == '${experiment}'):
                raise NotImplementedError("interpolation %s (at %s) is not supported: only ${experiment} inside "
                                          "hydra.run.dir is" % (m, where))


def load_config(config_dir, overrides=()):
    """`config_dir/defaults.yaml`, then `experiment=<name>` (-> `config_dir/experiment/<name>.yaml` merged over the
    root), then every other `key.path=value` with the right side parsed by yaml.safe_load.  -> Config.
    `config_dir` may also name one YAML file to start from instead, e.g. the merged `.hydra/config.yaml` a run wrote
    (experiment files are then looked up beside it)."""
    config_dir = str(config_dir)
    if os.path.isfile(config_dir):
        tree, config_dir = _load(config_dir), os.path.dirname(config_dir)
    else:
        tree = _load(os.path.join(config_dir, 'defaults.yaml'))
    pairs = []
    for item in overrides:
        key, eq, value = str(item).partition('=')
        key = key.strip()
        if not eq or not key:
            raise ValueError("override %r is not of the form key.path=value" % (item,))
        pairs.append((key, _parse_value(value)))
    for key, value in pairs:
        if key == 'experiment':
            tree['experiment'] = value                # the file usually names itself; this holds when it does not
            tree = merge(tree, _load(os.path.join(config_dir, 'experiment', '%s.yaml' % value)))
    for key, value in pairs:
        if key != 'experiment':
            _set_path(tree, key, value)
    _check_interpolations(tree)
    return Config(tree)


def run_dir(cfg):
    """The run directory: `hydra.run.dir` with ${experiment} substituted (the only use of the `hydra:` key)."""
    hydra = cfg.get('hydra') or {}
    run = hydra.get('run') or {}
    path = run.get('dir') or DEFAULT_RUN_DIR
    for m in _INTERPOLATION.findall(path):
        if m != '${experiment}':
            raise NotImplementedError("interpolation %s in hydra.run.dir is not supported: only ${experiment} is" % m)
    return path.replace('${experiment}', str(cfg.get('experiment', 'default')))
