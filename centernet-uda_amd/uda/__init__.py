"""UDA step plugins.  The driver resolves them by class name from the config (`uda.<ClassName>`, train.py:104-106);
the classes are imported on first use.  FDA lives at uda.fda.FDA (its module path in the reference too) and is not
registered here yet: the reference's transform is spelled with `torch.rfft`, which current PyTorch no longer has, and
this build replaces it with a HIP transform (utils/image.FDA_source_to_target)."""
import importlib

_PLUGINS = {
    'Model': 'uda.base',
    'EntropyMinimization': 'uda.entropy_minimization',
    'MaxSquaresMinimization': 'uda.max_squares_minimization',
    'IWMaxSquaresMinimization': 'uda.max_squares_minimization',
    'MultiLevelMaxSquaresMinimization': 'uda.max_squares_minimization',
    'AdversarialEntropyMinimization': 'uda.adversarial_entropy_minimization',
    'MeanTeacher': 'uda.mean_teacher',
    'WeakStrongTeacher': 'uda.mean_teacher',
    'DenseTeacher': 'uda.mean_teacher',
    'GeometricTeacher': 'uda.mean_teacher',
    'KeypointTeacher': 'uda.mean_teacher',
}
__all__ = sorted(_PLUGINS)


def __getattr__(name):
    if name in _PLUGINS:
        cls = getattr(importlib.import_module(_PLUGINS[name]), name)
        globals()[name] = cls
        return cls
    if name == 'FDA':
        raise AttributeError("uda.FDA is not registered in this build (the reference's uda/fda.py uses torch.rfft, "
                             "removed from PyTorch): use uda.fda.FDA, which runs on a HIP transform")
    raise AttributeError("module 'uda' has no attribute %r" % name)


def __dir__():
    return sorted(list(globals()) + list(_PLUGINS))
