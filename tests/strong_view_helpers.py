"""Shared pieces of tests/test_gpu_strong_view.py: the parameter records of the kernel cases, and the small ResNet-18
plugin set-up of tests/test_gpu_teacher.py restated for any mean-teacher class (an untrained model conditioned to detect
something, a threshold between its scores)."""
import numpy as np
import torch

import inputs as gin

DEV = 'cuda:0'
F = np.float32
KDET = 20
MEAN = F([0.40789654, 0.44719302, 0.47026115])
STD = F([0.28863828, 0.27408164, 0.27809835])
G = lambda a: torch.from_numpy(np.array(a, order='C')).to(DEV)       # (a copy: the shared references are read-only)
N = lambda t: t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def short(name):
    """demangled kernel symbol -> its bare name"""
    return name.replace('void ', '').replace('cnuda::(anonymous namespace)::', '').split('(')[0].strip()


# ---------------------------------------------------------------------------------------------------------------------
# kernel cases
# ---------------------------------------------------------------------------------------------------------------------
def images(B, H, W, seed):
    """uniform in [-3, 3): x std + mean leaves [0, 1] on both sides for about two thirds of the values"""
    return np.random.default_rng(seed).uniform(-3, 3, (B, 3, H, W)).astype(F)


def case_params(H, W, whole_on, seed=0x0123456789ABCDEF, first_id=1000):
    """Four images: 0 neutral; 1 rectangles only; 2 every operation at radius 6, with one rectangle in the top-left corner
    (touching two edges) and one overlapping it; 3 contrast + gray + radius 1.  `whole_on` (1 or 2): the image whose
    third rectangle covers the whole image."""
    from datasets.strong_view import StrongViewParams, gaussian_taps
    p = StrongViewParams.identity(4, first_id)
    p.seed = seed
    p.rects[1, 0] = (W // 3, H // 4, W // 3 + max(W // 4, 1), H // 4 + max(H // 2, 1))
    p.rects[1, 1] = (W - 2, H - 1, W, H)                           # the bottom-right corner
    p.rects[1, 2] = (3, 2, 3, 4)                                   # empty: x1 == x0
    p.photo[2] = (1.3, 0.7, 1.4, 1.0)
    p.radius[2], p.taps[2] = gaussian_taps(2.0)
    assert p.radius[2] == 6
    p.rects[2, 0] = (0, 0, max(W // 2, 1), max(H // 3, 1))         # touches the top and the left edge
    p.rects[2, 1] = (W // 4, H // 6, W // 4 + max(W // 2, 1), H // 6 + max(H // 3, 1))      # overlaps it
    p.rects[whole_on, 2] = (0, 0, W, H)
    p.photo[3] = (1.0, 1.35, 1.0, 1.0)
    p.radius[3], p.taps[3] = gaussian_taps(0.3)
    assert p.radius[3] == 1
    return p


def oracle_view(so, x, p, pivots=None):
    return so.strong_view(x, MEAN, STD, p.photo, p.taps, p.radius, p.rects, p.ids, p.seed, pivots=pivots)


# ---------------------------------------------------------------------------------------------------------------------
# the plugin
# ---------------------------------------------------------------------------------------------------------------------
class Cfg(dict):
    __getattr__ = dict.__getitem__


def cfg(num_classes, seed=42):
    return Cfg(max_detections=KDET, seed=seed, normalize=Cfg(mean=[float(v) for v in MEAN], std=[float(v) for v in STD]),
               model=Cfg(backend=Cfg(params=Cfg(rotated_boxes=False, num_classes=num_classes, num_keypoints=0))))


def _last_conv(head):
    from hip_runtime import nn as hnn
    return [m for m in head.modules() if isinstance(m, hnn.Conv2d)][-1]


def condition(model, x):
    """Make an untrained model detect something: sizes around 5 cells (the wh head's bias), heat-map logits spread to a
    standard deviation of 1.5 around -2.19.  -> its decoded scores in eval mode."""
    from backends.decode import decode_detection
    from hip_runtime import ops
    model.to(DEV)
    with torch.no_grad():
        _last_conv(model.wh).bias.fill_(5.0)
        _last_conv(model.hm).bias.fill_(-2.19)
        model.eval()
        std = float(model(x)['hm'].std())
        _last_conv(model.hm).weight.mul_(1.5 / std)
        heads = model(x)
        dets = decode_detection(ops.sigmoid_clamp_(heads['hm']), heads['wh'], heads['reg'], K=KDET)
    model.train()
    return N(dets)[..., 4]


def threshold_between(scores):
    """The middle of the widest gap between neighbouring scores of the middle half."""
    s = np.unique(scores.astype(np.float64))
    lo, hi = len(s) // 4, 3 * len(s) // 4
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    i = int(np.argmax(gaps))
    return float(F(0.5 * (s[lo + i] + s[lo + i + 1])))


def resnet_plugin(cls, target, seed=3, **kwargs):
    """`cls(0.5, **kwargs)` around a conditioned ResNet-18 with three classes, moved and in training phase."""
    from backends import resnet
    from hip_runtime import optim
    from losses.centernet import DetectionLoss
    torch.manual_seed(seed)
    model = resnet.build(18, num_classes=3, pretrained=False)
    scores = condition(model, target)
    kwargs.setdefault('score_threshold', threshold_between(scores))
    plugin = cls(kwargs.pop('pseudo_weight', 0.5), **kwargs)
    plugin.cfg, plugin.device, plugin.backend = cfg(3), torch.device(DEV), model
    plugin.optimizer = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(True)
    plugin.host_stats = False
    return plugin


def data(B=2, S=64, C=3, seed=60, n_obj=(3, 2)):
    out = {k: G(v) for k, v in gin.detection_batch(B, C, S // 4, S // 4, 8, n_obj, 2, seed + 1).items()}
    out['input'] = G(gin.image_batch(B, S, S, seed))
    out['target_domain_input'] = G(gin.image_batch(B, S, S, seed + 10))
    return out


def snapshot(module):
    return {k: N(v).copy() for k, v in module.state_dict().items()}


class Capture:
    """Forward pre-hooks on a plugin's student and teacher: every input either received, as numpy, in call order."""

    def __init__(self, plugin):
        self.student, self.teacher = [], []
        self.handles = [plugin.backend.register_forward_pre_hook(lambda m, args: self.student.append(N(args[0]).copy())),
                        plugin.teacher.register_forward_pre_hook(lambda m, args: self.teacher.append(N(args[0]).copy()))]

    def clear(self):
        self.student.clear(), self.teacher.clear()

    def remove(self):
        for h in self.handles:
            h.remove()
