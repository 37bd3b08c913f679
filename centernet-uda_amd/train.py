"""The training driver: a config directory and a folder of images in, checkpoints, logs and mAP out.

    python train.py [--config-dir DIR] [experiment=NAME] [key.path=value ...]

It follows the reference's driver step by step (train.py:70-271: seed, backend, optimizer, scheduler, plugin, attribute
injection, loaders, logger, evaluators, `init_done`, `pretrained` / `resume`, `to(device)`, the epoch loop with
`eval_at_n_epoch` and `save_best_metric`, `test_only`, the optional `test` dataset), with this project's pieces in the
places of hydra, torch's DataLoader and the per-step `.item()` calls:

  * utils.config.load_config composes `defaults.yaml`, the experiment file and the overrides; the run directory is
    `hydra.run.dir`, the process changes into it and writes the merged config to `.hydra/config.yaml` (where the
    reference's export tool looks for it); `model_last.pth`, `model_best.pth` and `logs/` land there.
  * datasets.loader.DeviceLoader feeds `datasets.build_batch` from a thread pool and a side stream.
  * with `device_meters: true` (this project's key) the running statistics live on the device
    (utils.helper.DeviceMeters) and the training loop reads nothing back until the epoch ends.

Every epoch logs the training loop's images per second, measured with one synchronisation at its end.
"""
import argparse
import logging
import os
import sys
import time
from importlib import import_module

import torch
import yaml
from tqdm import tqdm

PKG = os.path.dirname(os.path.abspath(__file__))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from utils.config import load_config, run_dir, to_plain   # noqa: E402
from utils.helper import AverageMeter, DeviceMeters   # noqa: E402

log = logging.getLogger("uda")


class HostMeters:
    """The reference's bookkeeping (train.py:162-166) behind DeviceMeters' interface: one `.item()` per statistic."""

    def __init__(self):
        self.meters = {}

    def update(self, stats, n):
        for k, v in stats.items():
            self.meters.setdefault(k, AverageMeter(name=k)).update(v.item() if hasattr(v, 'item') else v, n)

    def read(self):
        return dict(self.meters)

    def reset(self):
        for m in self.meters.values():
            m.reset()


def resolve_plugin(key):
    """`uda.<key>` as the reference looks it up (train.py:104); FDA is not registered in the package namespace and
    lives at uda.fda.FDA."""
    import uda
    try:
        return getattr(uda, key)
    except AttributeError:
        if key != 'FDA':
            raise
        return import_module('uda.fda').FDA


# Constructor arguments that an experiment file may still spell as an earlier version of a plugin did.  The reference
# ships `adversarial_entropy_minimization.yaml` with `entropy_weight` for the ADVENT plugin, whose constructor takes
# `adversarial_weight` (its sibling `..._dla.yaml` gives the same value under the current name); the reference's driver
# stops there with a TypeError.  The driver reads the old spelling as the new one and says so.
LEGACY_PLUGIN_ARGUMENTS = {'AdversarialEntropyMinimization': {'entropy_weight': 'adversarial_weight'}}


def plugin_from_config(uda_cfg):
    """`cfg.model.uda` (one key naming the plugin, its block the constructor arguments; empty: no UDA) ->
    (class, keyword arguments) as the driver will call it."""
    if uda_cfg is None:
        return import_module('uda.base').Model, {}
    method = list(uda_cfg.keys())[0]
    params = dict(uda_cfg[method] or {})
    for old, new in LEGACY_PLUGIN_ARGUMENTS.get(method, {}).items():
        if old in params and new not in params:
            log.warning("uda.%s: the config says %r, the plugin's argument is %r; taking it as that", method, old, new)
            params[new] = params.pop(old)
    return resolve_plugin(method), params


def select_device(gpu):
    """cfg.gpu: an integer, or a list of one, selects the device (no environment variable is set)."""
    if isinstance(gpu, (list, tuple)):
        if len(gpu) != 1:
            raise NotImplementedError(
                "gpu=%s: multi-GPU runs are launched one process per GPU (hip_runtime.parallel.DataParallel), and "
                "this driver does not start them yet; give one device" % (list(gpu),))
        gpu = gpu[0]
    if gpu is None:
        raise RuntimeError("gpu is empty: the kernels run on the MI355X only, there is no CPU path")
    torch.cuda.set_device(int(gpu))
    return torch.device('cuda', int(gpu))


def wants_keypoint_visibility(evaluation, num_keypoints):
    """Whether the validation and test batches must carry COCO's `v` flag: `coco_keypoints` is among the evaluators.
    A model without keypoints cannot feed that evaluator: ValueError, before a dataset is read."""
    if 'coco_keypoints' not in (evaluation or {}):
        return False
    if not num_keypoints:
        raise ValueError("evaluation.coco_keypoints is configured but model.backend.params.num_keypoints is %r: a model "
                         "without a keypoint head has no keypoint metrics; set num_keypoints (and kp_weight) or take "
                         "coco_keypoints out of `evaluation`" % (num_keypoints,))
    return True


def load_datasets(cfg, device, down_ratio, rotated_boxes):
    from datasets.loader import DeviceLoader
    visibility = wants_keypoint_visibility(cfg.evaluation, cfg.model.backend.params.num_keypoints)
    defaults = {"max_detections": cfg.max_detections,
                "down_ratio": down_ratio,
                "rotated_boxes": rotated_boxes,
                "num_classes": cfg.model.backend.params.num_classes,
                "num_keypoints": cfg.model.backend.params.num_keypoints,
                "mean": cfg.normalize.mean,
                "std": cfg.normalize.std}

    def loader(split, shuffle, keypoint_visibility=False):
        spec = cfg.datasets[split]
        dataset = import_module('datasets.%s' % spec.name).Dataset(**{**spec.params, **defaults})
        log.info("Found %d samples in %s dataset", len(dataset), split)
        return DeviceLoader(dataset, batch_size=cfg.batch_size, shuffle=shuffle, num_workers=cfg.num_workers,
                            device=device, seed=cfg.seed, num_classes=defaults["num_classes"],
                            num_keypoints=defaults["num_keypoints"], rotated_boxes=rotated_boxes,
                            down_ratio=down_ratio, mean=defaults["mean"], std=defaults["std"],
                            max_detections=cfg.max_detections, keypoint_visibility=keypoint_visibility)

    validation = loader('validation', False, visibility)
    training = loader('training', True)
    test = loader('test', False, visibility) if 'test' in cfg.datasets else None
    return training, validation, test


def _evaluate(uda, loader, evaluators, tensorboard_logger, meters, tag, epoch, desc):
    """One pass without gradients over `loader`: statistics, detections into the evaluators, previews."""
    uda.set_phase(is_training=False)
    with torch.no_grad():
        for data in tqdm(loader, total=len(loader), position=1, desc=desc, disable=None):
            outputs = uda.step(data, is_training=False)
            meters.update({f"{tag}/{k}": v for k, v in outputs["stats"].items()}, data["input"].size(0))
            detections = uda.get_detections(outputs, data)
            detections["image_shape"] = data["input"].shape[1:]
            for e in evaluators:
                e.add_batch(**detections)
            tensorboard_logger.log_detections(data, detections, epoch, tag=tag)


def _log_scalars(meters, results, tensorboard_logger, epoch):
    """Meter averages, then the evaluators' results (train.py:200-208); the meters start over."""
    scalars = {k: m.avg for k, m in meters.read().items()}
    scalars.update(results)
    for k, v in scalars.items():
        tensorboard_logger.log_stat(k, v, epoch)
    meters.reset()
    return scalars


def run(cfg):
    from hip_runtime import optim as hip_optim
    from utils.tensorboard import TensorboardLogger

    torch.manual_seed(cfg.seed)
    device = select_device(cfg.gpu)
    log.info("Use device %s for training", device)

    backend = import_module('backends.%s' % cfg.model.backend.name).build(**cfg.model.backend.params)
    optimizer = hip_optim.resolve(cfg.optimizer.name)(
        [p for p in backend.parameters() if p.requires_grad], **cfg.optimizer.params)
    scheduler = None
    if cfg.optimizer.scheduler is not None:
        scheduler = getattr(torch.optim.lr_scheduler, cfg.optimizer.scheduler.name)(
            **{"optimizer": optimizer, **cfg.optimizer.scheduler.params})

    uda_cls, uda_params = plugin_from_config(cfg.model.uda)
    uda = uda_cls(**uda_params)
    uda.cfg = cfg
    uda.device = device
    uda.backend = backend
    uda.optimizer = optimizer
    loss_module, loss_name = cfg.model.backend.loss.name.rsplit('.', 1)
    uda.centernet_loss = getattr(import_module('losses.%s' % loss_module), loss_name)(**cfg.model.backend.loss.params)
    uda.scheduler = scheduler

    train_loader, val_loader, test_loader = load_datasets(
        cfg, device, down_ratio=backend.down_ratio, rotated_boxes=backend.rotated_boxes)
    tensorboard_logger = TensorboardLogger(cfg, val_loader.dataset.classes)

    evaluators = []
    for e in cfg.evaluation:
        params = {'score_threshold': cfg.score_threshold, **(cfg.evaluation[e] or {})}
        rotated_iou = params.pop('rotated_iou', None)          # evaluation.coco.rotated_iou: 'mask' or 'polygon'
        e = import_module('evaluation.%s' % e).Evaluator(**params)
        if rotated_iou is not None:
            e.rotated_iou = rotated_iou
        e.classes = tensorboard_logger.classes
        e.num_workers = cfg.num_workers
        e.use_rotated_boxes = cfg.model.backend.params.rotated_boxes
        evaluators.append(e)

    uda.init_done()

    start_epoch = 1
    if cfg.pretrained is not None and cfg.resume is None:
        start_epoch = uda.load_model(cfg.pretrained)
    elif cfg.resume is not None:
        start_epoch = uda.load_model(cfg.resume, True)

    uda.to(device, False)

    device_meters = bool(cfg.get('device_meters', True))
    uda.host_stats = not device_meters
    meters = DeviceMeters(device) if device_meters else HostMeters()
    results = {}                       # the evaluators' scalars; like the reference's `stats`, they persist
    best = float("inf") if cfg.save_best_metric.mode == 'min' else -float("inf")
    summary = {'epochs': [], 'scalars': {}, 'error': None, 'images_per_second': []}
    epoch = start_epoch

    if not cfg.test_only:
        for epoch in tqdm(range(start_epoch, cfg.epochs + 1), initial=start_epoch, position=0, desc='Epoch',
                          disable=None):
            uda.epoch_start()
            uda.set_phase(is_training=True)
            train_loader.set_epoch(epoch)
            images, steps, began = 0, 0, time.perf_counter()
            for data in tqdm(train_loader, total=len(train_loader), position=1, desc='Training Steps', disable=None):
                outputs = uda.step(data)
                n = data["input"].size(0)
                meters.update({f"training/{k}": v for k, v in outputs["stats"].items()}, n)
                images, steps = images + n, steps + 1
            torch.cuda.synchronize(device)
            seconds = time.perf_counter() - began
            summary['epochs'].append(epoch)
            summary['images_per_second'].append(images / seconds if seconds > 0 else 0.0)
            log.info("epoch %d: %d images in %d steps, %.3f s: %.1f images/s, %.2f ms/step", epoch, images, steps,
                     seconds, images / max(seconds, 1e-9), 1e3 * seconds / max(steps, 1))

            if epoch % cfg.eval_at_n_epoch != 0:
                continue

            _evaluate(uda, val_loader, evaluators, tensorboard_logger, meters, 'validation', epoch, 'Validation Steps')
            for e in evaluators:
                results.update(e.evaluate())
            scalars = summary['scalars'] = _log_scalars(meters, results, tensorboard_logger, epoch)

            uda.epoch_end()
            tensorboard_logger.reset()
            uda.save_model("model_last.pth", epoch, True)

            if cfg.save_best_metric.name not in scalars:
                summary['error'] = (f"Metric {cfg.save_best_metric.name} not valid, valid values are "
                                    f"{' '.join(scalars.keys())}")
                log.error(summary['error'])
                return summary

            current = scalars[cfg.save_best_metric.name]
            if (cfg.save_best_metric.mode == 'min' and best > current
                    or cfg.save_best_metric.mode == 'max' and best < current):
                uda.save_model("model_best.pth", epoch, True)
                best = current
                log.info(f"Save best model with {cfg.save_best_metric.name} of {current:.4f}")

    if test_loader is not None:
        if cfg.test_only:
            epoch = start_epoch
        _evaluate(uda, test_loader, evaluators, tensorboard_logger, meters, 'test', epoch, 'Test Steps')
        for e in evaluators:
            results.update(e.evaluate())
        summary['scalars'] = _log_scalars(meters, results, tensorboard_logger, epoch)
        tensorboard_logger.reset()
    return summary


def main(argv=None):
    """-> {'run_dir', 'epochs' (trained), 'images_per_second' (per trained epoch), 'scalars' (last logged), 'error'}"""
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--config-dir', default=os.path.join(PKG, 'configs'),
                        help="directory with defaults.yaml and experiment/*.yaml (default: %(default)s)")
    parser.add_argument('overrides', nargs='*', help="experiment=NAME and key.path=value overrides")
    args = parser.parse_args(argv)
    cfg = load_config(os.path.abspath(args.config_dir), args.overrides)
    select_device(cfg.gpu)                      # a bad `gpu` fails before anything is written
    target = os.path.abspath(run_dir(cfg))
    before = os.getcwd()
    os.makedirs(os.path.join(target, '.hydra'), exist_ok=True)
    os.chdir(target)
    try:
        with open(os.path.join('.hydra', 'config.yaml'), 'w') as f:
            yaml.safe_dump(to_plain(cfg), f, sort_keys=False)
        summary = run(cfg)
    finally:
        os.chdir(before)
    summary['run_dir'] = target
    return summary


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format='[%(asctime)s][%(name)s][%(levelname)s] - %(message)s')
    main()
