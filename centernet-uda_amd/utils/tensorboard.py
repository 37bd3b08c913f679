"""`TensorboardLogger` with the reference's interface (utils/tensorboard.py:5-53): the driver's `log_stat`,
`log_image`, `log_detections` and `reset`.

`log_detections` keeps the reference's counter (at most `num_visualizations` previews between two `reset()` calls,
tagged `<tag>/detection_<id>`), but renders only the images it is going to log, in one launch on the device
(utils.visualize.Visualizer.visualize_batch), and brings them back in one copy of uint8; the reference copies the
whole float batch to the host first (utils/tensorboard.py:25).

The writer is `torch.utils.tensorboard.SummaryWriter('logs')` when the tensorboard package imports, else `FileWriter`:
scalars appended to `logs/scalars.jsonl`, images written as binary PPM under `logs/<tag>/`.  `writer=` injects one.
"""
import json
import os

import numpy as np
import torch

from utils.visualize import Visualizer


class FileWriter:
    """The two SummaryWriter calls the logger makes, on plain files."""

    def __init__(self, log_dir='logs'):
        self.log_dir = log_dir

    def add_scalar(self, name, value, step):
        os.makedirs(self.log_dir, exist_ok=True)
        with open(os.path.join(self.log_dir, 'scalars.jsonl'), 'a') as f:
            f.write(json.dumps({'name': name, 'value': float(value), 'step': int(step)}) + '\n')

    def add_image(self, name, image, step):
        """image: [3, H, W] uint8 (or float in [0, 1], as SummaryWriter accepts) -> logs/<name>/<step>.ppm"""
        image = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        if image.ndim != 3 or image.shape[0] != 3:
            raise ValueError("FileWriter.add_image: expected [3, H, W], got %s" % (image.shape,))
        if image.dtype != np.uint8:
            image = np.clip(image * 255.0, 0, 255).astype(np.uint8)
        parts = [p for p in str(name).replace('\\', '/').split('/') if p not in ('', '.', '..')]
        folder = os.path.join(self.log_dir, *parts)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, '%08d.ppm' % int(step)), 'wb') as f:
            f.write(b'P6\n%d %d\n255\n' % (image.shape[2], image.shape[1]))
            f.write(np.ascontiguousarray(image.transpose(1, 2, 0)).tobytes())


def default_writer(log_dir='logs'):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        return FileWriter(log_dir)
    return SummaryWriter(log_dir)


class TensorboardLogger:
    def __init__(self, cfg, classes, writer=None):
        super().__init__()
        self.classes = classes
        self.summary_writer = default_writer('logs') if writer is None else writer
        self.visualizer = Visualizer(
            classes,
            cfg.tensorboard.score_threshold,
            cfg.normalize.mean,
            cfg.normalize.std,
            font_size=cfg.tensorboard.font_size,
            alpha=cfg.tensorboard.alpha)
        self.num_visualizations = cfg.tensorboard.num_visualizations
        self.log_callback = None
        self.__num_logged_images = 0

    def log_detections(self, batch, detections, step, tag):
        left = self.num_visualizations - self.__num_logged_images
        if left <= 0:
            return
        count = min(int(left), int(batch["input"].shape[0]))
        if count <= 0:
            return
        ids = batch["id"]
        ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        results = self.visualizer.visualize_batch(batch["input"].detach(), detections, range(count))
        results = results.cpu().numpy()                       # the one copy back: n * 3 * H * 2W bytes
        for i in range(count):
            self.summary_writer.add_image(f'{tag}/detection_{ids[i]}', results[i], step)
            self.__num_logged_images += 1

    def log_stat(self, name, value, step):
        self.summary_writer.add_scalar(name, value, step)

    def log_image(self, name, image, step):
        self.summary_writer.add_image(name, image, step)

    def reset(self):
        self.__num_logged_images = 0
