"""Host-side helpers with the reference's names (utils/helper.py): AverageMeter
and the checkpoint wire format (`{'epoch','state_dict'[,'optimizer','scheduler']}`,
`module.` prefix stripping, shape-mismatch tolerance, start-epoch return values;
utils/helper.py:83-147)."""
import logging
from pathlib import Path

import torch

log = logging.getLogger(__name__)


class AverageMeter:
    """Running mean weighted by batch size, with the reference's constructor and text form
    (utils/helper.py:13-35; the driver builds `AverageMeter(name=k)`, train.py:164,182,243)."""

    def __init__(self, name, fmt=':f'):
        self.name = name
        self.fmt = fmt
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        if self.count > 0:                      # the reference divides unguarded; update(x, n=0) would raise there
            self.avg = self.sum / self.count

    def __str__(self):
        fmtstr = '{name} {val' + self.fmt + '} ({avg' + self.fmt + '})'
        return fmtstr.format(**self.__dict__)


class DeviceMeters:
    """The driver's AverageMeters (train.py:162-166) with their state on the device: `update` folds the 0-dim float32
    device tensors of a step's `stats` into sum / count / last arrays with one kernel launch per 32 of them
    (hip_runtime.ops.meter_update) and reads nothing back; `read` copies the arrays to the host once.  The sums are
    the float64 sums `AverageMeter.update(v.item(), n)` builds, bit for bit.  Anything that is not such a tensor (a
    Python number, a host tensor) goes to a host AverageMeter of that name."""

    def __init__(self, device, capacity=64):
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.slots = {}                 # name -> index, in order of first sight
        self.host = {}                  # name -> AverageMeter
        # one buffer, so that read() is one copy: sum [capacity] f64 | count [capacity] f64 | last [capacity] f32
        self._state = torch.zeros(self.capacity * 20, dtype=torch.uint8, device=self.device)
        c = self.capacity
        self._sum = self._state[:8 * c].view(torch.float64)
        self._count = self._state[8 * c:16 * c].view(torch.float64)
        self._last = self._state[16 * c:].view(torch.float32)

    def _on_device(self, v):
        return isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and v.dtype == torch.float32

    def update(self, stats, n):
        from hip_runtime import ops
        taken = []
        for name, v in stats.items():
            if name not in self.slots and name not in self.host and self._on_device(v):
                if len(self.slots) >= self.capacity:
                    raise RuntimeError("DeviceMeters: more than %d names (capacity=)" % self.capacity)
                self.slots[name] = len(self.slots)
            if name in self.slots and self._on_device(v):
                taken.append((self.slots[name], v.detach()))
            else:
                if name in self.slots:
                    raise RuntimeError("DeviceMeters: %r was a device scalar before and is a %s now"
                                       % (name, type(v).__name__))
                m = self.host.setdefault(name, AverageMeter(name=name))
                m.update(v.item() if isinstance(v, torch.Tensor) else v, n)
        taken.sort(key=lambda e: e[0])
        start = 0
        while start < len(taken):       # runs of consecutive slots, at most 32 per launch
            end = start + 1
            while end < len(taken) and end - start < ops.METER_SLOTS and taken[end][0] == taken[end - 1][0] + 1:
                end += 1
            first = taken[start][0]
            ops.meter_update([v for _, v in taken[start:end]], n, self._sum[first:], self._count[first:],
                             self._last[first:])
            start = end

    def read(self):
        """-> {name: AverageMeter} (val, sum, count, avg) after ONE copy to the host, which also synchronises."""
        host = self._state.cpu()
        c = self.capacity
        sums = host[:8 * c].view(torch.float64).tolist()
        counts = host[8 * c:16 * c].view(torch.float64).tolist()
        last = host[16 * c:].view(torch.float32).tolist()
        out = {}
        for name, i in self.slots.items():
            m = AverageMeter(name=name)
            m.val, m.sum, m.count = last[i], sums[i], counts[i]
            if m.count > 0:
                m.avg = m.sum / m.count
            out[name] = m
        out.update(self.host)
        return out

    def reset(self):
        """Values back to zero; the names keep their slots."""
        self._state.zero_()
        for m in self.host.values():
            m.reset()


def _unwrap(model):
    return model.module if hasattr(model, 'module') and isinstance(model.module, torch.nn.Module) else model


def load_model(model, optimizer, scheduler, path, resume=False, extra=None):
    """Returns the start epoch: 1 if the file is missing, 0 for `pretrained`,
    saved epoch + 1 for `resume` (utils/helper.py:85-90,128).  extra: a dict that takes 'found': True and whatever
    the checkpoint holds beside the wire format's four keys (uda.MeanTeacher's teacher)."""
    path = Path(path)
    if not path.exists():
        log.warning("Model path %s does not exists!", path)
        return 1
    checkpoint = torch.load(path, map_location='cpu', weights_only=False)
    epoch = checkpoint["epoch"] if resume else 0
    if extra is not None:
        extra['found'] = True
        extra.update({k: v for k, v in checkpoint.items() if k not in ('epoch', 'state_dict', 'optimizer', 'scheduler')})
    incoming = {}
    for k, v in checkpoint['state_dict'].items():
        # DataParallel checkpoints carry a 'module.' prefix ('module_list...' is a real name)
        incoming[k[7:] if k.startswith('module') and not k.startswith('module_list') else k] = v
    target = _unwrap(model)
    own = target.state_dict()
    for k in list(incoming):
        if k not in own:
            log.info("drop parameter %s", k)
        elif incoming[k].shape != own[k].shape:
            log.warning("skip parameter %s because of shape mismatch", k)
            incoming[k] = own[k]
    for k in own:
        if k not in incoming:
            log.warning("no parameter %s available", k)
            incoming[k] = own[k]
    target.load_state_dict(incoming, strict=False)
    if resume and optimizer is not None and 'optimizer' in checkpoint:
        optimizer.load_state_dict(checkpoint['optimizer'])
        if scheduler is not None and 'scheduler' in checkpoint:
            scheduler.load_state_dict(checkpoint['scheduler'])
    return (epoch + 1) if resume else epoch


def save_model(model, path, epoch, optimizer=None, scheduler=None, extra=None):
    """extra: further entries beside the wire format's keys, which stay as they are."""
    data = dict(extra or {}, epoch=epoch, state_dict=_unwrap(model).state_dict())
    if optimizer is not None:
        data['optimizer'] = optimizer.state_dict()
        if scheduler is not None:
            data['scheduler'] = scheduler.state_dict()
    torch.save(data, path)
