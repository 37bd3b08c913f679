"""utils.helper.DeviceMeters (csrc/meters.hip) against AverageMeter fed the same values.

The comparison is bit for bit, and that is derived, not measured: per update both sides compute, in float64,
one product `float64(v) * n` rounded to nearest, one sum `sum + product` rounded to nearest, and `count + n`; `avg` is
one division of the two on the host in both cases.  IEEE 754 fixes every one of these results.  (It does not fix
the sign and payload bits of a NaN: where both sides hold a NaN, that is all that is compared.)

The kernel must not fuse the product into the sum.  With the batch sizes of a real run it could not matter
(a 24-bit value times a small integer is exact in float64), so the test uses weights of about 2^30: the product then
needs up to 54 bits and is rounded, and `_separating_values` searches, on the CPU and in exact rational arithmetic,
for values where rounding once (a fused multiply-add) and rounding twice give different float64 sums."""
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import inputs as gin
from utils.helper import AverageMeter, DeviceMeters

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG_N = [(1 << 30) + 12345, 0, (1 << 29) + 7, (1 << 30) + 999983, 3]        # five updates, one with weight 0


def _bits(x):
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def _same(got, want, what):
    got, want = float(got), float(want)
    if want != want:
        assert got != got, (what, got, want)
    else:
        assert _bits(got) == _bits(want), (what, got, want, got - want)


def _fused(total, v, n):
    """sum + v * n rounded ONCE (what a fused multiply-add returns): exact rationals, then the nearest float64"""
    return float(Fraction(total) + Fraction(v) * n)


def _separating_values(count, seed):
    """`count` float32 values per update of BIG_N such that, along the sequence of five updates, the twice-rounded sum
    (AverageMeter) differs from the once-rounded one at least once for EVERY value column."""
    rng = np.random.RandomState(seed)
    columns = []
    while len(columns) < count:
        vals = rng.uniform(0.1, 9.0, len(BIG_N)).astype(np.float32)
        plain = fused = 0.0
        split = False
        for v, n in zip(vals, BIG_N):
            v = float(v)
            plain = plain + v * n
            fused = _fused(fused, v, n)
            split = split or plain != fused
            fused = plain                         # compare update by update, from the same running sum
        if split:
            columns.append(vals)
    return np.stack(columns, 1)                   # [updates, count]


def test_the_chosen_values_really_separate_fused_from_unfused():
    vals = _separating_values(40, 7)
    assert vals.shape == (5, 40) and vals.dtype == np.float32
    for i in range(40):
        total, split = 0.0, 0
        for v, n in zip(vals[:, i], BIG_N):
            v = float(v)
            two_roundings = total + v * n
            split += two_roundings != _fused(total, v, n)
            total = two_roundings
        assert split >= 1, i
    # and the premise: the product itself is inexact in float64 for these weights
    assert any(Fraction(float(vals[0, i])) * BIG_N[0] != Fraction(float(vals[0, i]) * BIG_N[0]) for i in range(40))


def _feed(names, rows, weights, device_meters, host_meters):
    for row, n in zip(rows, weights):
        flat = torch.tensor(np.asarray(row, dtype=np.float32), device=DEV)
        device_meters.update({name: flat[i] for i, name in enumerate(names)}, n)
        for name, v in zip(names, row):
            host_meters.setdefault(name, AverageMeter(name=name)).update(float(np.float32(v)), n)


def _compare(device_meters, host_meters):
    got = device_meters.read()
    assert list(got) == list(host_meters)
    for name, want in host_meters.items():
        m = got[name]
        for field in ('sum', 'count', 'avg', 'val'):
            _same(getattr(m, field), getattr(want, field), (name, field))


@pytest.mark.parametrize('S', [1, 3, 32, 33, 40])
def test_meters_equal_average_meter_bit_for_bit(S):
    """S = 33 and 40 cross the 32-pointer launch boundary (two launches per update)."""
    import hip_runtime as hr
    names = ['training/stat_%02d' % i for i in range(S)]
    rows = _separating_values(S, 100 + S)
    dm, host = DeviceMeters(DEV), {}
    with hr.launch_log() as log:
        _feed(names, rows, BIG_N, dm, host)
    launches = sum(v for k, v in log.counts.items() if 'meter_update_kernel' in k)
    assert launches == len(BIG_N) * (2 if S > 32 else 1)
    _compare(dm, host)
    got = dm.read()
    assert got[names[0]].count == float(sum(BIG_N)) and got[names[-1]].val == float(rows[-1, -1])
    # the ordinary case too: small weights, where the product is exact
    dm.reset()
    host = {}
    _feed(names, rows, [16, 16, 0, 7, 1], dm, host)
    _compare(dm, host)


def test_a_fused_multiply_add_would_have_been_caught():
    """The device sums differ from the once-rounded sums in at least one column: the test above can tell them apart."""
    S = 8
    rows = _separating_values(S, 5)
    dm, host = DeviceMeters(DEV), {}
    names = ['s%d' % i for i in range(S)]
    _feed(names, rows, BIG_N, dm, host)
    got = dm.read()
    differs = 0
    for i, name in enumerate(names):
        total = 0.0
        for v, n in zip(rows[:, i], BIG_N):
            total = _fused(total, float(v), n)
        differs += _bits(total) != _bits(got[name].sum)
    assert differs >= 1


def test_nan_zero_weight_reset_and_late_names():
    dm, host = DeviceMeters(DEV, capacity=8), {}
    _feed(['a', 'b'], [[1.5, float('nan')], [2.25, 4.0]], [4, 2], dm, host)
    _feed(['a', 'b', 'c'], [[0.1, 0.2, float('inf')]], [0], dm, host)              # weight 0: NaN * 0, inf * 0
    _compare(dm, host)
    got = dm.read()
    assert got['a'].sum == 1.5 * 4 + 2.25 * 2 + 0.0 and got['a'].count == 6 and got['a'].val == float(np.float32(0.1))
    assert got['b'].sum != got['b'].sum and got['c'].sum != got['c'].sum and got['c'].count == 0 and got['c'].avg == 0
    dm.reset()
    for m in host.values():
        m.reset()
    _compare(dm, host)
    assert all(m.sum == 0 and m.count == 0 and m.avg == 0 and m.val == 0 for m in dm.read().values())
    _feed(['c', 'a'], [[3.0, 5.0]], [2], dm, host)                                  # slots out of order: two launches
    _compare(dm, host)
    assert dm.read()['c'].avg == 3.0 and dm.read()['b'].count == 0
    with pytest.raises(RuntimeError, match='capacity'):
        dm.update({'n%d' % i: torch.zeros((), device=DEV) for i in range(6)}, 1)


def test_values_that_are_no_device_scalars_go_to_a_host_meter():
    dm = DeviceMeters(DEV)
    on_device = torch.tensor(2.0, device=DEV)
    for n in (2, 6):
        dm.update({'loss': on_device, 'number': 0.5 * n, 'host_tensor': torch.tensor(1.25 * n),
                   'double': torch.tensor(3.0, device=DEV, dtype=torch.float64)}, n)
    got = dm.read()
    assert list(dm.slots) == ['loss'] and sorted(dm.host) == ['double', 'host_tensor', 'number']
    assert got['loss'].avg == 2.0 and got['loss'].count == 8
    want = AverageMeter(name='number')
    want.update(1.0, 2), want.update(3.0, 6)
    assert (got['number'].sum, got['number'].avg, got['number'].val) == (want.sum, want.avg, want.val)
    assert got['host_tensor'].avg == (2.5 * 2 + 7.5 * 6) / 8 and got['double'].avg == 3.0
    dm.reset()
    assert dm.read()['number'].count == 0 and dm.read()['loss'].count == 0


def test_the_binding_refuses_bad_arguments():
    from hip_runtime import ops
    import hip_runtime as hr
    s, c = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    last = torch.zeros(4, device=DEV)
    v = torch.tensor(1.0, device=DEV)
    with pytest.raises(RuntimeError, match='negative'):
        ops.meter_update([v], -1, s, c, last)
    with pytest.raises(RuntimeError, match='1 to 32'):
        ops.meter_update([], 1, s, c, last)
    with pytest.raises(RuntimeError, match='1 to 32'):
        ops.meter_update([v] * 33, 1, torch.zeros(64, dtype=torch.float64, device=DEV),
                         torch.zeros(64, dtype=torch.float64, device=DEV), torch.zeros(64, device=DEV))
    with pytest.raises(RuntimeError, match='at least 5'):
        ops.meter_update([v] * 5, 1, s, c, last)
    with pytest.raises(RuntimeError, match='0-dim float32'):
        ops.meter_update([torch.zeros(2, device=DEV)], 1, s, c, last)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.meter_update([torch.tensor(1.0)], 1, s, c, last)
    L = hr.lib()
    assert L.cnuda_meter_update(None, 1, 1.0, None, None, None, None) == -1          # no launch, an error code
    torch.cuda.synchronize()
    assert not s.any() and not c.any() and not last.any()


def test_the_statistics_of_real_evaluation_steps():
    """The `stats` dicts of three is_training=False steps of the ResNet-18 plugin (128 x 128, the smallest input
    tests/test_gpu_resnet.py runs), kept on the device (host_stats = False), into both kinds of meter."""
    from backends import resnet
    from losses.centernet import DetectionLoss
    from uda.base import Model
    torch.manual_seed(0)
    plugin = Model()
    plugin.backend = resnet.build(18, num_classes=6, pretrained=False)
    plugin.device = torch.device(DEV)
    plugin.centernet_loss = DetectionLoss(hm_weight=1.0, wh_weight=0.1, off_weight=1.0)
    plugin.init_done()
    plugin.to(DEV)
    plugin.set_phase(False)
    assert Model.host_stats is True
    plugin.host_stats = False
    dm, host = DeviceMeters(DEV), {}
    for step, B in enumerate((2, 2, 1)):
        data = {k: torch.from_numpy(v) for k, v in gin.detection_batch(B, 6, 32, 32, 8, (5, 3), 2, 80 + step).items()}
        data['input'] = torch.from_numpy(gin.image_batch(B, 128, 128, 90 + step))
        with torch.no_grad():
            stats = plugin.step(data, is_training=False)['stats']
        assert sorted(stats) == ['centernet_loss', 'hm_loss', 'off_loss', 'total_loss', 'wh_loss']
        assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 and not v.requires_grad
                   for v in stats.values())
        dm.update({'validation/' + k: v for k, v in stats.items()}, B)
        for k, v in stats.items():
            host.setdefault('validation/' + k, AverageMeter(name=k)).update(v.item(), B)
    _compare(dm, host)
    assert not dm.host and all(np.isfinite(m.avg) and m.count == 5 for m in dm.read().values())
