"""Where the sparse backward of a detection head stops paying (hip_runtime.ops.HEAD_SPARSE_RATIO): the real head
(64 -> 256 3x3 + ReLU, 256 -> 2 1x1, B = 16) on a 128 x 128 and a 32 x 32 map, backward of reg_l1_loss(head(x)) timed with
the switch on and off for M = 32 ... 2048 rows per image, every row active and, while the map has that many cells, distinct (the sparse path's worst case).
The size rule is lifted for the measurement (HEAD_SPARSE_RATIO = 0) so that every M takes the path under test."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'centernet-uda_amd'))
import torch
import hip_runtime as hr
import hip_runtime.nn as hnn
from hip_runtime import ops

dev = torch.device('cuda', 0)
B, C, Ch, Co = 16, 64, 256, 2
torch.manual_seed(0)
head = hnn.Head(hnn.Conv2d(C, Ch, 3, padding=1, bias=True, act_slope=0.0), hnn.Slot(), hnn.Conv2d(Ch, Co, 1, bias=True)).to(dev)
ops.HEAD_SPARSE_RATIO = 0


def backward_us(x, mask, ind, target, sparse, reps=10):
    ops.HEAD_SPARSE = sparse
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total = 0.0
    for i in range(reps + 2):
        loss = ops.reg_l1_loss(head(x), mask, ind, target.clone())
        with hr.launch_log() as log:
            ev[0].record()
            loss.backward()
            ev[1].record()
        torch.cuda.synchronize()
        assert any('head_rows_kernel' in n for n in log.names) == sparse, log.names
        if i >= 2:
            total += ev[0].elapsed_time(ev[1]) * 1e3
    return total / reps


print('map      M     R=B*M   dense us   sparse us   (backward of loss + head; kernels + launch overhead of one stream)')
for S in (128, 32):
    HW = S * S
    x = torch.randn(B, C, S, S, device=dev, requires_grad=True)
    for M in (32, 150, 512, 2048):
        # (distinct cells while the map has that many; beyond that, repeated cells: fewer active rows, the same launches)
        ind = torch.stack([torch.randperm(HW)[:M] if M <= HW else torch.randint(0, HW, (M,)) for _ in range(B)]).to(dev)
        mask = torch.ones(B, M, dtype=torch.uint8, device=dev)
        target = torch.randn(B, M, Co, device=dev)
        d, s = backward_us(x, mask, ind, target, False), backward_us(x, mask, ind, target, True)
        print('%3dx%-3d %5d  %6d  %9.1f  %10.1f' % (S, S, M, B * M, d, s), flush=True)
