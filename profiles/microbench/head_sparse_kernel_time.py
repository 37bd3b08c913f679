"""Kernel time of a detection head's backward on SMALL inputs, dense against sparse: does the size rule of
hip_runtime.ops need a floor on B * H * W?  (It does not: profiles/head_sparse_ab.txt.)  Event timing (head_sparse_crossover.py) is bound by launch overhead there; this is the sum of the kernels' own durations from
a kernel trace.
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 head_sparse_kernel_time.py run
    python3 head_sparse_kernel_time.py parse DIR
`run`: for every (B, map) below and both paths, REPS x (head forward, reg_l1_loss, backward), the real head (64 -> 256 3x3 +
ReLU, 256 -> 2), M = 32 rows per image, all active; a torch cosine kernel closes each segment.  `parse`: the library's kernel
time per repetition and segment; forward and loss are the same launches on both paths, so the difference is the backward's."""
import csv
import glob
import os
import sys

CASES = [(4, 32), (16, 32), (2, 64), (8, 64), (1, 128), (2, 128), (4, 128)]      # B, map side
REPS, M = 10, 32


def run():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(root, 'centernet-uda_amd'))
    import torch
    import hip_runtime.nn as hnn
    from hip_runtime import ops
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    head = hnn.Head(hnn.Conv2d(64, 256, 3, padding=1, bias=True, act_slope=0.0), hnn.Slot(), hnn.Conv2d(256, 2, 1, bias=True)).to(dev)
    ops.HEAD_SPARSE_RATIO = 0
    mark = torch.zeros(64, device=dev)
    for B, S in CASES:
        x = torch.randn(B, 64, S, S, device=dev, requires_grad=True)
        ind = torch.stack([torch.randperm(S * S)[:M] for _ in range(B)]).to(dev)
        mask = torch.ones(B, M, dtype=torch.uint8, device=dev)
        target = torch.randn(B, M, 2, device=dev)
        for sparse in (False, True):
            ops.HEAD_SPARSE = sparse
            for i in range(REPS + 2):
                if i == 2:
                    mark.cos_()                   # (two warm-up repetitions lie before the segment)
                ops.reg_l1_loss(head(x), mask, ind, target.clone()).backward()
            mark.cos_()
            torch.cuda.synchronize()


def parse(d):
    rows = list(csv.DictReader(open(glob.glob(d + '/*/*kernel_trace.csv')[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    segs, cur = [], 0.0
    for r in rows:
        if 'cos' in r['Kernel_Name']:
            segs.append(cur)
            cur = 0.0
        elif 'cnuda' in r['Kernel_Name']:
            cur += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    timed = segs[1::2]                            # (every other segment is a warm-up)
    print('B  map      pixels   dense us  sparse us   (library kernel time of forward + loss + backward per repetition)')
    for i, (B, S) in enumerate(CASES):
        print('%-2d %3dx%-3d  %7d  %9.1f  %9.1f' % (B, S, S, B * S * S, timed[2 * i] / REPS, timed[2 * i + 1] / REPS))


if __name__ == '__main__':
    run() if sys.argv[1] == 'run' else parse(sys.argv[2])
