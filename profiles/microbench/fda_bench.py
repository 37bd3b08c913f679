"""FDA amplitude transfer (csrc/fda.hip, utils/image.FDA_source_to_target) on one MI355X: ms per call and achieved
bandwidth against the algorithmic bytes -- two images read, one written, and the two half spectra
(B*C*H*(W/2+1) complex fp32 each) written by the row pass, read and written by the forward column pass, read by the
inverse column pass (which writes one back), and that one read by the inverse row pass: 10 spectrum-sized transfers.

    python profiles/microbench/fda_bench.py [--iters 50] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'centernet-uda_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

from utils.image import FDA_source_to_target  # noqa: E402

HBM_PEAK = 8.0e12     # bytes/s, MI355X spec (MI355X_MICROARCH: ~6.3e12 reachable by a copy kernel)


def algorithmic_bytes(B, C, H, W):
    img = B * C * H * W * 4
    spec = B * C * H * (W // 2 + 1) * 8
    return 3 * img + 10 * spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = []
    for B, S in ((8, 512), (16, 512), (16, 640)):
        g = torch.Generator(device=dev).manual_seed(B * S)
        src = torch.randn(B, 3, S, S, device=dev, generator=g)
        trg = torch.randn(B, 3, S, S, device=dev, generator=g)
        for circular, L in ((False, 0.01), (True, 0.01)):
            for _ in range(5):
                FDA_source_to_target(src, trg, L, circular)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                FDA_source_to_target(src, trg, L, circular)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            nbytes = algorithmic_bytes(B, 3, S, S)
            rec = {'B': B, 'C': 3, 'H': S, 'W': S, 'mode': 'circular' if circular else 'square', 'L': L,
                   'ms_per_call': round(ms, 4), 'algorithmic_GB': round(nbytes / 1e9, 4),
                   'GB_per_s': round(nbytes / (ms * 1e-3) / 1e9, 1),
                   'fraction_of_8TBps': round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
