"""What the loader and the epoch loop cost: the training driver's milliseconds per step against bench.py's
`ms_per_step` of the same commit, on one MI355X, for the headline configuration (DLA-34, EntropyMinimization, 16 + 16
images, 512 x 512).

    python profiles/make_driver_dataset.py DATA --images 320
    python profiles/driver_loop_cost.py DATA OUT.jsonl

bench.py steps over one resident synthetic batch; the driver decodes 32 PNG files of 640 x 480 per step, pads,
uploads, augments, resizes, normalises and encodes them, and keeps its meters.  Both start from the same weights
(bench.build_plugin's: random DLA-34 with non-zero DCN offset convolutions, saved once and given to the driver as
`pretrained`) and use Adam with the same settings.  Every leg runs in a process of its own, one after the other; the
driver trains three epochs of 20 steps without validation (eval_at_n_epoch beyond the last epoch) and the first
epoch, which carries the warm-up, is dropped.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'centernet-uda_amd')

WEIGHTS = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(pkg)r]
import bench
from utils.helper import save_model
plugin = bench.build_plugin(torch.device('cuda', 0), False)
save_model(plugin.backend, %(path)r, 0)
"""

DRIVER = r"""
import json, logging, sys
sys.path[:0] = [%(pkg)r]
logging.basicConfig(level=logging.INFO)
import train
out = train.main(%(argv)r)
print('RESULT ' + json.dumps({'images_per_second': out['images_per_second'], 'epochs': out['epochs']}))
"""


def child(code, limit):
    done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=limit)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
        raise SystemExit('a leg failed with exit status %d; nothing more is started' % done.returncode)
    return done.stdout


def main():
    data, out_path = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    work = os.path.join(data, 'runs')
    os.makedirs(work, exist_ok=True)
    rows = []
    bench = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'],
                           capture_output=True, text=True, timeout=400)
    if bench.returncode != 0:
        sys.stderr.write(bench.stderr[-4000:])
        raise SystemExit('bench.py failed; nothing more is started')
    line = json.loads([l for l in bench.stdout.splitlines() if l.startswith('{')][-1])
    rows.append({'leg': 'bench.py', 'ms_per_step': line['ms_per_step'], 'images_per_s': line['value']})
    print(rows[-1], flush=True)
    weights = os.path.join(work, 'bench_weights.pth')
    child(WEIGHTS % {'root': ROOT, 'pkg': PKG, 'path': weights}, 300)
    common = ['experiment=entropy_minimization', 'pretrained=' + weights, 'epochs=2', 'eval_at_n_epoch=1000',
              'datasets.training.params.image_folder=%s/train/images' % data,
              'datasets.training.params.annotation_file=%s/train/instances.json' % data,
              'datasets.training.params.target_domain_glob=[%s/target/*.png]' % data,
              'datasets.validation.params.image_folder=%s/val/images' % data,
              'datasets.validation.params.annotation_file=%s/val/instances.json' % data,
              'datasets.validation.params.target_domain_glob=[%s/target/*.png]' % data]
    for workers, meters in ((16, 'true'), (0, 'true'), (16, 'false')):
        name = 'workers%d_meters_%s' % (workers, meters)
        argv = common + ['num_workers=%d' % workers, 'device_meters=' + meters,
                         'hydra.run.dir=%s' % os.path.join(work, name)]
        text = child(DRIVER % {'pkg': PKG, 'argv': argv}, 500)
        result = json.loads([l for l in text.splitlines() if l.startswith('RESULT ')][-1][7:])
        rates = result['images_per_second'][1:]                 # `pretrained` starts at epoch 0: epochs 0, 1, 2; drop the first
        ms = [16e3 / r for r in rates]
        rows.append({'leg': 'train.py', 'num_workers': workers, 'device_meters': meters == 'true',
                     'ms_per_step': [round(v, 3) for v in ms], 'images_per_s': [round(r, 2) for r in rates]})
        print(rows[-1], flush=True)
    with open(out_path, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
