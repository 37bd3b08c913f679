"""Same bits, same launches: the convolution call paths of two builds of the package, one fresh child process per build.

    python profiles/conv_call_path_ab.py PARENT_DIR [OUT_DIR]      (PARENT_DIR, THIS_DIR: directories that hold hip_runtime/,
                                                                    libs/, _ext.py and the built library of each side;
                                                                    THIS_DIR defaults to centernet-uda_amd)
Every child runs the cases below -- the small geometries of tests/test_gpu_ops.py -- with seeded inputs through hip_runtime.ops
(or, where the tests do, the C ABI), and writes one line per output tensor (SHA-256 of its bytes) and one per kernel the case
launched (name, count: the library's launch log).  A second pair of children runs the dense cases under CNUDA_BUF=0 (the
pointer and fast-pointer loaders).  The driver compares the files line by line; exit status 1 when they differ.
A child is     python profiles/conv_call_path_ab.py --side DIR --out FILE"""
import hashlib
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def child(side, out_path):
    sys.path[:0] = [side, os.path.join(ROOT, 'tests')]
    import torch
    import hip_runtime as hr
    from hip_runtime import ops
    from libs.DCNv2 import dcn_v2
    from test_gpu_ops import CAT_CASES, CONV_CASES, ROWQUAD_CASES
    L = hr.lib()
    lines = []

    def rand(gen, *shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(DEV)

    def record(case, log, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            h = 'none' if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
            lines.append('%s\t%s\t%s' % (case, k, h))
        for k in sorted(log.counts):
            lines.append('%s\tlaunch\t%s\t%d' % (case, k, log.counts[k]))

    def gen(name):
        return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 1000)

    def conv_case(name, tag='', stats=False, k=None):
        B, C, H, W, Co, kk, s, p, bias, act = CONV_CASES[name] if k is None else k
        g = gen(name)
        x, w = rand(g, B, C, H, W).requires_grad_(True), rand(g, Co, C, kk, kk, scale=(C * kk * kk) ** -0.5).requires_grad_(True)
        b = rand(g, Co).requires_grad_(True) if bias else None
        with hr.launch_log() as log:
            y = ops.conv2d(x, w, b, s, p, act, emit_stats=stats)
            st = getattr(y, '_cnuda_bn_stats', None)
            y.backward(rand(g, *y.shape))
        record('conv:%s%s' % (name, tag), log, y=y, stats=st and st[0], gx=x.grad, gw=w.grad, gb=None if b is None else b.grad)

    dense = sorted(CONV_CASES)
    if os.environ.get('CNUDA_BUF') == '0':           # the pointer loaders: the dense cases alone
        for name in dense:
            conv_case(name, ' [CNUDA_BUF=0]')
        open(out_path, 'w').write('\n'.join(lines) + '\n')
        return
    for name in dense:
        conv_case(name)
    for name in ('stem7x7', 'c16_3x3', 'c64_3x3', 'root1x1', 'head_out', 's2_even', 'offset27_w32'):
        conv_case(name, ' +stats', stats=True)
    # halo tiles for every eligible layer (tests/test_gpu_ops.py test_halo_tile_convolution_3x3), forward with bias + ReLU
    with hr.halo_conv(1, 1), hr.splitk(0):
        for B, C, Co, H, W in [(2, 32, 27, 8, 16), (2, 64, 64, 8, 64), (1, 128, 256, 6, 64), (2, 32, 48, 2, 128), (2, 32, 27, 8, 160),
                               (1, 64, 64, 16, 80)]:
            conv_case('halo_%d_%d_%d_%d_%d' % (B, C, Co, H, W), k=(B, C, H, W, Co, 3, 1, 1, True, 0.0))
    # the row-sigmoid epilogue (DCN's offset convolution): im2col, split-K and -- under the halo policy -- halo-tile instances
    for name, halo in (('offset27', False), ('sk_512to27_16sq', False), ('offset27_w32', False), ('offset27_w32', True)):
        B, C, H, W, Co, kk, s, p, _, _ = CONV_CASES[name]
        g = gen(name)
        x, w, b = (rand(g, B, C, H, W).requires_grad_(True), rand(g, Co, C, kk, kk, scale=0.05).requires_grad_(True),
                   rand(g, Co).requires_grad_(True))
        with hr.halo_conv(1, 1) if halo else hr.splitk(128), hr.launch_log() as log:
            y = ops.conv2d_rowsig(x, w, b, s, p, 18)
            y.backward(rand(g, *y.shape))
        record('rowsig:%s%s' % (name, ' halo' if halo else ''), log, y=y, gx=x.grad, gw=w.grad, gb=b.grad)
    # row quads against the plain layout, through the C ABI as the test does
    for name in sorted(ROWQUAD_CASES):
        B, K, H, W, M = ROWQUAD_CASES[name]
        g = gen(name)
        x, w = rand(g, B, K, H, W), rand(g, M, K, 1, 1, scale=K ** -0.5)
        geom = (B, K, H, W, M, 1, 1, 1, 1, 0, 0)
        plain, quads = torch.empty(B, M, H, W, device=DEV), torch.empty(B, M, H, W, device=DEV)
        wp, wn = ops._ws(L.cnuda_conv2d_workspace_bytes(*geom), x)
        with hr.launch_log() as log:
            hr.check(L.cnuda_conv2d_forward(hr.ptr(x), hr.ptr(w), None, hr.ptr(plain), *geom, -1.0, wp, wn, hr.stream()))
            if L.cnuda_conv2d_rowquads_supported(*geom):
                hr.check(L.cnuda_conv2d_forward_rowquads(hr.ptr(x), hr.ptr(w), hr.ptr(quads), *geom, wp, wn, hr.stream()))
            else:
                quads = None
        record('rowquads:' + name, log, plain=plain, quads=quads)
    # an addend that aliases grad_x (the fan-in slots accumulate in place): every input-gradient family
    for name in ('c16_3x3', 'c64_3x3', 'c16_s2', 's2_even', 's2_k1', 'sk_s2_mixed', 'sk_256to64_8sq', 'odd'):
        B, C, H, W, Co, kk, s, p, _, _ = CONV_CASES[name]
        g = gen(name)
        geom = (B, C, H, W, Co, kk, kk, s, s, p, p)
        w, gy = rand(g, Co, C, kk, kk, scale=0.05), rand(g, B, Co, (H + 2 * p - kk) // s + 1, (W + 2 * p - kk) // s + 1)
        acc, other = rand(g, B, C, H, W), rand(g, B, C, H, W)
        wp, wn = ops._ws(L.cnuda_conv2d_workspace_bytes(*geom), gy)
        with hr.launch_log() as log:
            hr.check(L.cnuda_conv2d_backward_data_add(hr.ptr(gy), hr.ptr(w), hr.ptr(acc), hr.ptr(other), hr.ptr(acc), *geom, wp, wn,
                                                      hr.stream()))
        record('aliased:' + name, log, acc=acc)
    # the concatenation-free Root: 2, 3 and 4 sources; training form with statistics, inference form with bias + ReLU
    for name in ('level2_64_64', 'level4_three_sources', 'level3_four_sources', 'ragged_pixels'):
        B, H, W, cs, Co = CAT_CASES[name]
        g = gen(name)
        xs = [rand(g, B, c, H, W).requires_grad_(True) for c in cs]
        w, b = rand(g, Co, sum(cs), 1, 1, scale=sum(cs) ** -0.5).requires_grad_(True), rand(g, Co)
        with hr.launch_log() as log:
            y = ops.conv1x1_cat(xs, w, 0, emit_stats=True)
            st = getattr(y, '_cnuda_bn_stats', None)
            y.backward(rand(g, *y.shape))
            yi = ops.conv1x1_cat_infer(xs, w, b, 0.0)
        record('cat:' + name, log, y=y, stats=st and st[0], gw=w.grad, infer=yi, **{'gx%d' % i: t.grad for i, t in enumerate(xs)})
    # the detection-head node (whole batch; leading images only), a folded residual block's forward, the transposed convolution
    for lead in (None, 1):
        g = gen('head')
        x, w1, b1 = rand(g, 2, 64, 8, 8).requires_grad_(True), rand(g, 256, 64, 3, 3, scale=0.04).requires_grad_(True), rand(g, 256).requires_grad_(True)
        w2, b2 = rand(g, 6, 256, 1, 1, scale=0.06).requires_grad_(True), rand(g, 6).requires_grad_(True)
        with hr.launch_log() as log:
            y = ops._ConvActConv1x1.apply(x, w1, b1, w2, b2, (1, 1), 0.0, 0, 0, lead)
            y.backward(rand(g, *y.shape))
        record('head lead=%s' % lead, log, y=y, gx=x.grad, gw1=w1.grad, gb1=b1.grad, gw2=w2.grad, gb2=b2.grad)
    g = gen('infer')
    x, w, b, r = rand(g, 1, 64, 12, 12), rand(g, 64, 64, 3, 3, scale=0.04), rand(g, 64), rand(g, 1, 64, 12, 12)
    with hr.launch_log() as log:
        y = ops.conv2d_infer(x, w, b, 1, 1, 0.0, residual=r)
    record('infer residual', log, y=y)
    g = gen('convT')
    x, w = rand(g, 2, 64, 8, 8).requires_grad_(True), rand(g, 64, 32, 4, 4, scale=0.03).requires_grad_(True)
    with hr.launch_log() as log:
        y = ops.conv_transpose2d(x, w, 2, 1, 0)
        y.backward(rand(g, *y.shape))
    record('conv_transpose2d', log, y=y, gx=x.grad, gw=w.grad)
    # a DCN layer with and without the saved columns (the weight gradient from the columns / sampling again)
    for keep in (True, False):
        dcn_v2._KEEP_COLUMNS = keep
        torch.manual_seed(7)
        m = dcn_v2.DCN(64, 64, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)
        with torch.no_grad():
            m.conv_offset_mask.weight.normal_(0, 0.05)
        m = m.to(DEV)
        g = gen('dcn')
        x = rand(g, 2, 64, 16, 16).requires_grad_(True)
        with hr.launch_log() as log:
            y = m(x)
            y.backward(rand(g, *y.shape))
        record('dcn columns=%s' % keep, log, y=y, gx=x.grad, **{'g_' + n: p.grad for n, p in m.named_parameters()})
    open(out_path, 'w').write('\n'.join(lines) + '\n')


def main():
    if sys.argv[1] == '--side':
        return child(os.path.abspath(sys.argv[2]), sys.argv[4])
    parent = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'abl', 'conv_call_path')
    os.makedirs(out, exist_ok=True)
    status = 0
    for tag, env in (('', {}), ('_ptr', {'CNUDA_BUF': '0'})):
        files = []
        for side, d in (('parent', parent), ('this', os.path.join(ROOT, 'centernet-uda_amd'))):
            files.append(os.path.join(out, 'conv_call_path_%s%s.txt' % (side, tag)))
            subprocess.run([sys.executable, os.path.abspath(__file__), '--side', d, '--out', files[-1]],
                           env=dict(os.environ, **env), check=True, timeout=600)
        a, b = (open(f).read().splitlines() for f in files)
        bad = [(u, v) for u, v in zip(a, b) if u != v]
        tensors = sum('\tlaunch\t' not in u for u in a)
        print('%s: %d lines (%d tensors, %d launch-log lines) against %d; differing lines: %d'
              % (env or 'default', len(a), tensors, len(a) - tensors, len(b), len(bad) + abs(len(a) - len(b))))
        for u, v in bad[:10]:
            print('  parent: %s\n  this:   %s' % (u, v))
        status |= 1 if bad or len(a) != len(b) else 0
    return status


if __name__ == '__main__':
    sys.exit(main())
