"""The planning queries of the convolution / DCN library over a sweep of geometries (tests/test_host_plan_table.py).

    python tests/golden/make_plan_table.py --sweep [--lib PATH]     one process: the answers under ITS environment, JSON on stdout
    python tests/golden/make_plan_table.py --write [--lib PATH]     plan_table.json: one child process per environment of ENVS

The queries are pure host code (no GPU).  The committed plan_table.json was written with `--lib` pointing at the library of
the commit BEFORE the kernel choice moved into ConvPlan / DcnPlan: the table pins that the plan answers what the scattered
rules answered.  Regenerate it only from a build whose answers are the intended ones -- never to make a red test green.
The CNUDA_* switches are read once per process, hence the children."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, 'plan_table.json')

ENVS = {
    'default': {},
    'buf0': {'CNUDA_BUF': '0'},
    'ws0': {'CNUDA_WS': '0'},
    'splitk0': {'CNUDA_SPLITK': '0'},
    'hconv0': {'CNUDA_HCONV': '0'},
    'hconv1': {'CNUDA_HCONV': '1'},
}
SWITCHES = sorted({k for e in ENVS.values() for k in e})


def _dla34(S, B, classes):
    """(conv cases, cat cases, dcn cases) of CenterNet DLA-34 on an S x S input, batch B (backends/dla.py)."""
    ch = [16, 32, 64, 128, 256, 512]
    conv = [(B, 3, S, S, 16, 7, 1, 3), (B, 16, S, S, 16, 3, 1, 1), (B, 16, S, S, 32, 3, 2, 1)]
    cat = []
    for i in range(2, 6):
        ci, co, hi, ho = ch[i - 1], ch[i], S >> (i - 1), S >> i
        conv += [(B, ci, hi, hi, co, 3, 2, 1), (B, co, ho, ho, co, 3, 1, 1), (B, ci, ho, ho, co, 1, 1, 0)]
        # roots: two tree outputs, + the level's pooled input (level_root), + earlier roots of a deeper tree
        for srcs in ([co, co], [co, co, ci], [co, co, co], [co, co, co, ci]):
            conv.append((B, sum(srcs), ho, ho, co, 1, 1, 0))
            cat.append((srcs, B, ho, ho, co))
    dcn = []
    for i in range(2, 6):                     # DLAUp / IDAUp: DeformConv between the levels' widths at each level's map
        for j in range(2, i + 1):
            for s in range(j, i + 1):
                g = (B, ch[i], S >> s, S >> s, ch[j])
                if g not in dcn:
                    dcn.append(g)
                    dcn.append((B, ch[j], S >> s, S >> s, ch[j]))
    dcn = sorted(set(dcn))
    conv += [(b, c, h, w, 27, 3, 1, 1) for (b, c, h, w, _) in dcn]      # their offset / mask convolutions
    conv += [(b, co, h, w, 9 * c, 1, 1, 0) for (b, c, h, w, co) in dcn]  # ... and column-gradient GEMMs
    q = S >> 2
    conv += [(B, 64, q, q, 256, 3, 1, 1)] + [(B, 256, q, q, n, 1, 1, 0) for n in (classes, 2, 1)]
    return conv, cat, [g + (3, 1, 1, 1, 1) for g in dcn]


def _resnet18(S, B, classes):
    conv = [(B, 3, S, S, 64, 7, 2, 3)]
    h, cin = S >> 2, 64
    for i, c in enumerate((64, 128, 256, 512)):
        if i:
            conv += [(B, cin, h, h, c, 3, 2, 1), (B, cin, h, h, c, 1, 2, 0)]
            h >>= 1
        conv.append((B, c, h, h, c, 3, 1, 1))
        cin = c
    q = S >> 2
    conv += [(B, 256, q, q, 64, 3, 1, 1)] + [(B, 64, q, q, n, 1, 1, 0) for n in (classes, 2)]
    return conv, [], []


def _advent(S, B, classes):
    conv, h, cin = [], S >> 2, classes          # uda/adversarial_entropy_minimization.py: 4x4 / stride 2 / padding 1
    for c in (64, 128, 256, 512, 1):
        conv.append((B, cin, h, h, c, 4, 2, 1))
        h, cin = h // 2, c
    return conv, [], []


def cases():
    """-> (conv, cat, dcn): conv (B, C, H, W, Co, k, s, p) or (B, C, H, W, Co, kh, kw, sh, sw, ph, pw); cat (cs, B, H, W, Co);
    dcn (B, C, H, W, Co, k, s, p, d, dg)."""
    conv, cat, dcn = [], [], []

    def add(t):
        conv.extend(t[0]); cat.extend(t[1]); dcn.extend(t[2])
    # the five bench.CONFIGS models at their bench sizes (source batch, and source + target stacked) and at the 128 x 128
    # fixture size
    for S, B in ((512, 16), (512, 32), (640, 16), (640, 32), (128, 2), (128, 4)):
        add(_dla34(S, B, 80))
    for S, B in ((640, 16), (640, 32), (128, 2), (128, 4)):
        add(_advent(S, B, 80))
    for S, B in ((256, 2), (128, 2)):
        add(_resnet18(S, B, 80))
    # the named cases of tests/test_gpu_ops.py::test_conv2d_fwd_bwd
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_gpu_ops import CONV_CASES
    conv += [CONV_CASES[n][:8] for n in sorted(CONV_CASES)]
    # the edges the rules test for
    for C in (3, 8, 16, 24, 63, 64):
        for Co in (2, 27, 32, 33, 64, 65, 128, 256):
            conv.append((2, C, 32, 32, Co, 3, 1, 1))
            conv.append((8, C, 64, 64, Co, 1, 1, 0))
    for k, p in ((1, 0), (3, 1), (4, 1), (7, 3)):
        for s in (1, 2, 4):
            for C, Co in ((16, 32), (64, 64), (128, 27)):
                conv.append((4, C, 64, 64, Co, k, s, p))
    for W in (1, 40, 96, 160):
        for C, Co in ((16, 16), (64, 27), (64, 128)):
            conv += [(2, C, 32, W, Co, 3, 1, 1), (2, C, 32, W, Co, 3, 2, 1), (16, C, 160, W, Co, 3, 1, 1)]
    conv += [(1, 64, 5, 5, 64, 3, 1, 1), (3, 64, 7, 9, 32, 1, 1, 0), (2, 32, 15, 15, 27, 3, 1, 1), (2, 16, 31, 33, 16, 3, 1, 1)]   # H W % 4 != 0
    conv += [(2, 64, 32, 48, 64, 3, 5, 1, 1, 1, 2), (2, 64, 32, 48, 64, 1, 3, 2, 1, 0, 1)]      # rectangular kernels / strides
    # tensors just under and just over 2 GiB: the input (B 64 128^2 floats: B = 511 | 512), the output, both
    for B in (511, 512):
        conv += [(B, 64, 128, 128, 64, 3, 1, 1), (B, 64, 128, 128, 27, 3, 1, 1), (B, 64, 128, 128, 16, 1, 1, 0),
                 (B, 16, 128, 128, 64, 1, 1, 0), (B, 64, 128, 128, 64, 3, 2, 1), (B, 16, 256, 256, 32, 3, 2, 1)]
        cat += [([64, 64], B // 2, 128, 128, 64), ([64, 64], B, 64, 64, 256)]
        dcn += [(B, 64, 128, 128, 64, 3, 1, 1, 1, 1), (B, 64, 64, 64, 27, 3, 1, 1, 1, 1)]
    cat += [([64, 64], 2, 32, 32, 64), ([64, 128, 64], 2, 16, 16, 128), ([64, 32], 2, 32, 32, 64), ([64, 64], 2, 5, 5, 64),
            ([128, 128, 128, 128], 4, 8, 8, 512), ([64] * 5, 2, 16, 16, 64), ([64, 64], 16, 128, 128, 27)]
    for dg in (1, 2):
        for C, Co in ((16, 8), (64, 64), (64, 128), (24, 65), (128, 27)):
            for H, W in ((9, 9), (16, 16), (32, 40), (64, 64), (24, 96), (160, 160), (7, 1), (5, 7)):
                dcn.append((2, C, H, W, Co, 3, 1, 1, 1, dg))
        dcn += [(4, 64, 32, 32, 64, 3, 2, 1, 1, dg), (4, 64, 32, 32, 64, 3, 1, 2, 2, dg), (4, 32, 32, 32, 32, 1, 1, 0, 1, dg),
                (2, 16, 16, 16, 16, 7, 1, 3, 1, dg), (2, 16, 16, 16, 16, 4, 4, 0, 1, dg)]

    def uniq(rows):
        seen, out = set(), []
        for r in rows:
            key = json.dumps(r)
            if key not in seen:
                seen.add(key)
                out.append(json.loads(key))
        return out
    conv = [list(c) if len(c) == 11 else [c[0], c[1], c[2], c[3], c[4], c[5], c[5], c[6], c[6], c[7], c[7]] for c in conv]
    return uniq(conv), uniq([list(c) for c in cat]), uniq([list(d) for d in dcn])


def sweep(lib_path):
    L = ctypes.CDLL(lib_path)
    I, P = ctypes.c_int, ctypes.c_void_p
    for name, n in (('cnuda_conv2d_workspace_bytes', 11), ('cnuda_dcn_v2_workspace_bytes', 14)):
        getattr(L, name).restype = ctypes.c_size_t
        getattr(L, name).argtypes = [I] * n
    for name in ('cnuda_conv2d_rowsig_supported', 'cnuda_conv2d_rowquads_supported', 'cnuda_conv2d_norm_input_supported'):
        getattr(L, name).restype = I
        getattr(L, name).argtypes = [I] * 11
    L.cnuda_conv2d_stats_block.restype = I
    L.cnuda_conv2d_stats_block.argtypes = [I] * 11 + [P, P]
    L.cnuda_dcn_v2_stats_block.restype = I
    L.cnuda_dcn_v2_stats_block.argtypes = [I] * 14 + [P]
    L.cnuda_conv2d_cat_supported.restype = I
    L.cnuda_conv2d_cat_supported.argtypes = [P, I, I, I, I, I]
    L.cnuda_dcn_set_offset_regime.restype = I
    L.cnuda_dcn_set_offset_regime.argtypes = [I]
    conv, cat, dcn = cases()
    out = {'conv': [], 'cat': [], 'dcn': []}
    for c in conv:
        rows, bpi = I(-1), I(-1)
        blk = L.cnuda_conv2d_stats_block(*c, ctypes.byref(rows), ctypes.byref(bpi))
        out['conv'].append([L.cnuda_conv2d_workspace_bytes(*c), blk, rows.value if blk else -1, bpi.value,
                            L.cnuda_conv2d_rowsig_supported(*c), L.cnuda_conv2d_rowquads_supported(*c),
                            L.cnuda_conv2d_norm_input_supported(*c)])
    for cs, B, H, W, Co in cat:
        arr = (I * len(cs))(*cs)
        out['cat'].append(L.cnuda_conv2d_cat_supported(arr, len(cs), B, H, W, Co))
    for B, C, H, W, Co, k, s, p, d, dg in dcn:
        a = (B, C, H, W, Co, k, k, s, s, p, p, d, d, dg)
        row = [L.cnuda_dcn_v2_workspace_bytes(*a)]
        for regime in (0, 2):               # bit 1: the forward leaves the LDS-window kernel (another statistics layout)
            L.cnuda_dcn_set_offset_regime(regime)
            rows = I(-1)
            blk = L.cnuda_dcn_v2_stats_block(*a, ctypes.byref(rows))
            row += [blk, rows.value if blk else -1]
        L.cnuda_dcn_set_offset_regime(0)
        out['dcn'].append(row)
    return out


def default_lib():
    return os.path.join(ROOT, 'centernet-uda_amd', 'libcenternet_uda_hip.so')


def sweep_in_child(env_name, lib_path=None):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and not k.startswith('CNUDA_')}
    env.update(ENVS[env_name])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--sweep', '--lib', lib_path or default_lib()],
                         env=env, check=True, stdout=subprocess.PIPE).stdout
    return json.loads(out)


def main():
    lib_path = sys.argv[sys.argv.index('--lib') + 1] if '--lib' in sys.argv else default_lib()
    if '--sweep' in sys.argv:
        json.dump(sweep(lib_path), sys.stdout)
        return
    assert '--write' in sys.argv, __doc__
    conv, cat, dcn = cases()
    table = {'columns': {'conv': ['workspace_bytes', 'stats_block', 'stats_rows', 'blocks_per_image', 'rowsig', 'rowquads',
                                  'norm_input'],
                         'cat': 'supported',
                         'dcn': ['workspace_bytes', 'stats_block', 'stats_rows', 'stats_block@regime2', 'stats_rows@regime2']},
             'cases': {'conv': conv, 'cat': cat, 'dcn': dcn},
             'envs': {name: sweep_in_child(name, lib_path) for name in ENVS}}
    with open(TABLE, 'w') as f:
        f.write(json.dumps(table, separators=(',', ':')).replace('],[', '],\n[').replace('"envs"', '\n"envs"'))
        f.write('\n')
    print('%s: %d conv, %d cat, %d dcn cases x %d environments' % (TABLE, len(conv), len(cat), len(dcn), len(ENVS)))


if __name__ == '__main__':
    main()
