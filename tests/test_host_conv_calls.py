"""The rejection paths of the eight convolution entry points that share one prologue (csrc/conv.hip, ConvCall): a workspace
that is too small and a geometry that cannot be, each answered with -1 and the exact text the entry point has always given
-- under the exported function's name, `cnuda_conv2d_forward_stats` and `cnuda_conv2d_backward_data_add` as
`cnuda_conv2d_forward` / `cnuda_conv2d_backward_data`.  The texts are those of the library before the prologue was shared.
Both rejections return before anything is launched: fake tensor pointers, no device."""
import ctypes

import pytest

P = 4096                                   # a non-null "tensor"
GEMM = (2, 64, 16, 16, 64, 3, 3, 1, 1, 1, 1)      # B, C, H, W, Cout, kh, kw, sh, sw, ph, pw: on the GEMM path (split-K forward)
ONE = (2, 64, 16, 16, 64, 1, 1, 1, 1, 0, 0)       # 1x1: the buffer-addressed GEMM without a K split (row quads)
SIG = (2, 64, 16, 16, 27, 3, 3, 1, 1, 1, 1)       # 27 output rows: a DCN offset convolution (row sigmoid)
BIG = (2, 64, 2, 2, 64, 7, 7, 1, 1, 1, 1)         # kernel larger than the padded input
BIG27 = BIG[:4] + (27,) + BIG[5:]
CAT, CAT_BAD = (2, 16, 16, 64), (2, 0, 16, 64)    # B, H, W, Cout of the 64 + 64 concatenation; no rows


def _cat_arrays():
    return (ctypes.c_void_p * 2)(P, P), (ctypes.c_int * 2)(64, 64)


def _call(L, name, g):
    xs, cs = _cat_arrays()
    ws = (None, 0, None)
    return {
        'forward_stats': lambda: L.cnuda_conv2d_forward_stats(P, P, P, None, P, None, *g, -1.0, *ws),
        'forward_rowquads': lambda: L.cnuda_conv2d_forward_rowquads(P, P, P, *g, *ws),
        'forward_rowsig': lambda: L.cnuda_conv2d_forward_rowsig(P, P, P, P, 18, *g, *ws),
        'backward_data_add': lambda: L.cnuda_conv2d_backward_data_add(P, P, None, None, P, *g, *ws),
        'backward_weight': lambda: L.cnuda_conv2d_backward_weight(P, P, P, P, *g, *ws),
        'cat_forward': lambda: L.cnuda_conv2d_cat_forward(xs, cs, 2, P, None, P, None, -1.0, *g, *ws),
        'cat_backward_data': lambda: L.cnuda_conv2d_cat_backward_data(P, P, xs, None, None, cs, 2, *g, *ws),
        'cat_backward_weight': lambda: L.cnuda_conv2d_cat_backward_weight(xs, cs, 2, P, P, *g, *ws),
    }[name]()


CASES = [
    # entry point, geometry, cnuda_last_error()
    ('forward_stats', GEMM, 'cnuda_conv2d_forward: workspace too small'),
    ('forward_stats', BIG, 'cnuda_conv2d_forward: kernel larger than padded input'),
    ('forward_rowquads', ONE, 'cnuda_conv2d_forward_rowquads: workspace too small'),
    ('forward_rowquads', BIG,
     'cnuda_conv2d_forward_rowquads: geometry without a quad-interleaved epilogue (cnuda_conv2d_rowquads_supported)'),
    ('forward_rowsig', SIG, 'cnuda_conv2d_forward_rowsig: workspace too small'),
    ('forward_rowsig', BIG27,
     'cnuda_conv2d_forward_rowsig: geometry without a row-sigmoid epilogue (cnuda_conv2d_rowsig_supported)'),
    ('backward_data_add', GEMM, 'cnuda_conv2d_backward_data: workspace too small'),
    ('backward_data_add', BIG, 'cnuda_conv2d_backward_data: kernel larger than padded input'),
    ('backward_weight', GEMM, 'cnuda_conv2d_backward_weight: workspace too small'),
    ('backward_weight', BIG, 'cnuda_conv2d_backward_weight: kernel larger than padded input'),
    ('cat_forward', CAT, 'cnuda_conv2d_cat_forward: workspace too small'),
    ('cat_forward', CAT_BAD, 'cnuda_conv2d_cat_forward: unsupported (cnuda_conv2d_cat_supported)'),
    ('cat_backward_data', CAT, 'cnuda_conv2d_cat_backward_data: workspace too small'),
    ('cat_backward_data', CAT_BAD, 'cnuda_conv2d_cat_backward_data: unsupported (cnuda_conv2d_cat_supported)'),
    ('cat_backward_weight', CAT, 'cnuda_conv2d_cat_backward_weight: workspace too small'),
    ('cat_backward_weight', CAT_BAD, 'cnuda_conv2d_cat_backward_weight: unsupported (cnuda_conv2d_cat_supported)'),
]


@pytest.mark.parametrize('name,geom,text', CASES, ids=['%s-%s' % (c[0], 'x'.join(map(str, c[1]))) for c in CASES])
def test_rejections_keep_their_code_and_text(name, geom, text):
    import hip_runtime as hr
    L = hr.lib()
    assert _call(L, name, geom) == -1
    assert L.cnuda_last_error().decode() == text

