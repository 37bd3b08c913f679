"""No-GPU checks of the sparse head backward's C ABI (cnuda_head_backward_sparse*): declared, bound, exported; the
geometry query and the workspace query answer without a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['cnuda_head_backward_sparse', 'cnuda_head_backward_sparse_supported',
               'cnuda_head_backward_sparse_workspace_bytes']


def test_new_symbols_in_header_signature_table_and_library():
    import hip_runtime as hr
    text = open(os.path.join(ROOT, 'include', 'centernet_uda_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    notes = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    L = hr.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(hr._Sig, name) and hasattr(L, name), name
    assert 'cnuda_head_backward_sparse' in notes
    # null pointers and bad geometry are rejected before anything touches the device
    geom = (16, 150, 64, 128, 128, 256, 2, 3, 3)
    assert L.cnuda_head_backward_sparse(*[None] * 12, *geom, 0.0, None, 0, None) == -1
    assert b'null' in L.cnuda_last_error()


def test_supported_and_workspace_queries_answer_without_a_gpu():
    import hip_runtime as hr
    L = hr.lib()
    ok = L.cnuda_head_backward_sparse_supported
    #          B   M    C   H    W    Ch   Co kh kw sh sw ph pw
    assert ok(16, 150, 64, 128, 128, 256, 2, 3, 3, 1, 1, 1, 1) == 1          # the wh / reg heads of the benched step
    assert ok(16, 150, 64, 160, 160, 256, 3, 3, 3, 1, 1, 1, 1) == 1          # the rotated wh head
    assert ok(1, 8, 16, 12, 12, 48, 8, 1, 1, 1, 1, 0, 0) == 1                # a 1x1 first layer
    assert ok(2, 8, 16, 12, 12, 48, 2, 5, 5, 1, 1, 2, 2) == 1
    assert ok(2, 8, 16, 12, 12, 48, 9, 3, 3, 1, 1, 1, 1) == 0                # more than 8 outputs: no fused node either
    assert ok(2, 8, 16, 12, 12, 48, 2, 3, 3, 2, 2, 1, 1) == 0                # strided
    assert ok(2, 8, 16, 12, 12, 48, 2, 3, 3, 1, 1, 0, 0) == 0                # not "same" padding
    assert ok(2, 8, 16, 12, 12, 48, 2, 2, 2, 1, 1, 0, 0) == 0                # even kernel
    assert ok(2, 8, 16, 12, 12, 48, 2, 3, 5, 1, 1, 1, 2) == 0                # not square
    assert ok(2, 4097, 16, 128, 128, 48, 2, 3, 3, 1, 1, 1, 1) == 0           # more rows per image than the duplicate scan takes
    ws = L.cnuda_head_backward_sparse_workspace_bytes
    B, M, C, Ch, Co, T = 16, 150, 64, 256, 2, 9
    rows = B * M
    compact = 4 * rows * (Co + 2 * Ch + 2 * T * C)          # gyrow, hrow, gh, xp, t
    assert compact <= ws(B, M, C, 128, 128, Ch, Co, 3, 3) <= 4 * compact
    assert ws(B, 2 * M, C, 128, 128, Ch, Co, 3, 3) > ws(B, M, C, 128, 128, Ch, Co, 3, 3)
    assert ws(B, M, C, 128, 128, Ch, 9, 3, 3) == 0 and b'unsupported' in L.cnuda_last_error()
