"""Restatements of the rotated-box IoU (csrc/polyiou.cuh; DESIGN.md, "Rotated IoU") in plain Python.

`quad_iou` follows the definition step by step on whatever number type `num` makes of a coordinate: `float` is the
float64 restatement the kernels must equal bit for bit (Python floats are IEEE doubles, every operator rounds once, no
fused multiply-add); `fractions.Fraction` is the same definition in exact rational arithmetic, the yardstick of the
restatement's own rounding error.  `soft_nms_image` is cnuda_soft_nms_merge_rotated on top of the float64 form."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
MAX_VERTICES = 8


def _doubled_area(p):
    """sum over ascending i of x_i y_{i+1} - x_{i+1} y_i, indices cyclic, one accumulator that starts at 0"""
    acc = type(p[0][0])(0)
    n = len(p)
    for i in range(n):
        (x0, y0), (x1, y1) = p[i], p[(i + 1) % n]
        acc = acc + (x0 * y1 - x1 * y0)
    return acc


def _oriented(q, num):
    p = [(num(float(x)), num(float(y))) for x, y in q]
    a2 = _doubled_area(p)
    if a2 < 0:
        p, a2 = p[::-1], -a2
    return p, a2


def _clip(pa, pb):
    """Sutherland-Hodgman: subject `pa` against the four edges of `pb`, both counter-clockwise"""
    poly = pa
    for k in range(4):
        (ax, ay), (bx, by) = pb[k], pb[(k + 1) % 4]
        ex, ey = bx - ax, by - ay
        d = [ex * (py - ay) - ey * (px - ax) for px, py in poly]
        out, m = [], len(poly)
        for j in range(m):
            (px, py), (qx, qy) = poly[j], poly[(j + 1) % m]
            dp, dq = d[j], d[(j + 1) % m]
            if dp >= 0:
                out.append((px, py))
            if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                t = dp / (dp - dq)
                out.append((px + t * (qx - px), py + t * (qy - py)))
        poly = out[:MAX_VERTICES]          # never reached by convex input; what is past it is dropped
        if not poly:
            break
    return poly


def prepared(q, num=float):
    """one quad, ready for `prepared_iou`: None when a coordinate is not finite, else (counter-clockwise vertices, a2)"""
    q = np.asarray(q, F).reshape(4, 2)
    return _oriented(q, num) if np.isfinite(q).all() else None


def prepared_iou(qa, qb, num=float):
    """steps 2 to 4 on two `prepared` quads -> (iou, area of a, area of b)"""
    zero = num(0)
    if qa is None or qb is None:
        return zero, zero, zero
    (pa, a2a), (pb, a2b) = qa, qb
    area_a, area_b = a2a / 2, a2b / 2
    if not (a2a > 0 and a2b > 0):
        return zero, area_a, area_b
    poly = _clip(pa, pb)
    i2 = _doubled_area(poly) if len(poly) >= 3 else zero
    if i2 < 0:
        i2 = zero
    if i2 > a2a:
        i2 = a2a
    if i2 > a2b:
        i2 = a2b
    u2 = a2a + a2b - i2
    return (i2 / u2 if u2 > 0 else zero), area_a, area_b


def quad_iou(A, B, num=float):
    """A, B: four (x, y) vertices each, float32 values, either winding -> (iou, area of A, area of B) in `num`.
    Subject A, clipper B.  A vertex that is not finite: (0, 0, 0)."""
    return prepared_iou(prepared(A, num), prepared(B, num), num)


def quad_area(q):
    """the area an entry reports for one quad on its own: steps 1 and 2, float64"""
    q = prepared(q)
    return 0.0 if q is None else q[1] / 2


def intersection_size(A, B):
    """vertices of the clipped polygon in the float64 restatement, for case counts"""
    pa, a2a = _oriented(np.asarray(A, F).reshape(4, 2), float)
    pb, a2b = _oriented(np.asarray(B, F).reshape(4, 2), float)
    return len(_clip(pa, pb)) if a2a > 0 and a2b > 0 else 0


def pairs(a, b):
    """a [N, 4, 2], b [M, 4, 2] float32 -> (iou [N, M], area_a [N], area_b [M]) float64, the restatement per pair"""
    a, b = np.asarray(a, F).reshape(-1, 4, 2), np.asarray(b, F).reshape(-1, 4, 2)
    pa, pb = [prepared(q) for q in a], [prepared(q) for q in b]
    iou = np.array([[prepared_iou(x, y)[0] for y in pb] for x in pa], dtype=np.float64).reshape(len(a), len(b))
    return iou, np.array([quad_area(q) for q in a], dtype=np.float64), np.array([quad_area(q) for q in b], dtype=np.float64)


def rotated_box(cx, cy, w, h, degrees):
    """float32 [4, 2]: the corners (-w, -h), (+w, -h), (+w, +h), (-w, +h) of the half extents, turned and rounded once"""
    r = math.radians(degrees)
    c, s = math.cos(r), math.sin(r)
    return F([[cx + (ox * c - oy * s), cy + (ox * s + oy * c)]
              for ox, oy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))])


def case_set(n=4000, seed=0, extent=4096.0):
    """Pairs of rotated rectangles with float32 vertices up to `extent` pixels: a quarter nearly parallel (0.01
    degrees apart), a quarter identical or turned by 90 degrees, a quarter sharing an edge, a quarter in general
    position; one pair in five has one quad's winding reversed.  -> (a [n, 4, 2], b [n, 4, 2]) float32"""
    rng = np.random.default_rng([977, seed])
    a, b = np.zeros((n, 4, 2), F), np.zeros((n, 4, 2), F)
    for i in range(n):
        w, h = rng.uniform(2, 400, 2)
        if i % 8 == 0:
            w = rng.uniform(2, 8)           # thin boxes
        cx, cy = rng.uniform(w + h, extent - (w + h), 2)
        ang = rng.uniform(-90, 90)
        kind = i % 4
        qa = rotated_box(cx, cy, w, h, ang)
        if kind == 0:                       # nearly parallel
            dx, dy = rng.uniform(-0.6, 0.6, 2) * (w, h)
            qb = rotated_box(cx + dx, cy + dy, w * rng.uniform(0.7, 1.3), h * rng.uniform(0.7, 1.3), ang + 0.01)
        elif kind == 1:                     # identical, or turned by 90 degrees about the same centre
            qb = qa.copy() if rng.random() < 0.5 else rotated_box(cx, cy, w, h, ang + 90)
            if rng.random() < 0.3:
                qb = np.roll(qb, int(rng.integers(1, 4)), axis=0)
        elif kind == 2:                     # shares the edge 1-2 of a, on one side or the other
            p1, p2 = qa[1].astype(np.float64), qa[2].astype(np.float64)
            r = math.radians(ang)
            ux, uy = math.cos(r), math.sin(r)
            depth = rng.uniform(2, 300) * (1 if rng.random() < 0.5 else -1)
            qb = F([p1, p1 + depth * np.array([ux, uy]), p2 + depth * np.array([ux, uy]), p2])
            qb[0], qb[3] = qa[1], qa[2]
        elif (i // 4) % 3 == 0:             # general position: near-squares about one centre (7 and 8 vertices)
            qa = rotated_box(cx, cy, h * rng.uniform(0.9, 1.1), h, ang)
            dx, dy = rng.uniform(-0.15, 0.15, 2) * h
            qb = rotated_box(cx + dx, cy + dy, h * rng.uniform(0.9, 1.1), h * rng.uniform(0.9, 1.1),
                             ang + rng.uniform(15, 75))
        elif (i // 4) % 3 == 1:             # general position: any two boxes near each other
            dx, dy = rng.uniform(-1.2, 1.2, 2) * max(w, h)
            qb = rotated_box(cx + dx, cy + dy, rng.uniform(2, 400), rng.uniform(2, 400), rng.uniform(-90, 90))
        else:                               # general position: b hangs on the corner 2 of a, by its own corner 0
            r = math.radians(ang)
            u, v = np.array([math.cos(r), math.sin(r)]), np.array([-math.sin(r), math.cos(r)])
            c2 = qa[2].astype(np.float64)
            su, sv = rng.uniform(2, 300, 2)
            qb = F([c2, c2 + su * u, c2 + su * u + sv * v, c2 + sv * v])
        if i % 5 == 0:
            if (i // 5) % 2:
                qa = qa[::-1]
            else:
                qb = qb[::-1]
        a[i], b[i] = qa, qb
    return a, b


# ---------------------------------------------------------------------------------------------------------------------
# the rotated soft-NMS merge (tests/predict_oracle.py's, on quads)
# ---------------------------------------------------------------------------------------------------------------------
def soft_nms_class(quads, scores, index):
    """One class: candidates `index` (ascending).  -> [(candidate index, emitted float64 score)] in emission order and
    the margins seen: 'gap' the smallest relative difference between two live scores of a round that differ ('ties'
    counts the pairs of live scores that are equal instead, which the candidate index decides), 'stop' the smallest
    relative distance of a round's largest score from 1e-3."""
    live = {int(i): float(scores[i]) for i in index}
    ready = {i: prepared(quads[i]) for i in live}
    emitted, margins = [], {'gap': np.inf, 'stop': np.inf, 'ties': 0}
    while live:
        order = sorted(live, key=lambda i: (-live[i], i))
        best = order[0]
        s = live[best]
        for u, v in zip(order, order[1:]):          # every neighbouring pair of the round's order: any two live scores
            if live[u] == live[v]:
                margins['ties'] += 1
            else:
                margins['gap'] = min(margins['gap'], abs(live[u] - live[v]) / max(abs(live[u]), 1e-300))
        margins['stop'] = min(margins['stop'], abs(s - 1e-3) / 1e-3)
        if not s >= 1e-3:
            break
        emitted.append((best, s))
        del live[best]
        for j in live:
            o = prepared_iou(ready[best], ready[j])[0]
            live[j] = live[j] * np.exp(-(o * o) / 0.5)
    return emitted, margins


def soft_nms_image(quads, scores, classes, num_classes, max_detections, threshold, kps=None):
    """One image's N candidates -> dict: 'index' (kept candidates in output order), 'scores' float64, 'classes',
    'boxes' float32 [n, 4, 2], 'kps', 'count' (kept rows whose float32 score >= threshold), 'kept' (emitted before the
    cut), 'margins' (soft_nms_class's, plus 'order': the smallest relative gap between neighbours of the final order)."""
    quads, scores, classes = np.asarray(quads, F).reshape(-1, 4, 2), np.asarray(scores, F), np.asarray(classes)
    rows, margins = [], {'gap': np.inf, 'stop': np.inf, 'ties': 0, 'order': np.inf}
    for c in range(num_classes):
        emitted, m = soft_nms_class(quads, scores, np.nonzero(classes == c)[0])
        rows += [(-s, c, i) for i, s in emitted]
        margins['gap'], margins['stop'] = min(margins['gap'], m['gap']), min(margins['stop'], m['stop'])
        margins['ties'] += m['ties']
    rows.sort()
    for a, b in zip(rows, rows[1:]):
        if a[0] != b[0]:
            margins['order'] = min(margins['order'], abs(a[0] - b[0]) / abs(a[0]))
    kept = rows[:max_detections]
    index = np.array([r[2] for r in kept], dtype=np.int64)
    s64 = np.array([-r[0] for r in kept], dtype=np.float64)
    out = {'index': index, 'scores': s64, 'classes': np.array([r[1] for r in kept], dtype=np.int32),
           'boxes': quads[index], 'count': int((s64.astype(F) >= F(threshold)).sum()), 'kept': len(rows),
           'margins': margins}
    if kps is not None:
        out['kps'] = np.asarray(kps, F)[index]
    return out
