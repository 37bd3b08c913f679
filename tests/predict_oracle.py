"""numpy restatements of the three prediction kernels (csrc/predict.hip), written from the formulas of DESIGN.md,
"Prediction": the mirror merge in float32, the projection and the soft-NMS merge in float64."""
import numpy as np

F = np.float32


def mirror(a):
    return np.ascontiguousarray(np.asarray(a)[..., ::-1])


def tta_merge(prob, wh, reg=None, kps=None, perm=None):
    """prob [2B,C,H,W]: the CLAMPED SIGMOID of the heat-map logits (images, then their mirrors); wh, reg, kps raw.
    -> dict of float32 arrays of B images; every value is one float32 rounding of exact operands."""
    prob, wh = np.asarray(prob, F), np.asarray(wh, F)
    B = prob.shape[0] // 2
    out = {'hm': F(0.5) * (prob[:B] + mirror(prob[B:]))}
    m = wh[:B].copy()
    m[:, :2] = F(0.5) * (wh[:B, :2] + mirror(wh[B:, :2]))
    out['wh'] = m
    if reg is not None:
        out['reg'] = np.asarray(reg, F)[:B].copy()
    if kps is not None:
        kps = np.asarray(kps, F)
        J = kps.shape[1] // 2
        perm = np.arange(J) if perm is None else np.asarray(perm)
        k = np.empty_like(kps[:B])
        for j in range(J):
            k[:, 2 * j] = F(0.5) * (kps[:B, 2 * j] - mirror(kps[B:, 2 * perm[j]]))
            k[:, 2 * j + 1] = F(0.5) * (kps[:B, 2 * j + 1] + mirror(kps[B:, 2 * perm[j] + 1]))
        out['kps'] = k
    return out


def _apply(m, x, y):
    return (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]


def project(dets, kps, matrix, sizes, threshold, rotated=False, scale=1.0):
    """dets [B,K,6|7] float32, kps [B,K,J,2] or None, matrix [B,6] float64, sizes [B,2] (h, w).  The geometry is
    multiplied by `scale` in float32 first, everything after that is float64.  -> dict: boxes ([B,K,4] or [B,K,4,2]),
    kps: float64 (round with .astype(float32) to compare); scores float32, classes int32, counts."""
    dets = np.asarray(dets, F)
    B, K, ncol = dets.shape
    geo = (dets[:, :, :4] * F(scale)).astype(np.float64)
    boxes = np.zeros((B, K, 4, 2) if rotated else (B, K, 4))
    for b in range(B):
        m = np.asarray(matrix[b], np.float64)
        h, w = float(sizes[b][0]), float(sizes[b][1])
        for k in range(K):
            g = geo[b, k]
            if rotated:
                rad = float(dets[b, k, 4]) * (np.pi / 180.0)
                c, s = np.cos(rad), np.sin(rad)
                hw, hh = g[2] / 2.0, g[3] / 2.0
                for v, (ox, oy) in enumerate(((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh))):
                    boxes[b, k, v] = _apply(m, g[0] + (ox * c + oy * (-s)), g[1] + (ox * s + oy * c))
            else:
                pts = [_apply(m, x, y) for x, y in ((g[0], g[1]), (g[2], g[1]), (g[2], g[3]), (g[0], g[3]))]
                xs, ys = [p[0] for p in pts], [p[1] for p in pts]
                boxes[b, k] = (min(max(min(xs), 0.0), w), min(max(min(ys), 0.0), h),
                               min(max(max(xs), 0.0), w), min(max(max(ys), 0.0), h))
    scores = dets[:, :, ncol - 2].copy()
    out = {'boxes': boxes, 'scores': scores, 'classes': dets[:, :, ncol - 1].astype(np.int32),
           'counts': (scores >= F(threshold)).sum(1).astype(np.int32)}
    if kps is not None:
        k64 = (np.asarray(kps, F) * F(scale)).astype(np.float64)
        mapped = np.empty_like(k64)
        for b in range(B):
            mapped[b, ..., 0], mapped[b, ..., 1] = _apply(np.asarray(matrix[b], np.float64), k64[b, ..., 0], k64[b, ..., 1])
        out['kps'] = mapped
    return out


def iou(a, b):
    """float64 boxes (x1, y1, x2, y2); area has no '+ 1'."""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if not (iw > 0.0 and ih > 0.0):
        return 0.0
    inter = iw * ih
    ua = ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
    return inter / ua if ua > 0.0 else 0.0


def soft_nms_class(boxes, scores, index):
    """One class: candidates `index` (ascending).  -> [(candidate index, emitted float64 score)] in emission order, and
    the margins seen: 'gap' the smallest relative difference between the two largest live scores of a round (exact ties
    are counted apart, in 'ties'), 'stop' the smallest relative distance of a round's largest score from 1e-3."""
    live = {int(i): float(scores[i]) for i in index}
    emitted, margins = [], {'gap': np.inf, 'stop': np.inf, 'ties': 0}
    while live:
        order = sorted(live, key=lambda i: (-live[i], i))
        best = order[0]
        s = live[best]
        if len(order) > 1:
            t = live[order[1]]
            if t == s:
                margins['ties'] += 1
            else:
                margins['gap'] = min(margins['gap'], abs(s - t) / max(abs(s), 1e-300))
        margins['stop'] = min(margins['stop'], abs(s - 1e-3) / 1e-3)
        if not s >= 1e-3:
            break
        emitted.append((best, s))
        del live[best]
        bi = [float(v) for v in boxes[best]]
        for j in live:
            o = iou(bi, [float(v) for v in boxes[j]])
            live[j] = live[j] * np.exp(-(o * o) / 0.5)
    return emitted, margins


def soft_nms_image(boxes, scores, classes, num_classes, max_detections, threshold, kps=None):
    """One image's N candidates -> dict: 'index' (kept candidates in output order), 'scores' float64, 'classes',
    'boxes' float32, 'kps', 'count' (kept rows whose float32 score >= threshold), 'kept' (emitted before the cut),
    'margins' (soft_nms_class's, plus 'order': the smallest relative gap between neighbours of the final order)."""
    boxes, scores, classes = np.asarray(boxes, F).reshape(-1, 4), np.asarray(scores, F), np.asarray(classes)
    rows, margins = [], {'gap': np.inf, 'stop': np.inf, 'ties': 0, 'order': np.inf}
    for c in range(num_classes):
        emitted, m = soft_nms_class(boxes, scores, np.nonzero(classes == c)[0])
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
           'boxes': boxes[index], 'count': int((s64.astype(F) >= F(threshold)).sum()), 'kept': len(rows),
           'margins': margins}
    if kps is not None:
        out['kps'] = np.asarray(kps, F)[index]
    return out
