"""numpy restatement of the mean teacher's device steps (csrc/teacher.hip), written from the definitions of DESIGN.md,
"Mean teacher": the EMA arithmetic, the decay schedule and the pseudo-label filter.  Shares no code with the library."""
import numpy as np


def decay_t(decay, n):
    """The decay of EMA update number n (0-based)."""
    return min(float(decay), (1.0 + n) / (10.0 + n))


def ema(t, s, decay):
    """float32: (t * d) + (s * omd), omd = float32(1) - float32(d); two rounded products, one rounded sum."""
    t, s = np.asarray(t, dtype=np.float32), np.asarray(s, dtype=np.float32)
    d = np.float32(decay)
    omd = np.float32(1) - d
    return (t * d + s * omd).astype(np.float32)


def rotated_corners(cx, cy, w, h, angle):
    """float32 scalars -> [4, 2] float64: utils.box.rotate_bboxes' vertex order and rotation, in double."""
    cx, cy, w, h = (np.float64(np.float32(v)) for v in (cx, cy, w, h))
    rad = np.float64(np.float32(angle)) * (np.pi / 180.0)
    c, s = np.cos(rad), np.sin(rad)
    hw, hh = w / 2.0, h / 2.0
    out = np.zeros((4, 2), np.float64)
    for v, (ox, oy) in enumerate(((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh))):
        out[v, 0] = cx + (ox * c + oy * (-s))
        out[v, 1] = cy + (ox * s + oy * c)
    return out


def pseudo_labels(dets, thresholds, map_width, rotated=False, mirror=False, min_size=0.0):
    """dets [B, K, 6 | 7] float32, thresholds [C] float32 -> {'classes' [B, K] int32, 'counts' [B] int32, 'kept' float32,
    'boxes' [B, K, 4] float64 | 'corners' [B, K, 4, 2] float64}."""
    dets = np.asarray(dets, dtype=np.float32)
    thresholds = np.asarray(thresholds, dtype=np.float32)
    B, K, ncol = dets.shape
    assert ncol == (7 if rotated else 6)
    C = thresholds.shape[0]
    W, smin = np.float64(int(map_width)), np.float64(np.float32(min_size))
    classes = np.zeros((B, K), np.int32)
    counts = np.zeros(B, np.int32)
    geom = np.zeros((B, K, 4, 2) if rotated else (B, K, 4), np.float64)
    for b in range(B):
        n = 0
        for k in range(K):
            row = dets[b, k]
            cf, score = row[ncol - 1], row[ncol - 2]
            if not (np.isfinite(cf) and cf == np.floor(cf) and 0 <= cf < C):
                continue
            cls = int(cf)
            if not score >= thresholds[cls]:
                continue
            ngeo = 5 if rotated else 4
            if not np.all(np.isfinite(row[:ngeo])):
                continue
            g = row[:4].astype(np.float64)
            if rotated:
                if not (g[2] >= smin and g[3] >= smin):
                    continue
                out = rotated_corners(row[0], row[1], row[2], row[3], row[4])
                if mirror:
                    out[:, 0] = W - out[:, 0]
            else:
                if not (g[2] - g[0] >= smin and g[3] - g[1] >= smin):
                    continue
                out = np.array([W - g[2], g[1], W - g[0], g[3]]) if mirror else g
            classes[b, n] = cls
            geom[b, n] = out
            n += 1
        counts[b] = n
    return {'classes': classes, 'counts': counts, 'kept': np.float32(np.float64(counts.sum()) / np.float64(B)),
            'corners' if rotated else 'boxes': geom}
