"""numpy float64 restatement of the two keypoint stages of uda.KeypointTeacher (include/centernet_uda_hip.h:
cnuda_pseudo_labels_kps in csrc/teacher.hip, cnuda_labels_transform_kps in csrc/geomview.hip), written from the header's
definitions.  The boxes, classes and counts are those of tests/teacher_oracle.py and tests/geometric_view_oracle.py; this
file adds which input row fills which slot, and what becomes of the row's joints.  Shares no code with the library."""
import math

import numpy as np

import geometric_view_oracle as go
import teacher_oracle as to

F = np.float32
D = np.float64


def surviving_rows(dets, thresholds, rotated=False, min_size=0.0):
    """-> per image the input rows that pass the score filter, in input order (the rule of cnuda_pseudo_labels)."""
    dets = np.asarray(dets, dtype=F)
    thresholds = np.asarray(thresholds, dtype=F)
    B, K, ncol = dets.shape
    smin = D(F(min_size))
    rows = []
    for b in range(B):
        rows.append([])
        for k in range(K):
            r = dets[b, k]
            cf, score = r[ncol - 1], r[ncol - 2]
            if not (np.isfinite(cf) and cf == np.floor(cf) and 0 <= cf < len(thresholds)):
                continue
            if not score >= thresholds[int(cf)] or not np.isfinite(r[:5 if rotated else 4]).all():
                continue
            g = r[:4].astype(D)
            extent = (g[2], g[3]) if rotated else (g[2] - g[0], g[3] - g[1])
            if extent[0] >= smin and extent[1] >= smin:
                rows[b].append(k)
    return rows


def pseudo_labels_kps(dets, kps, thresholds, map_width, map_height, rotated=False, mirror=False, min_size=0.0, perm=None):
    """dets [B, K, 6 | 7] float32, kps [B, K, J, 2] float32, perm [J] or None -> teacher_oracle.pseudo_labels' dict plus
    'keypoints' [B, K, J, 2] float64, 'visibility' [B, K, J] int32 and 'joints' float32."""
    out = to.pseudo_labels(dets, thresholds, map_width, rotated=rotated, mirror=mirror, min_size=min_size)
    kps = np.asarray(kps)
    assert kps.dtype == F and kps.ndim == 4 and kps.shape[3] == 2
    B, K, J = kps.shape[:3]
    rows = surviving_rows(dets, thresholds, rotated, min_size)
    assert [len(r) for r in rows] == out['counts'].tolist()
    W, H = D(int(map_width)), D(int(map_height))
    keypoints = np.zeros((B, K, J, 2), D)
    visibility = np.zeros((B, K, J), np.int32)
    for b in range(B):
        for slot, k in enumerate(rows[b]):
            for j in range(J):
                x, y = kps[b, k, j if perm is None else int(perm[j])]
                if not (np.isfinite(x) and np.isfinite(y)):
                    continue                                       # (0, 0), v = 0
                xd, yd = (W - D(x) if mirror else D(x)), D(y)
                keypoints[b, slot, j] = (xd, yd)
                visibility[b, slot, j] = 2 if (0 <= xd < W and 0 <= yd < H) else 0
    out.update(keypoints=keypoints, visibility=visibility,
               joints=F(D(int((visibility == 2).sum())) / D(B)))
    return out


def kept_rows(labels, forward_map, map_h, map_w, rotated=False, min_size=0.0, min_visible=0.5):
    """-> per image the rows below its count that survive the view, in input order (the rule of cnuda_labels_transform,
    decided by geometric_view_oracle.row)."""
    flat = np.asarray(labels['corners' if rotated else 'boxes'], dtype=D)
    B, K = flat.shape[:2]
    flat = flat.reshape(B, K, -1)
    m = go._six(forward_map)
    rows = []
    for b in range(B):
        n = min(max(int(labels['counts'][b]), 0), K)
        if (m[b] == D([1, 0, 0, 0, 1, 0])).all():
            rows.append(list(range(n)))
            continue
        rows.append([])
        for k in range(n):
            _, extent, area, visible = go.row(m[b], flat[b, k], rotated, map_h, map_w)
            if (extent[0] >= min_size and extent[1] >= min_size and area > 0.0 and math.isfinite(area)
                    and visible >= min_visible):
                rows[b].append(k)
    return rows


def transform_labels_kps(labels, forward_map, map_h, map_w, rotated=False, min_size=0.0, min_visible=0.5):
    """The dict of pseudo_labels_kps under the view -> (geometric_view_oracle.transform_labels' dict plus 'keypoints',
    'visibility' and 'joints', its list of judged rows)."""
    out, judged = go.transform_labels(labels, forward_map, map_h, map_w, rotated=rotated, min_size=min_size,
                                      min_visible=min_visible)
    kin, vin = np.asarray(labels['keypoints'], dtype=D), np.asarray(labels['visibility'])
    B, K, J = vin.shape
    rows = kept_rows(labels, forward_map, map_h, map_w, rotated, min_size, min_visible)
    assert [len(r) for r in rows] == out['counts'].tolist()
    m = go._six(forward_map)
    keypoints = np.zeros((B, K, J, 2), D)
    visibility = np.zeros((B, K, J), np.int32)
    for b in range(B):
        m0, m1, m2, m3, m4, m5 = (float(v) for v in m[b])
        identity = (m[b] == D([1, 0, 0, 0, 1, 0])).all()
        for slot, k in enumerate(rows[b]):
            for j in range(J):
                x, y, v = float(kin[b, k, j, 0]), float(kin[b, k, j, 1]), int(vin[b, k, j])
                if not identity:
                    qx, qy = (m0 * x + m1 * y) + m2, (m3 * x + m4 * y) + m5
                    finite = math.isfinite(qx) and math.isfinite(qy)
                    v = 2 if (v == 2 and finite and 0.0 <= qx < map_w and 0.0 <= qy < map_h) else 0
                    x, y = (qx, qy) if finite else (0.0, 0.0)
                keypoints[b, slot, j] = (x, y)
                visibility[b, slot, j] = v
    out.update(keypoints=keypoints, visibility=visibility,
               joints=F(D(int((visibility == 2).sum())) / D(B)))
    return out, judged
