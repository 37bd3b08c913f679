"""numpy oracle of the keypoint and rotated modes of the dataset's target loop (test helper, not collected).

Restates datasets/coco.py:176-184,191-233 (axis-aligned boxes with keypoints and "area") and 303-376 (rotated boxes)
one image at a time, on top of the frozen oracle/targets.py (gaussian_radius, draw_gaussian).  Nothing of the
reference's Dataset can be run here (it needs imgaug, cv2 and pycocotools), so no golden file comes from it;
tests/test_host_targets_modes.py pins this file by closed-form answers instead.

cv2.minAreaRect is replaced by its geometric definition: the convex hull of the distinct points (monotone chain),
and, exhaustively over the hull's edges, the enclosing rectangle with a side along that edge; the least area wins.
All of it in float64 from the float32 points.  The normalisation is the project's utils.box.get_annotation_with_angle
(the reference's `rbbox` branch on float32 values), fed the direction of the chosen edge folded into [-90, 90); its
result is the direction of the short side (y down, the convention of utils.box.rotate_bboxes) in [-90, 90).  Both
OpenCV angle conventions reduce to that after the reference's swap.
"""
import numpy as np

from oracle import targets as ot
from utils.box import get_annotation_with_angle


def clip_points(corners, output_h, output_w):
    """[4, 2] float64 -> float32 points clipped to the map (coco.py:331-337)."""
    p = np.array(corners, dtype=np.float64).reshape(4, 2)
    p[:, 0] = np.clip(p[:, 0], 0, output_w - 1)
    p[:, 1] = np.clip(p[:, 1], 0, output_h - 1)
    return p.astype(np.float32)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Andrew's monotone chain over the distinct points, float64; collinear points are dropped."""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def enclosing_rect(points):
    """float32 [4, 2] -> None (fewer than three hull vertices) or (centre [2], extent along the hull edge, extent
    across it, edge direction [2] (unit)), all float64: the least-area rectangle over the hull's edges."""
    hull = convex_hull(points)
    if len(hull) < 3:
        return None
    P = np.array(hull, dtype=np.float64)
    best = None
    for i in range(len(hull)):
        d = P[(i + 1) % len(hull)] - P[i]
        u = d / np.hypot(d[0], d[1])
        v = np.array([-u[1], u[0]])
        a, c = P @ u, P @ v
        lu, lv = a.max() - a.min(), c.max() - c.min()
        if best is None or lu * lv < best[0]:
            centre = u * (a.max() + a.min()) / 2 + v * (c.max() + c.min()) / 2
            best = (lu * lv, centre, lu, lv, u)
    return best[1:]


def rotated_annotation(points):
    """float32 [4, 2] -> None (the reference's `continue`) or float32 (cx, cy, w, h, angle): the rectangle as
    (centre, extent along the edge, extent across it, direction of the edge folded into [-90, 90)) in float32, handed
    to utils.box.get_annotation_with_angle like the reference hands it cv2's result (coco.py:338-344).  A direction
    and the one 180 degrees from it are the same line, so the fold loses nothing; the helper's swap then turns the
    angle onto the short side."""
    rect = enclosing_rect(points)
    if rect is None:
        return None
    centre, lu, lv, u = rect
    if np.float32(lu) == 0 or np.float32(lv) == 0:
        return None
    deg = np.degrees(np.arctan2(u[1], u[0]))
    if deg >= 90:
        deg -= 180
    if deg < -90:
        deg += 180
    return get_annotation_with_angle({'rbbox': np.array([centre[0], centre[1], lu, lv, deg])})


def keypoint_rows(kpts, vis, ct_int, output_w):
    """one object's (kps [2J], gt_kps [J, 2], kp_reg_mask [2J]) (coco.py:217-228)."""
    J = len(kpts)
    kp, gt, mask = np.zeros(2 * J, np.float32), np.zeros((J, 2), np.float32), np.zeros(2 * J, np.uint8)
    for i in range(J):
        x, y = float(kpts[i][0]), float(kpts[i][1])
        kp[2 * i], kp[2 * i + 1] = x - int(ct_int[0]), y - int(ct_int[1])
        # is_out_of_image((output_w, output_w)): the "height" the reference passes is the width
        inside = 0 <= x < output_w and 0 <= y < output_w
        mask[2 * i] = mask[2 * i + 1] = int(vis[i] == 2 and inside)
        gt[i] = x, y
    return kp, gt, mask


def encode_targets_modes(classes, num_classes, output_h, output_w, max_detections, boxes=None, corners=None,
                         keypoints=None, visibility=None, areas=None):
    """One image.  boxes [n, 4] or corners [n, 4, 2] float64 (exactly one), classes [n]; keypoints [n, J, 2],
    visibility [n, J], areas [n] (NaN = no "area") optional -> dict with the schema of coco.py:242-259 / 384-401.
    Also returns, under '_radius_args', the (h, w) the radius was computed from (for the tests' tie checks)."""
    assert (boxes is None) != (corners is None)
    rot = corners is not None
    geom = corners if rot else boxes
    M = max_detections
    hm = np.zeros((num_classes, output_h, output_w), np.float32)
    wh = np.zeros((M, 3 if rot else 2), np.float32)
    reg = np.zeros((M, 2), np.float32)
    ind = np.zeros(M, np.int64)
    reg_mask = np.zeros(M, np.uint8)
    gt_det = np.zeros((M, 7 if rot else 6), np.float32)
    gt_areas = np.zeros(M, np.float32)
    J = 0 if keypoints is None else np.asarray(keypoints).shape[1]
    kp, gt_kp, kp_mask = np.zeros((M, 2 * J), np.float32), np.zeros((M, J, 2), np.float32), np.zeros((M, 2 * J), np.uint8)
    radius_args = {}
    for k in range(min(len(geom), M)):
        cls_id = int(classes[k])
        if rot:
            ann = rotated_annotation(clip_points(geom[k], output_h, output_w))
            if ann is None:
                continue
            cx, cy, w, h, angle = ann                       # float32 scalars
            ct = np.array((cx, cy))
            rh, rw = np.ceil(np.float64(h)), np.ceil(np.float64(w))
            area = w * h                                    # float32 product
        else:
            bbox = np.array(geom[k], dtype=np.float64)
            bbox[[0, 2]] = np.clip(bbox[[0, 2]], 0, output_w - 1)
            bbox[[1, 3]] = np.clip(bbox[[1, 3]], 0, output_h - 1)
            h, w = bbox[3] - bbox[1], bbox[2] - bbox[0]
            if not (h > 0 and w > 0):
                continue
            ct = np.array([(bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2], dtype=np.float32)
            rh, rw = np.ceil(h), np.ceil(w)
            area = w * h
        radius_args[k] = (float(h), float(w))
        radius = max(0, int(ot.gaussian_radius((rh, rw))))
        ct_int = ct.astype(np.int32)
        ot.draw_gaussian(hm[cls_id], ct_int, radius)
        ind[k] = ct_int[1] * output_w + ct_int[0]
        reg[k] = ct - ct_int
        reg_mask[k] = 1
        if rot:
            wh[k] = w, h, angle
            gt_det[k] = (ct[0], ct[1], w, h, angle, 1, cls_id)
        else:
            wh[k] = w, h
            gt_det[k] = (ct[0] - w / 2, ct[1] - h / 2, ct[0] + w / 2, ct[1] + h / 2, 1, cls_id)
        if J:
            kp[k], gt_kp[k], kp_mask[k] = keypoint_rows(keypoints[k], visibility[k], ct_int, output_w)
        gt_areas[k] = area if areas is None or np.isnan(areas[k]) else areas[k]
    out = dict(hm=hm, reg_mask=reg_mask, ind=ind, wh=wh, reg=reg, gt_dets=gt_det, gt_areas=gt_areas,
               _radius_args=radius_args)
    if J:
        out.update(kps=kp, gt_kps=gt_kp, kp_reg_mask=kp_mask)
    return out
