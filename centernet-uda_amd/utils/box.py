"""`rotate_bbox` (utils/box.py:41-52): the four corners of a box [centre x, centre y, width, height, angle in
degrees] as integer pixel coordinates -- the polygon the COCO evaluator rasterises in rotated mode
(evaluation/coco.py).

`get_annotation_with_angle` (utils/box.py:4-38) is the dataset-side normalisation of a rotated annotation: w the
short side, h the long one, the angle in [-90, 90).  `datasets.encode_targets(corners=...)` applies the same rules on
the device; this is the host form for annotations read from a file."""
import numpy as np


def rotate_bboxes(boxes):
    """boxes [N, 5] (x, y, w, h, angle) -> int64 [N, 4, 2] corners (x, y), in the order (-w, -h), (+w, -h), (+w, +h),
    (-w, +h) of the half extents.  Every step runs in the dtype of `boxes` (float32 boxes: float32 cosine, sine,
    products and sums, as numpy does for the reference's float32 scalars); the corner is the centre plus the half
    extents times [[cos, sin], [-sin, cos]] (one numpy matmul per box, so the products round as numpy's matmul rounds
    them), truncated toward zero."""
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] != 5:
        raise ValueError("rotate_bboxes: expected [N, 5] boxes (x, y, w, h, angle), got %s" % (boxes.shape,))
    if not np.issubdtype(boxes.dtype, np.floating):
        boxes = boxes.astype(np.float64)
    x, y, w, h, angle = boxes.T
    rad = np.radians(angle)
    c, s = np.cos(rad), np.sin(rad)
    half_w, half_h = w / 2, h / 2
    corners = np.stack([np.stack([-half_w, half_w, half_w, -half_w], 1),
                        np.stack([-half_h, -half_h, half_h, half_h], 1)], 2)            # [N, 4, 2]
    rot = np.stack([np.stack([c, s], 1), np.stack([-s, c], 1)], 1)                       # [N, 2, 2]
    centre = np.stack([x, y], 1)[:, None, :]
    return (centre + np.matmul(corners, rot)).astype(int)


def rotate_bboxes_float(boxes):
    """boxes [N, 5] (x, y, w, h, angle) -> float32 [N, 4, 2] corners in `rotate_bboxes`' order, not truncated: the
    given values widened to float64, cosine, sine, products and sums in float64 (x' = x + (ox cos - oy sin),
    y' = y + (ox sin + oy cos) for the half extents (ox, oy)), rounded once to float32 -- the polygon the COCO evaluator
    measures with `rotated_iou = 'polygon'`."""
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] != 5:
        raise ValueError("rotate_bboxes_float: expected [N, 5] boxes (x, y, w, h, angle), got %s" % (boxes.shape,))
    x, y, w, h, angle = boxes.astype(np.float64).T
    rad = np.radians(angle)
    c, s = np.cos(rad), np.sin(rad)
    ox = np.stack([-w / 2, w / 2, w / 2, -w / 2], 1)
    oy = np.stack([-h / 2, -h / 2, h / 2, h / 2], 1)
    c, s = c[:, None], s[:, None]
    return np.stack([x[:, None] + (ox * c - oy * s), y[:, None] + (ox * s + oy * c)], 2).astype(np.float32)


def rotate_bbox(x, y, w, h, angle):
    """-> list of four integer [x, y] vertices of the rotated box"""
    dtype = np.result_type(*[np.asarray(v).dtype for v in (x, y, w, h, angle)])
    return list(rotate_bboxes(np.array([[x, y, w, h, angle]], dtype=dtype))[0])


def get_annotation_with_angle(ann):
    """ann['rbbox'] = (cx, cy, w, h, angle in degrees) -> float32 [5] with w < h and -90 <= angle < 90, by the
    reference's arithmetic on float32 values: w > h swaps the sides and turns the angle by 90 degrees towards zero
    (a positive angle loses 90, any other gains 90); w == h makes h += 1; an angle of exactly 90 becomes -90; the
    angle is then clipped to [-90, 90 - eps] with the float64 eps the reference's `np.float` meant.
    Only annotations that carry `rbbox` are accepted: the reference's branch for plain `bbox` annotations calls
    `.append` on an ndarray and cannot run, so there is nothing to restate -- ValueError."""
    if 'rbbox' not in ann:
        raise ValueError("get_annotation_with_angle: the annotation has no 'rbbox' (cx, cy, w, h, angle)")
    box = np.array(ann['rbbox'], dtype=np.float32)
    if box.shape != (5,):
        raise ValueError("get_annotation_with_angle: 'rbbox' must be (cx, cy, w, h, angle), got shape %s" % (box.shape,))
    if box[2] > box[3]:
        box[2:4] = box[3], box[2]
        box[4] += np.float32(-90 if box[4] > 0 else 90)
    if box[2] == box[3]:
        box[3] += 1
    if box[4] == 90:
        box[4] = -90
    box[4] = np.clip(box[4], -90, 90 - np.finfo(np.float64).eps)
    if not (box[2] < box[3] and -90 <= box[4] < 90):
        raise ValueError("get_annotation_with_angle: %s does not normalise to w < h, -90 <= angle < 90" % (box,))
    return box
