"""`rotate_bbox` (utils/box.py:41-52): the four corners of a box [centre x, centre y, width, height, angle in
degrees] as integer pixel coordinates -- the polygon the COCO evaluator rasterises in rotated mode
(evaluation/coco.py).

`get_annotation_with_angle` of the reference's file is dataset-side code and not part of this build."""
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


def rotate_bbox(x, y, w, h, angle):
    """-> list of four integer [x, y] vertices of the rotated box"""
    dtype = np.result_type(*[np.asarray(v).dtype for v in (x, y, w, h, angle)])
    return list(rotate_bboxes(np.array([[x, y, w, h, angle]], dtype=dtype))[0])
