"""CenterNet targets for a whole batch on the GPU.

`encode_targets(boxes, classes, counts, num_classes, output_h, output_w)` replaces the per-image numpy loop of
the reference's `__getitem__` (datasets/coco.py:168-174,191-221: gaussian splat into `hm`, `ind`, `wh`, `reg`,
`reg_mask`, `gt_dets`, `gt_areas`) with one kernel launch over all images, so that the batch the train step
consumes is produced where it is used.  Inputs are the augmented boxes at output resolution (what the loop
starts from): `boxes` [B, M, 4] (x1, y1, x2, y2; float64 like the reference's box arithmetic), `classes` [B, M]
int32 (already mapped through `cat_mapping`), `counts` [B] int32.  Returns the dict with the dataset's keys
and dtypes (`reg_mask` uint8, `ind` int64).

Keyword arguments select the loop's other modes (all coordinates at output-map resolution: after `resize_out`,
before the loop's `np.clip`).  Every call, with or without them, is one `cnuda_encode_targets_modes`:

`corners` [B, M, 4, 2] float64, with `boxes=None`: rotated boxes (coco.py:303-312,329-358).  The four points are
    clipped to the map and rounded to float32; the object is their minimum-area enclosing rectangle -- the
    least-area rectangle with a side along an edge of the points' convex hull, which is what the reference asks of
    `cv2.minAreaRect`, computed in double -- normalised as `utils.box.get_annotation_with_angle` does on float32
    values: w the short side, h the long one, `angle` the direction of the short side in degrees in the y-down
    convention of `utils.box.rotate_bboxes`, folded into [-90, 90).  The reference's quirks stay: w == h makes
    h += 1, and 90 becomes -90.  Points with fewer than three hull vertices, or a rectangle with a zero extent,
    are skipped like the reference's `continue`: the slot's rows stay zero.  `wh` becomes [B, M, 3] (w, h, angle)
    and `gt_dets` [B, M, 7] (cx, cy, w, h, angle, 1, class).
`keypoints` [B, M, J, 2] float64 with `visibility` [B, M, J] int32 (COCO's v): adds `kps` [B, M, 2J] float32
    (offsets from the integer centre), `gt_kps` [B, M, J, 2] float32 and `kp_reg_mask` [B, M, 2J] uint8
    (coco.py:176-184,217-228), written for slots whose box is valid.  A keypoint counts when v == 2 and
    0 <= x < output_w and 0 <= y < output_w: the reference tests y against the WIDTH
    (`is_out_of_image((output_w, output_w))`), and so does this.
`areas` [B, M] float32: the annotation's `area` for `gt_areas`; NaN means absent and falls back to w*h, as does
    leaving the argument out (coco.py:230-233).
"""
import torch

from hip_runtime import check, lib, ptr, require_gpu, stream


def _alloc(B, M, num_classes, output_h, output_w, ncol, dev):
    return {
        'hm': torch.empty((B, num_classes, output_h, output_w), dtype=torch.float32, device=dev),
        'reg_mask': torch.empty((B, M), dtype=torch.uint8, device=dev),
        'ind': torch.empty((B, M), dtype=torch.int64, device=dev),
        'wh': torch.empty((B, M, ncol), dtype=torch.float32, device=dev),
        'reg': torch.empty((B, M, 2), dtype=torch.float32, device=dev),
        'gt_dets': torch.empty((B, M, ncol + 4), dtype=torch.float32, device=dev),
        'gt_areas': torch.empty((B, M), dtype=torch.float32, device=dev),
    }


def encode_targets(boxes, classes, counts, num_classes, output_h, output_w, *,
                   corners=None, keypoints=None, visibility=None, areas=None):
    require_gpu(boxes, classes, counts, corners, keypoints, visibility, areas)
    if (boxes is None) == (corners is None):
        raise RuntimeError("encode_targets: boxes or corners must be given" if boxes is None else
                           "encode_targets: give either boxes or corners (with boxes=None), not both")
    rotated = corners is not None
    geom = corners if rotated else boxes
    tail = (4, 2) if rotated else (4,)
    if geom.dim() != 2 + len(tail) or tuple(geom.shape[2:]) != tail:
        raise RuntimeError("encode_targets: %s must be [B, M, %s], got %s"
                           % ("corners" if rotated else "boxes", ", ".join(map(str, tail)), tuple(geom.shape)))
    B, M = geom.shape[0], geom.shape[1]
    if tuple(classes.shape) != (B, M) or tuple(counts.shape) != (B,):
        raise RuntimeError("encode_targets: classes %s / counts %s do not match %s %s"
                           % (tuple(classes.shape), tuple(counts.shape), "corners" if rotated else "boxes",
                              tuple(geom.shape)))
    if (keypoints is None) != (visibility is None):
        raise RuntimeError("encode_targets: keypoints and visibility must be given together")
    J = 0
    if keypoints is not None:
        if keypoints.dim() != 4 or tuple(keypoints.shape[:2]) != (B, M) or keypoints.shape[3] != 2 \
                or keypoints.shape[2] < 1:
            raise RuntimeError("encode_targets: keypoints must be [%d, %d, J, 2], got %s"
                               % (B, M, tuple(keypoints.shape)))
        J = keypoints.shape[2]
        if tuple(visibility.shape) != (B, M, J):
            raise RuntimeError("encode_targets: visibility %s does not match keypoints %s"
                               % (tuple(visibility.shape), tuple(keypoints.shape)))
        keypoints = keypoints.to(torch.float64).contiguous()
        visibility = visibility.to(torch.int32).contiguous()
    if areas is not None:
        if tuple(areas.shape) != (B, M):
            raise RuntimeError("encode_targets: areas must be [%d, %d], got %s" % (B, M, tuple(areas.shape)))
        areas = areas.to(torch.float32).contiguous()
    geom = geom.to(torch.float64).contiguous()
    classes = classes.to(torch.int32).contiguous()
    counts = counts.to(torch.int32).clamp(max=M).contiguous()
    dev = geom.device
    out = _alloc(B, M, num_classes, output_h, output_w, 3 if rotated else 2, dev)
    if J:
        out['kps'] = torch.empty((B, M, 2 * J), dtype=torch.float32, device=dev)
        out['gt_kps'] = torch.empty((B, M, J, 2), dtype=torch.float32, device=dev)
        out['kp_reg_mask'] = torch.empty((B, M, 2 * J), dtype=torch.uint8, device=dev)
    check(lib().cnuda_encode_targets_modes(
        ptr(None if rotated else geom), ptr(geom if rotated else None), ptr(classes), ptr(counts), ptr(keypoints),
        ptr(visibility), ptr(areas), ptr(out['hm']), ptr(out['reg_mask']), ptr(out['ind']), ptr(out['wh']),
        ptr(out['reg']), ptr(out['gt_dets']), ptr(out['gt_areas']), ptr(out.get('kps')), ptr(out.get('gt_kps')),
        ptr(out.get('kp_reg_mask')), B, num_classes, output_h, output_w, M, J, stream()), 'encode_targets')
    return out
