"""The device side of the reference's dataset classes, from the decoded uint8 image and the COCO
annotation to the batch the train step consumes: `Augmentation` draws the reference's imgaug list on the host
(datasets/coco.py:60-67) and `augment_images` / `transform_points` / `transform_boxes` apply it, the resize to
`input_size` included, in HIP kernels; `prepare_input` turns the uint8 result into the normalised `input` /
`target_domain_input`; `encode_targets` produces every target key of the batch schema (datasets/coco.py:242-259 and
384-401: axis-aligned or rotated boxes, keypoints, areas); `build_batch` chains them into the batch dict.  The
augmenters are defined geometrically ("Augmentation on the device"); nothing was compared with imgaug or
cv2.  Image decoding stays on the host."""
from .augment import (AugmentParams, Augmentation, augment_images, build_batch, transform_boxes,   # noqa: F401
                      transform_points)
from .prepare import prepare_input   # noqa: F401
from .strong_view import StrongView, StrongViewParams   # noqa: F401  (the function: datasets.strong_view.strong_view)
from .geometric_view import GeometricView, GeometricViewParams, warp_batch   # noqa: F401
from .targets import encode_targets   # noqa: F401
