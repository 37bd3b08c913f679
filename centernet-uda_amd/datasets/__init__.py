"""The device side of the reference's dataset classes: `encode_targets` produces every target key
of the batch schema (datasets/coco.py:242-259 and 384-401: axis-aligned or rotated boxes, keypoints, areas) and
`prepare_input` the normalised `input` / `target_domain_input` from uint8 images.  Image decoding, augmentation and
resizing stay outside this build."""
from .prepare import prepare_input   # noqa: F401
from .targets import encode_targets   # noqa: F401
