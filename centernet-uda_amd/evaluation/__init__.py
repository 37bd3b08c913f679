"""Evaluators, by the reference's package name: `evaluation.coco.Evaluator`, and this project's
`evaluation.coco_keypoints.Evaluator`."""
