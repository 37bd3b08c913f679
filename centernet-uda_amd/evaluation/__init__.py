"""Evaluators, by the reference's package name: `evaluation.coco.Evaluator`."""
