"""Command-line / library tools around the engine (weight preparation), and the reference's tools.py names that run on
the GPU here: gt_creator, multi_gt_creator, iou_score, loss (yolo355/loss.py)."""
from ..loss import gt_creator, iou_score, loss, multi_gt_creator  # noqa: F401
