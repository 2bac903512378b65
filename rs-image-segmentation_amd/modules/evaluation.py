"""
Drop-in counterpart of the reference's modules/evaluation.py (evaluate_classification, :32-84): the valid pixels
(ground_truth > 0) are counted into one joint table on the GPU (rsseg.evaluate.joint_counts), and the confusion matrix,
overall accuracy, Cohen's kappa and the printed classification report come from that table.  The heatmap PNG is plotting:
the name of the file is resolved and reported, nothing is drawn (the rule of PLOTTING_NAMES in modules/features/extract.py).
"""
from __future__ import annotations

import os

import numpy as np

from rsseg import evaluate as E

__all__ = ["evaluate_classification", "np", "os"]


def evaluate_classification(prediction, ground_truth, class_names, save_dir="output/supervised/evaluation"):
    """prediction, ground_truth: maps of equal size (NumPy arrays or device tensors).  Returns {"confusion_matrix" (int64
    over labels 1..len(class_names)), "overall_accuracy", "kappa"}; OA and kappa are over every valid pixel and the raw
    predictions, kappa over the union of the labels present (modules/evaluation.py:48-50)."""
    os.makedirs(save_dir, exist_ok=True)
    jc = E.joint_counts(prediction, ground_truth)
    labels = list(range(1, len(class_names) + 1))
    cm = E.confusion(jc, labels=labels)
    oa = E.accuracy(jc)
    kappa = E.kappa(jc)
    print("🔎 分类报告：")
    print(E.format_report(jc, labels=labels, target_names=class_names, digits=3))
    print(f"✅ 总体精度（OA）: {oa:.3f}")
    print(f"✅ Kappa 系数: {kappa:.3f}")
    print(f"[rsseg] evaluate_classification: plotting is out of scope, '{os.path.join(save_dir, 'confusion_matrix.png')}' not written")
    return {"confusion_matrix": cm, "overall_accuracy": oa, "kappa": kappa}
