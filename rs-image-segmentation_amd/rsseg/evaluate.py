"""
Accuracy assessment on the GPU: the counterpart of the reference's scripts/4_evaluate.py (ClassificationEvaluator) and the
shared logic of modules/evaluation.py.

Every metric both evaluators report follows exactly from ONE joint count table of (truth value, predicted value) over the
pixels where truth > 0 (rsseg_confusion_counts, csrc/k14_eval.hip): the confusion matrices (with and without `labels=`),
overall accuracy, Cohen's kappa, the classification report and the cluster -> class majority mapping.  The metrics come
from scikit-learn itself, called on the table's non-zero cells (t, p) with sample_weight = count: its integer-weighted
sums are the counts of the expanded samples, so its results are those of the reference's calls.  Only the TEXT form of
classification_report differs (it prints a weighted support as 4318.0): format_report prints it as the reference sees it.

    python -m rsseg.evaluate CLASSIFICATION ROI_MASK OUTPUT_DIR        (scripts/4_evaluate.py:main)
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .runtime import Context, RssegUnsupported, default_context

_TRUTH_DT = (np.uint8, np.int16, np.uint16, np.int32, np.int64)
_PRED_DT = (np.uint8, np.int32, np.int64)
NO_VALID_SAMPLES = "ROI掩膜中没有找到有效的采样点"          # scripts/4_evaluate.py:86


class JointCounts:
    """The table: truth_values (sorted, truth dtype) x pred_values (sorted, prediction dtype) -> int64 counts, every row and
    column non-empty."""

    def __init__(self, truth_values, pred_values, table):
        self.truth_values = np.asarray(truth_values)
        self.pred_values = np.asarray(pred_values)
        self.table = np.asarray(table, dtype=np.int64)
        if self.table.shape != (self.truth_values.size, self.pred_values.size):
            raise ValueError(f"table {self.table.shape} for {self.truth_values.size} truth x {self.pred_values.size} predicted values")

    @property
    def n_valid(self) -> int:
        return int(self.table.sum())

    def triples(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(y_true, y_pred, sample_weight) of the non-zero cells, in the input dtypes."""
        i, j = np.nonzero(self.table)
        return self.truth_values[i], self.pred_values[j], self.table[i, j]

    def majority_mapping(self) -> Dict:
        """For each predicted value, the truth value with the highest count; ties go to the smallest truth value (np.unique +
        argmax of map_clusters_to_classes, scripts/4_evaluate.py:112-117).  {pred value: truth value}, NumPy scalars."""
        best = np.argmax(self.table, axis=0)
        return {self.pred_values[j]: self.truth_values[best[j]] for j in range(self.pred_values.size)}

    def mapped(self) -> "JointCounts":
        """The table of (truth, mapped prediction): columns merged by their majority class.  The mapped values are cast to the
        prediction's dtype, as np.copy(y_pred) + assignment does (scripts/4_evaluate.py:124-126)."""
        mv = self.truth_values[np.argmax(self.table, axis=0)].astype(self.pred_values.dtype)
        vals, inv = np.unique(mv, return_inverse=True)
        out = np.zeros((self.truth_values.size, vals.size), np.int64)
        np.add.at(out.T, inv, self.table.T)
        return JointCounts(self.truth_values, vals, out)


def _np_dtype(t):
    return np.dtype(str(t.dtype).split(".")[1]) if _is_tensor(t) else np.asarray(t).dtype


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy().reshape(-1) if _is_tensor(a) else np.asarray(a).reshape(-1)


def joint_counts(prediction, ground_truth, ctx: Optional[Context] = None, keep_all: bool = False) -> JointCounts:
    """The joint table of (ground_truth, prediction) over the pixels where ground_truth > 0.  Either may be a NumPy array
    or a device tensor (a map already on the device is not copied back); any shape, equal sizes.  Integer maps of the
    kernel's dtypes whose table fits in 4096 cells go to the device as they are.  A float map, another dtype, or a range
    beyond the cap is first compacted on the host (np.unique(..., return_inverse=True) -> int32 codes), then the same
    kernel counts the codes; with more than one rank that is refused (per-rank codes disagree).  keep_all: count every
    sample, truth <= 0 included (calculate_metrics on arbitrary 1-D arrays)."""
    n_t = ground_truth.numel() if _is_tensor(ground_truth) else np.asarray(ground_truth).size
    n_p = prediction.numel() if _is_tensor(prediction) else np.asarray(prediction).size
    if n_t != n_p:
        raise ValueError(f"ground truth has {n_t} values, prediction {n_p}")
    tdt, pdt = _np_dtype(ground_truth), _np_dtype(prediction)
    ctx = ctx or default_context()
    if not keep_all and tdt in _TRUTH_DT and pdt in _PRED_DT:
        try:
            tv, pv, tab = ctx.confusion_counts(_device(ctx, ground_truth), _device(ctx, prediction))
        except RssegUnsupported:
            if ctx.world > 1:
                raise
        else:
            if tab.size == 0:
                raise ValueError(NO_VALID_SAMPLES)
            return JointCounts(tv, pv, tab)
    if ctx.world > 1:
        raise RssegUnsupported(f"joint_counts: a {tdt} truth / {pdt} prediction needs host compaction, which disagrees across "
                               f"{ctx.world} ranks: give every rank integer maps of a table within {L.EVAL_MAX_CELLS} cells")
    return _compacted(ctx, _host(prediction), _host(ground_truth), keep_all)


def _device(ctx: Context, a):
    return a.reshape(-1) if _is_tensor(a) else ctx.to_device(np.asarray(a).reshape(-1))


def _compacted(ctx: Context, pred: np.ndarray, truth: np.ndarray, keep_all: bool) -> JointCounts:
    if not keep_all:
        valid = truth > 0
        truth, pred = truth[valid], pred[valid]
    if truth.size == 0:
        raise ValueError(NO_VALID_SAMPLES)
    tv, tc = np.unique(truth, return_inverse=True)
    pv, pc = np.unique(pred, return_inverse=True)
    if tv.size * pv.size > L.EVAL_MAX_CELLS:
        raise RssegUnsupported(f"joint_counts: {tv.size} truth x {pv.size} predicted values exceed {L.EVAL_MAX_CELLS} cells")
    # codes: truth 1..K (every sample valid), prediction 0..M-1, both int32, range known
    tcode = ctx.to_device((tc.reshape(-1) + 1).astype(np.int32))
    pcode = ctx.to_device(pc.reshape(-1).astype(np.int32))
    rows, cols, tab = ctx.confusion_counts(tcode, pcode, known_range=(1, tv.size, 0, pv.size - 1))
    return JointCounts(tv[rows - 1], pv[cols], tab)


# ---- metrics from the table (scikit-learn on the weighted cells) ---------------------------------------------------------
def confusion(jc: JointCounts, labels=None) -> np.ndarray:
    from sklearn.metrics import confusion_matrix
    t, p, w = jc.triples()
    return confusion_matrix(t, p, labels=labels, sample_weight=w)


def accuracy(jc: JointCounts) -> float:
    from sklearn.metrics import accuracy_score
    t, p, w = jc.triples()
    return accuracy_score(t, p, sample_weight=w)


def kappa(jc: JointCounts):
    from sklearn.metrics import cohen_kappa_score
    t, p, w = jc.triples()
    return cohen_kappa_score(t, p, sample_weight=w)


def report_dict(jc: JointCounts, labels=None, target_names=None, digits: int = 2) -> Dict:
    from sklearn.metrics import classification_report
    t, p, w = jc.triples()
    return classification_report(t, p, labels=labels, target_names=target_names, digits=digits, output_dict=True, sample_weight=w)


def format_report(jc: JointCounts, labels=None, target_names=None, digits: int = 2) -> str:
    """The text form of classification_report(y_true, y_pred, labels, target_names, digits) on the expanded samples: the
    layout of scikit-learn's text report, with the per-class and average figures of the weighted call and the support
    printed as the integer it is."""
    from sklearn.metrics import precision_recall_fscore_support
    from sklearn.utils.multiclass import unique_labels
    t, p, w = jc.triples()
    present = unique_labels(t, p)
    labels_given = labels is not None
    labels = present if labels is None else np.asarray(labels)
    micro_is_accuracy = not labels_given or set(labels) >= set(present)
    if target_names is None:
        target_names = ["%s" % lb for lb in labels]
    elif len(labels) != len(target_names):
        if not labels_given:
            raise ValueError(f"Number of classes, {len(labels)}, does not match size of target_names, {len(target_names)}. "
                             "Try specifying the labels parameter")
        warnings.warn(f"labels size, {len(labels)}, does not match size of target_names, {len(target_names)}")
    pr, rc, f1, s = precision_recall_fscore_support(t, p, labels=labels, average=None, sample_weight=w)
    width = max(max(len(cn) for cn in target_names), len("weighted avg"), digits)
    head = "{:>{width}s} " + " {:>9}" * 4
    row = "{:>{width}s} " + " {:>9.{digits}f}" * 3 + " {:>9}\n"
    out = head.format("", "precision", "recall", "f1-score", "support", width=width) + "\n\n"
    for name, a, b, c, d in zip(target_names, pr, rc, f1, s):
        out += row.format(name, a, b, c, int(round(d)), width=width, digits=digits)
    out += "\n"
    total = int(round(float(np.sum(s))))
    for average in ("micro", "macro", "weighted"):
        ap, ar, af, _ = precision_recall_fscore_support(t, p, labels=labels, average=average, sample_weight=w)
        if average == "micro" and micro_is_accuracy:
            out += ("{:>{width}s} " + " {:>9.{digits}}" * 2 + " {:>9.{digits}f}" + " {:>9}\n").format(
                "accuracy", "", "", af, total, width=width, digits=digits)
        else:
            out += row.format(average + " avg", ap, ar, af, total, width=width, digits=digits)
    return out


# ---- scripts/4_evaluate.py -----------------------------------------------------------------------------------------------
def _plot_stub(name: str, path) -> None:
    print(f"[rsseg] {name}: plotting is out of scope, '{path}' not written")


class ClassificationEvaluator:
    """scripts/4_evaluate.py:28-402 with the counting on the GPU.  The reference's method names, signatures and messages;
    the three plot methods draw nothing.  Deviation: a ROI mask of another shape than the classification raises
    RssegUnsupported (the reference resizes it with skimage.transform.resize(order=0), :74-80)."""

    def __init__(self, ctx: Optional[Context] = None):
        self.class_mapping = {0: '未分类/背景', 1: '植被', 2: '水体', 3: '建设用地', 4: '裸地/其他'}
        self.color_mapping = {0: [0, 0, 0], 1: [0, 128, 0], 2: [0, 0, 255], 3: [255, 0, 0], 4: [255, 255, 0]}
        self._ctx = ctx

    @property
    def ctx(self) -> Context:
        return self._ctx or default_context()

    @staticmethod
    def _load(file_path):
        if file_path.endswith('.npy'):
            return np.load(file_path)
        if file_path.endswith('.tif') or file_path.endswith('.tiff'):
            from .tiff import read_tiff
            return read_tiff(file_path)[0]
        raise ValueError("不支持的文件格式，请使用 .npy 或 .tif 文件")

    def load_classification_result(self, file_path):
        return self._load(file_path)

    def load_roi_mask(self, file_path):
        return self._load(file_path)

    def _check_shapes(self, classification_map, roi_mask):
        if tuple(classification_map.shape) != tuple(roi_mask.shape):
            print(f"警告：分类图像形状 {tuple(classification_map.shape)} 与ROI掩膜形状 {tuple(roi_mask.shape)} 不一致")
            raise RssegUnsupported(f"ROI mask of shape {tuple(roi_mask.shape)} for a classification of shape "
                                   f"{tuple(classification_map.shape)}: the nearest-neighbour resize of the reference is not implemented")

    def _valid_counts(self, classification_map, roi_mask) -> JointCounts:
        """extract_valid_samples' checks and messages from the table alone (no per-pixel arrays)."""
        self._check_shapes(classification_map, roi_mask)
        jc = joint_counts(classification_map, roi_mask, self.ctx)
        print(f"提取到 {jc.n_valid} 个有效采样点")
        print(f"真实标签类别: {jc.truth_values}")
        print(f"预测标签类别: {jc.pred_values}")
        return jc

    def extract_valid_samples(self, classification_map, roi_mask):
        self._valid_counts(classification_map, roi_mask)
        cm, rm = np.asarray(classification_map), np.asarray(roi_mask)
        valid_mask = rm > 0
        return rm[valid_mask], cm[valid_mask], valid_mask

    def _mapping(self, jc: JointCounts) -> Dict:
        print(f"\n聚类标签: {jc.pred_values}")
        print(f"真实类别: {jc.truth_values}")
        mapping = jc.majority_mapping()
        for cluster, cls in mapping.items():
            print(f"聚类 {cluster} -> 类别 {cls} ({self.class_mapping.get(cls, '未知')})")
        return mapping

    def map_clusters_to_classes(self, y_true, y_pred):
        y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
        jc = joint_counts(y_pred, y_true, self.ctx, keep_all=not bool(np.all(y_true > 0)))
        mapping = self._mapping(jc)
        mv = np.array([mapping[c] for c in jc.pred_values]).astype(y_pred.dtype)
        return mv[np.searchsorted(jc.pred_values, y_pred)], mapping

    def _metrics(self, jc: JointCounts) -> Dict:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # the reference silences every warning (scripts/4_evaluate.py:22-23)
            class_names = [self.class_mapping.get(i, f'类别{i}') for i in np.union1d(jc.truth_values, jc.pred_values)]
            report = report_dict(jc, target_names=class_names)
            class_metrics = {name: {k: report[name][k] for k in ('precision', 'recall', 'f1-score', 'support')}
                             for name in class_names if name in report}
            return {'overall_accuracy': accuracy(jc), 'kappa_coefficient': kappa(jc), 'confusion_matrix': confusion(jc),
                    'classification_report': report, 'class_metrics': class_metrics}

    def calculate_metrics(self, y_true, y_pred):
        y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
        return self._metrics(joint_counts(y_pred, y_true, self.ctx, keep_all=not bool(np.all(y_true > 0))))

    def plot_confusion_matrix(self, cm, class_names, save_path=None):
        _plot_stub("plot_confusion_matrix", save_path)

    def plot_accuracy_comparison(self, metrics, save_path=None):
        _plot_stub("plot_accuracy_comparison", save_path)

    def plot_classification_comparison(self, classification_map, roi_mask, valid_mask, save_path=None):
        _plot_stub("plot_classification_comparison", save_path)

    def report_text(self, metrics, cluster_mapping) -> str:
        rule = "=" * 60
        lines = [rule, "遥感影像分类精度评估报告", rule, "", "聚类到类别的映射关系:"]
        lines += [f"  聚类 {c} -> {self.class_mapping.get(v, f'类别{v}')}" for c, v in cluster_mapping.items()]
        oa, k = metrics['overall_accuracy'], metrics['kappa_coefficient']
        lines += ["", "总体精度指标:", f"  总体精度: {oa:.4f} ({oa * 100:.2f}%)", f"  Kappa系数: {k:.4f}", "", "各类别精度指标:"]
        for name, m in (metrics['class_metrics'] or {}).items():
            lines.append(f"  {name}:")
            for label, key in (("精确度", 'precision'), ("召回率", 'recall'), ("F1分数", 'f1-score')):
                lines.append(f"    {label}: {m[key]:.4f} ({m[key] * 100:.2f}%)")
            lines += [f"    样本数: {m['support']}", ""]
        cm = metrics['confusion_matrix']
        lines += ["混淆矩阵:", " " * 8 + "  ".join(f"{i:>8}" for i in range(len(cm)))]
        lines += [f"  {i:>2}    " + "  ".join(f"{v:>8}" for v in r) for i, r in enumerate(cm)]
        lines.append("")
        return "\n".join(lines)

    def generate_evaluation_report(self, metrics, cluster_mapping, output_path):
        text = self.report_text(metrics, cluster_mapping)
        with open(output_path, 'w', encoding='utf-8') as f:
            f.write(text)
        print(f"评估报告已保存至: {output_path}")
        print("\n" + text)

    def evaluate_maps(self, classification_map, roi_mask, output_dir="evaluation_results"):
        """Steps 2-6 of evaluate_classification on maps already in memory (NumPy arrays or device tensors): ONE table pass
        over the raster; the mapped metrics come from its merged columns."""
        os.makedirs(output_dir, exist_ok=True)
        print("\n2. 提取有效采样点...")
        jc = self._valid_counts(classification_map, roi_mask)
        print("\n3. 映射聚类结果到真实类别...")
        cluster_mapping = self._mapping(jc)
        print("\n4. 计算评估指标...")
        metrics = self._metrics(jc.mapped())
        print("\n5. 生成可视化结果...")
        self.plot_confusion_matrix(metrics['confusion_matrix'], None, os.path.join(output_dir, "confusion_matrix.png"))
        self.plot_accuracy_comparison(metrics, os.path.join(output_dir, "accuracy_comparison.png"))
        self.plot_classification_comparison(classification_map, roi_mask, None, os.path.join(output_dir, "classification_comparison.png"))
        print("\n6. 生成评估报告...")
        self.generate_evaluation_report(metrics, cluster_mapping, os.path.join(output_dir, "evaluation_report.txt"))
        print("\n" + "=" * 50)
        print("分类精度评估完成！")
        print(f"所有结果已保存至目录: {output_dir}")
        return metrics, cluster_mapping

    def evaluate_classification(self, classification_file, roi_mask_file, output_dir="evaluation_results"):
        os.makedirs(output_dir, exist_ok=True)
        print("开始分类精度评估...")
        print("=" * 50)
        print("1. 加载数据文件...")
        classification_map = self.load_classification_result(classification_file)
        roi_mask = self.load_roi_mask(roi_mask_file)
        print(f"分类结果形状: {classification_map.shape}")
        print(f"ROI掩膜形状: {roi_mask.shape}")
        return self.evaluate_maps(classification_map, roi_mask, output_dir)


def main(argv: Optional[Sequence[str]] = None) -> int:
    """scripts/4_evaluate.py:main with the three paths on the command line."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rsseg.evaluate", description="accuracy assessment of a classification against a ROI mask (scripts/4) on the GPU")
    ap.add_argument("classification")
    ap.add_argument("roi_mask")
    ap.add_argument("output_dir")
    a = ap.parse_args(argv)
    if not os.path.exists(a.classification):
        print(f"错误: 分类结果文件不存在: {a.classification}")
        print("请确保已运行分类流程并生成了分类结果文件")
        return 1
    if not os.path.exists(a.roi_mask):
        print(f"错误: ROI掩膜文件不存在: {a.roi_mask}")
        print("请确保已生成ROI掩膜文件")
        return 1
    try:
        metrics, _ = ClassificationEvaluator().evaluate_classification(a.classification, a.roi_mask, a.output_dir)
    except Exception as e:  # noqa: BLE001 — scripts/4_evaluate.py prints the error and its traceback
        print(f"评估过程中发生错误: {e}")
        import traceback
        traceback.print_exc()
        return 1
    print(f"\n评估完成! 总体精度: {metrics['overall_accuracy'] * 100:.2f}%")
    print(f"Kappa系数: {metrics['kappa_coefficient']:.4f}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
