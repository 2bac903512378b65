"""CPU tests of the accuracy assessment (rsseg/evaluate.py, modules/evaluation.py): every metric derived from a joint count
table equals scikit-learn on the expanded samples; the text report and evaluation_report.txt layouts; the C ABI entry point."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expand(tv, pv, table):
    i, j = np.nonzero(table)
    w = table[i, j]
    return np.repeat(tv[i], w), np.repeat(pv[j], w)


def _random_table(rng, tv, pv, density=0.7, hi=50):
    t = rng.integers(0, hi, (len(tv), len(pv))) * (rng.random((len(tv), len(pv))) < density)
    # every row and column non-empty, as the kernel's compact form guarantees
    for r in range(len(tv)):
        if t[r].sum() == 0:
            t[r, rng.integers(len(pv))] = 1 + rng.integers(hi)
    for c in range(len(pv)):
        if t[:, c].sum() == 0:
            t[rng.integers(len(tv)), c] = 1 + rng.integers(hi)
    return t.astype(np.int64)


CASES = [
    # (truth values, pred values, dtypes): predictions outside 1..n, a class never predicted, a single class, uint8 predictions
    (np.array([1, 2, 3, 4, 5], np.int16), np.arange(0, 8, dtype=np.int32)),
    (np.array([1, 2, 3], np.int16), np.array([-3, 1, 2, 9], np.int64)),
    (np.array([1, 2, 3, 4], np.uint8), np.array([1, 2], np.uint8)),          # classes 3, 4 never predicted
    (np.array([2], np.int32), np.array([2], np.int32)),                      # one class: kappa NaN
    (np.array([7], np.int64), np.array([0, 1, 5], np.int64)),
    (np.array([1, 3, 200], np.uint16), np.array([0, 1, 2, 3], np.uint8)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_table_metrics_equal_sklearn_on_expanded_samples(case, seed):
    from sklearn.metrics import accuracy_score, classification_report, cohen_kappa_score, confusion_matrix
    from rsseg import evaluate as E
    tv, pv = CASES[case]
    rng = np.random.default_rng(case * 10 + seed)
    jc = E.JointCounts(tv, pv, _random_table(rng, tv, pv))
    yt, yp = _expand(tv, pv, jc.table)
    assert jc.n_valid == yt.size
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b = E.confusion(jc), confusion_matrix(yt, yp)
        assert a.dtype == b.dtype and np.array_equal(a, b)
        labels = list(range(1, 4))
        if np.intersect1d(tv, labels).size:
            a, b = E.confusion(jc, labels=labels), confusion_matrix(yt, yp, labels=labels)
            assert a.dtype == b.dtype and np.array_equal(a, b)
        else:   # the same refusal as on the samples
            with pytest.raises(ValueError, match="At least one label"):
                E.confusion(jc, labels=labels)
        assert E.accuracy(jc) == accuracy_score(yt, yp)
        ka, kb = E.kappa(jc), cohen_kappa_score(yt, yp)
        assert (np.isnan(ka) and np.isnan(kb)) or ka == kb
        assert E.report_dict(jc) == classification_report(yt, yp, output_dict=True)
        names = [f"c{i}" for i in labels]
        if not np.intersect1d(tv, labels).size:
            return
        assert E.report_dict(jc, labels=labels, target_names=names) == classification_report(yt, yp, labels=labels, target_names=names,
                                                                                            output_dict=True)


def test_single_class_kappa_is_nan_in_both():
    from sklearn.metrics import cohen_kappa_score
    from rsseg import evaluate as E
    jc = E.JointCounts(np.array([3], np.int16), np.array([3], np.int32), np.array([[17]]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(E.kappa(jc)) and np.isnan(cohen_kappa_score(np.full(17, 3), np.full(17, 3)))


@pytest.mark.parametrize("seed", range(6))
def test_majority_mapping_and_merged_columns_equal_the_per_cluster_loop(seed):
    from rsseg import evaluate as E
    rng = np.random.default_rng(100 + seed)
    tv = np.array([1, 2, 3, 4, 5], np.int16)
    pv = np.arange(8, dtype=np.int32) if seed % 2 else np.array([1, 2, 3, 4, 6, 9], np.uint8)
    tab = _random_table(rng, tv, pv, hi=4)
    tab[:2, 0] = 3            # a tie in column 0: goes to the smaller truth value
    jc = E.JointCounts(tv, pv, tab)
    yt, yp = _expand(tv, pv, tab)
    perm = rng.permutation(yt.size)
    yt, yp = yt[perm], yp[perm]
    # the mapping restated: per cluster, np.unique of the truth values of its samples and the first maximum count
    want = {}
    for c in np.unique(yp):
        u, n = np.unique(yt[yp == c], return_counts=True)
        want[c] = u[np.argmax(n)]
    got = jc.majority_mapping()
    assert got == want
    assert all(type(k) is type(k2) and type(got[k]) is type(want[k2]) for k, k2 in zip(got, want))
    mapped = yp.copy()
    for c, v in want.items():
        mapped[yp == c] = v
    m = jc.mapped()
    assert m.pred_values.dtype == yp.dtype
    ut, um = _expand(m.truth_values, m.pred_values, m.table)
    assert np.array_equal(np.unique(np.stack([ut, um]), axis=1, return_counts=True)[1],
                          np.unique(np.stack([yt, mapped]), axis=1, return_counts=True)[1])
    assert np.array_equal(m.pred_values, np.unique(mapped))


@pytest.mark.parametrize("labels,names", [(None, None), ([1, 2, 3], ["水体", "植被", "建设用地"]), ([1, 2, 3, 4, 5, 6], None),
                                          ([2, 3], ["a", "bb"])])
@pytest.mark.parametrize("seed", [0, 1])
def test_text_report_equals_sklearn(labels, names, seed):
    from sklearn.metrics import classification_report
    from rsseg import evaluate as E
    rng = np.random.default_rng(seed)
    tv, pv = np.array([1, 2, 3, 4], np.int16), np.array([0, 1, 2, 3, 5], np.int32)
    jc = E.JointCounts(tv, pv, _random_table(rng, tv, pv, hi=3000))
    yt, yp = _expand(tv, pv, jc.table)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = classification_report(yt, yp, labels=labels, target_names=names, digits=3)
        got = E.format_report(jc, labels=labels, target_names=names, digits=3)
    assert got == want


def _report_layout(metrics, mapping, class_mapping):
    """The layout of the reference's evaluation_report.txt, written out independently."""
    out = ["=" * 60, "遥感影像分类精度评估报告", "=" * 60, "", "聚类到类别的映射关系:"]
    for c, v in mapping.items():
        out.append("  聚类 %s -> %s" % (c, class_mapping.get(v, "类别%s" % v)))
    oa, k = metrics["overall_accuracy"], metrics["kappa_coefficient"]
    out += ["", "总体精度指标:", "  总体精度: %.4f (%.2f%%)" % (oa, oa * 100), "  Kappa系数: %.4f" % k, "", "各类别精度指标:"]
    for name, m in metrics["class_metrics"].items():
        out.append("  %s:" % name)
        out.append("    精确度: %.4f (%.2f%%)" % (m["precision"], m["precision"] * 100))
        out.append("    召回率: %.4f (%.2f%%)" % (m["recall"], m["recall"] * 100))
        out.append("    F1分数: %.4f (%.2f%%)" % (m["f1-score"], m["f1-score"] * 100))
        out.append("    样本数: %s" % (m["support"],))
        out.append("")
    cm = metrics["confusion_matrix"]
    out.append("混淆矩阵:")
    out.append(" " * 8 + "  ".join("%8d" % i for i in range(len(cm))))
    for i, row in enumerate(cm):
        out.append("  %2d    " % i + "  ".join("%8d" % v for v in row))
    out.append("")
    return "\n".join(out)


def test_evaluation_report_file_layout(tmp_path):
    from sklearn.metrics import accuracy_score, classification_report, cohen_kappa_score, confusion_matrix
    from rsseg import evaluate as E
    rng = np.random.default_rng(7)
    tv, pv = np.array([1, 2, 3, 4], np.int16), np.arange(6, dtype=np.int32)
    jc = E.JointCounts(tv, pv, _random_table(rng, tv, pv, hi=500))
    ev = E.ClassificationEvaluator()
    mapping = jc.majority_mapping()
    metrics = ev._metrics(jc.mapped())
    # the same metrics from scikit-learn on the expanded, mapped samples, as calculate_metrics computes them
    yt, yp = _expand(tv, pv, jc.table)
    ym = yp.copy()
    for c, v in mapping.items():
        ym[yp == c] = v
    names = [ev.class_mapping.get(i, f"类别{i}") for i in np.unique(np.concatenate([yt, ym]))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = classification_report(yt, ym, target_names=names, output_dict=True)
        assert metrics["overall_accuracy"] == accuracy_score(yt, ym)
        assert metrics["kappa_coefficient"] == cohen_kappa_score(yt, ym)
    assert np.array_equal(metrics["confusion_matrix"], confusion_matrix(yt, ym))
    assert metrics["classification_report"] == rep
    assert metrics["class_metrics"] == {n: {k: rep[n][k] for k in ("precision", "recall", "f1-score", "support")} for n in names if n in rep}
    path = tmp_path / "evaluation_report.txt"
    ev.generate_evaluation_report(metrics, mapping, str(path))
    assert path.read_bytes() == _report_layout(metrics, mapping, ev.class_mapping).encode("utf-8")


def test_confusion_counts_declared_and_exported():
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    assert re.search(r"\bint rsseg_confusion_counts\s*\(", hdr)
    for name, val in (("RSSEG_I64", 2), ("RSSEG_U8", 3), ("RSSEG_I16", 4), ("RSSEG_U16", 5), ("RSSEG_I32", 6)):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    lib = _lib.load()
    assert hasattr(lib, "rsseg_confusion_counts") and "rsseg_confusion_counts" in _lib.SIGNATURES
    assert (_lib.U8, _lib.I16, _lib.U16, _lib.I32, _lib.I64) == (3, 4, 5, 6, 2)


def test_confusion_counts_argument_errors():
    from rsseg import _lib
    lib = _lib.load()
    rng, nv = (C.c_int64 * 4)(), C.c_int64(0)
    cnt = (C.c_int64 * 8)()
    # no context: RSSEG_ERR_INVALID without touching a device
    assert lib.rsseg_confusion_counts(None, None, _lib.I16, None, _lib.I32, 0, None, rng, C.byref(nv), cnt, 8) == -1


def test_python_argument_errors(tmp_path):
    from rsseg import evaluate as E
    from rsseg.runtime import RssegUnsupported
    with pytest.raises(ValueError):
        E.JointCounts(np.array([1, 2]), np.array([0]), np.zeros((1, 1), np.int64))
    with pytest.raises(ValueError):
        E.joint_counts(np.zeros(5, np.int32), np.zeros(6, np.int16))

    class TwoRanks:   # a float map needs host codes, which would disagree across ranks: refused before any device work
        world = 2
    with pytest.raises(RssegUnsupported):
        E.joint_counts(np.zeros(4, np.float32), np.ones(4, np.int16), ctx=TwoRanks())
    ev = E.ClassificationEvaluator()
    with pytest.raises(RssegUnsupported, match=r"\(4, 5\).*\(4, 4\)"):
        ev.extract_valid_samples(np.zeros((4, 4), np.int32), np.ones((4, 5), np.int16))
    with pytest.raises(ValueError):
        ev.load_roi_mask(str(tmp_path / "mask.csv"))
