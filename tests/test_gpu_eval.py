"""GPU tests of the accuracy assessment: the K14 joint count table (rsseg_confusion_counts) against np.bincount /
torch.bincount, and the two evaluators (modules.evaluation.evaluate_classification, rsseg.evaluate.ClassificationEvaluator)
against scikit-learn run the reference's way on the same arrays."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TRUTH_DT = [np.uint8, np.int16, np.uint16, np.int32, np.int64]
PRED_DT = [np.uint8, np.int32, np.int64]


def _bincount_table(truth, pred):
    """(truth values, pred values, table) of the pixels where truth > 0, by np.bincount on the combined index."""
    v = truth > 0
    t, p = truth[v].astype(np.int64), pred[v].astype(np.int64)
    if t.size == 0:
        return np.zeros(0, truth.dtype), np.zeros(0, pred.dtype), np.zeros((0, 0), np.int64)
    tv, ti = np.unique(t, return_inverse=True)
    pv, pi = np.unique(p, return_inverse=True)
    tab = np.bincount(ti * pv.size + pi, minlength=tv.size * pv.size).reshape(tv.size, pv.size)
    return tv.astype(truth.dtype), pv.astype(pred.dtype), tab


def _labels(rng, n, dt, lo, hi):
    return rng.integers(lo, hi, n).astype(dt)


@pytest.mark.parametrize("tdt", TRUTH_DT)
@pytest.mark.parametrize("pdt", PRED_DT)
@pytest.mark.parametrize("n", [0, 1, 15, 17, 1000, 4099, 65536 + 7])
def test_counts_equal_bincount_for_every_dtype_pair(ctx, tdt, pdt, n):
    rng = np.random.default_rng(n + 7 * TRUTH_DT.index(tdt) + 31 * PRED_DT.index(pdt))
    signed_t, signed_p = np.issubdtype(tdt, np.signedinteger), np.issubdtype(pdt, np.signedinteger)
    truth = _labels(rng, n, tdt, -3 if signed_t else 0, 9)            # truth <= 0 excluded
    pred = _labels(rng, n, pdt, -5 if signed_p else 0, 11)            # negative predictions
    want = _bincount_table(truth, pred)
    got = ctx.confusion_counts(ctx.to_device(truth), ctx.to_device(pred))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_offset_views_and_wide_values(ctx):
    """A plane that starts off a 16-byte boundary (a slice of a device tensor) and labels far from zero."""
    rng = np.random.default_rng(3)
    truth = rng.integers(1000, 1010, 5003).astype(np.int32)
    pred = (rng.integers(0, 40, 5003) - 2**40).astype(np.int64)
    dt, dp = ctx.to_device(truth), ctx.to_device(pred)
    got = ctx.confusion_counts(dt[3:], dp[3:])
    want = _bincount_table(truth[3:], pred[3:])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_table_of_exactly_4096_cells_runs_on_the_gpu(ctx):
    rng = np.random.default_rng(4096)
    truth = rng.integers(1, 17, 300000).astype(np.int16)              # 16 truth values
    pred = rng.integers(0, 256, 300000).astype(np.int32)              # 256 predicted values
    truth[:16], pred[:256] = np.arange(1, 17), np.arange(256)
    tv, pv, tab = ctx.confusion_counts(ctx.to_device(truth), ctx.to_device(pred))
    assert tab.shape == (16, 256)
    want = _bincount_table(truth, pred)
    assert np.array_equal(tv, want[0]) and np.array_equal(pv, want[1]) and np.array_equal(tab, want[2])


def test_4097_cells_and_int64_labels_take_the_host_compaction_path(ctx):
    from rsseg import evaluate as E
    from rsseg.runtime import RssegUnsupported
    rng = np.random.default_rng(4097)
    truth = rng.choice(np.array([1, 17], np.int16), 200000)           # range 1..17 x 0..240 = 4097 cells, 2 x 241 present
    pred = rng.integers(0, 241, 200000).astype(np.int32)
    with pytest.raises(RssegUnsupported):
        ctx.confusion_counts(ctx.to_device(truth), ctx.to_device(pred))
    jc = E.joint_counts(pred, truth, ctx)
    want = _bincount_table(truth, pred)
    assert np.array_equal(jc.truth_values, want[0]) and np.array_equal(jc.pred_values, want[1]) and np.array_equal(jc.table, want[2])
    # int64 labels beyond int32 on both sides, and a float map
    t64 = rng.choice(np.array([0, 5, 2**35, 2**40 + 1], np.int64), 50000)
    p64 = rng.choice(np.array([-2**45, 3, 2**33], np.int64), 50000)
    for pred_map in (p64, p64.astype(np.float64)):
        jc = E.joint_counts(pred_map, t64, ctx)
        want = _bincount_table(t64, p64)
        assert np.array_equal(jc.truth_values, want[0]) and jc.truth_values.dtype == np.int64
        assert np.array_equal(jc.pred_values, want[1]) and jc.pred_values.dtype == pred_map.dtype
        assert np.array_equal(jc.table, want[2])


def test_no_valid_pixel_raises_the_reference_error(ctx, tmp_path):
    from rsseg import evaluate as E
    truth = np.zeros((32, 32), np.int16)
    truth[3, 4] = -2
    pred = np.ones((32, 32), np.int32)
    tv, pv, tab = ctx.confusion_counts(ctx.to_device(truth.reshape(-1)), ctx.to_device(pred.reshape(-1)))
    assert tab.shape == (0, 0)
    with pytest.raises(ValueError, match=E.NO_VALID_SAMPLES):
        E.joint_counts(pred, truth, ctx)
    with pytest.raises(ValueError, match=E.NO_VALID_SAMPLES):
        E.ClassificationEvaluator(ctx).evaluate_maps(pred, truth, str(tmp_path))
    with pytest.raises(ValueError, match=E.NO_VALID_SAMPLES):
        E.joint_counts(np.zeros(0, np.int32), np.zeros(0, np.int16), ctx)


def test_known_range_skips_the_range_pass_and_is_checked(ctx):
    rng = np.random.default_rng(11)
    truth = rng.integers(0, 6, 100003).astype(np.int16)
    pred = rng.integers(0, 8, 100003).astype(np.int32)
    want = _bincount_table(truth, pred)
    got = ctx.confusion_counts(ctx.to_device(truth), ctx.to_device(pred), known_range=(1, 5, 0, 7))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    with pytest.raises(ValueError, match="known_range"):
        ctx.confusion_counts(ctx.to_device(truth), ctx.to_device(pred), known_range=(1, 5, 0, 6))


# ---- the evaluators against scikit-learn, the reference's way -------------------------------------------------------------
def _sk_modules_way(prediction, ground_truth, class_names):
    from sklearn.metrics import accuracy_score, cohen_kappa_score, confusion_matrix
    y_pred, y_true = prediction.flatten(), ground_truth.flatten()
    keep = y_true > 0
    y_true, y_pred = y_true[keep], y_pred[keep]
    labels = list(range(1, len(class_names) + 1))
    return {"confusion_matrix": confusion_matrix(y_true, y_pred, labels=labels), "overall_accuracy": accuracy_score(y_true, y_pred),
            "kappa": cohen_kappa_score(y_true, y_pred)}, (y_true, y_pred, labels)


def _check_modules_eval(prediction, truth, class_names, tmp_path, capsys):
    from sklearn.metrics import classification_report
    from modules.evaluation import evaluate_classification
    got = evaluate_classification(prediction, truth, class_names, save_dir=str(tmp_path / "ev"))
    out = capsys.readouterr().out
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, (yt, yp, labels) = _sk_modules_way(prediction, truth, class_names)
        text = classification_report(yt, yp, labels=labels, target_names=class_names, digits=3)
    assert got["confusion_matrix"].dtype == np.int64 and np.array_equal(got["confusion_matrix"], want["confusion_matrix"])
    assert got["overall_accuracy"] == want["overall_accuracy"]
    assert got["kappa"] == want["kappa"] or (np.isnan(got["kappa"]) and np.isnan(want["kappa"]))
    assert text in out and f"总体精度（OA）: {want['overall_accuracy']:.3f}" in out
    assert (tmp_path / "ev").is_dir()


def _sk_scripts4_way(classification_map, roi_mask, class_mapping):
    """scripts/4's steps on the host: valid samples, the per-cluster majority, metrics on the mapped predictions."""
    from sklearn.metrics import accuracy_score, classification_report, cohen_kappa_score, confusion_matrix
    valid = roi_mask > 0
    y_true, y_pred = roi_mask[valid], classification_map[valid]
    mapping = {}
    for c in np.unique(y_pred):
        vals, cnt = np.unique(y_true[y_pred == c], return_counts=True)
        mapping[c] = vals[np.argmax(cnt)]
    mapped = np.copy(y_pred)
    for c, v in mapping.items():
        mapped[y_pred == c] = v
    names = [class_mapping.get(i, f"类别{i}") for i in np.unique(np.concatenate([y_true, mapped]))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = classification_report(y_true, mapped, target_names=names, output_dict=True)
        m = {"overall_accuracy": accuracy_score(y_true, mapped), "kappa_coefficient": cohen_kappa_score(y_true, mapped),
             "confusion_matrix": confusion_matrix(y_true, mapped), "classification_report": rep,
             "class_metrics": {n: {k: rep[n][k] for k in ("precision", "recall", "f1-score", "support")} for n in names if n in rep}}
    return m, mapping, y_true


def _check_scripts4(classification_map, roi_mask, tmp_path, capsys):
    from rsseg.evaluate import ClassificationEvaluator
    tmp_path.mkdir(parents=True, exist_ok=True)
    np.save(tmp_path / "cls.npy", classification_map)
    np.save(tmp_path / "roi.npy", roi_mask)
    ev = ClassificationEvaluator()
    metrics, mapping = ev.evaluate_classification(str(tmp_path / "cls.npy"), str(tmp_path / "roi.npy"), str(tmp_path / "out"))
    out = capsys.readouterr().out
    want, want_map, y_true = _sk_scripts4_way(classification_map, roi_mask, ev.class_mapping)
    assert mapping == want_map
    assert np.array_equal(metrics.pop("confusion_matrix"), want.pop("confusion_matrix"))
    assert metrics == want
    assert f"提取到 {y_true.size} 个有效采样点" in out
    assert f"真实标签类别: {np.unique(y_true)}" in out and f"预测标签类别: {np.unique(classification_map[roi_mask > 0])}" in out
    assert (tmp_path / "out" / "evaluation_report.txt").exists()
    # the 1-D methods give the same through the same path
    yt, yp, valid = ev.extract_valid_samples(classification_map, roi_mask)
    ym, m2 = ev.map_clusters_to_classes(yt, yp)
    assert m2 == want_map and ym.dtype == yp.dtype
    m3 = ev.calculate_metrics(yt, ym)
    m3.pop("confusion_matrix")
    assert m3 == want


def test_bundled_scene_both_evaluators(golden_dir, tmp_path, capsys):
    g = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    ko = np.load(os.path.join(golden_dir, "scene_aa_ref_outputs.npz"))
    roi = g["roi_mask"]
    assert (roi > 0).sum() == 33
    _check_modules_eval(g["class_map"], roi, ["水体", "植被", "建设用地"], tmp_path / "a", capsys)
    _check_scripts4(g["class_map"], roi, tmp_path / "b", capsys)
    for key in ("kmeans_idx7_k6", "kmeans_idx7_k8"):
        labels = ko[key]
        _check_modules_eval(labels, roi, ["水体", "植被", "建设用地", "裸地"], tmp_path / f"c{key}", capsys)
        _check_scripts4(labels, roi, tmp_path / f"d{key}", capsys)
        _check_scripts4(labels.astype(np.int32), roi, tmp_path / f"e{key}", capsys)   # a KMeans int32 map


def test_dense_truth_at_4096(ctx, tmp_path, capsys):
    rng = np.random.default_rng(4096)
    n = 4096
    truth = rng.integers(0, 6, (n, n)).astype(np.int16)
    # a KMeans-like map: correlated with the truth, 8 clusters
    pred = np.where(rng.random((n, n)) < 0.7, truth.astype(np.int32) + 2, rng.integers(0, 8, (n, n))).astype(np.int32) % 8
    _check_modules_eval(pred, truth, ["a", "b", "c", "d", "e"], tmp_path / "m", capsys)
    _check_scripts4(pred, truth, tmp_path / "s", capsys)


def test_full_size_table_equals_torch_bincount(ctx):
    import torch
    n = 16384
    g = torch.Generator(device="cuda").manual_seed(5)
    truth = torch.randint(0, 6, (n * n,), device="cuda", dtype=torch.int16, generator=g)
    pred = torch.randint(0, 8, (n * n,), device="cuda", dtype=torch.int32, generator=g)
    tv, pv, tab = ctx.confusion_counts(truth, pred)
    v = truth > 0
    want = torch.bincount((truth[v].long() - 1) * 8 + pred[v].long(), minlength=40).reshape(5, 8).cpu().numpy()
    assert np.array_equal(tv, np.arange(1, 6)) and np.array_equal(pv, np.arange(8)) and np.array_equal(tab, want)
    assert int(tab.sum()) == int(v.sum())


class _ThreadWorld:
    """N ranks as N threads of this process on one GPU: every rank's all-reduce hook meets at a barrier, rank 0 reduces the
    N device buffers, every rank copies the result back."""

    def __init__(self, world):
        import threading
        self.world = world
        self.bar = threading.Barrier(world, timeout=120)
        self.slots = [None] * world
        self.result = None
        self.calls = 0

    def hook(self, rank):
        import torch
        from rsseg import _lib as L
        views = {L.F32: torch.float32, L.F64: torch.float64, L.I64: torch.int64}

        def fn(buf, offset, count, dtype, op):
            t = buf[offset:offset + count * (4 if dtype == L.F32 else 8)].view(views[dtype])
            torch.cuda.synchronize()
            self.slots[rank] = t
            self.bar.wait()
            if rank == 0:
                st = torch.stack(self.slots)
                self.result = st.sum(0) if op == L.SUM else (st.amin(0) if op == L.MIN else st.amax(0))
                self.calls += 1
                torch.cuda.synchronize()
            self.bar.wait()
            t.copy_(self.result)
            torch.cuda.synchronize()
            self.bar.wait()

        return fn

    def run(self, target):
        import threading
        errs = []

        def wrap(r):
            try:
                target(r)
            except BaseException as e:  # noqa: BLE001
                errs.append((r, e))
                self.bar.abort()

        th = [threading.Thread(target=wrap, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0][1]


@pytest.mark.parametrize("world", [2, 3])
def test_row_sharded_map_gives_every_rank_the_whole_table(ctx, world):
    from rsseg import evaluate as E
    from rsseg.runtime import Context
    rng = np.random.default_rng(world)
    H, W = 517, 300
    truth = rng.integers(-1, 6, (H, W)).astype(np.int16)
    truth[: H // 2 + 40] = np.minimum(truth[: H // 2 + 40], 3)      # ranks see different ranges
    pred = rng.integers(0, 8, (H, W)).astype(np.int32)
    pred[-20:] = -4
    want = E.joint_counts(pred, truth, ctx)
    tw = _ThreadWorld(world)
    out = [None] * world
    big = [None] * world

    def rank_main(r):
        c = Context(0, use_dist=False)
        c.install_comm_hook(r, world, tw.hook(r))
        r0, r1 = r * H // world, (r + 1) * H // world
        out[r] = E.joint_counts(c.to_device(pred[r0:r1].reshape(-1)), c.to_device(truth[r0:r1].reshape(-1)), c)
        # a table over the cap: every rank makes the same calls and raises alike
        try:
            c.confusion_counts(c.to_device(truth[r0:r1].reshape(-1)), c.to_device((pred[r0:r1] * 1000).reshape(-1)))
        except E.RssegUnsupported:
            big[r] = True
        c.close()

    tw.run(rank_main)
    assert tw.calls == 4 + 3     # range (SUM, MIN, MAX) + table; the over-cap call stops after its range
    for r in range(world):
        assert np.array_equal(out[r].truth_values, want.truth_values) and np.array_equal(out[r].pred_values, want.pred_values)
        assert np.array_equal(out[r].table, want.table), r
        assert big[r], r


def test_stages_cli_evaluate_writes_the_report(ctx, golden_dir, tmp_path):
    from rsseg import stages
    from rsseg.tiff import write_tiff
    g = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    write_tiff(str(tmp_path / "in.tif"), g["dn"], transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    np.save(tmp_path / "roi.npy", g["roi_mask"])
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "out"), "--classify", "kmeans", "--n-clusters", "6",
                        "--evaluate", str(tmp_path / "roi.npy")]) == 0
    rep = tmp_path / "out" / "evaluation_results" / "evaluation_report.txt"
    assert rep.exists()
    text = rep.read_text(encoding="utf-8")
    assert text.startswith("=" * 60) and "总体精度指标:" in text and "混淆矩阵:" in text
    cls = np.load(tmp_path / "out" / "segmentation_results" / "classification_kmeans.npy")
    from rsseg.evaluate import ClassificationEvaluator
    want, want_map, _ = _sk_scripts4_way(cls, g["roi_mask"], ClassificationEvaluator().class_mapping)
    assert f"  总体精度: {want['overall_accuracy']:.4f}" in text


def test_evaluate_module_cli(ctx, golden_dir, tmp_path):
    from rsseg import evaluate as E
    g = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    np.save(tmp_path / "cls.npy", g["class_map"])
    np.save(tmp_path / "roi.npy", g["roi_mask"])
    assert E.main([str(tmp_path / "cls.npy"), str(tmp_path / "roi.npy"), str(tmp_path / "o")]) == 0
    assert (tmp_path / "o" / "evaluation_report.txt").exists()
    assert E.main([str(tmp_path / "missing.npy"), str(tmp_path / "roi.npy"), str(tmp_path / "o")]) == 1
