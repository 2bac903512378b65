"""Permutation importance on the GPU (rsseg_forest_permutation_counts, rsseg/forest_importance.py) against
sklearn.inspection.permutation_importance (n_jobs=None) with exact equality: the six forests of tests/test_gpu_forest_proba.py
(one per kernel path, each asserting its own path condition first), the row subsample of max_samples, a NaN carried by the
substitution into a workgroup that holds none of its own, the status codes, the image function and the stage's flag."""
import json
import os

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier
from sklearn.inspection import permutation_importance as sk_permutation_importance

from rsseg import forest_importance as FI
from test_forest_proba_host import int_data, sk_fit
from test_gpu_forest_proba import CASES, SIZES, case_data, fitted, fresh_rows, largest_tree, lds_cap, planes_of

pytestmark = pytest.mark.gpu
REPEATS = 2
BUNCH = ("importances", "importances_mean", "importances_std")


def bunch_equal(got, want, what):
    for k in BUNCH:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)


def scored_labels(model, Xn):
    """The model's own prediction with every fifth row moved to the next class and row 2 given a label outside classes_:
    a baseline that is neither 0 nor 1."""
    y = model.predict(Xn).copy()
    idx = np.searchsorted(model.classes_, y)
    y[::5] = model.classes_[(idx[::5] + 1) % len(model.classes_)]
    y[2] = model.classes_.max() + 7
    return y


def load(ctx, model):
    from rsseg import forest as FO
    ctx.forest_load(FO._flat_for_proba(model))


def permuted(X, rows, sources, f, r):
    Xp = X[rows].copy()
    Xp[:, f] = X[rows][sources[r], f]
    return Xp


@pytest.mark.parametrize("name", list(CASES))
def test_importance_equals_sklearn(ctx, name):
    model, _ = fitted(name)
    X, _, kw, cond, Xn = case_data(name)
    assert cond(model), name
    y = scored_labels(model, Xn)
    F = Xn.shape[1]
    for n in SIZES:
        for seed in (0, 42):
            want = sk_permutation_importance(model, Xn[:n], y[:n], n_repeats=REPEATS, random_state=seed)
            got = FI.permutation_importance(model, Xn[:n], y[:n], n_repeats=REPEATS, random_state=seed, ctx=ctx)
            assert sorted(got) == sorted(BUNCH)
            bunch_equal(got, want, (name, n, seed))
    # the raw counts: the baseline and three jobs picked by a fixed rule, against model.predict on the permuted matrix
    n = SIZES[-1]
    base = float((model.predict(Xn) == y).mean())
    assert 0.0 < base < 1.0
    rows, sources = FI.permutation_plan(n, REPEATS, 0, 1.0)
    picks = [(-1, 0), (0, 0), (F - 1, REPEATS - 1), (F // 2, 1 % REPEATS)]
    load(ctx, model)
    got = ctx.forest_permutation_counts(planes_of(ctx, Xn), ctx.to_device(FI.encode_labels(model.classes_, y), np.int32),
                                        ctx.to_device(sources.reshape(-1), np.int32), np.array(picks, np.dtype(FI.L.PERM_JOB)))
    want = [int((model.predict(Xn if f < 0 else permuted(Xn, rows, sources, f, r)) == y).sum()) for f, r in picks]
    assert got.dtype == np.int64 and got.tolist() == want
    again = ctx.forest_permutation_counts(planes_of(ctx, Xn), ctx.to_device(FI.encode_labels(model.classes_, y), np.int32),
                                          ctx.to_device(sources.reshape(-1), np.int32), np.array(picks, np.dtype(FI.L.PERM_JOB)))
    assert again.tolist() == want                   # the same from run to run


_wide = {}


def wide_forest():
    """A seventh path, the permutation kernels' own: 20 classes (rows 32 wide) at 1024 threads with a tree larger than the
    LDS area -> the general kernel, which at that width fetches the next four trees' nodes behind the barrier instead of
    holding them in registers across the walk; five trees, so that the fetch happens."""
    if not _wide:
        X, y = int_data(12000, 6, 20, 18, 16)
        _wide["model"] = sk_fit(X, y, n_estimators=5, random_state=0)[0]
    return _wide["model"]


def test_wide_rows_general_kernel_equals_sklearn(ctx):
    model = wide_forest()
    assert len(model.classes_) == 20 and lds_cap(6, 20) == 12288 and largest_tree(model) > 12288
    Xn = fresh_rows(6, 18, 16)
    y = scored_labels(model, Xn)
    for n in (1025, 3001):
        want = sk_permutation_importance(model, Xn[:n], y[:n], n_repeats=REPEATS, random_state=42)
        got = FI.permutation_importance(model, Xn[:n], y[:n], n_repeats=REPEATS, random_state=42, ctx=ctx)
        bunch_equal(got, want, ("wide", n))
    assert (want["importances"] != 0).any()


@pytest.mark.parametrize("name", ["deep", "genB"])
@pytest.mark.parametrize("max_samples", [0.5, 1025])
def test_row_subsample_equals_sklearn(ctx, name, max_samples):
    model, _ = fitted(name)
    Xn = case_data(name)[4]
    y = scored_labels(model, Xn)
    rows, _ = FI.permutation_plan(len(Xn), REPEATS, 42, max_samples)
    assert len(rows) == (1500 if max_samples == 0.5 else 1025) and not np.array_equal(rows, np.sort(rows))
    want = sk_permutation_importance(model, Xn, y, n_repeats=REPEATS, random_state=42, max_samples=max_samples)
    got = FI.permutation_importance(model, Xn, y, n_repeats=REPEATS, random_state=42, max_samples=max_samples, ctx=ctx)
    bunch_equal(got, want, (name, max_samples))
    assert (want["importances"] != 0).any()


# ---- the NaN seam ------------------------------------------------------------------------------------------------------------
SEAM_ROWS = 2049
SEAM_SEED = 0        # permutation_importance(random_state=0): the shuffles checked below carry the NaN where the test needs it


def seam_data(name, nan_rows, feature):
    (_, F, _, seed, values), _, _ = CASES[name]
    X = np.random.RandomState(2000 + seed).randint(0, values, (SEAM_ROWS, F)).astype(np.float32)
    X[list(nan_rows), feature] = np.nan
    return X


def used_features(model):
    return sorted(set(int(f) for e in model.estimators_ for f in e.tree_.feature if f >= 0))


@pytest.mark.parametrize("name, th, nan_rows", [("deep", 1024, (2048,)), ("genA", 1024, (2048,)), ("genB", 512, (2047, 2048))])
def test_nan_carried_into_a_workgroup_without_one(ctx, name, th, nan_rows):
    """Rows 0 .. 2047 - (th == 512) hold no NaN; the last workgroup's do, in one feature.  Repeat 0 of seed SEAM_SEED puts
    that NaN into a row of an earlier workgroup, whose walk must then be the NaN-aware one: the feature is chosen, on
    scikit-learn's trees alone, so that a walk that sends the NaN left at every node (which is what the plain walk does
    with it: NaN > threshold is false) labels that row differently, and y holds the right label there, so the count of
    that job is one less when the kernel chooses the walk from the workgroup's own rows."""
    model, _ = fitted(name)
    (_, F, C, _, _), _, cond = CASES[name]
    assert cond(model) and (1024 if F <= 32 and C <= 32 else 512) == th
    rows, sources = FI.permutation_plan(SEAM_ROWS, REPEATS, SEAM_SEED, 1.0)
    clean_end = min(nan_rows) // th * th                    # rows [0, clean_end) lie in workgroups without a NaN of their own
    land = [i for i in range(clean_end) if int(sources[0][i]) in nan_rows]
    assert land, "seed %d does not carry the NaN into an earlier workgroup" % SEAM_SEED
    i = land[0]
    chosen = None
    for f in used_features(model):
        X = seam_data(name, nan_rows, f)
        row = X[i:i + 1].copy()
        row[0, f] = np.nan
        left = row.copy()
        left[0, f] = np.float32(-3e38)                      # below every threshold of these forests: left at every node
        if model.predict(row)[0] != model.predict(left)[0]:
            chosen = f
            break
    assert chosen is not None, "no feature whose NaN-aware walk labels the row differently"
    X = seam_data(name, nan_rows, chosen)
    assert not np.isnan(X[:clean_end]).any() and np.isnan(X[list(nan_rows), chosen]).all()
    y = scored_labels(model, X)
    y[i] = model.predict(permuted(X, rows, sources, chosen, 0)[i:i + 1])[0]
    want = sk_permutation_importance(model, X, y, n_repeats=REPEATS, random_state=SEAM_SEED)
    got = FI.permutation_importance(model, X, y, n_repeats=REPEATS, random_state=SEAM_SEED, ctx=ctx)
    assert np.array_equal(got["importances"][chosen], want["importances"][chosen])
    bunch_equal(got, want, name)


def test_nan_in_an_unused_feature_changes_nothing(ctx):
    """The same rows with the NaN in a feature no tree splits on (the one-tree forest `tiny` leaves most of its 19 unused;
    `deep` and `genA` use every feature): its importance is exactly 0.0, and everything equals scikit-learn's."""
    model, _ = fitted("tiny")
    unused = [f for f in range(19) if f not in used_features(model)]
    assert unused
    X = seam_data("tiny", (2048,), unused[0])
    _, sources = FI.permutation_plan(SEAM_ROWS, REPEATS, SEAM_SEED, 1.0)
    assert any(int(sources[0][i]) == 2048 for i in range(2048))
    y = scored_labels(model, X)
    want = sk_permutation_importance(model, X, y, n_repeats=REPEATS, random_state=SEAM_SEED)
    got = FI.permutation_importance(model, X, y, n_repeats=REPEATS, random_state=SEAM_SEED, ctx=ctx)
    bunch_equal(got, want, "tiny")
    assert np.array_equal(got["importances"][unused[0]], np.zeros(REPEATS)) and got["importances_std"][unused[0]] == 0.0


# ---- status codes ----------------------------------------------------------------------------------------------------------
def test_refusals_are_status_codes():
    """Every refusal is RSSEG_ERR_INVALID (-1) with a message and leaves `counts` alone, n == 0 and n_jobs == 0 are
    RSSEG_OK, and the context still answers correctly afterwards."""
    import ctypes as C
    import torch
    from rsseg.runtime import Context
    c = Context(0, use_dist=False)
    try:
        lib, h = c.lib, c.h
        model, _ = fitted("two")
        Xn = case_data("two")[4]
        n = 100
        long = [c.to_device(np.ascontiguousarray(Xn[:2 * n, f])) for f in range(3)]      # planes twice as long as the call says
        pl = [t[:n] for t in long]
        y = FI.encode_labels(model.classes_, scored_labels(model, Xn)[:n])
        d_y = c.to_device(y, np.int32)
        src = np.stack([np.arange(n)[::-1], np.roll(np.arange(n), 3)]).astype(np.int32)
        d_src = c.to_device(src.reshape(-1), np.int32)
        jobs = np.array([(-1, 0), (0, 0), (2, 1)], np.dtype(FI.L.PERM_JOB))
        counts = np.full(3, -7, np.int64)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        err = lambda: lib.rsseg_last_error(h).decode()   # noqa: E731

        def call(planes=pl, F=3, nn=n, yy=d_y, ss=d_src, n_src=2, jj=jobs, n_jobs=None, out=counts):
            return lib.rsseg_forest_permutation_counts(h, c._pp(planes), F, nn, None if yy is None else vp(yy), None if ss is None else vp(ss),
                                                       n_src, None if jj is None else jj.ctypes.data_as(C.c_void_p),
                                                       len(jobs) if n_jobs is None else n_jobs,
                                                       None if out is None else out.ctypes.data_as(C.POINTER(C.c_int64)))
        assert call() == -1 and "forest_permutation_counts: no forest loaded" in err()
        with pytest.raises(ValueError, match="no forest loaded"):
            c.forest_permutation_counts(pl, d_y, d_src, jobs)
        load(c, model)
        assert call(planes=pl[:2], F=2) == -1 and "X has 2 features, but the forest is expecting 3 features as input" in err()
        assert call(planes=[pl[0], None, pl[2]]) == -1 and "plane 1 is null" in err()
        assert call(yy=None) == -1 and "labels are null" in err()
        assert call(jj=None) == -1 and "jobs are null" in err()
        assert call(out=None) == -1 and "counts are null" in err()
        assert call(ss=None) == -1 and "source rows are null, but job 1 substitutes feature 0" in err()
        assert call(jj=np.array([(-1, 0), (3, 0), (2, 1)], jobs.dtype)) == -1 and "job 1 has feature 3 outside [-1, 3)" in err()
        assert call(jj=np.array([(-2, 0), (0, 0), (2, 1)], jobs.dtype)) == -1 and "job 0 has feature -2 outside [-1, 3)" in err()
        assert call(jj=np.array([(-1, 9), (0, 0), (2, 2)], jobs.dtype)) == -1 and "job 2 has source 2 outside [0, 2)" in err()
        assert call(jj=np.array([(-1, 0), (0, -1), (2, 1)], jobs.dtype)) == -1 and "job 1 has source -1 outside [0, 2)" in err()
        assert call(nn=1 << 31) == -1 and "2147483648 samples exceed 2^31 - 1" in err()
        bad = src.copy()
        bad[1, 40] = n                                   # one past the call's rows; the tensors behind the planes are 2 n long
        assert call(ss=c.to_device(bad.reshape(-1), np.int32)) == -1 and "source index out of range [0, 100)" in err()
        bad[1, 40] = -1
        assert call(ss=c.to_device(bad.reshape(-1), np.int32)) == -1 and "source index out of range" in err()
        with pytest.raises(ValueError, match="source index out of range"):
            c.forest_permutation_counts(pl, d_y, c.to_device(bad.reshape(-1), np.int32), jobs)
        assert counts.tolist() == [-7, -7, -7]           # untouched by every refusal
        assert call(n_jobs=0) == 0 and counts.tolist() == [-7, -7, -7]
        assert call(nn=0) == 0 and counts.tolist() == [0, 0, 0]
        assert call(ss=None, n_src=0, jj=jobs[:1], n_jobs=1) == 0            # the baseline alone needs no source rows
        got = c.forest_permutation_counts(pl, d_y, d_src, jobs)
        X = Xn[:n]
        want = [int((np.searchsorted(model.classes_, model.predict(Xp)) == y).sum())
                for Xp in (X, permuted(X, np.arange(n), src, 0, 0), permuted(X, np.arange(n), src, 2, 1))]
        assert got.tolist() == want and counts[0] == want[0]
    finally:
        c.close()


# ---- the image function and the stage ----------------------------------------------------------------------------------------
def stage_setup(golden_dir, tmp_path):
    """As test_stage_writes_confidence_and_probabilities: features from the stage on a 96 x 96 crop, a 12-tree forest, and
    a seeded mask of 500 labelled pixels, one of them a pixel with a NaN feature."""
    from rsseg import stages
    from rsseg.tiff import write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain")]) == 0
    allf = np.load(tmp_path / "plain" / "feature_outputs" / "all_hierarchical_features.npy").copy()
    rs = np.random.RandomState(3)
    idx = rs.choice(96 * 96, 500, replace=False)
    X = allf.reshape(-1, 19)
    model = RandomForestClassifier(n_estimators=12, random_state=0).fit(np.nan_to_num(X[idx], nan=0.0), rs.randint(1, 5, 500))
    mask = np.zeros(96 * 96, np.int32)
    pick = rs.choice(96 * 96, 500, replace=False)
    mask[pick] = rs.randint(1, 6, 500)                  # label 5 is not among the forest's classes
    return model, allf, mask.reshape(96, 96), pick


def test_image_importance_equals_sklearn(ctx, golden_dir, tmp_path):
    model, allf, mask, pick = stage_setup(golden_dir, tmp_path)
    allf[pick[0] // 96, pick[0] % 96, 4] = np.nan
    sel = mask > 0
    X, y = np.nan_to_num(allf[sel], nan=0.0), mask[sel]
    assert sel.sum() == 500 and np.isnan(allf[sel]).any() and 5 in y
    want = sk_permutation_importance(model, X, y, n_repeats=5, random_state=42)
    got = FI.permutation_importance_image(model, allf, mask, n_repeats=5, random_state=42, ctx=ctx)
    bunch_equal(got, want, "image")
    assert got["n_samples"] == 500 and got["baseline_score"] == model.score(X, y) and 0.0 < got["baseline_score"] < 1.0
    assert got["importances"].shape == (19, 5)


def test_stage_writes_the_importance(ctx, golden_dir, tmp_path):
    """python -m rsseg.stages <image> <out> --classify random_forest --importance mask.npy: the JSON equals the function's
    result, and every other file of segmentation_results is byte-identical to a run without the flag."""
    import joblib
    from rsseg import stages
    model, allf, mask, _ = stage_setup(golden_dir, tmp_path)
    np.save(tmp_path / "mask.npy", mask)
    for d in ("plain", "imp"):
        os.makedirs(tmp_path / d / "segmentation_results", exist_ok=True)
        joblib.dump(model, tmp_path / d / "segmentation_results" / stages.RF_MODEL_FILE)
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain"), "--classify", "random_forest"]) == 0
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "imp"), "--classify", "random_forest", "--importance",
                        str(tmp_path / "mask.npy")]) == 0
    plain, imp = tmp_path / "plain" / "segmentation_results", tmp_path / "imp" / "segmentation_results"
    assert sorted(set(os.listdir(imp)) - set(os.listdir(plain))) == ["rf_permutation_importance.json"]
    for name in os.listdir(plain):
        if name != stages.RF_MODEL_FILE:                # the model file is the test's own
            assert (plain / name).read_bytes() == (imp / name).read_bytes(), name
    for sub in ("feature_outputs",):
        for name in os.listdir(tmp_path / "plain" / sub):
            if not name.endswith(".pkl"):
                assert (tmp_path / "plain" / sub / name).read_bytes() == (tmp_path / "imp" / sub / name).read_bytes(), name
    js = json.load(open(imp / "rf_permutation_importance.json"))
    want = FI.permutation_importance_image(model, allf, mask, n_repeats=5, random_state=42, ctx=ctx)
    assert js["feature_names"] == [f"hierarchical_feature_{i + 1}" for i in range(19)]
    assert js["n_repeats"] == 5 and js["random_state"] == 42 and js["n_samples"] == 500
    assert js["baseline_score"] == want["baseline_score"]
    for k in BUNCH:
        assert np.array_equal(np.asarray(js[k]), want[k]), k
