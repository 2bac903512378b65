"""K11's outputs beyond the label, on the GPU, against scikit-learn (n_jobs=None) with exact equality: class probabilities,
confidence and labels of rsseg_forest_predict_proba, the out-of-bag sums of rsseg_forest_oob through fit_oob and
oob_estimate, the status codes, and the --confidence flag of the classification stage.

Each case names the kernel path it is there for and first asserts, on scikit-learn's objects alone, the condition that
puts it on that path.  The LDS-group kernel takes a forest whose every tree fits the node area beside the features,

    cap(F, TH) = min((160 KiB - 256 - (F | 1) * TH * 4 - 16) / 8, 12 * TH) & ~1      nodes,
    TH = 1024 threads when F <= 32 and classes <= 32, else 512,

and the general kernel takes the others; the vote rows are 4 / 8 / 16 / 32 / 64 doubles wide."""
import os
import sys
import warnings

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier

from test_forest_fit_host import state_equal
from test_forest_proba_host import flat_proba, int_data, sk_fit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 1023, 1025, 3001)


def lds_cap(F, C):
    th = 1024 if F <= 32 and C <= 32 else 512
    return min((160 * 1024 - 256 - (F | 1) * th * 4 - 16) // 8, 12 * th) & ~1


def mixed_leaves(model):
    """Leaves of the forest whose class fractions are not one-hot (they get rows of their own in the vote table)."""
    k = 0
    for e in model.estimators_:
        t = e.tree_
        v = t.value[t.children_left == -1, 0, :]
        k += int(((v != 0) & (v != 1)).any(axis=1).sum())
    return k


def largest_tree(model):
    return max(e.tree_.node_count for e in model.estimators_)


#        name     samples, F, classes, seed, values   forest settings                                    condition
CASES = {
    "tiny": ((33, 19, 3, 11, 16), dict(n_estimators=1, random_state=0),
             lambda m: largest_tree(m) <= lds_cap(19, 3)),
    "two": ((700, 3, 2, 17, 64), dict(n_estimators=2, random_state=0, max_depth=3),
            lambda m: bool((np.diff(np.sort(m.predict_proba(fresh_rows(3, 17, 64)), axis=1)[:, -2:], axis=1) == 0).any())),
    "nc16": ((1500, 4, 9, 13, 16), dict(n_estimators=5, random_state=0, max_depth=6),
             lambda m: mixed_leaves(m) > 0 and largest_tree(m) <= lds_cap(4, 9)),
    "deep": ((2000, 8, 5, 14, 4), dict(n_estimators=7, random_state=0, min_samples_leaf=3),
             lambda m: max(e.tree_.max_depth for e in m.estimators_) >= 10 and mixed_leaves(m) > 100
             and largest_tree(m) <= lds_cap(8, 5)),
    "genA": ((20000, 31, 3, 15, 16), dict(n_estimators=2, random_state=0),
             lambda m: lds_cap(31, 3) == 4574 and largest_tree(m) > 4574),
    "genB": ((9000, 6, 33, 16, 16), dict(n_estimators=5, random_state=0),
             lambda m: lds_cap(6, 33) == 6144 and largest_tree(m) > 6144),
}
_fitted = {}


def fresh_rows(F, seed, values=16):
    """3001 rows the forest has not seen; rows 0, 7, 64, 300, 1024 and 1500 carry NaN in two features and +-3e38 in a
    third (with one feature: NaN only), so that workgroups with and without a NaN both occur at every size above 1."""
    rs = np.random.RandomState(1000 + seed)
    X = rs.randint(0, values, (SIZES[-1], F)).astype(np.float32)
    for k, r in enumerate((0, 7, 64, 300, 1024, 1500)):
        X[r, k % F] = np.nan
        X[r, (k + 1) % F] = np.nan
        X[r, (k + 2) % F] = np.float32(3e38) if k % 2 else np.float32(-3e38)
    return X


def case_data(name):
    (n, F, C, seed, values), kw, cond = CASES[name]
    X, y = int_data(n, F, C, seed, values)
    return X, y, kw, cond, fresh_rows(F, seed, values)


def fitted(name):
    """scikit-learn's forest with oob_score=True (fitted once per case and never modified) and its warnings."""
    if name not in _fitted:
        X, y, kw, cond, _ = case_data(name)
        _fitted[name] = sk_fit(X, y, oob_score=True, **kw)
    return _fitted[name]


def planes_of(ctx, X):
    return [ctx.to_device(np.ascontiguousarray(X[:, f])) for f in range(X.shape[1])]


def check_outputs(ctx, Xn, want_proba, want_labels):
    """The three outputs over the prefixes of Xn against the oracle; single-output calls against the all-outputs call.
    The forest is loaded by the caller; want_labels are in the terms of its classes."""
    for n in SIZES:
        pl = planes_of(ctx, Xn[:n])
        proba, conf, lab = ctx.forest_predict_proba(pl, proba=True, confidence=True, labels=True)
        C = want_proba.shape[1]
        assert proba.shape == (C, n) and proba.dtype.is_floating_point and proba.element_size() == 8
        p = proba.cpu().numpy().T
        assert np.array_equal(p, want_proba[:n]), n
        assert np.array_equal(conf.cpu().numpy(), want_proba[:n].max(1)), n
        assert np.array_equal(lab.cpu().numpy(), want_labels[:n]), n
        assert np.array_equal(ctx.forest_predict(pl).cpu().numpy(), want_labels[:n]), n
        p1, c1, l1 = ctx.forest_predict_proba(pl)
        assert c1 is None and l1 is None and np.array_equal(p1.cpu().numpy(), proba.cpu().numpy()), n
        p2, c2, l2 = ctx.forest_predict_proba(pl, proba=False, confidence=True)
        assert p2 is None and l2 is None and np.array_equal(c2.cpu().numpy(), conf.cpu().numpy()), n
        p3, c3, l3 = ctx.forest_predict_proba(pl, proba=False, labels=True)
        assert p3 is None and c3 is None and np.array_equal(l3.cpu().numpy(), lab.cpu().numpy()), n


@pytest.mark.parametrize("name", list(CASES))
def test_predict_proba_equals_sklearn(ctx, name):
    from rsseg import forest as FO
    model, _ = fitted(name)
    X, y, kw, cond, Xn = case_data(name)
    assert cond(model), name
    want = model.predict_proba(Xn)
    ctx.forest_load(FO.flatten_forest(model))
    check_outputs(ctx, Xn, want, model.predict(Xn))
    got = FO.predict_proba(model, Xn[:1025].astype(np.float64), ctx=ctx)        # the host entry: float32 cast, (n, C)
    assert got.shape == (1025, len(model.classes_)) and got.dtype == np.float64 and np.array_equal(got, want[:1025])
    assert np.array_equal(FO.predict_proba(FO.flatten_forest(model), Xn[:7], ctx=ctx), want[:7])


def test_bundled_forest_equals_the_numpy_walk(ctx, golden_dir):
    """The reference's committed model on crop96's stack: 100 trees of at most 13 nodes, 3 classes -> 25 LDS groups of four
    trees, rows 4 wide.  The oracle is the NumPy walk of tests/test_forest_proba_host.py (checked there against
    scikit-learn's predict_proba)."""
    from rsseg import forest as FO
    flat = dict(np.load(os.path.join(golden_dir, "rf_samples_model_flat.npz")))
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    assert len(flat["tree_off"]) - 1 == 100 and flat["value"].shape[1] <= 4
    assert int(np.diff(flat["tree_off"]).max()) * 4 <= lds_cap(19, flat["value"].shape[1])
    stack = crop["stack19"].reshape(-1, 19)
    assert stack.shape[0] == 9216
    X = np.ascontiguousarray(stack[:9216 - 5], np.float32)
    want = flat_proba(flat, X)
    labels = np.asarray(flat["classes"])[np.argmax(want, axis=1)]
    ctx.forest_load(flat)
    proba, conf, lab = ctx.forest_predict_proba(planes_of(ctx, X), proba=True, confidence=True, labels=True)
    assert np.array_equal(proba.cpu().numpy().T, want)
    assert np.array_equal(conf.cpu().numpy(), want.max(1))
    assert np.array_equal(lab.cpu().numpy(), labels)
    assert np.array_equal(ctx.forest_predict(planes_of(ctx, X)).cpu().numpy(), labels)
    Xn = X[:3001].copy()
    Xn[[0, 7, 300, 1024], 3] = np.nan
    Xn[[0, 64, 1500], 11] = np.nan
    Xn[[7, 1500], 0] = np.float32(3e38)
    Xn[[0, 300], 5] = np.float32(-3e38)
    wn = flat_proba(flat, Xn)
    check_outputs(ctx, Xn, wn, np.asarray(flat["classes"])[np.argmax(wn, axis=1)])
    img = FO.predict_image_proba(flat, crop["stack19"], ctx=ctx)
    assert img.shape == (96, 96, want.shape[1]) and np.array_equal(img.reshape(-1, want.shape[1])[:len(X)], want)
    cm = FO.confidence_map(flat, crop["stack19"], ctx=ctx)
    assert cm.shape == (96, 96) and cm.dtype == np.float64 and np.array_equal(cm, img.max(-1))


@pytest.mark.parametrize("name", list(CASES))
def test_out_of_bag_equals_sklearn(ctx, name):
    from rsseg import forest as FO
    from rsseg.forest_fit import fit_oob
    want, msgs = fitted(name)
    X, y, kw, cond, _ = case_data(name)
    assert cond(want), name
    counts = np.stack([np.bincount(np.random.RandomState(e.random_state).randint(0, len(y), len(y)), minlength=len(y))
                       for e in want.estimators_])
    assert kw["n_estimators"] > 7 or ((counts > 0).all(axis=0).any() and len(msgs) == 1)    # the max(count, 1) branch
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = fit_oob(RandomForestClassifier(oob_score=True, **kw), X, y, ctx=ctx)
    assert [str(m.message) for m in w if issubclass(m.category, UserWarning)] == msgs
    state_equal(want, got)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        dec, score = FO.oob_estimate(want, X, y, ctx=ctx)
    assert [str(m.message) for m in w if issubclass(m.category, UserWarning)] == msgs
    assert np.array_equal(dec, want.oob_decision_function_) and score == want.oob_score_
    n_oob = ctx.forest_oob(planes_of(ctx, X), ctx.to_device(counts.reshape(-1), np.int32))[1].cpu().numpy()
    assert n_oob.dtype == np.int32 and np.array_equal(n_oob, (counts == 0).sum(axis=0))


def test_refusals_are_status_codes():
    """Every refusal is RSSEG_ERR_INVALID (-1) with a message, n == 0 is RSSEG_OK and writes nothing, and the context
    still answers correctly afterwards."""
    import ctypes as C
    import torch
    from rsseg import forest as FO
    from rsseg.runtime import Context
    c = Context(0, use_dist=False)
    try:
        lib, h = c.lib, c.h
        X, y, kw, _, Xn = case_data("two")
        model, _ = fitted("two")
        pl = planes_of(c, Xn[:100])
        n = 100
        proba = torch.full((2 * n,), -1.0, dtype=torch.float64, device=c.device)
        n_oob = torch.full((n,), -1, dtype=torch.int32, device=c.device)
        counts = torch.zeros(2 * n, dtype=torch.int32, device=c.device)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        err = lambda: lib.rsseg_last_error(h).decode()   # noqa: E731
        assert lib.rsseg_forest_predict_proba(h, c._pp(pl), 3, n, vp(proba), None, None) == -1 and "no forest loaded" in err()
        assert lib.rsseg_forest_oob(h, c._pp(pl), 3, n, vp(counts), vp(proba), vp(n_oob)) == -1 and "no forest loaded" in err()
        with pytest.raises(ValueError, match="no forest loaded"):
            c.forest_predict_proba(pl)
        c.forest_load(FO.flatten_forest(model))
        assert lib.rsseg_forest_predict_proba(h, c._pp(pl[:2]), 2, n, vp(proba), None, None) == -1 and "expecting 3 features" in err()
        assert lib.rsseg_forest_oob(h, c._pp(pl[:2]), 2, n, vp(counts), vp(proba), vp(n_oob)) == -1 and "expecting 3 features" in err()
        holed = [pl[0], None, pl[2]]
        assert lib.rsseg_forest_predict_proba(h, c._pp(holed), 3, n, vp(proba), None, None) == -1 and "plane 1 is null" in err()
        assert lib.rsseg_forest_oob(h, c._pp(holed), 3, n, vp(counts), vp(proba), vp(n_oob)) == -1 and "plane 1 is null" in err()
        assert lib.rsseg_forest_predict_proba(h, c._pp(pl), 3, n, None, None, None) == -1 and "output is null" in err()
        assert lib.rsseg_forest_oob(h, c._pp(pl), 3, n, None, vp(proba), vp(n_oob)) == -1 and "counts are null" in err()
        assert lib.rsseg_forest_oob(h, c._pp(pl), 3, n, vp(counts), None, vp(n_oob)) == -1 and "output is null" in err()
        with pytest.raises(ValueError, match="counts"):
            c.forest_oob(pl, counts[:n])                                        # one tree's counts for a forest of two
        assert lib.rsseg_forest_predict_proba(h, c._pp(pl), 3, 0, vp(proba), None, None) == 0
        assert lib.rsseg_forest_oob(h, c._pp(pl), 3, 0, vp(counts), vp(proba), vp(n_oob)) == 0
        c.sync()
        assert bool((proba == -1.0).all()) and bool((n_oob == -1).all())       # nothing was touched by any of the above
        got, conf, lab = c.forest_predict_proba(pl, confidence=True, labels=True)
        want = model.predict_proba(Xn[:n])
        assert np.array_equal(got.cpu().numpy().T, want) and np.array_equal(conf.cpu().numpy(), want.max(1))
        assert np.array_equal(lab.cpu().numpy(), model.predict(Xn[:n]))
    finally:
        c.close()


def test_stage_writes_confidence_and_probabilities(ctx, golden_dir, tmp_path):
    """python -m rsseg.stages <image> <out> --classify random_forest --confidence: the probability file equals
    predict_image_proba, the confidence files its maximum, and the label map is the one a run without the flag writes."""
    import joblib
    from rsseg import forest as FO
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain")]) == 0          # features only: a model to classify with
    allf = np.load(tmp_path / "plain" / "feature_outputs" / "all_hierarchical_features.npy")
    X = allf.reshape(-1, 19)
    rs = np.random.RandomState(3)
    idx = rs.choice(len(X), 500, replace=False)
    model = RandomForestClassifier(n_estimators=12, random_state=0).fit(X[idx], rs.randint(1, 5, 500))
    for d in ("plain", "conf"):
        os.makedirs(tmp_path / d / "segmentation_results", exist_ok=True)
        joblib.dump(model, tmp_path / d / "segmentation_results" / stages.RF_MODEL_FILE)
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain"), "--classify", "random_forest"]) == 0
    assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "conf"), "--classify", "random_forest", "--confidence"]) == 0
    plain, conf = tmp_path / "plain" / "segmentation_results", tmp_path / "conf" / "segmentation_results"
    assert sorted(os.listdir(plain)) == ["classification_random_forest.npy", "random_forest_classification_map.tif", stages.RF_MODEL_FILE]
    assert sorted(set(os.listdir(conf)) - set(os.listdir(plain))) == ["random_forest_confidence_map.tif", "rf_class_probabilities.npy",
                                                                       "rf_confidence.npy"]
    for name in ("classification_random_forest.npy", "random_forest_classification_map.tif"):
        assert (plain / name).read_bytes() == (conf / name).read_bytes(), name
    proba = np.load(conf / "rf_class_probabilities.npy")
    feats = np.nan_to_num(allf, nan=0.0)
    assert proba.shape == (96, 96, 4) and proba.dtype == np.float64
    assert np.array_equal(proba, FO.predict_image_proba(model, feats, ctx=ctx))
    assert np.array_equal(proba.reshape(-1, 4), model.predict_proba(feats.reshape(-1, 19)))
    cmap = np.load(conf / "rf_confidence.npy")
    assert cmap.shape == (96, 96) and np.array_equal(cmap, proba.max(-1))
    assert np.array_equal(cmap, FO.confidence_map(model, feats, ctx=ctx))
    tif = read_tiff(str(conf / "random_forest_confidence_map.tif"))
    assert tif.dtype == np.float64 and np.array_equal(tif[0], cmap)
    assert np.array_equal(np.load(conf / "classification_random_forest.npy"), model.predict(feats.reshape(-1, 19)).reshape(96, 96))
