"""The host side of the permutation importance (rsseg/forest_importance.py) against scikit-learn itself, without a GPU:
the random draws (permutation_plan) against what sklearn.inspection.permutation_importance hands its estimator, the finish
from integer counts against its Bunch, the refusals and their texts, and the declaration of the C entry point."""
import os
import re

import numpy as np
import pytest
from sklearn.base import BaseEstimator
from sklearn.ensemble import RandomForestClassifier
from sklearn.inspection import permutation_importance as sk_permutation_importance

from rsseg import _lib as L
from rsseg import forest_importance as FI
from rsseg.runtime import RssegUnsupported
from test_forest_proba_host import HostContext, flat_proba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder(BaseEstimator):
    """Keeps a copy of every (X, y) it is asked to score."""

    def __init__(self):
        self.seen = []

    def fit(self, X, y):
        return self

    def predict(self, X):
        self.seen.append((np.array(X, copy=True), None))
        return np.zeros(len(X))

    def score(self, X, y):
        self.seen.append((np.array(X, copy=True), np.array(y, copy=True)))
        return 0.0


def data(n, F, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, F)
    X[rs.rand(n, F) < 0.1] = np.nan
    return X, rs.randint(0, 3, n)


def seeds():
    return [0, 42, np.random.RandomState(7)]


@pytest.mark.parametrize("n", [1, 2, 33, 257])
@pytest.mark.parametrize("which", ["1.0", "0.5", "int<n", "n"])
def test_plan_equals_what_sklearn_hands_its_estimator(n, which):
    F, R = 3, 3
    X, y = data(n, F, 100 + n)
    # scikit-learn takes integers from 1: with one sample there is no integer below n, and 0.5 scores on no row at all
    max_samples = {"1.0": 1.0, "0.5": 0.5, "int<n": max(n // 2, 1), "n": n}[which]
    for k, seed in enumerate(seeds()):
        rec = Recorder()
        sk_permutation_importance(rec, X, y, n_repeats=R, random_state=seed, max_samples=max_samples)
        rows, sources = FI.permutation_plan(n, R, seeds()[k], max_samples)       # a RandomState instance: a fresh one, same state
        m = max_samples if which in ("int<n", "n") else int(max_samples * n)
        assert len(rows) == m and sources.shape == (R, m) and sources.dtype == np.int32
        if m == n:
            assert np.array_equal(rows, np.arange(n))
        assert len(rec.seen) == 1 + F * R
        assert np.array_equal(rec.seen[0][0], X, equal_nan=True) and np.array_equal(rec.seen[0][1], y)      # the baseline: all rows
        for f in range(F):
            for r in range(R):
                Xs, ys = rec.seen[1 + f * R + r]
                want = X[rows].copy()
                want[:, f] = X[rows][sources[r], f]
                assert np.array_equal(Xs, want, equal_nan=True), (seed, f, r)
                assert np.array_equal(ys, y[rows]), (seed, f, r)


def test_plan_resolves_max_samples_as_sklearn_does():
    with pytest.raises(ValueError, match="^max_samples must be <= n_samples$"):
        FI.permutation_plan(10, 2, 0, 11)
    assert FI.permutation_plan(10, 2, 0, 0.99)[1].shape == (2, 9)     # int(0.99 * 10)
    assert FI.permutation_plan(10, 2, 0, np.int64(10))[1].shape == (2, 10)
    rows, _ = FI.permutation_plan(300, 1, 0, 100)
    assert len(set(rows.tolist())) == 100 and not np.array_equal(rows, np.sort(rows))


def small_forest(strings):
    rs = np.random.RandomState(5)
    X = rs.randint(0, 8, (120, 4)).astype(np.float64)
    y = (X[:, 0] + X[:, 2] > 7).astype(int) + (X[:, 1] > 5)
    X[rs.rand(*X.shape) < 0.05] = np.nan
    if strings:
        y = np.asarray(["bare", "crop", "water"])[y]
    return RandomForestClassifier(n_estimators=7, random_state=0).fit(X, y), X, y


def host_importance(model, X, y, **kw):
    index = lambda Xp: np.searchsorted(model.classes_, model.predict(Xp))   # noqa: E731
    return FI._importance(model.classes_, model.n_features_in_, X, y, kw.get("n_repeats", 5), kw.get("random_state"),
                          kw.get("max_samples", 1.0), FI.host_counts(index))[0]


def bunch_equal(got, want):
    assert sorted(want) == ["importances", "importances_mean", "importances_std"]
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("strings", [False, True])
@pytest.mark.parametrize("max_samples", [1.0, 0.5, 100])
def test_finish_equals_sklearn(strings, max_samples):
    model, Xtr, ytr = small_forest(strings)
    rs = np.random.RandomState(9)
    X = rs.randint(0, 8, (257, 4)).astype(np.float64)
    X[rs.rand(*X.shape) < 0.05] = np.nan
    y = model.predict(X)
    y[::5] = model.classes_[(np.searchsorted(model.classes_, y[::5]) + 1) % 3]
    y = y.astype(object) if strings else y
    y[3] = "never seen" if strings else 77                      # a label absent from classes_
    y = np.asarray(y.tolist())
    for seed in (0, 42):
        want = sk_permutation_importance(model, X, y, n_repeats=3, random_state=seed, max_samples=max_samples)
        got = host_importance(model, X, y, n_repeats=3, random_state=seed, max_samples=max_samples)
        bunch_equal(got, want)
        assert (want["importances"] != 0).any()


def test_one_sample_has_importance_zero():
    model, X, y = small_forest(True)
    want = sk_permutation_importance(model, X[:1], y[:1], n_repeats=4, random_state=0)
    got = host_importance(model, X[:1], y[:1], n_repeats=4, random_state=0)
    bunch_equal(got, want)
    assert np.array_equal(got["importances"], np.zeros((4, 4)))


class HostPermContext(HostContext):
    """HostContext with rsseg_forest_permutation_counts restated on the flattened forest (first maximum of the float64 sums)."""

    def forest_permutation_counts(self, planes, y, src, jobs):
        X = np.stack([p.a for p in planes], 1)
        S = None if src is None else src.a.reshape(-1, len(X))
        if S is not None and ((S < 0) | (S >= len(X))).any():
            raise ValueError("forest_permutation_counts: source index out of range")
        return FI.host_counts(lambda Xp: np.argmax(flat_proba(self.flat, Xp), axis=1))(X, y.a, S, jobs)


@pytest.mark.parametrize("as_dict", [False, True])
def test_whole_call_on_a_host_context(as_dict):
    """permutation_importance itself (label encoding, float32 cast, row gather, one call when m == n and two otherwise)
    with the device call replaced by its restatement."""
    from rsseg.forest import flatten_forest
    model, X, y = small_forest(True)
    y = y.copy()
    y[::4] = "never seen"
    for max_samples, calls in ((1.0, 4 + 2), (60, 4 + 1 + 4 + 2)):
        want = sk_permutation_importance(model, X, y, n_repeats=3, random_state=42, max_samples=max_samples)
        c = HostPermContext()
        got = FI.permutation_importance(flatten_forest(model) if as_dict else model, X, y, n_repeats=3, n_jobs=16, random_state=42,
                                        max_samples=max_samples, ctx=c)
        bunch_equal(got, want)
        assert c.uploads == calls           # planes, y and the source rows: once per set of rows, not per job
    model, X, _ = small_forest(False)                  # classes 0, 1, 2; the mask labels 1, 2 and 3
    mask = (np.arange(120) % 4).reshape(10, 12)
    img = FI.permutation_importance_image(model, X.reshape(10, 12, 4), mask, n_repeats=2, random_state=0, ctx=HostPermContext())
    sel = mask.reshape(-1) > 0
    Xs, ys = np.nan_to_num(X[sel], nan=0.0), mask.reshape(-1)[sel]
    want = sk_permutation_importance(model, Xs, ys, n_repeats=2, random_state=0)
    assert img["n_samples"] == 90 and img["baseline_score"] == model.score(Xs, ys)
    bunch_equal({k: img[k] for k in want}, want)


def test_labels_are_encoded_against_classes():
    assert FI.encode_labels(np.array([2, 5, 9]), np.array([9, 2, 3, 5.0, -1])).tolist() == [2, 0, -1, 1, -1]
    assert FI.encode_labels(np.array(["a", "c"]), np.array(["c", "b", "a"])).tolist() == [1, -1, 0]
    assert FI.encode_labels(np.array(["a", "c"]), np.array([1, 2])).tolist() == [-1, -1]
    assert FI.encode_labels(np.array([1]), np.array([], dtype=int)).dtype == np.int32
    jobs = FI.importance_jobs(3, 2)
    assert jobs["feature"].tolist() == [0, 0, 1, 1, 2, 2] and jobs["source"].tolist() == [0, 1, 0, 1, 0, 1]


def test_refusals_name_the_argument():
    from sklearn.cluster import KMeans
    model, X, y = small_forest(False)
    with pytest.raises(RssegUnsupported, match="scoring='f1'"):
        FI.permutation_importance(model, X, y, scoring="f1")
    with pytest.raises(RssegUnsupported, match="sample_weight"):
        FI.permutation_importance(model, X, y, sample_weight=np.ones(len(y)))
    with pytest.raises(RssegUnsupported, match="model: KMeans"):
        FI.permutation_importance(KMeans(2, n_init=1, random_state=0).fit(np.nan_to_num(X)), X, y)
    multi = RandomForestClassifier(n_estimators=2, random_state=0).fit(np.nan_to_num(X), np.stack([y, y], axis=1))
    with pytest.raises(RssegUnsupported, match="model: multi-output forest"):
        FI.permutation_importance(multi, X, y)
    with pytest.raises(ValueError, match=r"^X has 3 features, but the forest is expecting 4 features as input\.$"):
        FI.permutation_importance(model, X[:, :3], y)
    with pytest.raises(ValueError, match="^max_samples must be <= n_samples$"):
        FI.permutation_importance(model, X, y, max_samples=len(y) + 1)
    with pytest.raises(RssegUnsupported, match="scoring"):
        FI.permutation_importance_image(model, X.reshape(10, 12, 4), np.ones((10, 12), np.int32), scoring="f1")


def test_stage_flag_needs_the_forest():
    from rsseg import stages
    ap = stages.build_parser()
    with pytest.raises(SystemExit):
        stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans", "--importance", "mask.npy"])
    with pytest.raises(SystemExit):
        stages.parse_args(ap, ["in.tif", "out", "--importance", "mask.npy"])
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "random_forest", "--importance", "mask.npy"])
    assert a.importance == "mask.npy"
    assert stages.parse_args(ap, ["in.tif", "out", "--classify", "random_forest"]).importance is None
    import inspect
    params = list(inspect.signature(stages.run_scripts_2_3).parameters.values())
    assert params[-1].name == "importance" and params[-1].default is None


def test_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    m = re.search(r"int rsseg_forest_permutation_counts\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 10
    assert re.search(r"typedef struct rsseg_perm_job \{\s*int32_t feature;\s*int32_t source;\s*\} rsseg_perm_job;", hdr)
    res, args = L.SIGNATURES["rsseg_forest_permutation_counts"]
    assert len(args) == 10
    dt = np.dtype(L.PERM_JOB)
    assert dt.itemsize == 8 and dt.names == ("feature", "source") and dt.fields["source"][1] == 4
    assert hasattr(L.load(), "rsseg_forest_permutation_counts")
