"""rsseg.forest_grid without a GPU: the job table of a grid search (count rows per fold, shared across the candidates of a fold,
weight_total, seeds, parameters resolved on the fold's training size, node capacities), the zero-count argument behind it
(the NumPy restatement of K16 on all rows with scattered counts equals scikit-learn's fit on the subset), the formatting of
cv_results_ against GridSearchCV's own, the refusals, and the mirror's signature.

tests/golden/supervised_classifiers_names.json holds identifiers only: module_public_names and module_signatures of
oracle/gen_names.py over the reference's modules/supervised_classifiers.py, made as tests/test_preprocess_host.py describes
for its own fixture.
"""
import inspect
import json
import os
import warnings

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier
from sklearn.model_selection import GridSearchCV, ParameterGrid, check_cv

import forest_fit_cases as K
import forest_fit_ref as R
from test_forest_fit_host import tie_heavy

from rsseg import forest_fit as FF
from rsseg import forest_grid as G
from rsseg.runtime import RssegUnsupported


def folds_of(X, y, cv=3):
    return [(tr, te) for tr, te in check_cv(cv, y, classifier=True).split(X, y)]


def assert_results_equal(want: dict, got: dict):
    """cv_results_ of GridSearchCV against format_results': every key but the four time keys, floats bitwise, the param_*
    masked arrays by data, mask and dtype; the same keys in the same order."""
    assert list(want) == list(got)
    for k in want:
        if k in G.TIME_KEYS:
            continue
        a, b = want[k], got[k]
        if k == "params":
            assert a == b
        elif isinstance(a, np.ma.MaskedArray):
            assert isinstance(b, np.ma.MaskedArray) and a.dtype == b.dtype, (k, a.dtype, b.dtype)
            assert np.array_equal(np.ma.getmaskarray(a), np.ma.getmaskarray(b)), k
            assert a.tolist() == b.tolist(), k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype)
            assert a.tobytes() == b.tobytes(), (k, a, b)


def assert_search_equal(want, got):
    """A fitted GridSearchCV against a GridSearchResult (without the best estimator)."""
    assert_results_equal(want.cv_results_, got.cv_results_)
    assert want.best_index_ == got.best_index_
    assert want.best_params_ == got.best_params_
    assert np.float64(want.best_score_).tobytes() == np.float64(got.best_score_).tobytes()
    assert want.n_splits_ == got.n_splits_


# ---- the job table ------------------------------------------------------------------------------------------------------
def problem_601():
    X, _ = tie_heavy(601, F=8, C=3, seed=4)
    y = np.arange(601) % 3
    return X, y


def test_job_table_of_uneven_folds():
    X, y = problem_601()
    folds = folds_of(X, y)
    n_train = [len(tr) for tr, _ in folds]
    assert sorted(n_train) == [400, 401, 401] and sum(len(te) for _, te in folds) == 601   # uneven: weight_total differs per fold
    grid = {"n_estimators": [5], "max_depth": [2, 7, None], "min_samples_leaf": [0.01], "random_state": [42]}
    cand = list(ParameterGrid(grid))
    t = G.job_table(RandomForestClassifier(), cand, folds, y.astype(np.int32), 8, 3)
    jobs = t["jobs"]
    assert len(jobs) == 3 * 3 * 5 and len(t["forests"]) == 9
    # rows: one per fold and tree seed, shared by the three depth candidates
    assert len(t["rows"]) == 3 * 5
    seeds = FF.tree_seeds(42, 5)
    for f in t["forests"]:
        tr, te = folds[f["fold"]]
        p = cand[f["candidate"]]
        j = jobs[f["start"]:f["stop"]]
        assert f["n_train"] == len(tr) and np.all(j["weight_total"] == len(tr))
        assert np.array_equal(t["tree_seed"][f["start"]:f["stop"]], seeds)
        assert np.array_equal(j["seed"], [FF.splitter_seed(int(s)) for s in seeds])
        assert np.all(j["max_depth"] == (np.iinfo(np.int32).max if p["max_depth"] is None else p["max_depth"]))
        # the float min_samples_leaf resolves against the fold's training size (ceil(0.01 * 401) = 5, ceil(0.01 * 400) = 4), not n (7)
        msl = 5 if len(tr) == 401 else 4
        assert np.all(j["min_samples_leaf"] == msl) and np.all(j["min_samples_split"] == 2 * msl)
        assert np.all(j["max_features"] == 2)       # sqrt(8)
        for i, s in enumerate(seeds):
            row = t["rows"][j["counts_row"][i]]
            assert row.dtype == np.int32 and row.shape == (601,)
            assert int(row.sum()) == len(tr) and not row[te].any()
            assert np.array_equal(row[tr], FF.bootstrap_counts(int(s), len(tr)))
            assert t["caps"][f["start"] + i] == 2 * np.count_nonzero(row) - 1
    # the depth candidates of a fold name the same rows
    by_fold = {}
    for f in t["forests"]:
        by_fold.setdefault(f["fold"], []).append(tuple(jobs["counts_row"][f["start"]:f["stop"]]))
    assert all(len(set(v)) == 1 and len(v) == 3 for v in by_fold.values())
    assert len({r for v in by_fold.values() for r in v[0]}) == 15
    # forests are ordered fold-major: forests that share rows are neighbours
    assert [f["fold"] for f in t["forests"]] == [0, 0, 0, 1, 1, 1, 2, 2, 2]


def test_job_table_without_bootstrap_has_one_membership_row_per_fold():
    X, y = problem_601()
    folds = folds_of(X, y)
    t = G.job_table(RandomForestClassifier(bootstrap=False), [{"n_estimators": 4, "random_state": 1}], folds, y.astype(np.int32), 8, 3)
    assert len(t["rows"]) == 3
    for f in t["forests"]:
        tr, te = folds[f["fold"]]
        rows = set(t["jobs"]["counts_row"][f["start"]:f["stop"]].tolist())
        assert len(rows) == 1
        row = t["rows"][rows.pop()]
        assert np.all(row[tr] == 1) and not row[te].any()
        assert np.all(t["caps"][f["start"]:f["stop"]] == 2 * len(tr) - 1)


def test_calls_within_a_byte_budget_hold_whole_forests():
    X, y = problem_601()
    t = G.job_table(RandomForestClassifier(), [{"n_estimators": 5, "random_state": 0, "max_depth": d} for d in (2, None)], folds_of(X, y),
                    y.astype(np.int32), 8, 3)
    assert G.plan_calls(t, 601, 3, G.DEFAULT_MAX_BYTES) == [list(range(6))]
    one = G.forest_bytes(t, t["forests"][0], 3)[0] + 4 * 601 * 5
    assert G.plan_calls(t, 601, 3, 1) == [[i] for i in range(6)]                   # a forest beyond the budget goes alone
    calls = G.plan_calls(t, 601, 3, 2 * one)
    assert len(calls) > 1 and [i for c in calls for i in c] == list(range(6))


# ---- the zero-count argument --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(bootstrap=False, max_features=None, min_samples_leaf=0.01), dict(max_depth=3, min_samples_split=7)])
def test_scattered_counts_on_all_rows_equal_the_fit_on_the_subset(kw):
    X, y = tie_heavy(601, F=8, C=3, seed=4)
    y[:3] = [0, 1, 2]
    folds = folds_of(X, y)
    t = G.job_table(RandomForestClassifier(**kw), [{"n_estimators": 3, "random_state": 42}], folds, y.astype(np.int32), 8, 3)
    f = t["forests"][1]
    tr, _ = folds[1]
    want = RandomForestClassifier(n_estimators=3, random_state=42, **kw).fit(X[tr], y[tr])
    for i, est in enumerate(want.estimators_):
        j = t["jobs"][f["start"] + i]
        got = R.build_tree(X, y, t["rows"][j["counts_row"]], 3, int(j["seed"]), int(j["max_depth"]), int(j["min_samples_split"]),
                           int(j["min_samples_leaf"]), int(j["max_features"]))
        assert len(got["left"]) <= t["caps"][f["start"] + i]
        K.assert_nodes_equal(FF.tree_nodes(est), got, f"fold 1 tree {i}")


# ---- result formatting --------------------------------------------------------------------------------------------------
def small_search(scoring=None, grid=None):
    X, y = tie_heavy(150, seed=6)
    grid = grid or {"n_estimators": [3], "max_depth": [1, 4, None], "random_state": [42]}
    return GridSearchCV(RandomForestClassifier(), grid, cv=3, n_jobs=1, scoring=scoring).fit(X, y)


def table_of(search):
    return np.stack([search.cv_results_[f"split{k}_test_score"] for k in range(search.n_splits_)], axis=1)


def formatted(search):
    res = G.GridSearchResult()
    res.cv_results_ = G.format_results(list(search.cv_results_["params"]), search.n_splits_, table_of(search))
    res.best_index_, res.best_params_, res.best_score_ = G.best_of(res.cv_results_)
    res.n_splits_ = search.n_splits_
    return res


def test_format_results_reproduces_gridsearchcv():
    want = small_search()
    assert_search_equal(want, formatted(want))
    two = small_search(grid=[{"n_estimators": [2, 3], "random_state": [0]}, {"max_depth": [2], "bootstrap": [False], "n_estimators": [2]}])
    assert_search_equal(two, formatted(two))        # param_* masked where a candidate lacks the parameter


@pytest.mark.parametrize("by_depth,best", [({1: 0.5, 4: 0.5, None: 0.5}, 0), ({1: 0.25, 4: 0.75, None: 0.75}, 1)])
def test_format_results_on_ties(by_depth, best):
    """All candidates tied: ranks [1 1 1] and the first wins.  Candidates 1 and 2 tied for first: ranks [3 1 1], candidate 1 wins."""
    want = small_search(scoring=lambda est, X, y: by_depth[est.max_depth])
    got = formatted(want)
    assert_search_equal(want, got)
    assert got.best_index_ == best
    assert list(got.cv_results_["rank_test_score"]) == ([1, 1, 1] if best == 0 else [3, 1, 1])


# ---- refusals: decided on the host, before any device call ---------------------------------------------------------------
def test_refusals_name_the_cause():
    X, y = tie_heavy(120, seed=2)
    with pytest.raises(RssegUnsupported, match="criterion"):
        G.grid_search(RandomForestClassifier(), {"criterion": ["gini", "entropy"], "n_estimators": [2]}, X, y)
    Xn = X.copy()
    Xn[7, 1] = np.nan
    with pytest.raises(RssegUnsupported, match="NaN"):
        G.grid_search(RandomForestClassifier(), {"n_estimators": [2]}, Xn, y)
    y1 = y.copy()
    y1[y1 == 2] = 1
    y1[5] = 2                                                          # a class with one member
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(RssegUnsupported, match="fold .* lacks one of the 3 classes"):
            G.grid_search(RandomForestClassifier(), {"n_estimators": [2]}, X, y1, cv=3)
    assert any("least populated class" in str(x.message) for x in w)   # scikit-learn's own warning, from its own splitter
    with pytest.raises(RssegUnsupported, match="features"):
        G.grid_search(RandomForestClassifier(), {"n_estimators": [2]}, np.zeros((30, 65), np.float32), np.arange(30) % 2)
    with pytest.raises(RssegUnsupported, match="cv='three'"):
        G.grid_search(RandomForestClassifier(), {"n_estimators": [2]}, X, y, cv="three")
    from sklearn.model_selection import ShuffleSplit
    with pytest.raises(RssegUnsupported, match="not sorted"):
        G.grid_search(RandomForestClassifier(), {"n_estimators": [2]}, X, y, cv=ShuffleSplit(2, random_state=0))
    from sklearn.tree import DecisionTreeClassifier
    with pytest.raises(RssegUnsupported, match="DecisionTreeClassifier"):
        G.grid_search(DecisionTreeClassifier(), {"max_depth": [2]}, X, y)


# ---- the mirror ---------------------------------------------------------------------------------------------------------
def test_train_random_forest_keeps_the_reference_signature():
    from modules import supervised_classifiers as S
    spec = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "supervised_classifiers_names.json")))["modules.supervised_classifiers"]
    assert spec["public_names"]["train_random_forest"] == "function"
    assert "train_random_forest" in S.__all__
    for name in ("train_random_forest", "train_random_forest_from_samples", "prepare_training_samples", "predict_image"):
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(getattr(S, name)).parameters.values()]
        assert got == spec["signatures"][name], name
