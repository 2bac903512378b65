"""Grid-searched forest training on the GPU: rsseg_forest_fit_jobs (per-tree count row, weight_total, depth, leaf and split
sizes, max_features in one launch chain) against scikit-learn's fits on the folds' training subsets, whole node state, floats
bitwise; rsseg.forest_grid.grid_search against GridSearchCV(cv=3, n_jobs=1): score keys, ranks, best parameters and the
refitted model; the train_random_forest mirror; the byte budget."""
import os
import subprocess
import sys

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier
from sklearn.model_selection import GridSearchCV, ParameterGrid

import forest_fit_cases as K
from test_forest_fit_host import state_equal, tie_heavy
from test_forest_grid_host import assert_search_equal, folds_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def upload(ctx, X, y, rows):
    planes = [ctx.upload_f32(np.ascontiguousarray(X[:, f])) for f in range(X.shape[1])]
    return planes, ctx.to_device(y, np.int32), ctx.to_device(np.concatenate(rows), np.int32)


def grow_jobs(ctx, base, grid, X, y, cv=3):
    """Every (fold, candidate) forest of the search grown by one Context.forest_fit_jobs call.  Returns (table, folds,
    candidates, trees)."""
    from rsseg import forest_grid as G
    X = np.ascontiguousarray(X, np.float32)
    classes, y_enc = np.unique(y, return_inverse=True)
    folds = folds_of(X, y_enc, cv)
    cand = list(ParameterGrid(grid))
    table = G.job_table(base, cand, folds, y_enc.astype(np.int32), X.shape[1], len(classes))
    planes, d_y, d_counts = upload(ctx, X, y_enc, table["rows"])
    trees = ctx.forest_fit_jobs(planes, d_y, d_counts, table["jobs"], table["caps"], len(classes))
    return table, folds, cand, trees


def check_jobs(ctx, base, grid, X, y, cv=3):
    """... and every tree against the tree of RandomForestClassifier.fit(X[train], y[train]) of its fold and candidate."""
    from sklearn.base import clone
    from rsseg import forest_fit as FF
    table, folds, cand, trees = grow_jobs(ctx, base, grid, X, y, cv)
    assert len(trees) == len(table["jobs"])
    wants = []
    for f in table["forests"]:
        tr = folds[f["fold"]][0]
        want = clone(base).set_params(**cand[f["candidate"]]).fit(X[tr], y[tr])
        assert len(want.estimators_) == f["stop"] - f["start"]
        for i, est in enumerate(want.estimators_):
            K.assert_nodes_equal(FF.tree_nodes(est), trees[f["start"] + i], f"fold {f['fold']} candidate {f['candidate']} tree {i}")
        wants.append(want)
    return table, wants


def test_jobs_of_three_folds_and_three_depths_in_one_call(ctx):
    X, y = tie_heavy(3000, F=8, C=4, seed=11)
    table, _ = check_jobs(ctx, RandomForestClassifier(n_estimators=6, random_state=42), {"max_depth": [1, 6, None]}, X, y)
    assert len(table["jobs"]) == 54 and len(table["rows"]) == 18          # the depth candidates of a fold share its count rows
    assert len(set(table["jobs"]["max_depth"].tolist())) == 3


@pytest.mark.parametrize("n", [601, 33])
def test_uneven_folds(ctx, n):
    X, y = tie_heavy(n, F=8, C=3, seed=n)
    y[:6] = [0, 1, 2, 0, 1, 2]
    y[-6:] = [0, 1, 2, 0, 1, 2]
    table, _ = check_jobs(ctx, RandomForestClassifier(n_estimators=5, random_state=3), {"max_depth": [2, None], "min_samples_leaf": [1, 0.05]}, X, y)
    totals = set(table["jobs"]["weight_total"].tolist())
    assert totals == {f["n_train"] for f in table["forests"]} and max(totals) < n
    if n == 601:
        assert len(totals) == 2                                            # weight_total differs between jobs of the call


def test_continuation_launches_with_uneven_trees(ctx):
    """Depth-1 trees (3 nodes, done in the first launch) beside unbounded trees of more than 2048 nodes (a second launch)."""
    X, y = K.continuous(6000, F=6, C=3, seed=9, noise=0.9)
    table, wants = check_jobs(ctx, RandomForestClassifier(n_estimators=3, random_state=5), {"max_depth": [1, None]}, X, y)
    sizes = {c: [t.tree_.node_count for w, f in zip(wants, table["forests"]) if f["candidate"] == c for t in w.estimators_] for c in (0, 1)}
    assert max(sizes[0]) <= 3 and min(sizes[1]) > 2048, sizes


def test_jobs_without_bootstrap_and_the_uniform_wrapper(ctx):
    from rsseg.forest_fit import fit
    X, y = tie_heavy(601, F=8, C=3, seed=5)
    base = RandomForestClassifier(n_estimators=4, random_state=7, bootstrap=False)
    table, _ = check_jobs(ctx, base, {"max_features": [2, None]}, X, y)
    assert len(table["rows"]) == 3                                         # one membership row per fold
    # rsseg_forest_fit (uniform jobs: one shared row, then one row per tree) gives the trees it gave before
    for kw in (dict(bootstrap=False), dict()):
        kw = dict(n_estimators=4, random_state=7, **kw)
        state_equal(RandomForestClassifier(**kw).fit(X, y), fit(RandomForestClassifier(**kw), X, y, ctx=ctx))


def test_jobs_with_their_own_leaf_split_and_feature_settings(ctx):
    X, y = tie_heavy(1500, F=8, C=4, seed=12)
    grid = [{"min_samples_leaf": [1, 5], "max_features": ["sqrt", None]}, {"min_samples_split": [10, 0.05], "max_features": [3]},
            {"n_estimators": [2], "min_samples_leaf": [0.02], "max_depth": [4]}]
    table, _ = check_jobs(ctx, RandomForestClassifier(n_estimators=3, random_state=8), grid, X, y)
    j = table["jobs"]
    assert len(set(j["min_samples_leaf"].tolist())) >= 3 and len(set(j["min_samples_split"].tolist())) >= 3 and len(set(j["max_features"].tolist())) == 3


def test_count_rows_are_checked_against_their_own_weight_total(ctx):
    from rsseg import forest_fit as FF
    from rsseg import forest_grid as G
    X, y = tie_heavy(601, F=8, C=3, seed=5)
    X = np.ascontiguousarray(X, np.float32)
    y = y.astype(np.int32)
    folds = folds_of(X, y)
    table = G.job_table(RandomForestClassifier(n_estimators=2, random_state=0), [{}], folds, y, 8, 3)
    jobs, rows = table["jobs"], table["rows"]
    assert all(int(r.sum()) in (400, 401) for r in rows)                   # rows that sum to weight_total, none to n = 601: accepted
    planes, d_y, d_counts = upload(ctx, X, y, rows)
    trees = ctx.forest_fit_jobs(planes, d_y, d_counts, jobs, table["caps"], 3)
    tr = folds[0][0]
    want = RandomForestClassifier(n_estimators=2, random_state=0).fit(X[tr], y[tr])
    K.assert_nodes_equal(FF.tree_nodes(want.estimators_[1]), trees[1], "accepted row")
    # a row whose sum is not its weight_total (m unchanged), a negative count, a weight_total that is not the row's sum
    r = int(jobs["counts_row"][1])
    k = int(np.flatnonzero(rows[r] > 1)[0])
    for delta in (1, -1):
        bad = [x.copy() for x in rows]
        bad[r][k] += delta
        with pytest.raises(ValueError, match=f"forest_fit_jobs: tree 1: the counts of row {r} are negative or do not sum to weight_total = {jobs['weight_total'][1]}"):
            ctx.forest_fit_jobs(planes, d_y, ctx.to_device(np.concatenate(bad), np.int32), jobs, table["caps"], 3)
    neg = [x.copy() for x in rows]
    neg[r][int(np.flatnonzero(rows[r] == 0)[0])] = -1
    neg[r][k] += 1
    assert neg[r].sum() == rows[r].sum()
    with pytest.raises(ValueError, match="tree 1: the counts of row"):
        ctx.forest_fit_jobs(planes, d_y, ctx.to_device(np.concatenate(neg), np.int32), jobs, table["caps"], 3)
    other = jobs.copy()
    other["weight_total"][3] = 601
    with pytest.raises(ValueError, match="tree 3: .*weight_total = 601"):
        ctx.forest_fit_jobs(planes, d_y, d_counts, other, table["caps"], 3)
    # decided from the records alone, before any launch
    for field, value, text in (("counts_row", len(rows), "counts_row"), ("weight_total", 0, "weight_total=0"), ("weight_total", 1 << 26, "weight_total=67108864"),
                               ("min_samples_split", 1, "min_samples_split=1"), ("min_samples_leaf", 0, "min_samples_leaf=0"), ("max_depth", -1, "max_depth=-1")):
        other = jobs.copy()
        other[field][2] = value
        with pytest.raises(ValueError, match=f"forest_fit_jobs: tree 2: bad job .*{text}"):
            ctx.forest_fit_jobs(planes, d_y, d_counts, other, table["caps"], 3)
    with pytest.raises(ValueError, match="whole rows"):
        ctx.forest_fit_jobs(planes, d_y, d_counts[:-1], jobs, table["caps"], 3)
    # the context is as good as before
    again = ctx.forest_fit_jobs(planes, d_y, d_counts, jobs, table["caps"], 3)
    K.assert_nodes_equal(trees[5], again[5], "after refusals")


# ---- grid_search -----------------------------------------------------------------------------------------------------------
def both_searches(ctx, grid, X, y, **kw):
    from rsseg.forest_grid import grid_search
    want = GridSearchCV(RandomForestClassifier(), grid, cv=3, n_jobs=1).fit(X, y)
    got = grid_search(RandomForestClassifier(), grid, X, y, cv=3, ctx=ctx, **kw)
    assert_search_equal(want, got)
    state_equal(want.best_estimator_, got.best_estimator_)
    return want, got


@pytest.fixture(scope="module")
def reference_problem(ctx, golden_dir):
    from test_gpu_forest_fit import scene_samples
    _, X, y, _ = scene_samples(ctx, golden_dir)
    assert X.shape == (33, 19)
    return X, y


def test_grid_search_on_the_reference_problem_with_the_default_grid(ctx, reference_problem):
    X, y = reference_problem
    both_searches(ctx, {"n_estimators": [100], "max_depth": [10, 20, None], "random_state": [42]}, X, y)


def test_grid_search_on_3000_samples(ctx):
    X, y = tie_heavy(3000, F=8, C=4, seed=11)
    want, got = both_searches(ctx, {"n_estimators": [20], "max_depth": [3, 6, None], "random_state": [42]}, X, y)
    for k in got.cv_results_:
        if k.endswith("_time"):
            assert got.cv_results_[k].shape == (3,) and np.all(got.cv_results_[k] >= 0)
    assert got.refit_time_ > 0


def test_grid_search_over_a_list_of_two_grids(ctx):
    X, y = tie_heavy(900, F=8, C=3, seed=13)
    y = np.array(["water", "soil", "forest"])[y]
    grid = [{"n_estimators": [5, 8], "max_depth": [4], "random_state": [1]}, {"n_estimators": [6], "bootstrap": [False], "min_samples_leaf": [2, 0.01], "random_state": [2]}]
    both_searches(ctx, grid, X, y)


def test_a_small_byte_budget_gives_the_same_results_in_several_calls(ctx):
    from rsseg import forest_grid as G
    X, y = tie_heavy(900, F=8, C=3, seed=14)
    grid = {"n_estimators": [6], "max_depth": [2, None], "random_state": [42]}
    one = G.grid_search(RandomForestClassifier(), grid, X, y, ctx=ctx)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        two = G.grid_search(RandomForestClassifier(), grid, X, y, ctx=ctx, max_bytes=600_000)
        _, calls = ctx.prof_get("forest_fit_jobs")
    finally:
        ctx.prof_enable(False)
    assert calls >= 2
    assert_search_equal(one, two)
    state_equal(one.best_estimator_, two.best_estimator_)


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def test_train_random_forest_returns_and_saves_the_best_model(ctx, reference_problem, tmp_path, capsys):
    from modules import supervised_classifiers as S
    X, y = reference_problem
    path = str(tmp_path / "sub" / "rf_model.pkl")                            # the directory is made, as the reference makes it
    ctx2 = S._ctx()
    ctx2.prof_enable(True)
    ctx2.prof_reset()
    try:
        model = S.train_random_forest(X, y, save_path=path)
        _, calls = ctx2.prof_get("forest_fit_jobs")
    finally:
        ctx2.prof_enable(False)
    assert calls >= 1                                                       # grown on the device, not by the host fallback
    assert f"✅ 模型训练完成，保存至 {path}" in capsys.readouterr().out
    want = GridSearchCV(RandomForestClassifier(), {"n_estimators": [100], "max_depth": [10, 20, None], "random_state": [42]}, cv=3, n_jobs=1).fit(X, y)
    assert type(model) is RandomForestClassifier
    state_equal(want.best_estimator_, model)
    code = ("import joblib, numpy as np, sys; m = joblib.load(sys.argv[1]); from sklearn.ensemble import RandomForestClassifier; "
            "assert type(m) is RandomForestClassifier and 'rsseg' not in sys.modules; np.save(sys.argv[2], m.predict_proba(np.load(sys.argv[3])))")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH",)}
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    np.save(tmp_path / "X.npy", X)
    r = subprocess.run([sys.executable, "-c", code, path, str(tmp_path / "p.npy"), str(tmp_path / "X.npy")], capture_output=True, text=True,
                       timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.load(tmp_path / "p.npy"), want.best_estimator_.predict_proba(X))


def test_train_random_forest_falls_back_and_reports_errors(ctx, tmp_path, capsys):
    from modules import supervised_classifiers as S
    X, y = tie_heavy(150, seed=6)
    grid = {"n_estimators": [3], "criterion": ["entropy"], "max_depth": [2, None], "random_state": [42]}
    ctx2 = S._ctx()
    ctx2.prof_enable(True)
    ctx2.prof_reset()
    try:
        model = S.train_random_forest(X, y, param_grid=grid, save_path=str(tmp_path / "rf.pkl"))
        _, calls = ctx2.prof_get("forest_fit_jobs")
    finally:
        ctx2.prof_enable(False)
    assert calls == 0                                                       # scikit-learn's GridSearchCV on the host
    state_equal(GridSearchCV(RandomForestClassifier(), grid, cv=3, n_jobs=1).fit(X, y).best_estimator_, model)
    capsys.readouterr()
    assert S.train_random_forest(X, y[:-1], save_path=str(tmp_path / "no.pkl")) is None
    assert "❌ 随机森林训练失败:" in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "no.pkl")
