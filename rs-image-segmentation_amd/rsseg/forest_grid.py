"""
GridSearchCV(RandomForestClassifier(), param_grid, cv=...) on the GPU: `grid_search(estimator, param_grid, X, y)` gives
scikit-learn 1.7.2's cv_results_ (scores, ranks, params), best_index_, best_params_, best_score_ and best_estimator_, the
score keys bit for bit.

Every fold fit of every candidate is grown by K16 in one call (rsseg_forest_fit_jobs): the trees of all forests side by
side, one workgroup each.  A fold's training subset needs no copy of the feature planes.  scikit-learn's splitter drops
samples of weight zero, so the tree RandomForestClassifier.fit(X[train], y[train]) grows is the tree grown on all rows with
that tree's bootstrap counts over the subset scattered into a full-length row (zeros at the held-out rows) and
weighted_n_samples equal to the subset's size, as long as `train` is sorted (the relative order of the samples is kept).
Candidates that differ only in parameters the bootstrap does not depend on (max_depth, ...) share the count rows of a fold.
Each forest is then loaded and walked over the held-out rows by K11 (rsseg_forest_load / rsseg_forest_predict), and the
matches with y are counted on the device: the score is correct / n_test in float64, which is what accuracy_score returns (the
mean of 0/1 values is an exact integer sum divided once).  The host formats the results as BaseSearchCV._format_results
does and refits the best candidate with forest_fit.fit.

Scorers other than accuracy and error_score handling are not implemented.  Anything the device path does not take raises
RssegUnsupported naming the reason.
"""
from __future__ import annotations

import copy
import time

import numpy as np

from . import _lib as L
from . import forest_fit as FF
from .runtime import RssegUnsupported

# The default byte budget of one growing call: count rows, sample and sort scratch, node storage.  Node storage is sized for
# the worst case (2m - 1 nodes per tree of m samples, 37 + 8 C bytes each) and dominates: the default search (3 folds x 3
# candidates x 100 trees) on 200 000 samples of 3 classes needs about 11 GiB.  16 GiB holds that in one call and is 1/18 of
# an MI355X's 288 GB, so the search leaves room for the planes and for other work on the device.
DEFAULT_MAX_BYTES = 16 << 30

TIME_KEYS = ("mean_fit_time", "std_fit_time", "mean_score_time", "std_score_time")


class GridSearchResult:
    """What GridSearchCV holds after fit: cv_results_, best_index_, best_params_, best_score_, n_splits_, and with refit
    best_estimator_ (a plain scikit-learn RandomForestClassifier) and refit_time_."""

    def __repr__(self):
        return f"GridSearchResult(best_params_={self.best_params_!r}, best_score_={self.best_score_!r})"


def format_results(candidate_params, n_splits: int, test_scores, fit_time=None, score_time=None) -> dict:
    """cv_results_ as BaseSearchCV._format_results (model_selection/_search.py) builds it for one scorer without train scores.
    test_scores, fit_time, score_time: (n_candidates, n_splits).  Means by np.average, standard deviations as
    sqrt(average((x - mean)^2)), ranks by rankdata(-mean, method='min'); param_* are scikit-learn's own masked arrays."""
    from scipy.stats import rankdata
    from sklearn.model_selection._search import _yield_masked_array_for_each_param
    n_candidates = len(candidate_params)
    results = {}

    def store(key, array, splits=False, rank=False):
        array = np.array(array, dtype=np.float64).reshape(n_candidates, n_splits)
        if splits:
            for k in range(n_splits):
                results["split%d_%s" % (k, key)] = array[:, k]
        means = np.average(array, axis=1)
        results["mean_%s" % key] = means
        results["std_%s" % key] = np.sqrt(np.average((array - means[:, np.newaxis]) ** 2, axis=1))
        if rank:
            results["rank_%s" % key] = rankdata(-means, method="min").astype(np.int32, copy=False)

    zeros = np.zeros((n_candidates, n_splits))
    store("fit_time", zeros if fit_time is None else fit_time)
    store("score_time", zeros if score_time is None else score_time)
    for param, ma in _yield_masked_array_for_each_param(candidate_params):
        results[param] = ma
    results["params"] = candidate_params
    store("test_score", test_scores, splits=True, rank=True)
    return results


def best_of(results: dict):
    """(best_index_, best_params_, best_score_): the first candidate of rank 1 (BaseSearchCV._select_best_index)."""
    i = int(results["rank_test_score"].argmin())
    return i, results["params"][i], results["mean_test_score"][i]


def _candidate(estimator, params):
    from sklearn.base import clone
    return clone(estimator).set_params(**clone(params, safe=False))


def _folds(cv, X, y_enc):
    """(n_splits, [(train, test)]) from scikit-learn's own check_cv, so its warnings and errors about small classes read the same."""
    from sklearn.model_selection import check_cv
    try:
        splitter = check_cv(cv, y_enc, classifier=True)
    except (ValueError, TypeError) as e:
        raise RssegUnsupported(f"forest_grid: cv={cv!r} is not an integer or a splitter check_cv accepts ({e})") from e
    if not hasattr(splitter, "split"):
        raise RssegUnsupported(f"forest_grid: cv={cv!r} is not an integer or a splitter check_cv accepts")
    return splitter.get_n_splits(X, y_enc, None), [(np.asarray(tr), np.asarray(te)) for tr, te in splitter.split(X, y_enc, None)]


def job_table(estimator, candidate_params, folds, y_enc, n_features: int, n_classes: int) -> dict:
    """The trees of every (fold, candidate) forest as records of rsseg_forest_fit_jobs.  Returns
      rows      list of distinct full-length int32 count rows (a fold's bootstrap counts scattered to all rows, zeros at the
                held-out samples; one membership row per fold for bootstrap=False), shared by the candidates of a fold that
                draw the same tree seeds
      jobs      structured array (rsseg._lib.FOREST_JOB), forest after forest
      caps      2 m - 1 per tree (m = non-zero counts of its row)
      tree_seed the integer random_state of each tree
      forests   per forest: dict(candidate, fold, start, stop, n_train, params (resolved))
    ordered fold-major, so forests that share rows are neighbours."""
    n = len(y_enc)
    rows, row_of, row_m = [], {}, []
    jobs, caps, tree_seed, forests = [], [], [], []
    for k, (train, test) in enumerate(folds):
        if len(train) == 0 or np.any(np.diff(train) <= 0):
            raise RssegUnsupported(f"forest_grid: the training indices of fold {k} are not sorted and unique (the zero-count rows "
                                   "keep the sample order of X)")
        n_tr = len(train)
        if len(np.unique(y_enc[train])) != n_classes:
            raise RssegUnsupported(f"forest_grid: the training part of fold {k} lacks one of the {n_classes} classes (the class "
                                   "encoding would differ per fold)")
        if n_tr >= FF.MAX_SAMPLES:
            raise RssegUnsupported(f"forest_grid: {n_tr} training samples: fewer than {FF.MAX_SAMPLES} on the GPU")
        for c, params in enumerate(candidate_params):
            est = _candidate(estimator, params)
            p = est.get_params()
            rp = FF.resolve_params(p, n_tr, n_features)
            seeds = FF.tree_seeds(copy.deepcopy(est.random_state), int(est.n_estimators))
            start = len(jobs)
            for s in seeds:
                key = (k, int(s) if est.bootstrap else None)
                if key not in row_of:
                    row = np.zeros(n, np.int32)
                    row[train] = FF.bootstrap_counts(int(s), n_tr) if est.bootstrap else 1
                    row_of[key] = len(rows)
                    rows.append(row)
                    row_m.append(int(np.count_nonzero(row)))
                r = row_of[key]
                jobs.append((r, n_tr, FF.splitter_seed(int(s)), rp["max_depth"], rp["min_samples_split"], rp["min_samples_leaf"],
                             rp["max_features"], 0))
                caps.append(2 * row_m[r] - 1)
                tree_seed.append(int(s))
            forests.append(dict(candidate=c, fold=k, start=start, stop=len(jobs), n_train=n_tr, params=rp))
    return dict(rows=rows, jobs=np.array(jobs, np.dtype(L.FOREST_JOB)), caps=np.array(caps, np.int64),
                tree_seed=np.array(tree_seed, np.int64), forests=forests)


def forest_bytes(table: dict, forest: dict, n_classes: int):
    """(bytes of sample / sort scratch and node storage of the forest's trees, the set of count rows it reads)."""
    caps = table["caps"][forest["start"]:forest["stop"]]
    m = (caps + 1) // 2
    return int((20 * m + (37 + 8 * n_classes) * caps).sum()), set(table["jobs"]["counts_row"][forest["start"]:forest["stop"]].tolist())


def plan_calls(table: dict, n: int, n_classes: int, max_bytes: int) -> list:
    """Whole forests per growing call, in order, each call within max_bytes (a forest larger than the budget goes alone)."""
    calls, cur, cur_bytes, cur_rows = [], [], 0, set()
    for i, forest in enumerate(table["forests"]):
        b, rows = forest_bytes(table, forest, n_classes)
        if cur and cur_bytes + b + 4 * n * len(cur_rows | rows) > max_bytes:
            calls.append(cur)
            cur, cur_bytes, cur_rows = [], 0, set()
        cur.append(i)
        cur_bytes += b
        cur_rows |= rows
    if cur:
        calls.append(cur)
    return calls


def flat_forest(trees, n_features: int, n_classes: int) -> dict:
    """The dict rsseg_forest_load takes, straight from K16's node arrays (class indices as the classes)."""
    off = np.zeros(len(trees) + 1, np.int64)
    off[1:] = np.cumsum([len(t["left"]) for t in trees])
    cat = lambda k: np.concatenate([t[k] for t in trees])   # noqa: E731
    return dict(tree_off=off, left=cat("left"), right=cat("right"), feature=cat("feature"), threshold=cat("threshold"),
                missing_left=cat("missing_go_to_left"), value=np.ascontiguousarray(cat("value")),
                classes=np.arange(n_classes, dtype=np.int64), n_features=n_features)


def grid_search(estimator, param_grid, X, y, cv=3, refit=True, ctx=None, max_bytes: int = DEFAULT_MAX_BYTES):
    """GridSearchCV(estimator, param_grid, cv=cv, refit=refit).fit(X, y) for a RandomForestClassifier `estimator`, on the GPU.
    max_bytes: the budget of one growing call for count rows, sample and sort scratch and node storage (DEFAULT_MAX_BYTES,
    16 GiB: the default search on 200 000 samples in one call, a small share of the device's memory); beyond it the forests
    go in several calls, whole forests per call, with the same results.  Scoring loads every fold forest into `ctx`
    (rsseg_forest_load), with ctx=None the process-wide default context: a forest loaded there before for prediction is
    replaced and has to be loaded again afterwards.  Returns a GridSearchResult."""
    from sklearn.model_selection import ParameterGrid
    from sklearn.ensemble import RandomForestClassifier
    from .runtime import _torch, default_context
    if not isinstance(estimator, RandomForestClassifier):
        raise RssegUnsupported(f"forest_grid: {type(estimator).__name__} is not a RandomForestClassifier")
    candidate_params = list(ParameterGrid(param_grid))
    for params in candidate_params:
        est = _candidate(estimator, params)
        FF.check_supported(est.get_params())
        est._validate_params()
    X32, y_enc, classes, _ = FF.prepare(_candidate(estimator, candidate_params[0]), X, y)
    n, F = X32.shape
    C = len(classes)
    n_splits, folds = _folds(cv, X32, y_enc)
    table = job_table(estimator, candidate_params, folds, y_enc, F, C)

    torch = _torch()
    ctx = ctx if ctx is not None else default_context()
    planes = [ctx.upload_f32(np.ascontiguousarray(X32[:, f])) for f in range(F)]
    d_y = ctx.to_device(y_enc, np.int32)
    d_y64 = d_y.to(torch.int64)
    d_test = [ctx.to_device(te, np.int64) for _, te in folds]
    test_planes = [[p.index_select(0, idx) for p in planes] for idx in d_test]
    test_y = [d_y64.index_select(0, idx) for idx in d_test]

    shape = (len(candidate_params), n_splits)
    scores, fit_time, score_time = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for call in plan_calls(table, n, C, max_bytes):
        forests = [table["forests"][i] for i in call]
        sel = np.concatenate([np.arange(f["start"], f["stop"]) for f in forests])
        jobs = table["jobs"][sel].copy()
        used, jobs["counts_row"] = np.unique(jobs["counts_row"], return_inverse=True)
        t0 = time.perf_counter()
        d_counts = ctx.to_device(np.concatenate([table["rows"][r] for r in used]), np.int32)
        trees = ctx.forest_fit_jobs(planes, d_y, d_counts, jobs, table["caps"][sel], C)
        del d_counts
        grow = (time.perf_counter() - t0) / len(forests)   # one chain of launches grew them all: an equal share each
        pos = 0
        for f in forests:
            T = f["stop"] - f["start"]
            t0 = time.perf_counter()
            ctx.forest_load(flat_forest(trees[pos:pos + T], F, C))
            pred = ctx.forest_predict(test_planes[f["fold"]])
            correct = int((pred == test_y[f["fold"]]).sum().item())
            scores[f["candidate"], f["fold"]] = correct / len(folds[f["fold"]][1])
            fit_time[f["candidate"], f["fold"]] = grow
            score_time[f["candidate"], f["fold"]] = time.perf_counter() - t0
            pos += T

    res = GridSearchResult()
    res.cv_results_ = format_results(candidate_params, n_splits, scores, fit_time, score_time)
    res.best_index_, res.best_params_, res.best_score_ = best_of(res.cv_results_)
    res.n_splits_ = n_splits
    if refit:
        from sklearn.base import clone
        t0 = time.perf_counter()
        res.best_estimator_ = FF.fit(clone(_candidate(estimator, res.best_params_)), X, y, ctx=ctx)
        res.refit_time_ = time.perf_counter() - t0
    return res
