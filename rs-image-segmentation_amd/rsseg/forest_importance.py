"""Permutation importance of a fitted forest on the GPU, equal to sklearn.inspection.permutation_importance bit for bit
(accuracy scoring): the host side of rsseg_forest_permutation_counts (csrc/k11_forest_perm.hip).

permutation_importance draws ONE integer seed and hands it to every column's worker, which starts a fresh RandomState from
it (inspection/_permutation_importance.py:277-278, :43): every feature sees the same row subsample and the same shuffles.
A worker shuffles its column cumulatively (:66-74), so after repeat r the column holds X[rows][g_r] with g_0 = arange(m),
g_r = g_{r-1}[idx_r], idx_r the running shuffled index.  The whole call therefore needs n_repeats source-index vectors
shared by all features (permutation_plan), F * n_repeats + 1 counts of correctly labelled samples from one device call,
and a finish in float64 that divides them as accuracy_score does (importance_from_counts)."""
from __future__ import annotations

import numbers

import numpy as np

from . import _lib as L
from .forest import _check_width, _flat_for_proba


def _resolve_max_samples(max_samples, n: int) -> int:
    if not isinstance(max_samples, numbers.Integral):   # _permutation_importance.py:280-283
        return int(max_samples * n)
    if max_samples > n:
        raise ValueError("max_samples must be <= n_samples")
    return int(max_samples)


def permutation_plan(n: int, n_repeats: int, random_state, max_samples=1.0):
    """The random draws of sklearn.inspection.permutation_importance for n samples -> (rows, sources).  rows: the m sample
    indices every column's worker scores on (arange(n) when m == n, else the worker's draw without replacement, unsorted);
    sources: (n_repeats, m) int32, sources[r][i] = the row of X[rows] whose value sits in row i of the permuted column after
    repeat r."""
    from sklearn.ensemble._bagging import _generate_indices
    from sklearn.utils import check_random_state
    n, n_repeats = int(n), int(n_repeats)
    seed = check_random_state(random_state).randint(np.iinfo(np.int32).max + 1)
    m = _resolve_max_samples(max_samples, n)
    rs = check_random_state(seed)
    if m < n:
        rows = np.asarray(_generate_indices(random_state=rs, bootstrap=False, n_population=n, n_samples=m))
    else:
        rows = np.arange(n)
    m = len(rows)
    idx = np.arange(m)
    g = np.arange(m)
    sources = np.empty((n_repeats, m), np.int32)
    for r in range(n_repeats):
        rs.shuffle(idx)
        g = g[idx]
        sources[r] = g
    return rows, sources


def encode_labels(classes, y) -> np.ndarray:
    """y in the terms of the forest's classes_: int32 class indices, -1 for a label that is not among them."""
    classes, y = np.asarray(classes), np.asarray(y).reshape(-1)
    if classes.dtype.kind in "OUS" or y.dtype.kind in "OUS":
        lookup = {c: i for i, c in enumerate(classes.tolist())}
        return np.asarray([lookup.get(v, -1) for v in y.tolist()], np.int32).reshape(-1)
    order = np.argsort(classes, kind="stable")
    pos = np.clip(np.searchsorted(classes[order], y), 0, len(classes) - 1)
    return np.where(classes[order][pos] == y, order[pos], -1).astype(np.int32)


def importance_jobs(n_features: int, n_repeats: int) -> np.ndarray:
    """One job per (feature, repeat), feature-major: job f * n_repeats + r substitutes feature f from source row r."""
    jobs = np.zeros(n_features * n_repeats, np.dtype(L.PERM_JOB))
    jobs["feature"] = np.repeat(np.arange(n_features, dtype=np.int32), n_repeats)
    jobs["source"] = np.tile(np.arange(n_repeats, dtype=np.int32), n_features)
    return jobs


BASELINE_JOB = np.array([(-1, 0)], np.dtype(L.PERM_JOB))


def importance_from_counts(baseline_count, n: int, counts, m: int):
    """The finish of permutation_importance from integer counts.  baseline_count of n samples labelled correctly as they
    are; counts (F, n_repeats) of m samples with a column permuted.  accuracy_score is count / samples in float64, the
    importances are baseline - scores (_create_importances_bunch)."""
    from sklearn.utils import Bunch
    baseline = np.float64(baseline_count) / np.float64(n)
    scores = np.asarray(counts, np.int64).astype(np.float64) / np.float64(m)
    importances = baseline - scores
    return Bunch(importances_mean=np.mean(importances, axis=1), importances_std=np.std(importances, axis=1),
                 importances=importances), float(baseline)


def host_counts(predict_index):
    """The host restatement of rsseg_forest_permutation_counts: a counter for _importance from `predict_index`, a function
    (k, F) float32 -> (k,) class indices (for checking: one whole-forest prediction per job)."""
    def count(X32, y_enc, src, jobs):
        out = np.zeros(len(jobs), np.int64)
        for j, (f, s) in enumerate(np.asarray(jobs).tolist()):
            Xp = X32
            if f >= 0:
                Xp = X32.copy()
                Xp[:, f] = X32[src[s], f]
            out[j] = int((np.asarray(predict_index(Xp)) == y_enc).sum())
        return out
    return count


def device_counts(ctx):
    """The counter for _importance on the loaded forest of `ctx`: one rsseg_forest_permutation_counts call per set of rows."""
    def count(X32, y_enc, src, jobs):
        planes = [ctx.to_device(np.ascontiguousarray(X32[:, f])) for f in range(X32.shape[1])]
        d_src = None if src is None else ctx.to_device(np.ascontiguousarray(src, np.int32).reshape(-1))
        return ctx.forest_permutation_counts(planes, ctx.to_device(y_enc, np.int32), d_src, jobs)
    return count


def _check_model(model) -> None:
    from .runtime import RssegUnsupported
    if isinstance(model, dict):
        if not all(k in model for k in ("tree_off", "value", "classes", "n_features")):
            raise RssegUnsupported("permutation_importance: model: a dict must be what flatten_forest returns (with its classes)")
        return
    from sklearn.ensemble._forest import ForestClassifier
    if not isinstance(model, ForestClassifier) or not hasattr(model, "estimators_"):
        raise RssegUnsupported(f"permutation_importance: model: {type(model).__name__} is not a fitted forest classifier "
                               "(RandomForestClassifier or a flatten_forest dict)")
    if getattr(model, "n_outputs_", 1) != 1:
        raise RssegUnsupported(f"permutation_importance: model: multi-output forest ({model.n_outputs_} outputs) is not supported on the GPU")


def _check_arguments(model, scoring, sample_weight) -> None:
    from .runtime import RssegUnsupported
    if scoring is not None and scoring != "accuracy":
        raise RssegUnsupported(f"permutation_importance: scoring={scoring!r} is not supported on the GPU (only None or 'accuracy': "
                               "the kernel counts correct labels)")
    if sample_weight is not None:
        raise RssegUnsupported("permutation_importance: sample_weight is not supported on the GPU (only sample_weight=None)")
    _check_model(model)


def _importance(classes, n_features: int, X, y, n_repeats, random_state, max_samples, count):
    """permutation_importance behind the checks: `count(X32, y_enc, src, jobs) -> int64 counts` does the scoring."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    _check_width({"n_features": n_features}, X.shape[1])
    n, F = X.shape
    y_enc = encode_labels(classes, y)
    if len(y_enc) != n:
        raise ValueError(f"Found input variables with inconsistent numbers of samples: [{n}, {len(y_enc)}]")
    rows, sources = permutation_plan(n, n_repeats, random_state, max_samples)
    m = len(rows)
    if n == 0 or m == 0:
        raise ValueError(f"Found array with 0 sample(s) (shape=({m}, {F})) while a minimum of 1 is required by RandomForestClassifier.")
    X32 = np.ascontiguousarray(X, dtype=np.float32)   # RandomForestClassifier.predict's cast (_forest.py:640)
    jobs = importance_jobs(F, int(n_repeats))
    if m == n:      # rows = arange(n): the baseline and the permuted columns read the same planes, one call
        c = count(X32, y_enc, sources, np.concatenate([BASELINE_JOB, jobs]))
        base, perm = c[0], c[1:]
    else:           # the baseline over all n rows, the permuted columns over the m rows drawn (gathered once)
        base = count(X32, y_enc, None, BASELINE_JOB)[0]
        perm = count(np.ascontiguousarray(X32[rows]), np.ascontiguousarray(y_enc[rows]), sources, jobs)
    return importance_from_counts(base, n, np.asarray(perm).reshape(F, int(n_repeats)), m)


def _scored(model, X, y, scoring, n_repeats, random_state, sample_weight, max_samples, ctx):
    from .runtime import default_context
    _check_arguments(model, scoring, sample_weight)
    classes = np.asarray(model["classes"] if isinstance(model, dict) else model.classes_)
    flat = _flat_for_proba(model)      # class indices in place of classes_ (which may hold strings)
    X = np.asarray(X)
    if X.ndim == 2:                     # what can be refused is refused before any device call
        _check_width(flat, X.shape[1])
        _resolve_max_samples(max_samples, X.shape[0])
    ctx = ctx if ctx is not None else default_context()
    ctx.forest_load(flat)
    return _importance(classes, int(flat["n_features"]), X, y, n_repeats, random_state, max_samples, device_counts(ctx))


def permutation_importance(model, X, y, *, scoring=None, n_repeats=5, n_jobs=None, random_state=None, sample_weight=None,
                           max_samples=1.0, ctx=None):
    """sklearn.inspection.permutation_importance(model, X, y, ...) of a fitted single-output forest classifier (scikit-learn's,
    K16's, or a flatten_forest dict, whose 'classes' are the labels) with accuracy scoring, on the GPU and bit for bit: a
    Bunch with importances (F, n_repeats), importances_mean and importances_std.  X is cast to float32 as predict does; y may
    hold labels the forest does not know (never correct).  The baseline is scored over all n rows, the permuted columns over
    the max_samples rows scikit-learn draws.  n_jobs is accepted and ignored (every job runs in one launch).  scoring other
    than None / 'accuracy', a sample_weight, or anything that is not such a forest raises RssegUnsupported."""
    return _scored(model, X, y, scoring, n_repeats, random_state, sample_weight, max_samples, ctx)[0]


def permutation_importance_image(model, features, roi_mask, **kw):
    """permutation_importance over the labelled pixels of an image: features (H, W, D), roi_mask (H, W) integers; the
    pixels with mask > 0 are scored against their mask value, NaN features counted as 0 (as supervised_classification_predict
    feeds the forest).  Returns the Bunch with `baseline_score` (accuracy on those pixels) and `n_samples` added."""
    features, roi_mask = np.asarray(features), np.asarray(roi_mask)
    if features.ndim != 3:
        raise ValueError("features must be a 3-D array (height, width, n_features)")
    if roi_mask.shape != features.shape[:2] or roi_mask.dtype.kind not in "iub":
        raise ValueError(f"roi_mask must be an integer array of shape {features.shape[:2]}, got {roi_mask.dtype} {roi_mask.shape}")
    sel = roi_mask > 0
    X = np.nan_to_num(features[sel], nan=0.0)
    args = dict(scoring=None, n_repeats=5, random_state=None, sample_weight=None, max_samples=1.0, ctx=None)
    kw.pop("n_jobs", None)
    unknown = set(kw) - set(args)
    if unknown:
        raise TypeError(f"permutation_importance_image() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    args.update(kw)
    res, baseline = _scored(model, X, roi_mask[sel], args["scoring"], args["n_repeats"], args["random_state"], args["sample_weight"],
                            args["max_samples"], args["ctx"])
    res["baseline_score"] = baseline
    res["n_samples"] = int(sel.sum())
    return res
