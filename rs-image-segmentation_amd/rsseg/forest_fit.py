"""
RandomForestClassifier.fit on the GPU (K16, csrc/k16_forest_fit.hip): the same trees scikit-learn 1.7.2 grows, node for
node and bit for bit.  `fit(estimator, X, y)` takes an unfitted sklearn RandomForestClassifier, fits it on the device and
returns that same estimator, fitted: a plain scikit-learn object (joblib files need nothing from this package to load).

The host does what NumPy does in sklearn: validation (sklearn's own checks, so errors read the same), the label encoding,
the parameter resolution of tree/_classes.py, the tree seeds (ensemble/_base.py:73-75), the bootstrap counts
(ensemble/_forest.py:124-133, 176-179) and each splitter's xorshift seed (tree/_splitter.pyx:160); the device grows the
trees; the host assembles DecisionTreeClassifier objects from the node arrays.  Settings K16 does not implement raise
RssegUnsupported naming the parameter (callers that want the reference's behaviour anyway fall back to `clf.fit`).
`fit_oob(estimator, X, y)` is `fit` for oob_score=True (or a callable): the grown forest walks its own training planes
(K11, rsseg_forest_oob) and the estimator gets scikit-learn's oob_decision_function_ and oob_score_, bit for bit.
"""
from __future__ import annotations

import numbers
from math import ceil
import numpy as np

from .runtime import RssegUnsupported

MAX_FEATURES = 64
MAX_CLASSES = 64
MAX_SAMPLES = 1 << 26     # every sum of squared integer counts stays exact in double below this total weight
RAND_R_MAX = 2147483647   # sklearn/utils/_random.pxd

# parameters that must keep their default (the value sklearn's constructor gives them)
_DEFAULTS = {
    "criterion": "gini", "class_weight": None, "max_leaf_nodes": None, "min_impurity_decrease": 0.0,
    "min_weight_fraction_leaf": 0.0, "max_samples": None, "ccp_alpha": 0.0, "monotonic_cst": None, "oob_score": False,
    "warm_start": False,
}


def check_supported(params: dict) -> None:
    """Raises RssegUnsupported naming the first parameter K16 does not implement."""
    for k, v in _DEFAULTS.items():
        got = params.get(k, v)
        if (got is not None) if v is None else (isinstance(got, (bool, np.bool_)) != isinstance(v, bool) or got != v):
            raise RssegUnsupported(f"forest_fit: {k}={params[k]!r} is not supported on the GPU (only {k}={v!r})")


def resolve_params(params: dict, n_samples: int, n_features: int) -> dict:
    """max_depth, min_samples_split, min_samples_leaf and max_features as DecisionTreeClassifier._fit resolves them
    (tree/_classes.py:320-348) for a tree of the forest."""
    md = params["max_depth"]
    max_depth = np.iinfo(np.int32).max if md is None else int(md)
    msl = params["min_samples_leaf"]
    min_samples_leaf = int(msl) if isinstance(msl, numbers.Integral) else int(ceil(msl * n_samples))
    mss = params["min_samples_split"]
    if isinstance(mss, numbers.Integral):
        min_samples_split = int(mss)
    else:
        min_samples_split = max(2, int(ceil(mss * n_samples)))
    min_samples_split = max(min_samples_split, 2 * min_samples_leaf)
    mf = params["max_features"]
    if isinstance(mf, str):
        max_features = max(1, int(np.sqrt(n_features))) if mf == "sqrt" else max(1, int(np.log2(n_features)))
    elif mf is None:
        max_features = n_features
    elif isinstance(mf, numbers.Integral):
        max_features = int(mf)
    else:
        max_features = max(1, int(mf * n_features)) if mf > 0.0 else 0
    return dict(max_depth=max_depth, min_samples_split=min_samples_split, min_samples_leaf=min_samples_leaf,
                max_features=max_features)


def tree_seeds(random_state, n_estimators: int) -> np.ndarray:
    """The integer random_state of each tree: _make_estimator's draws from check_random_state(random_state)."""
    from sklearn.utils import check_random_state
    rs = check_random_state(random_state)
    return np.array([rs.randint(np.iinfo(np.int32).max) for _ in range(n_estimators)], np.int64)


def bootstrap_counts(seed: int, n_samples: int) -> np.ndarray:
    """bincount of _generate_sample_indices(seed, n, n): the tree's sample weights."""
    idx = np.random.RandomState(seed).randint(0, n_samples, n_samples, dtype=np.int32)
    return np.bincount(idx, minlength=n_samples).astype(np.int32)


def splitter_seed(seed: int) -> int:
    """The splitter's initial xorshift state: check_random_state(seed).randint(0, RAND_R_MAX)."""
    return int(np.random.RandomState(seed).randint(0, RAND_R_MAX))


def prepare(estimator, X, y):
    """Validation and encoding as RandomForestClassifier.fit does them.  Returns (X float32 C-order, y_encoded int32, classes,
    resolved params)."""
    from scipy.sparse import issparse
    from sklearn.utils.validation import validate_data
    params = estimator.get_params()
    check_supported(params)
    estimator._validate_params()
    if issparse(y):
        raise ValueError("sparse multilabel-indicator for y is not supported.")
    if issparse(X):
        raise RssegUnsupported("forest_fit: sparse X is not supported on the GPU")
    X, y = validate_data(estimator, X, y, multi_output=True, accept_sparse="csc", dtype=np.float32, ensure_all_finite=False)
    type(estimator.estimator)(criterion=estimator.criterion)._compute_missing_values_in_feature_mask(
        X, estimator_name=estimator.__class__.__name__)   # raises on inf, as fit does
    if np.isnan(X).any():
        raise RssegUnsupported("forest_fit: X contains NaN (the missing-value search is not implemented on the GPU)")
    y = np.atleast_1d(y)
    if y.ndim == 2 and y.shape[1] == 1:
        import warnings
        from sklearn.exceptions import DataConversionWarning
        warnings.warn("A column-vector y was passed when a 1d array was expected. Please change the shape of y to "
                      "(n_samples,), for example using ravel().", DataConversionWarning, stacklevel=3)
        y = y.reshape(-1)
    if y.ndim != 1:
        raise RssegUnsupported(f"forest_fit: multi-output y ({y.shape[1]} outputs) is not supported on the GPU")
    from sklearn.utils.multiclass import check_classification_targets
    check_classification_targets(y)
    classes, y_enc = np.unique(y, return_inverse=True)
    n, F = X.shape
    if F > MAX_FEATURES or len(classes) > MAX_CLASSES:
        raise RssegUnsupported(f"forest_fit: {F} features, {len(classes)} classes: at most {MAX_FEATURES} of each on the GPU")
    if n >= MAX_SAMPLES:
        raise RssegUnsupported(f"forest_fit: {n} samples: fewer than {MAX_SAMPLES} on the GPU")
    return np.ascontiguousarray(X), y_enc.astype(np.int32).reshape(-1), classes, resolve_params(params, n, F)


def assemble_tree(tree, nodes: dict, n_features: int, n_classes: int, max_features: int, classes_f) -> None:
    """Sets the fitted state of DecisionTreeClassifier `tree` from K16's node arrays (the layout of Tree.__getstate__)."""
    from sklearn.tree._tree import Tree
    k = len(nodes["left"])
    rec = np.zeros(k, dtype=Tree(n_features, np.array([n_classes], np.intp), 1).__getstate__()["nodes"].dtype)
    rec["left_child"] = nodes["left"]
    rec["right_child"] = nodes["right"]
    rec["feature"] = nodes["feature"]
    rec["threshold"] = nodes["threshold"]
    rec["impurity"] = nodes["impurity"]
    rec["n_node_samples"] = nodes["n_node_samples"]
    rec["weighted_n_node_samples"] = nodes["weighted_n_node_samples"].astype(np.float64)
    rec["missing_go_to_left"] = nodes["missing_go_to_left"]
    t = Tree(n_features, np.array([n_classes], np.intp), 1)
    t.__setstate__({"max_depth": int(nodes["max_depth"]), "node_count": k, "nodes": rec,
                    "values": np.ascontiguousarray(nodes["value"], np.float64).reshape(k, 1, n_classes)})
    tree.n_features_in_ = n_features
    tree.n_outputs_ = 1
    tree.classes_ = classes_f.copy()
    tree.n_classes_ = np.int64(n_classes)
    tree.max_features_ = max_features
    tree.tree_ = t


def tree_nodes(tree) -> dict:
    """The node arrays of a fitted DecisionTreeClassifier in K16's layout (the inverse of assemble_tree)."""
    st = tree.tree_.__getstate__()
    nd = st["nodes"]
    return dict(left=nd["left_child"].astype(np.int32), right=nd["right_child"].astype(np.int32), feature=nd["feature"].astype(np.int32),
                threshold=nd["threshold"].copy(), impurity=nd["impurity"].copy(), n_node_samples=nd["n_node_samples"].astype(np.int32),
                weighted_n_node_samples=nd["weighted_n_node_samples"].astype(np.int32), missing_go_to_left=nd["missing_go_to_left"].copy(),
                value=st["values"][:, 0, :].copy(), max_depth=int(st["max_depth"]))


def assemble_forest(estimator, trees_nodes, seeds, n_samples: int, n_features: int, classes, max_features: int) -> None:
    """The forest's fitted attributes, as RandomForestClassifier.fit sets them (n_outputs 1, no oob, no warm start)."""
    from sklearn.ensemble._forest import _get_n_samples_bootstrap
    C = len(classes)
    estimator._n_samples = n_samples
    estimator.n_outputs_ = 1
    estimator.n_features_in_ = n_features
    estimator._n_samples_bootstrap = _get_n_samples_bootstrap(n_samples, estimator.max_samples) if estimator.bootstrap else None
    estimator._validate_estimator()
    classes_f = np.arange(C, dtype=np.float64)
    ests = []
    for nodes, seed in zip(trees_nodes, seeds):
        tree = estimator._make_estimator(append=False, random_state=np.random.RandomState(0))
        tree.set_params(random_state=int(seed))
        assemble_tree(tree, nodes, n_features, C, max_features, classes_f)
        ests.append(tree)
    estimator.estimators_ = ests
    estimator.classes_ = classes
    estimator.n_classes_ = C


def _fit_on_device(estimator, X, y, ctx, before_growing=None):
    """The steps of `fit`.  Returns what an out-of-bag pass over the training set needs besides the fitted estimator: the
    context, the device planes and bootstrap counts (uploaded once) and the encoded labels."""
    from .runtime import default_context
    X, y_enc, classes, rp = prepare(estimator, X, y)
    if before_growing is not None:
        before_growing()
    n, F = X.shape
    C = len(classes)
    T = int(estimator.n_estimators)
    seeds = tree_seeds(estimator.random_state, T)
    if estimator.bootstrap:
        counts = np.stack([bootstrap_counts(int(s), n) for s in seeds]) if T else np.zeros((0, n), np.int32)
    else:
        counts = np.ones((1, n), np.int32)
    m = (counts > 0).sum(axis=1)
    caps = 2 * (m if estimator.bootstrap else np.repeat(m, T)) - 1
    xs = np.array([splitter_seed(int(s)) for s in seeds], np.uint32)
    trees = []
    planes = d_counts = None
    if T:
        ctx = ctx if ctx is not None else default_context()
        planes = [ctx.upload_f32(np.ascontiguousarray(X[:, f])) for f in range(F)]
        d_y = ctx.to_device(y_enc, np.int32)
        d_counts = ctx.to_device(counts.reshape(-1), np.int32)
        trees = ctx.forest_fit(planes, d_y, d_counts, xs, caps, rp["max_depth"], rp["min_samples_split"], rp["min_samples_leaf"],
                               rp["max_features"], C)
    assemble_forest(estimator, trees, seeds, n, F, classes, rp["max_features"])
    return estimator, ctx, planes, d_counts, y_enc


def fit(estimator, X, y, ctx=None):
    """Fits the unfitted RandomForestClassifier `estimator` on the GPU and returns it (bit-identical to estimator.fit(X, y))."""
    return _fit_on_device(estimator, X, y, ctx)[0]


def fit_oob(estimator, X, y, ctx=None):
    """`fit` for an estimator whose oob_score is True or a callable: the forest is grown as `fit` grows it (the setting held
    aside meanwhile, so `prepare` and `check_supported` keep refusing it), then loaded and walked over the training
    planes by rsseg_forest_oob with the bootstrap counts already on the device, and the host finishes as
    _forest.py:558-622, 805-827 do.  Returns the estimator with oob_decision_function_ and oob_score_ set and the
    parameter restored: its whole state equals RandomForestClassifier(oob_score=...).fit(X, y)."""
    from .forest import _flat_for_proba, oob_device, oob_finish
    scoring = estimator.oob_score
    if not (scoring is True or callable(scoring)):
        raise ValueError(f"fit_oob: oob_score={scoring!r}: True or a callable (use fit otherwise)")

    def bootstrap_needed():   # where RandomForestClassifier.fit raises it: after the validation of X and y (_forest.py:446)
        if not estimator.bootstrap:
            raise ValueError("Out of bag estimation only available if bootstrap=True")

    estimator.oob_score = False
    try:
        _, ctx, planes, d_counts, y_enc = _fit_on_device(estimator, X, y, ctx, before_growing=bootstrap_needed)
    finally:
        estimator.oob_score = scoring
    oob, n_oob = oob_device(ctx, _flat_for_proba(estimator), planes, d_counts)
    estimator.oob_decision_function_, estimator.oob_score_ = oob_finish(oob, n_oob, y_enc, None if scoring is True else scoring)
    return estimator
