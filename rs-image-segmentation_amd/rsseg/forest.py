"""sklearn RandomForestClassifier -> the flat arrays rsseg_forest_load takes, and the host side of K11's outputs beyond the
label: predict_proba / predict_image_proba / confidence_map (rsseg_forest_predict_proba) and the out-of-bag estimate
(rsseg_forest_oob), each equal to scikit-learn's value bit for bit (host plumbing only).
tree_ node records: children_left/right (-1 = leaf), feature, threshold (float64), missing_go_to_left,
value (n_nodes, 1, n_classes) class fractions (sklearn >= 1.3) — SURVEY.md §8c item 2."""
from __future__ import annotations

import numpy as np


def flatten_forest(model) -> dict:
    offs, left, right, feat, thr, miss, val = [0], [], [], [], [], [], []
    n_classes = len(model.classes_)
    for est in model.estimators_:
        t = est.tree_
        left.append(np.asarray(t.children_left, np.int32))
        right.append(np.asarray(t.children_right, np.int32))
        feat.append(np.asarray(t.feature, np.int32))
        thr.append(np.asarray(t.threshold, np.float64))
        mg = getattr(t, "missing_go_to_left", None)
        miss.append(np.zeros(t.node_count, np.uint8) if mg is None else np.asarray(mg, np.uint8))
        v = np.asarray(t.value[:, 0, :n_classes], np.float64)
        s = v.sum(axis=1, keepdims=True)
        if not np.allclose(s[s > 0], 1.0):  # models pickled by sklearn < 1.3 store counts
            s[s == 0] = 1.0
            v = v / s
        val.append(v)
        offs.append(offs[-1] + t.node_count)
    return dict(tree_off=np.asarray(offs, np.int64), left=np.concatenate(left), right=np.concatenate(right),
                feature=np.concatenate(feat), threshold=np.concatenate(thr), missing_left=np.concatenate(miss),
                value=np.ascontiguousarray(np.concatenate(val)), classes=np.asarray(model.classes_),
                n_features=int(model.n_features_in_))


# ---- class probabilities, confidence, out-of-bag estimate (K11's outputs beyond the label) ----------------------------
def _flat_for_proba(model) -> dict:
    """The flattened forest with class indices 0..C-1 in place of classes_ (probabilities do not need the labels, and
    classes_ may hold strings)."""
    flat = dict(model if isinstance(model, dict) else flatten_forest(model))
    flat["classes"] = np.arange(np.asarray(flat["value"]).shape[1], dtype=np.int64)
    return flat


def _check_width(flat: dict, width: int) -> None:
    if width != int(flat["n_features"]):   # sklearn's wording (validate_data), raised before any device call
        raise ValueError(f"X has {width} features, but the forest is expecting {int(flat['n_features'])} features as input.")


def _outputs(model, planes, proba: bool, confidence: bool, ctx=None):
    """One launch of rsseg_forest_predict_proba over host planes (cast to float32 as RandomForestClassifier.predict does,
    _forest.py:640).  Returns host arrays (proba (n, C) or None, confidence (n,) or None)."""
    from .runtime import default_context
    flat = _flat_for_proba(model)
    _check_width(flat, len(planes))
    ctx = ctx if ctx is not None else default_context()
    ctx.forest_load(flat)
    dev = [ctx.to_device(np.ascontiguousarray(p, dtype=np.float32).reshape(-1)) for p in planes]
    p, c, _ = ctx.forest_predict_proba(dev, proba=proba, confidence=confidence)
    return (None if p is None else p.t().contiguous().cpu().numpy()), (None if c is None else c.cpu().numpy())


def predict_proba(model, X, ctx=None) -> np.ndarray:
    """RandomForestClassifier.predict_proba on the GPU, bit for bit: (n, C) float64.  model: a fitted forest or a
    flattened dict (flatten_forest)."""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    return _outputs(model, [X[:, f] for f in range(X.shape[1])], True, False, ctx)[0]


def _image_planes(features):
    features = np.asarray(features)
    if features.ndim != 3:
        raise ValueError("features must be a 3-D array (height, width, n_features)")
    return features.shape[:2], [features[:, :, i] for i in range(features.shape[2])]


def predict_image_proba(model, features, ctx=None) -> np.ndarray:
    """predict_proba of every pixel of an (H, W, D) feature array: (H, W, C) float64."""
    (h, w), planes = _image_planes(features)
    return _outputs(model, planes, True, False, ctx)[0].reshape(h, w, -1)


def confidence_map(model, features, ctx=None) -> np.ndarray:
    """The largest class probability of every pixel of an (H, W, D) feature array: (H, W) float64."""
    (h, w), planes = _image_planes(features)
    return _outputs(model, planes, False, True, ctx)[1].reshape(h, w)


def image_proba_and_confidence(model, features, ctx=None, mask=None):
    """predict_image_proba and confidence_map from one launch.  mask ((H, W), non-zero = valid): the forest walks the valid
    pixels only; the masked pixels get probability rows of 0 and confidence 0 (rsseg.masked)."""
    if mask is not None:
        from .masked import forest_proba_and_confidence_masked
        return forest_proba_and_confidence_masked(model, features, mask, ctx)
    (h, w), planes = _image_planes(features)
    p, c = _outputs(model, planes, True, True, ctx)
    return p.reshape(h, w, -1), c.reshape(h, w)


OOB_WARNING = ("Some inputs do not have OOB scores. This probably means too few trees were used to compute any reliable OOB "
               "estimates.")   # _forest.py:611-618


def oob_finish(oob, n_oob, y_enc, scoring=None):
    """The host end of the out-of-bag estimate (_forest.py:609-622, 805-827).  oob: (C, n) float64 as rsseg_forest_oob
    writes it (already divided by max(n_oob, 1)); n_oob: (n,) counts of out-of-bag trees; y_enc: (n,) class indices.
    Returns (oob_decision_function (n, C), oob_score): scikit-learn's UserWarning when a sample has no out-of-bag tree,
    the score from accuracy_score (or `scoring`) on the encoded float64 column y that fit holds at that point."""
    import warnings
    from sklearn.metrics import accuracy_score
    if (np.asarray(n_oob) == 0).any():
        warnings.warn(OOB_WARNING, UserWarning, stacklevel=3)
    dec = np.ascontiguousarray(np.asarray(oob, np.float64).T)
    y_col = np.ascontiguousarray(np.asarray(y_enc).reshape(-1, 1), dtype=np.float64)
    score = (accuracy_score if scoring is None else scoring)(y_col, np.argmax(dec, axis=1))
    return dec, score


def oob_device(ctx, flat: dict, planes, d_counts):
    """Loads `flat` and runs rsseg_forest_oob over device planes and counts -> host (oob (C, n), n_oob (n,))."""
    ctx.forest_load(flat)
    oob, n_oob = ctx.forest_oob(planes, d_counts)
    return oob.cpu().numpy(), n_oob.cpu().numpy()


def check_oob_model(model) -> None:
    """Raises RssegUnsupported naming the setting of a fitted forest the out-of-bag kernel does not cover."""
    from .runtime import RssegUnsupported
    if not getattr(model, "bootstrap", True):
        raise RssegUnsupported("oob_estimate: bootstrap=False: the out-of-bag estimate needs a forest fitted with bootstrap=True")
    if getattr(model, "max_samples", None) is not None:
        raise RssegUnsupported(f"oob_estimate: max_samples={model.max_samples!r} is not supported on the GPU (only max_samples=None)")
    if getattr(model, "n_outputs_", 1) != 1:
        raise RssegUnsupported(f"oob_estimate: multi-output forest ({model.n_outputs_} outputs) is not supported on the GPU")


def oob_estimate(model, X, y, ctx=None):
    """The out-of-bag estimate of any fitted bootstrap forest (scikit-learn's or K16's) on its training set (X, y):
    (oob_decision_function (n, C), oob_score), equal to the attributes RandomForestClassifier(oob_score=True).fit sets.
    Each tree's bootstrap is redrawn from its random_state (forest_fit.bootstrap_counts); the score is accuracy, or the
    forest's own oob_score when that is a callable."""
    from .forest_fit import bootstrap_counts
    from .runtime import default_context
    check_oob_model(model)
    flat = _flat_for_proba(model)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"Expected 2D array, got {X.ndim}D array instead")
    _check_width(flat, X.shape[1])
    n = X.shape[0]
    classes, y_enc = np.unique(np.asarray(y).reshape(-1), return_inverse=True)
    if len(y_enc) != n or not np.array_equal(classes, np.asarray(model.classes_)):
        raise ValueError("oob_estimate: (X, y) is not the training set of the forest (other length or other classes)")
    counts = np.stack([bootstrap_counts(int(t.random_state), n) for t in model.estimators_])
    ctx = ctx if ctx is not None else default_context()
    planes = [ctx.to_device(np.ascontiguousarray(X[:, f], dtype=np.float32)) for f in range(X.shape[1])]
    oob, n_oob = oob_device(ctx, flat, planes, ctx.to_device(counts.reshape(-1), np.int32))
    scoring = model.oob_score if callable(getattr(model, "oob_score", None)) else None
    return oob_finish(oob, n_oob, y_enc, scoring)
