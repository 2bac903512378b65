"""
Nodata-aware classification: the classifiers run on the VALID pixels of a raster only, by K19's order-preserving compaction
(Context.compact_plan / compact / expand, csrc/k19_compact.hip).

  mask (H, W) or flat, non-zero = valid  ->  plan  ->  X[valid] in raster order  ->  the unchanged entry point  ->  expand + fill

X[valid] is exactly the matrix scikit-learn sees for KMeans(...).fit_predict(MinMaxScaler().fit_transform(X[valid])), so the
seeds, the iteration count and the labels of the masked fit are those of the unmasked fit on the compacted planes, and the
classifier's cost shrinks by the share of nodata.  Nodata pixels no longer set the scaler's range, are never drawn as
k-means++ seeds and pull no centre; the forest does not walk its trees for them.

Feature extraction is not masked: a window feature within its window's reach of the collar has still seen the collar.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

NO_VALID = "no valid pixels"


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .runtime import default_context
    return default_context()


def mask_to_device(ctx, mask, n: int):
    """A mask as compact_plan takes it: a host array (any dtype, any shape of n elements; non-zero = valid) is uploaded as 0 / 1
    bytes, a device tensor is taken as it is (flat uint8)."""
    if isinstance(mask, np.ndarray) or not hasattr(mask, "numel"):
        a = np.asarray(mask)
        if a.size != n:
            raise ValueError(f"mask: {a.size} elements, the planes have {n} pixels")
        return ctx.to_device(np.ascontiguousarray(a != 0, dtype=np.uint8).reshape(-1))
    if mask.numel() != n:
        raise ValueError(f"mask: {mask.numel()} elements, the planes have {n} pixels")
    return mask


def make_plan(ctx, mask, n: int):
    """compact_plan of `mask`; ValueError("no valid pixels") when the mask is empty."""
    plan = ctx.compact_plan(mask_to_device(ctx, mask, n))
    if plan.n_valid == 0:
        raise ValueError(NO_VALID)
    return plan


def planes_to_device(ctx, planes: Sequence, float32_only: bool = False):
    """(device planes, host?, shape): host planes are stacked to float32 iff every one is float32 (np.vstack's promotion, as the
    unmasked entry points do), else float64; float32_only: the forest's cast (RandomForestClassifier.predict, _forest.py:640)."""
    host = isinstance(planes[0], np.ndarray)
    if not host:
        return list(planes), False, None
    shape = planes[0].shape
    if float32_only:
        dt = np.float32
    else:
        dt = np.result_type(*[p.dtype for p in planes])
        dt = np.float32 if dt == np.float32 else np.float64
    return [ctx.to_device(np.ascontiguousarray(p, dtype=dt).reshape(-1)) for p in planes], True, shape


def kmeans_fit_predict_masked(planes: Sequence, mask, n_clusters: int, seed: int = 42, max_iter: int = 300, tol: float = 1e-4, fill: int = -1,
                              ctx=None):
    """Context.kmeans_fit_predict on the valid pixels only -> (labels over the whole raster, meta).
    planes: NumPy arrays of one shape (labels come back as an int32 array of that shape) or flat device tensors (a flat device
    tensor comes back); mask: non-zero = valid, of the planes' size.  Masked pixels get `fill`.
    meta is kmeans_fit_predict's own (centers, scale, min, mean, n_iter, relocated, tol, init_indices, timings) plus n_valid.
    init_indices are in COMPACTED numbering: seed j is the init_indices[j]-th valid pixel in raster order, i.e. pixel
    np.flatnonzero(mask)[init_indices[j]] of the raster.
    ValueError: "no valid pixels" for an empty mask; the fit's own "n_samples=... should be >= n_clusters=..." when fewer valid
    pixels than clusters."""
    ctx = _ctx(ctx)
    dev, host, shape = planes_to_device(ctx, planes)
    plan = make_plan(ctx, mask, dev[0].numel())
    labels_c, meta = ctx.kmeans_fit_predict(ctx.compact(plan, dev), int(n_clusters), seed, max_iter, tol)
    labels = ctx.expand(plan, labels_c, fill)
    meta = dict(meta)
    meta["n_valid"] = plan.n_valid
    return (labels.cpu().numpy().reshape(shape) if host else labels), meta


def kmeans_predict_masked(ctx, planes: Sequence, mask, centers, scale, min_, want_distance: bool = False, want_summary: bool = False,
                          fill: int = -1):
    """Context.kmeans_predict on the valid pixels of flat device planes -> (labels with `fill`, distance with NaN or None, summary
    or None, n_valid).  Counts and inertia cover the valid pixels only."""
    plan = make_plan(ctx, mask, planes[0].numel())
    labels_c, dist_c, summary = ctx.kmeans_predict(ctx.compact(plan, planes), centers, scale, min_, want_distance=want_distance,
                                                   want_summary=want_summary)
    labels = ctx.expand(plan, labels_c, fill)
    dist = None if dist_c is None else ctx.expand(plan, dist_c, float("nan"))
    return labels, dist, summary, plan.n_valid


def _forest_planes(features):
    features = np.asarray(features)
    if features.ndim != 3:
        raise ValueError("features must be a 3-D array (height, width, n_features)")
    # the pixels the unmasked path classifies: NaN -> 0 (supervised_classification_predict, extract.py:690-719)
    return features.shape[:2], [np.nan_to_num(features[:, :, i], nan=0.0) for i in range(features.shape[2])]


def forest_predict_masked(model, features, mask, fill=0, ctx=None) -> np.ndarray:
    """supervised_classification_predict on the valid pixels only: (H, W) class labels in the dtype of classes_, `fill` at the
    masked pixels.  The trees are walked for the valid pixels alone.  model: a fitted forest or a flattened dict."""
    from .forest import _check_width, flatten_forest
    ctx = _ctx(ctx)
    (h, w), planes = _forest_planes(features)
    flat = model if isinstance(model, dict) else flatten_forest(model)
    _check_width(flat, len(planes))
    dev, _, _ = planes_to_device(ctx, planes, float32_only=True)
    plan = make_plan(ctx, mask, h * w)
    ctx.forest_load(flat)
    out = ctx.expand(plan, ctx.forest_predict(ctx.compact(plan, dev)), fill)
    return out.cpu().numpy().astype(np.asarray(flat["classes"]).dtype, copy=False).reshape(h, w)


def forest_proba_and_confidence_masked(model, features, mask, ctx=None):
    """image_proba_and_confidence on the valid pixels only: ((H, W, C) float64 probabilities, (H, W) float64 confidence), rows
    of 0 and confidence 0 at the masked pixels."""
    from .forest import _check_width, _flat_for_proba
    ctx = _ctx(ctx)
    (h, w), planes = _forest_planes(features)
    flat = _flat_for_proba(model)
    _check_width(flat, len(planes))
    dev, _, _ = planes_to_device(ctx, planes, float32_only=True)
    plan = make_plan(ctx, mask, h * w)
    ctx.forest_load(flat)
    p, c, _ = ctx.forest_predict_proba(ctx.compact(plan, dev), proba=True, confidence=True)
    proba = np.stack([ctx.expand(plan, p[k], 0.0).cpu().numpy() for k in range(len(p))], axis=-1)
    return proba.reshape(h, w, -1), ctx.expand(plan, c, 0.0).cpu().numpy().reshape(h, w)
