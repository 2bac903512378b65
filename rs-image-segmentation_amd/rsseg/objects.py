"""
Object features per segment and object-based classification (K25, csrc/k25_objects.hip).  This goes beyond the reference, which
has no segmentation step: object_table() takes, in one pass over the raster on the GPU, what describes every segment of a
segment map (rsseg.segment.slic) as exact integers; object_features() turns that table into a float64 feature matrix (mean,
spread, extremes, size, shape); training_segments() picks the segments that carry ground truth; classify_objects() trains a
forest (K16) or a Gaussian classifier (K22) on those, labels every segment and paints the labels back.

The table is rsseg_segment_features' (include/rsseg.h): int64 [(n_segments + 1), 11 + 4 P], restated in NumPy in
tests/objects_ref.py, to which it is equal bit for bit.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import segment as SG
from .runtime import Context, RssegUnsupported

GEO_COLUMNS = 11
STATS = ("mean", "std", "min", "max")
SHAPE_COLUMNS = ("area", "centroid_y", "centroid_x", "bbox_h", "bbox_w", "extent", "perimeter", "compactness", "axis_ratio", "orientation")
FOREST_METHODS = ("random_forest",)
GAUSS_METHODS = {"maximum_likelihood": "ml", "mahalanobis": "mahalanobis", "minimum_distance": "mindist"}
Q_SCALE_BITS, Q2_SCALE_BITS = 40, 24     # a float32 plane's columns: sum q in units of 2^-40, sum q2 in units of 2^-24


class ObjectFeatures(NamedTuple):
    table: np.ndarray      # int64 [(n + 1), 11 + 4 P]
    X: np.ndarray          # float64 [(n + 1), D]; row 0 and empty segments NaN
    columns: List[str]
    area: np.ndarray       # int64 [n + 1]


class ObjectClassification(NamedTuple):
    class_map: object      # uint8 (H, W): NumPy, or a device tensor with device=True
    table: np.ndarray      # uint8 [n + 1]: the class of every segment, 0 = none
    model: object
    X: np.ndarray
    columns: List[str]
    train_idx: np.ndarray
    train_y: np.ndarray


def check_moment_range(shape) -> None:
    """The coordinate moments of an (H, W) raster stay inside int64 when H W max(H, W)^2 < 2^63 (32768 x 32768 does);
    RssegUnsupported otherwise.  A pure function of the shape."""
    h, w = int(shape[0]), int(shape[1])
    if h * w * max(h, w) ** 2 >= 2 ** 63:
        raise RssegUnsupported(f"object_table: a raster of {h} x {w} pixels: H W max(H, W)^2 reaches 2^63, the coordinate moments leave int64")


def _planes_arg(planes, what: str):
    if SG._is_tensor(planes) or isinstance(planes, np.ndarray) or len(planes):
        return SG._plane_list(planes, "planes", what)
    return []


def object_table(segments, planes=(), mask=None, n_segments: Optional[int] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """int64 NumPy table [(n_segments + 1), 11 + 4 P] of rsseg_segment_features over the pixels of every segment whose mask byte is
    non-zero: n, sum y, sum x, sum y^2, sum x^2, sum y x, min y, max y, min x, max x, perimeter, then per plane sum q, sum q2,
    min q, max q (uint8: q = v, q2 = v v; float32: q = llrint(v 2^40), q2 = llrint(v v 2^24)).  uint8 and float32 planes may be
    mixed and be more than 16: they go in calls of at most 16 of one dtype, the geometry in the first call only.  float32 planes
    are checked as segment_means checks them (no NaN, |v| < 2^11, largest area * max|v| < 2^23 over the counted pixels;
    ValueError naming the plane)."""
    import torch
    seg = SG.check_segments(segments, "object_table")
    pls = _planes_arg(planes, "object_table")
    shape = SG._check_shapes(pls, "planes", "object_table", shape=seg.shape)
    for i, p in enumerate(pls):
        if not SG._is_u8(p) and p.dtype != (torch.float32 if SG._is_tensor(p) else np.float32):
            raise ValueError(f"object_table: planes[{i}] must be uint8 or float32, got {p.dtype}")
    mask = SG._check_mask(mask, shape, "object_table")
    check_moment_range(shape)
    ctx = SG._context(ctx, "object_table")
    d_seg, h, w, ns = SG._upload_segments(ctx, seg, n_segments)
    dmask = SG._dev_mask(ctx, mask)
    out = np.zeros((ns + 1, GEO_COLUMNS + 4 * len(pls)), np.int64)
    out[:, :GEO_COLUMNS] = ctx.segment_features(d_seg, h, w, ns, (), mask=dmask, geometry=True).cpu().numpy()
    max_area = int(out[:, 0].max())
    for p0 in range(0, len(pls), SG.MAX_PLANES):
        for is_u8 in (True, False):
            idx = [i for i in range(p0, min(p0 + SG.MAX_PLANES, len(pls))) if SG._is_u8(pls[i]) == is_u8]
            if not idx:
                continue
            dev = [SG._dev_flat(ctx, pls[i], torch.uint8 if is_u8 else torch.float32) for i in idx]
            if not is_u8:
                for i, d in zip(idx, dev):
                    SG._check_float_domain(ctx, d, f"planes[{i}]", dmask, max_area)
            t = ctx.segment_features(d_seg, h, w, ns, dev, mask=dmask, geometry=False).cpu().numpy()
            for j, i in enumerate(idx):
                out[:, GEO_COLUMNS + 4 * i:GEO_COLUMNS + 4 * i + 4] = t[:, GEO_COLUMNS + 4 * j:GEO_COLUMNS + 4 * j + 4]
    return out


# ---- the feature matrix ------------------------------------------------------------------------------------------------------
def _ints(col) -> np.ndarray:
    """an int64 column as Python integers: products and differences below are exact"""
    return np.asarray(col).astype(object)


_true_div = np.frompyfunc(lambda a, b: a / b if b else math.nan, 2, 1)   # int / int: correctly rounded
_to_float = np.frompyfunc(float, 1, 1)


def _ratio(num, den) -> np.ndarray:
    """the correctly rounded float64 of the exact rationals num / den (object arrays of Python integers); NaN where den == 0"""
    return _true_div(num, den).astype(np.float64)


def plane_statistics(table: np.ndarray, p: int, is_u8: bool):
    """(mean, var, min, max) float64 [n + 1] of plane p of an object table.  mean and var are the correctly rounded float64 of the
    exact rationals sum q / (n s1) and (n sum q2 s1^2 / s2 - (sum q)^2) / (n s1)^2, s1 / s2 the plane's fixed-point scales (1 / 1
    for uint8, 2^40 / 2^24 for float32); var is clamped at 0.  Empty rows are NaN."""
    n = _ints(table[:, 0])
    c = GEO_COLUMNS + 4 * p
    s1, s2 = _ints(table[:, c]), _ints(table[:, c + 1])
    b1, b2 = (0, 0) if is_u8 else (Q_SCALE_BITS, Q2_SCALE_BITS)
    mean = _ratio(s1, n * (1 << b1))
    num = n * s2 * (1 << (2 * b1 - b2)) - s1 * s1
    num = np.where(num > 0, num, 0)
    var = _ratio(num, n * n * (1 << (2 * b1)))
    empty = table[:, 0] == 0
    scale = 2.0 ** -b1
    with np.errstate(invalid="ignore"):
        mn = np.where(empty, np.nan, table[:, c + 2].astype(np.float64) * scale)   # |q| < 2^51: exact
        mx = np.where(empty, np.nan, table[:, c + 3].astype(np.float64) * scale)
    return mean, var, mn, mx


def shape_statistics(table: np.ndarray) -> np.ndarray:
    """float64 [(n + 1), 10]: SHAPE_COLUMNS from the geometry columns of an object table; empty rows are NaN.
    extent = n / (bbox_h bbox_w); compactness = 4 pi n / perimeter^2 (1 for a disc, pi / 4 for a square of pixels counted by
    sides); axis_ratio = sqrt(lambda_min / lambda_max) of the coordinate scatter matrix [[M_yy, M_xy], [M_xy, M_xx]] with the
    exact integers M_yy = n sum y^2 - (sum y)^2, M_xx = n sum x^2 - (sum x)^2, M_xy = n sum y x - sum y sum x (1 where
    lambda_max = 0); orientation = atan2(2 M_xy, M_xx - M_yy) / 2, the angle of the long axis from the x axis."""
    t = table
    n = t[:, 0].astype(np.float64)
    empty = t[:, 0] == 0
    N, Sy, Sx, Syy, Sxx, Syx = (_ints(t[:, c]) for c in range(6))
    myy, mxx, mxy = N * Syy - Sy * Sy, N * Sxx - Sx * Sx, N * Syx - Sy * Sx
    det = myy * mxx - mxy * mxy                                    # >= 0 (Cauchy-Schwarz), exact
    det = np.where(det > 0, det, 0)
    disc = (myy - mxx) * (myy - mxx) + 4 * mxy * mxy
    f = lambda a: _to_float(a).astype(np.float64)                  # noqa: E731 — int -> float64, correctly rounded
    with np.errstate(divide="ignore", invalid="ignore"):
        lam_max = (f(myy + mxx) + np.sqrt(f(disc))) / 2.0
        axis = np.where(lam_max > 0, np.sqrt(f(det)) / lam_max, 1.0)   # sqrt(lambda_min / lambda_max), lambda_min = det / lambda_max
        orient = 0.5 * np.arctan2(f(2 * mxy), f(mxx - myy))
        bh = (t[:, 7] - t[:, 6] + 1).astype(np.float64)
        bw = (t[:, 9] - t[:, 8] + 1).astype(np.float64)
        per = t[:, 10].astype(np.float64)
        cols = [n, t[:, 1].astype(np.float64) / n, t[:, 2].astype(np.float64) / n, bh, bw, n / (bh * bw), per,
                4.0 * math.pi * n / (per * per), axis, orient]
    out = np.stack(cols, axis=1)
    out[empty] = np.nan
    return out


def features_from_table(table: np.ndarray, plane_is_u8: Sequence[bool], names=None, stats=STATS, shape: bool = True) -> ObjectFeatures:
    """object_features' second half: the feature matrix of an object table (no device needed)."""
    table = np.asarray(table)
    P = len(plane_is_u8)
    if table.ndim != 2 or table.dtype != np.int64 or table.shape[1] != GEO_COLUMNS + 4 * P:
        raise ValueError(f"object_features: the table must be int64 [(n + 1), {GEO_COLUMNS + 4 * P}] for {P} planes, got {table.dtype} {table.shape}")
    names = [f"p{i}" for i in range(P)] if names is None else [str(s) for s in names]
    if len(names) != P:
        raise ValueError(f"object_features: {len(names)} names for {P} planes")
    stats = tuple(stats)
    for s in stats:
        if s not in STATS:
            raise ValueError(f"object_features: stats holds {s!r}, must be among {STATS}")
    cols, columns = [], []
    for p in range(P):
        if not stats:
            break
        mean, var, mn, mx = plane_statistics(table, p, bool(plane_is_u8[p]))
        have = {"mean": mean, "std": np.sqrt(var), "min": mn, "max": mx}
        for s in stats:
            cols.append(have[s])
            columns.append(f"{names[p]}_{s}")
    X = np.stack(cols, axis=1) if cols else np.zeros((table.shape[0], 0), np.float64)
    if shape:
        X = np.concatenate([X, shape_statistics(table)], axis=1)
        columns += list(SHAPE_COLUMNS)
    X[table[:, 0] == 0] = np.nan
    return ObjectFeatures(table, X, columns, table[:, 0].copy())


def object_features(segments, planes, names=None, stats=STATS, shape: bool = True, mask=None, n_segments: Optional[int] = None,
                    ctx: Optional[Context] = None, neighbours: bool = False) -> ObjectFeatures:
    """ObjectFeatures(table, X, columns, area): X is float64 [(n + 1), D] with, per plane, <name>_mean, _std, _min, _max (those
    named in `stats`; names default to p0, p1, ...) and, with shape, SHAPE_COLUMNS (shape_statistics).  Row 0 and segments
    without a counted pixel are NaN.
    Means and variances are the correctly rounded float64 of exact rationals of the integer table (plane_statistics), std =
    sqrt(var).  For uint8 planes they are the exact population statistics of the pixels.  For float32 planes the table holds
    sum llrint(v 2^40) and sum llrint(v^2 2^24): per term the square is off by at most 2^-25 and the mean by at most 2^-41, so
    the variance is within 2^-24 of the population variance of the inputs.  _min / _max of a float32 plane are the extremes of
    llrint(v 2^40) 2^-40: the value itself where |v| >= 2^-16, else rounded to 2^-40.
    neighbours: append the columns of rsseg.regions.neighbour_features (n_neighbours, shared_border, per plane
    <name>_boundary_contrast and <name>_neighbour_diff) from the region adjacency graph of the segments (K27: at most 16 planes;
    float planes cross a border as slic() quantises them, in 8-bit steps of their own finite range)."""
    pls = _planes_arg(planes, "object_features")
    table = object_table(segments, pls, mask=mask, n_segments=n_segments, ctx=ctx)
    feats = features_from_table(table, [SG._is_u8(p) for p in pls], names=names, stats=stats, shape=shape)
    if not neighbours:
        return feats
    from . import regions as RG
    graph = RG.adjacency(segments, pls, mask=mask, n_segments=table.shape[0] - 1, ctx=ctx)
    X = np.concatenate([feats.X, RG.neighbour_features(graph, table, [SG._is_u8(p) for p in pls])], axis=1)
    X[table[:, 0] == 0] = np.nan
    cols = feats.columns + RG.neighbour_columns([f"p{i}" for i in range(len(pls))] if names is None else [str(s) for s in names])
    return ObjectFeatures(table, X, cols, feats.area)


# ---- training and classification ---------------------------------------------------------------------------------------------
def training_segments(segments, roi, mask=None, n_segments: Optional[int] = None, ctx: Optional[Context] = None):
    """(idx int64, y uint8): the segments with at least one counted pixel of roi > 0, ascending, and their label: the majority ROI
    class among those pixels, ties to the smallest label (object_majority(segments, roi, nodata=0) under the mask)."""
    seg = SG.check_segments(segments, "training_segments")
    roi = roi.cpu().numpy() if SG._is_tensor(roi) else np.asarray(roi)
    if tuple(roi.shape) != tuple(seg.shape):
        raise ValueError(f"training_segments: roi has shape {tuple(roi.shape)}, segments {tuple(seg.shape)}")
    if mask is not None:
        mask = SG._check_mask(mask, seg.shape, "training_segments")
        m = mask.cpu().numpy() if SG._is_tensor(mask) else np.asarray(mask)
        roi = np.where(m != 0, roi, 0).astype(roi.dtype)
    table = SG.object_majority(seg, roi, nodata=0, n_segments=n_segments, ctx=ctx)
    idx = np.flatnonzero(table > 0).astype(np.int64)
    return idx, table[idx]


def classify_objects(segments, planes, roi, method: str = "random_forest", stats=("mean", "std"), shape: bool = False, estimator=None,
                     mask=None, names=None, device: bool = False, ctx: Optional[Context] = None,
                     features: Optional[ObjectFeatures] = None) -> ObjectClassification:
    """Object-based supervised classification: the segments that carry ROI pixels train a classifier on their object features,
    every segment is labelled and the labels are painted back.
    method 'random_forest': rsseg.forest_fit.fit(estimator or RandomForestClassifier(n_estimators=100, random_state=42),
    float32(X)[train_idx], y), then the forest walk of K11 over the table's columns as planes of n + 1 "pixels".
    'maximum_likelihood' / 'mahalanobis' / 'minimum_distance': GaussianClassifier(method).fit(X[train_idx], y).predict(X); a
    singular class covariance raises GaussianClassifier's own error (the default stats and shape=False leave out the columns
    that are constant by construction, such as the extent of grid cells).
    Segments with a non-finite feature or without a counted pixel get class 0, as does entry 0.
    features: the ObjectFeatures of these segments, planes and mask when the caller has them already (planes, stats, shape and
    names are then not read).
    Returns ObjectClassification(class_map uint8 (H, W), table uint8 [n + 1], model, X, columns, train_idx, train_y)."""
    if method not in FOREST_METHODS and method not in GAUSS_METHODS:
        raise ValueError(f"classify_objects: method {method!r}, must be one of {FOREST_METHODS + tuple(GAUSS_METHODS)}")
    ctx = SG._context(ctx, "classify_objects")
    seg = SG.check_segments(segments, "classify_objects")
    d_seg, h, w, ns = SG._upload_segments(ctx, seg, None)
    seg2 = d_seg.reshape(h, w)
    feats = features if features is not None else object_features(seg2, planes, names=names, stats=stats, shape=shape, mask=mask,
                                                                  n_segments=ns, ctx=ctx)
    X = feats.X
    if X.shape[0] != ns + 1:
        raise ValueError(f"classify_objects: features describe {X.shape[0] - 1} segments, the map holds {ns}")
    if X.shape[1] == 0:
        raise ValueError("classify_objects: no feature column: give stats or shape=True")
    usable = np.isfinite(X).all(axis=1) & (feats.area > 0)
    idx, y = training_segments(seg2, roi, mask=mask, n_segments=ns, ctx=ctx)
    keep = usable[idx]
    idx, y = idx[keep], y[keep]
    if idx.size == 0:
        raise ValueError("classify_objects: no segment holds a pixel of roi > 0")
    if method in FOREST_METHODS:
        from . import forest_fit
        from .forest import flatten_forest
        if estimator is None:
            from sklearn.ensemble import RandomForestClassifier
            estimator = RandomForestClassifier(n_estimators=100, random_state=42)
        X32 = X.astype(np.float32)
        model = forest_fit.fit(estimator, X32[idx], y, ctx=ctx)
        ctx.forest_load(flatten_forest(model))
        dev = [ctx.to_device(np.ascontiguousarray(np.nan_to_num(X32[:, f], nan=0.0))) for f in range(X32.shape[1])]
        pred = ctx.forest_predict(dev).cpu().numpy()
    else:
        from .gaussian import GaussianClassifier
        model = GaussianClassifier(GAUSS_METHODS[method]).fit(X[idx], y)
        pred = model.predict(X, ctx=ctx)
    table = np.where(usable, pred, 0).astype(np.uint8)
    table[0] = 0
    out = ctx.segment_paint(d_seg, ns, ctx.to_device(table))
    class_map = out.reshape(h, w) if device else out.cpu().numpy().reshape(h, w)
    return ObjectClassification(class_map, table, model, X, feats.columns, idx, y)
