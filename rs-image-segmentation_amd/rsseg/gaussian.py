"""
Gaussian maximum-likelihood classification and its two simpler forms (K22, csrc/k22_gauss.hip; no counterpart in the
reference, whose supervised_classifiers module has the random forest alone):

  'ml'           g_c(x) = (x - mu_c)' S_c^-1 (x - mu_c) + ln |S_c| - 2 ln prior_c      the maximum-likelihood classifier
  'mahalanobis'  g_c(x) = (x - mu_c)' S^-1 (x - mu_c)      one pooled within-class covariance S, no priors
  'mindist'      g_c(x) = |x - mu_c|^2                      minimum distance to the class means

and the label of a pixel is the class with the smallest g.  All three are ONE kernel: a whitened quadratic form per class,
|W_c (x - mu_c)|^2 + offset_c with W_c lower triangular, then an arg-min.  fit() runs on the host in float64 (a few thousand
ROI samples); every per-pixel step runs on the GPU (Context.gauss_classify), bit for bit what tests/gaussian_ref.py
restates.  Class labels must be integers in 1..255: the class map is a uint8 raster whose 0 means "unclassified" (no class
won, or the winner is farther than max_dist2), which is also the GeoTIFF's nodata.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

METHODS = ("ml", "mahalanobis", "mindist")
# the names the stage driver takes (python -m rsseg.stages --classify ...)
STAGE_METHODS = {"maximum_likelihood": "ml", "mahalanobis": "mahalanobis", "minimum_distance": "mindist"}


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .runtime import default_context
    return default_context()


def pack_lower(W: np.ndarray) -> np.ndarray:
    """(k, F, F) lower-triangular matrices -> (k, F (F + 1) / 2): their rows packed row-major, as the kernel reads them."""
    W = np.asarray(W, np.float64)
    i, f = np.tril_indices(W.shape[-1])
    return np.ascontiguousarray(W[..., i, f])


def _whitening(cov: np.ndarray, what: str):
    """(W, 2 sum log diag L) of a covariance: L its Cholesky factor, W = L^-1.  ValueError naming `what` when it has none."""
    from scipy.linalg import solve_triangular
    if not np.all(np.isfinite(cov)):
        raise ValueError(f"GaussianClassifier: the covariance of {what} is not finite")
    try:
        Lc = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(f"GaussianClassifier: the covariance of {what} is not positive definite (singular: constant or linearly "
                         f"dependent features, or too few distinct samples)") from None
    # a pivot is the variance a feature has left once the features before it are taken out: rounding alone can leave a tiny
    # positive one where the features are linearly dependent
    if np.any(np.diag(Lc) ** 2 <= cov.shape[0] * np.finfo(np.float64).eps * np.diag(cov)):
        raise ValueError(f"GaussianClassifier: the covariance of {what} is not positive definite (linearly dependent features)")
    W = np.tril(solve_triangular(Lc, np.eye(cov.shape[0]), lower=True))
    logdet = 2.0 * float(np.sum(np.log(np.diag(Lc))))
    if not (np.all(np.isfinite(W)) and np.isfinite(logdet)):
        raise ValueError(f"GaussianClassifier: the covariance of {what} is not positive definite (its whitening is not finite)")
    return W, logdet


class GaussianClassifier:
    """GaussianClassifier(method='ml' | 'mahalanobis' | 'mindist', priors='empirical' | 'equal' | array, threshold=None,
    max_dist2=None).  priors count for 'ml' only.  threshold=p in (0, 1): a pixel farther from its class than the chi-square
    quantile p with F degrees of freedom (in squared Mahalanobis distance) stays unclassified (label 0); max_dist2 names that
    squared distance directly.  Neither: every pixel is classified."""

    def __init__(self, method: str = "ml", priors="empirical", threshold: Optional[float] = None, max_dist2: Optional[float] = None):
        if method not in METHODS:
            raise ValueError(f"GaussianClassifier: method {method!r}, must be one of {METHODS}")
        if isinstance(priors, str) and priors not in ("empirical", "equal"):
            raise ValueError(f"GaussianClassifier: priors {priors!r}, must be 'empirical', 'equal' or one probability per class")
        if threshold is not None and max_dist2 is not None:
            raise ValueError("GaussianClassifier: give threshold or max_dist2, not both")
        if threshold is not None and not (0.0 < float(threshold) < 1.0):
            raise ValueError(f"GaussianClassifier: threshold={threshold!r} must lie in (0, 1)")
        if max_dist2 is not None and not (float(max_dist2) >= 0.0):
            raise ValueError(f"GaussianClassifier: max_dist2={max_dist2!r} must be >= 0")
        self.method, self.priors, self.threshold = method, priors, threshold
        self.max_dist2 = None if max_dist2 is None else float(max_dist2)

    # ---- fitting (host, float64) ------------------------------------------------------------------------------------
    def fit(self, X, y) -> "GaussianClassifier":
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.size or X.shape[0] == 0:
            raise ValueError(f"GaussianClassifier.fit: X {X.shape} and y {y.shape} are not n samples of F features")
        if not np.all(np.isfinite(X)):
            raise ValueError("GaussianClassifier.fit: X holds NaN or infinite values")
        n, F = X.shape
        classes = np.unique(y)
        as_int = classes.astype(np.int64)
        if np.any(as_int != classes) or as_int.min() < 1 or as_int.max() > 255:
            bad = [c for c, i in zip(classes.tolist(), as_int.tolist()) if c != i or i < 1 or i > 255]
            raise ValueError(f"GaussianClassifier.fit: class labels must be integers in 1..255 (0 is 'unclassified'), got {bad[:5]}")
        k = classes.size
        counts = np.array([(y == c).sum() for c in classes], np.int64)
        if isinstance(self.priors, str):
            pri = counts / float(n) if self.priors == "empirical" else np.full(k, 1.0 / k)
        else:
            pri = np.asarray(self.priors, np.float64).reshape(-1)
            if pri.size != k or not np.all(np.isfinite(pri)) or np.any(pri <= 0) or abs(pri.sum() - 1.0) > 1e-8:
                raise ValueError(f"GaussianClassifier.fit: priors must be {k} positive probabilities that sum to 1")
        mean = np.stack([X[y == c].mean(0) for c in classes])
        W = np.zeros((k, F, F))
        offset = np.zeros(k)
        if self.method == "ml":
            for j, c in enumerate(classes):
                if counts[j] < F + 1:
                    raise ValueError(f"GaussianClassifier.fit: class {c} has {counts[j]} samples, a covariance of {F} features needs "
                                     f"at least {F + 1}")
                cov = np.cov(X[y == c], rowvar=False).reshape(F, F)
                W[j], logdet = _whitening(cov, f"class {c}")
                offset[j] = logdet - 2.0 * np.log(pri[j])
        elif self.method == "mahalanobis":
            if n - k < 1:
                raise ValueError(f"GaussianClassifier.fit: {n} samples of {k} classes leave nothing for the pooled covariance")
            pooled = np.zeros((F, F))
            for j, c in enumerate(classes):
                if counts[j] > 1:
                    pooled += (counts[j] - 1) * np.cov(X[y == c], rowvar=False).reshape(F, F)
            W[:], _ = _whitening(pooled / (n - k), "the pooled classes")
        else:
            W[:] = np.eye(F)
        self.classes_ = classes
        self.class_counts_ = counts
        self.priors_ = pri
        self.n_features_in_ = F
        self.mean_ = mean
        self.whiten_ = pack_lower(W)
        self.offset_ = offset
        self.class_values_ = as_int.astype(np.uint8)
        self.max_dist2_ = self._resolve_max_dist2(F)
        return self

    def _resolve_max_dist2(self, F: int) -> float:
        if self.threshold is not None:
            from scipy.stats import chi2
            return float(chi2.ppf(float(self.threshold), F))
        return float("inf") if self.max_dist2 is None else self.max_dist2

    @staticmethod
    def training_samples(features, roi_mask):
        """(X, y) as prepare_training_samples gathers them from a label raster: the rows of the (H, W, F) stack under the
        non-zero (and non-NaN) pixels of roi_mask in raster order, NaN features -> 0."""
        features = np.asarray(features)
        if features.ndim != 3:
            raise ValueError("features must be a 3-D array (height, width, n_features)")
        roi = np.asarray(roi_mask)
        if roi.shape != features.shape[:2]:
            raise ValueError(f"roi_mask: shape {roi.shape}, the features are {features.shape[:2]}")
        flat = roi.reshape(-1)
        keep = np.flatnonzero((flat != 0) & ~np.isnan(flat.astype(np.float64)))
        if keep.size == 0:
            raise ValueError("roi_mask labels no pixel")
        return np.nan_to_num(features.reshape(-1, features.shape[2])[keep, :], nan=0.0), flat[keep]

    def fit_image(self, features, roi_mask, device: bool = False, ctx=None) -> "GaussianClassifier":
        """device=True: the classes' moments are taken from the raster on the GPU (rsseg.signatures.class_moments, K24) and the
        model comes from them (fit_moments); no host sample matrix is built.  features may then also be device planes."""
        if device:
            from .signatures import class_moments
            roi = roi_mask
            if not hasattr(roi, "data_ptr"):   # a host raster: 0 and NaN label nothing (training_samples' rule), the rest is 1..255
                roi = np.asarray(roi)
                if roi.dtype != np.uint8:
                    r64 = np.nan_to_num(roi.astype(np.float64), nan=0.0)
                    if np.any(r64 != np.floor(r64)) or np.any(r64 < 0) or np.any(r64 > 255):
                        raise ValueError("GaussianClassifier.fit: class labels must be integers in 1..255 (0 is 'unclassified')")
                    roi = r64.astype(np.uint8)
            return self.fit_moments(class_moments(features, roi, ignore=0, ctx=ctx))
        return self.fit(*self.training_samples(features, roi_mask))

    def fit_moments(self, moments) -> "GaussianClassifier":
        """fit() from the counts, means and covariances of a rsseg.signatures.ClassMoments (the table's row is the class label)
        instead of a sample matrix: the same checks, priors and whitening."""
        if moments.n_left_out:
            raise ValueError("GaussianClassifier.fit: X holds NaN or infinite values")
        classes = np.asarray(moments.classes, np.int64)
        if classes.size == 0:
            raise ValueError("roi_mask labels no pixel")
        if classes.min() < 1 or classes.max() > 255:
            raise ValueError(f"GaussianClassifier.fit: class labels must be integers in 1..255 (0 is 'unclassified'), got "
                             f"{[int(c) for c in classes if c < 1 or c > 255][:5]}")
        F, k = moments.n_features, classes.size
        counts = moments.counts[classes].astype(np.int64)
        n = int(counts.sum())
        if isinstance(self.priors, str):
            pri = counts / float(n) if self.priors == "empirical" else np.full(k, 1.0 / k)
        else:
            pri = np.asarray(self.priors, np.float64).reshape(-1)
            if pri.size != k or not np.all(np.isfinite(pri)) or np.any(pri <= 0) or abs(pri.sum() - 1.0) > 1e-8:
                raise ValueError(f"GaussianClassifier.fit: priors must be {k} positive probabilities that sum to 1")
        W = np.zeros((k, F, F))
        offset = np.zeros(k)
        if self.method == "ml":
            for j, c in enumerate(classes):
                if counts[j] < F + 1:
                    raise ValueError(f"GaussianClassifier.fit: class {c} has {counts[j]} samples, a covariance of {F} features needs "
                                     f"at least {F + 1}")
            cov = moments.cov()
            for j, c in enumerate(classes):
                W[j], logdet = _whitening(cov[j], f"class {c}")
                offset[j] = logdet - 2.0 * np.log(pri[j])
        elif self.method == "mahalanobis":
            if n - k < 1:
                raise ValueError(f"GaussianClassifier.fit: {n} samples of {k} classes leave nothing for the pooled covariance")
            W[:], _ = _whitening(moments.pooled_cov(), "the pooled classes")
        else:
            W[:] = np.eye(F)
        self.classes_ = classes
        self.class_counts_ = counts
        self.priors_ = pri
        self.n_features_in_ = F
        self.mean_ = moments.mean()
        self.whiten_ = pack_lower(W)
        self.offset_ = offset
        self.class_values_ = classes.astype(np.uint8)
        self.max_dist2_ = self._resolve_max_dist2(F)
        return self

    # ---- the model as arrays -------------------------------------------------------------------------------------------
    def _check_fitted(self):
        if not hasattr(self, "mean_"):
            raise ValueError("GaussianClassifier: not fitted (fit, fit_image, from_params or load first)")

    def params(self) -> dict:
        """Everything predict needs, as arrays: method, classes, class_values (uint8), mean (k, F), whiten (k, F (F + 1) / 2),
        offset (k,), max_dist2, priors."""
        self._check_fitted()
        return dict(method=self.method, classes=self.classes_.copy(), class_values=self.class_values_.copy(), mean=self.mean_.copy(),
                    whiten=self.whiten_.copy(), offset=self.offset_.copy(), max_dist2=float(self.max_dist2_), priors=self.priors_.copy())

    @classmethod
    def from_params(cls, mean, whiten, offset, class_values, max_dist2: float = float("inf"), method: str = "ml", classes=None,
                    priors=None) -> "GaussianClassifier":
        """A model from its arrays (params()' keys).  whiten: (k, F (F + 1) / 2) packed rows, or (k, F, F) lower-triangular
        matrices.  classes: the labels predict returns (default: class_values)."""
        mean = np.array(mean, dtype=np.float64, ndmin=2)
        k, F = mean.shape
        whiten = np.asarray(whiten, np.float64)
        if whiten.ndim == 3:
            if whiten.shape != (k, F, F) or np.any(np.triu(whiten, 1) != 0):
                raise ValueError("GaussianClassifier.from_params: whiten must be (k, F, F) lower-triangular matrices or their packed rows")
            whiten = pack_lower(whiten)
        offset = np.asarray(offset, np.float64).reshape(-1)
        cv = np.asarray(class_values).reshape(-1)
        if whiten.shape != (k, F * (F + 1) // 2) or offset.size != k or cv.size != k:
            raise ValueError(f"GaussianClassifier.from_params: mean {mean.shape}, whiten {whiten.shape}, offset {offset.shape} and "
                             f"class_values {cv.shape} do not describe one model")
        if np.any(cv != cv.astype(np.int64)) or np.any(cv < 1) or np.any(cv > 255) or np.unique(cv).size != k:
            raise ValueError("GaussianClassifier.from_params: class_values must be distinct integers in 1..255")
        if max_dist2 != max_dist2:
            raise ValueError("GaussianClassifier.from_params: max_dist2 is NaN")
        self = cls(method=method)
        self.classes_ = np.asarray(cv if classes is None else classes).copy()
        if self.classes_.shape != (k,):
            raise ValueError("GaussianClassifier.from_params: one class label per class")
        self.class_values_ = cv.astype(np.uint8)
        self.priors_ = np.full(k, 1.0 / k) if priors is None else np.asarray(priors, np.float64).copy()
        self.n_features_in_ = F
        self.mean_, self.whiten_, self.offset_ = mean, np.ascontiguousarray(whiten), offset.copy()
        self.max_dist2_ = float(max_dist2)
        return self

    def save(self, path) -> str:
        """The model as an .npz of plain arrays (no pickled objects)."""
        p = self.params()
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, method=np.array(p["method"]), classes=p["classes"], class_values=p["class_values"], mean=p["mean"], whiten=p["whiten"],
                 offset=p["offset"], max_dist2=np.float64(p["max_dist2"]), priors=p["priors"])
        return path

    @classmethod
    def load(cls, path) -> "GaussianClassifier":
        with np.load(str(path), allow_pickle=False) as z:
            return cls.from_params(z["mean"], z["whiten"], z["offset"], z["class_values"], float(z["max_dist2"]), str(z["method"]),
                                   classes=z["classes"], priors=z["priors"])

    # ---- prediction (GPU) ----------------------------------------------------------------------------------------------
    def _classify(self, ctx, dev: Sequence, want_dist2: bool, want_margin: bool):
        return ctx.gauss_classify(dev, self.mean_, self.whiten_, self.offset_, self.class_values_, self.max_dist2_, want_dist2=want_dist2,
                                  want_margin=want_margin)

    def _to_classes(self, labels_u8: np.ndarray) -> np.ndarray:
        lut = np.zeros(256, self.classes_.dtype)
        lut[self.class_values_] = self.classes_
        return lut[labels_u8]

    def predict(self, X, ctx=None) -> np.ndarray:
        """Labels of the rows of X (n, F; float32 stays float32, anything else is read as float64) in the dtype of classes_,
        0 for an unclassified row.  A NaN feature reads as 0."""
        self._check_fitted()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError(f"GaussianClassifier.predict: X {X.shape}, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        dt = np.float32 if X.dtype == np.float32 else np.float64
        dev = [ctx.to_device(np.ascontiguousarray(X[:, f], dtype=dt)) for f in range(X.shape[1])]
        labels, _, _ = self._classify(ctx, dev, False, False)
        return self._to_classes(labels.cpu().numpy())

    def predict_image(self, features, mask=None, want_dist2: bool = False, want_margin: bool = False, ctx=None):
        """The class map of an (H, W, F) array or a list of F (H, W) planes: (H, W) uint8 of class values, 0 = unclassified.
        With want_dist2 / want_margin: (map, dist2 or None, margin or None), float32 (H, W): the squared distance of every pixel
        to its class (in the class's own metric) and the runner-up's g minus the winner's.
        mask ((H, W), non-zero = valid): only the valid pixels are classified (rsseg.masked: Context.compact_plan / compact /
        expand); label 0 and NaN planes elsewhere."""
        from .masked import make_plan, planes_to_device
        self._check_fitted()
        if isinstance(features, np.ndarray):
            if features.ndim != 3:
                raise ValueError("features must be a 3-D array (height, width, n_features) or a list of planes")
            planes = [features[:, :, i] for i in range(features.shape[2])]
        else:
            planes = [np.asarray(p) for p in features]
        if len(planes) != self.n_features_in_:
            raise ValueError(f"GaussianClassifier.predict_image: {len(planes)} planes, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        dev, _, shape = planes_to_device(ctx, planes)
        if mask is not None:
            plan = make_plan(ctx, mask, dev[0].numel())
            lab_c, d_c, m_c = self._classify(ctx, ctx.compact(plan, dev), want_dist2, want_margin)
            labels = ctx.expand(plan, lab_c, 0)
            dist2 = None if d_c is None else ctx.expand(plan, d_c, float("nan"))
            margin = None if m_c is None else ctx.expand(plan, m_c, float("nan"))
        else:
            labels, dist2, margin = self._classify(ctx, dev, want_dist2, want_margin)
        out = labels.cpu().numpy().reshape(shape)
        if not (want_dist2 or want_margin):
            return out
        return (out, None if dist2 is None else dist2.cpu().numpy().reshape(shape),
                None if margin is None else margin.cpu().numpy().reshape(shape))

    def class_counts(self, labels, ctx=None) -> dict:
        """Pixels per label of a uint8 class map (Context.hist_u8): {0: unclassified, class value: count, ...}."""
        self._check_fitted()
        ctx = _ctx(ctx)
        if isinstance(labels, np.ndarray) or not hasattr(labels, "data_ptr"):
            a = np.asarray(labels)
            if a.dtype != np.uint8:
                raise ValueError("class_counts: the class map must be uint8")
            labels = ctx.to_device(np.ascontiguousarray(a).reshape(-1))
        h = ctx.hist_u8(labels)
        return {0: int(h[0]), **{int(v): int(h[int(v)]) for v in self.class_values_}}
