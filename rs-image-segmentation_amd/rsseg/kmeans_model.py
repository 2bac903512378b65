"""
A fitted KMeans model that outlives the call that fitted it: MinMaxScaler (scale_, min_) + KMeans (cluster_centers_), applied
to rasters it was not fitted on by K18 (Context.kmeans_predict, rsseg_kmeans_predict): the next tile of a mosaic, the next
date of a series, the whole scene after a fit on a part of it.  Cluster ids then mean the same thing in every map.

  model, labels = KMeansModel.fit(planes, 7)      one kmeans_fit_predict call; `labels` are that call's, unchanged
  model.predict(other_planes)                     sklearn.cluster.KMeans.predict(MinMaxScaler.transform(X)), label for label
  model.predict_with_distance(other_planes)       ... and the distance of every pixel to its centre
  model.summary(other_planes)                     counts, inertia (an exact sum, quantum 2^-40), score = -inertia
  model.save(path) / KMeansModel.load(path)       an .npz of plain arrays and strings, no pickle
  model.to_sklearn() / KMeansModel.from_sklearn   the same model as scikit-learn objects, for cross-checks

predict() on the raster the model was fitted on can differ from the fit's own labels at near-ties: fit assigns on mean-centred
data, predict on uncentred data against centres with the mean added back.  scikit-learn's fit_predict / predict differ the
same way.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

FORMAT_VERSION = 1
_FORMAT_NAME = "rsseg.KMeansModel"


def _exact(a, dt, what: str) -> np.ndarray:
    a64 = np.asarray(a, dtype=np.float64)
    out = a64.astype(dt)
    if not np.all(np.isfinite(a64)):
        raise ValueError(f"KMeansModel: {what} is not finite")
    if not np.array_equal(out.astype(np.float64), a64):
        raise ValueError(f"KMeansModel: {what} does not hold {np.dtype(dt).name} values: a model fitted in float64 cannot be "
                         f"applied to float32 planes")
    return np.ascontiguousarray(out)


class KMeansModel:
    def __init__(self, cluster_centers, scale, min_, feature_names: Optional[Sequence[str]] = None, n_iter: int = 0, seed: int = -1,
                 n_samples_fit: int = 0):
        c = np.asarray(cluster_centers)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
            raise ValueError("KMeansModel: cluster_centers must be (n_clusters, n_features)")
        dt = np.float32 if c.dtype == np.float32 else np.float64
        k, F = c.shape
        self.cluster_centers_ = _exact(c, dt, "cluster_centers")
        self.scale_ = _exact(np.asarray(scale).reshape(-1), dt, "scale")
        self.min_ = _exact(np.asarray(min_).reshape(-1), dt, "min_")
        if self.scale_.size != F or self.min_.size != F:
            raise ValueError(f"KMeansModel: {F} features in the centres, {self.scale_.size} in scale, {self.min_.size} in min_")
        self.feature_names = None if feature_names is None else [str(s) for s in feature_names]
        if self.feature_names is not None and len(self.feature_names) != F:
            raise ValueError(f"KMeansModel: {len(self.feature_names)} feature names for {F} features")
        self.n_iter_ = int(n_iter)
        self.seed = int(seed)
        self.n_samples_fit_ = int(n_samples_fit)

    # ---- shape -------------------------------------------------------------------------------------
    @property
    def n_clusters(self) -> int:
        return self.cluster_centers_.shape[0]

    @property
    def n_features_in_(self) -> int:
        return self.cluster_centers_.shape[1]

    @property
    def dtype(self):
        return self.cluster_centers_.dtype

    # ---- fitting -----------------------------------------------------------------------------------
    @classmethod
    def fit(cls, planes: Sequence, n_clusters: int, seed: int = 42, max_iter: int = 300, tol: float = 1e-4, feature_names=None, ctx=None,
            mask=None):
        """One Context.kmeans_fit_predict call -> (model, labels); the labels are the call's own.
        mask (non-zero = valid, of the planes' size): the fit sees the valid pixels only (rsseg.masked), labels are -1 at the
        masked pixels and n_samples_fit_ is the valid count."""
        ctx = ctx or _default_ctx()
        if mask is not None:
            from .masked import kmeans_fit_predict_masked
            labels, meta = kmeans_fit_predict_masked(planes, mask, int(n_clusters), seed, max_iter, tol, -1, ctx)
            dt = np.float32 if all("float32" in str(p.dtype) for p in planes) else np.float64
            return cls(meta["centers"].astype(dt), meta["scale"].astype(dt), meta["min"].astype(dt), feature_names, meta["n_iter"], seed,
                       meta["n_valid"]), labels
        host = isinstance(planes[0], np.ndarray)
        shape = planes[0].shape if host else None
        if host:
            dt = np.result_type(*[p.dtype for p in planes])
            dt = np.float32 if dt == np.float32 else np.float64
            planes = [ctx.to_device(np.ascontiguousarray(p, dtype=dt).reshape(-1)) for p in planes]
        labels, meta = ctx.kmeans_fit_predict(planes, int(n_clusters), seed, max_iter, tol)
        dt = np.float32 if "float32" in str(planes[0].dtype) else np.float64
        model = cls(meta["centers"].astype(dt), meta["scale"].astype(dt), meta["min"].astype(dt), feature_names, meta["n_iter"], seed,
                    int(planes[0].numel()))
        return model, (labels.cpu().numpy().reshape(shape) if host else labels)

    # ---- applying ----------------------------------------------------------------------------------
    def _apply(self, planes: Sequence, want_distance: bool, want_summary: bool, ctx, mask=None):
        ctx = ctx or _default_ctx()
        if len(planes) != self.n_features_in_:
            raise ValueError(f"KMeansModel: {len(planes)} planes, the model was fitted on {self.n_features_in_}")
        host = isinstance(planes[0], np.ndarray)
        shape = planes[0].shape if host else None
        if host:
            dt = np.result_type(*[p.dtype for p in planes])
            dt = np.float32 if dt == np.float32 else np.float64
            if dt != self.dtype:
                raise ValueError(f"KMeansModel: {np.dtype(dt).name} planes, the model was fitted in {self.dtype.name}")
            planes = [ctx.to_device(np.ascontiguousarray(p, dtype=dt).reshape(-1)) for p in planes]
        elif self.dtype.name not in str(planes[0].dtype):
            raise ValueError(f"KMeansModel: {planes[0].dtype} planes, the model was fitted in {self.dtype.name}")
        model = (self.cluster_centers_.astype(np.float64), self.scale_.astype(np.float64), self.min_.astype(np.float64))
        if mask is None:
            labels, dist, summary = ctx.kmeans_predict(planes, *model, want_distance=want_distance, want_summary=want_summary)
        else:
            from .masked import kmeans_predict_masked
            labels, dist, summary, n_valid = kmeans_predict_masked(ctx, planes, mask, *model, want_distance=want_distance,
                                                                   want_summary=want_summary)
            if summary is not None:
                summary = dict(summary, n_valid=n_valid)
        if host:
            labels = labels.cpu().numpy().reshape(shape)
            dist = None if dist is None else dist.cpu().numpy().reshape(shape)
        if summary is not None:
            summary = dict(summary)
            summary["score"] = -summary["inertia"]
        return labels, dist, summary

    def predict(self, planes: Sequence, ctx=None, mask=None):
        """int32 labels: NumPy planes in -> an array of the planes' shape; device tensors in -> a flat device tensor.
        mask (non-zero = valid): only the valid pixels are labelled, the others get -1."""
        return self._apply(planes, False, False, ctx, mask)[0]

    def predict_with_distance(self, planes: Sequence, ctx=None, mask=None):
        """(labels, distance): the Euclidean distance of every scaled pixel to the centre of its label, in the planes' dtype.
        With a mask: -1 and NaN at the masked pixels."""
        return self._apply(planes, True, False, ctx, mask)[:2]

    def summary(self, planes: Sequence, ctx=None, mask=None) -> dict:
        """counts (int64 per cluster), inertia, overflow, score = -inertia of this scene under the model.  With a mask they
        cover the valid pixels only, and n_valid is added."""
        return self._apply(planes, False, True, ctx, mask)[2]

    def select_planes(self, features_dict, feature_keys_to_use=None):
        """The planes unsupervised_kmeans_classification would cluster, checked against the model -> (planes, (H, W))."""
        from modules.features.extract import _select_planes
        planes, shape = _select_planes(features_dict, feature_keys_to_use)
        if len(planes) != self.n_features_in_:
            raise ValueError(f"KMeansModel: the selection gives {len(planes)} planes, the model was fitted on {self.n_features_in_}")
        if self.feature_names is not None:
            names = plane_names(features_dict, feature_keys_to_use)
            if names != self.feature_names:
                diff = [f"{a!r} != {b!r}" for a, b in zip(names, self.feature_names) if a != b]
                raise ValueError(f"KMeansModel: the selected planes are not the ones the model was fitted on ({', '.join(diff[:4])})")
        return planes, shape

    def predict_features(self, features_dict, feature_keys_to_use=None, ctx=None, mask=None):
        """unsupervised_kmeans_classification's selection of planes, labelled by this model -> (H, W) int32 (-1 where an (H, W)
        `mask` is zero)."""
        planes, shape = self.select_planes(features_dict, feature_keys_to_use)
        return self.predict([np.asarray(p) for p in planes], ctx=ctx, mask=mask).reshape(shape)

    @classmethod
    def fit_features(cls, features_dict, n_clusters: int = 5, feature_keys_to_use=None, seed: int = 42, ctx=None, mask=None):
        """unsupervised_kmeans_classification that keeps its model -> (model, (H, W) int32 labels; -1 where an (H, W) `mask` is
        zero, and the fit has not seen those pixels)."""
        from modules.features.extract import _select_planes
        planes, shape = _select_planes(features_dict, feature_keys_to_use)
        model, labels = cls.fit([np.asarray(p) for p in planes], n_clusters, seed=seed,
                                feature_names=plane_names(features_dict, feature_keys_to_use), ctx=ctx, mask=mask)
        return model, labels.reshape(shape)

    # ---- scikit-learn ------------------------------------------------------------------------------
    @classmethod
    def from_sklearn(cls, scaler, kmeans, feature_names=None):
        if tuple(getattr(scaler, "feature_range", (0, 1))) != (0, 1) or getattr(scaler, "clip", False):
            raise ValueError("KMeansModel.from_sklearn: a MinMaxScaler with feature_range=(0, 1) and clip=False is what the kernels restate")
        c = np.asarray(kmeans.cluster_centers_)
        return cls(c, scaler.scale_, scaler.min_, feature_names, int(getattr(kmeans, "n_iter_", 0)),
                   kmeans.random_state if isinstance(getattr(kmeans, "random_state", None), (int, np.integer)) else -1,
                   int(getattr(scaler, "n_samples_seen_", 0)))

    def to_sklearn(self):
        """(MinMaxScaler, KMeans) carrying this model's attributes: transform / predict work, nothing was fitted."""
        from sklearn.cluster import KMeans
        from sklearn.preprocessing import MinMaxScaler
        from sklearn.utils._openmp_helpers import _openmp_effective_n_threads
        F = self.n_features_in_
        sc = MinMaxScaler()
        sc.scale_, sc.min_, sc.n_features_in_ = self.scale_.copy(), self.min_.copy(), F
        sc.n_samples_seen_ = self.n_samples_fit_
        km = KMeans(n_clusters=self.n_clusters, n_init=1, random_state=self.seed if self.seed >= 0 else None)
        km.cluster_centers_ = self.cluster_centers_.copy()
        km.n_features_in_ = F
        km._n_threads = _openmp_effective_n_threads()
        km._n_features_out = self.n_clusters
        km.n_iter_ = self.n_iter_
        return sc, km

    # ---- persistence -------------------------------------------------------------------------------
    def save(self, path: str) -> str:
        """An .npz of plain arrays and strings (np.load(..., allow_pickle=False) reads it).  Returns the path written
        (NumPy appends '.npz' to a path without it)."""
        names = self.feature_names
        with open(path, "wb") as f:
            np.savez(f, format=np.array(_FORMAT_NAME), format_version=np.array(FORMAT_VERSION, np.int64),
                     cluster_centers=self.cluster_centers_, scale=self.scale_, min=self.min_,
                     has_feature_names=np.array(names is not None), feature_names=np.array(names or [], dtype=np.str_),
                     n_iter=np.array(self.n_iter_, np.int64), seed=np.array(self.seed, np.int64),
                     n_samples_fit=np.array(self.n_samples_fit_, np.int64))
        return path

    @classmethod
    def load(cls, path: str) -> "KMeansModel":
        try:
            with np.load(path, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        except ValueError as e:   # a pickle, or an archive with pickled members
            raise ValueError(f"{path}: not a KMeansModel file (pickled data is refused): {e}") from None
        if "format" not in d or str(d["format"]) != _FORMAT_NAME:
            raise ValueError(f"{path}: not a KMeansModel file")
        if int(d["format_version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: KMeansModel format version {int(d['format_version'])}, this code reads {FORMAT_VERSION}")
        names = [str(s) for s in d["feature_names"]] if bool(d["has_feature_names"]) else None
        return cls(d["cluster_centers"], d["scale"], d["min"], names, int(d["n_iter"]), int(d["seed"]), int(d["n_samples_fit"]))


def plane_names(features_dict, feature_keys_to_use=None):
    """One name per plane of modules.features.extract._select_planes(features_dict, feature_keys_to_use), in its order: the key
    of a 2-D array, 'key[i]' for channel i of a 3-D one."""
    shape = (features_dict["height"], features_dict["width"])
    keys = feature_keys_to_use
    if keys is None:
        meta = ["transform", "crs", "width", "height", "dimensions", "geo_transform"]
        keys = [k for k, v in features_dict.items() if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape == shape and k not in meta]
        if not keys:
            cands = ["ndvi", "ndwi", "ndbi", "texture_mean", "evi", "savi", "hierarchical_level_1", "hierarchical_level_2", "hierarchical_all"]
            keys = [k for k in cands if isinstance(features_dict.get(k), np.ndarray)]
    names = []
    for key in keys:
        v = features_dict.get(key)
        if isinstance(v, np.ndarray) and v.ndim == 3 and v.shape[:2] == shape:
            names.extend(f"{key}[{i}]" for i in range(v.shape[2]))
        elif isinstance(v, np.ndarray) and v.ndim == 2 and v.shape == shape:
            names.append(str(key))
    return names


def _default_ctx():
    from .runtime import default_context
    return default_context()
