"""
Support vector machine classification (K28, csrc/k28_svm.hip; no counterpart in the reference, whose supervised_classifiers
module has the random forest alone).  Training is scikit-learn's (sklearn.svm.SVC, libsvm) on the host, on samples standardised
in float64; every per-pixel step runs on the GPU (Context.svm_classify): the kernel value of every support vector, the
one-vs-one pair decisions and libsvm's vote, bit for bit what tests/svm_ref.py restates.

The model is libsvm's own: the support vectors in scaled units grouped by class, scikit-learn's private _dual_coef_,
_intercept_ (libsvm's -rho) and _n_support.  The public dual_coef_ / intercept_ are not used: for two classes scikit-learn
flips their sign.  Kernels: 'rbf' exp(-gamma |z - sv|^2), 'poly' (gamma <z, sv> + coef0)^degree, 'linear' <z, sv> (its pair
weights folded once at model build, so prediction does not loop over the support vectors).
Class labels are any integers; the kernel sees class_values 1..k and the object maps them back, 0 standing for a pixel that
was not classified (an infinite feature value, or outside the mask).

    python -m rsseg.svm OUTDIR --roi ROI [--kernel rbf|poly|linear] [--C C] [--gamma scale|auto|G] [--degree D] [--coef0 R]
                               [--model PATH] [--rule-image] [--mask-nodata [VALUE]]
trains and applies an SVM on the output directory of an earlier `python -m rsseg.stages image.tif OUTDIR` run
(rsseg.stages.run_svm_stage); --model PATH applies a saved model instead of training one.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

KERNELS = ("rbf", "poly", "linear")
MAX_CLASSES = 16        # RSSEG_SVM_MAX_CLASSES
MAX_SV = 16384          # RSSEG_SVM_MAX_SV
MAX_DEGREE = 8          # RSSEG_SVM_MAX_DEGREE
MAX_FEATURES = 64       # RSSEG_MAX_FEATURES


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .runtime import default_context
    return default_context()


def fold_linear(sv, n_support, coef) -> np.ndarray:
    """w (P, F) of the linear kernel: per pair (a, b) and feature f the fma chain from +0 of coef[b-1][i] * sv[i][f] over class
    a's support vectors ascending, then coef[a][i] * sv[i][f] over class b's (rsseg_host_svm_fold_linear)."""
    from . import _lib
    sv = np.ascontiguousarray(sv, np.float64)
    ns = np.ascontiguousarray(n_support, np.int32)
    coef = np.ascontiguousarray(coef, np.float64)
    S, F = sv.shape
    k = ns.size
    w = np.zeros((k * (k - 1) // 2, F), np.float64)
    dp = C.POINTER(C.c_double)
    rc = _lib.load().rsseg_host_svm_fold_linear(F, k, S, sv.ctypes.data_as(dp), ns.ctypes.data_as(C.POINTER(C.c_int)), coef.ctypes.data_as(dp),
                                                w.ctypes.data_as(dp))
    if rc != 0:
        raise ValueError(f"SVMClassifier: the model's arrays do not fold into linear weights (code {rc})")
    return w


class SVMClassifier:
    """SVMClassifier(kernel='rbf' | 'poly' | 'linear', C=1.0, gamma='scale' | 'auto' | number, degree=3, coef0=0.0,
    class_weight=None): sklearn.svm.SVC's parameters of the same names."""

    def __init__(self, kernel: str = "rbf", C: float = 1.0, gamma="scale", degree: int = 3, coef0: float = 0.0, class_weight=None):
        if callable(kernel):
            raise ValueError("SVMClassifier: callable kernels are not supported, the kernel must be one of " + repr(KERNELS))
        if kernel not in KERNELS:
            raise ValueError(f"SVMClassifier: kernel {kernel!r} is not supported, must be one of {KERNELS}")
        if isinstance(gamma, str):
            if gamma not in ("scale", "auto"):
                raise ValueError(f"SVMClassifier: gamma {gamma!r}, must be 'scale', 'auto' or a positive number")
        elif not (float(gamma) > 0.0 and np.isfinite(float(gamma))):
            raise ValueError(f"SVMClassifier: gamma={gamma!r} must be a finite number > 0")
        if not (float(C) > 0.0):
            raise ValueError(f"SVMClassifier: C={C!r} must be > 0")
        if int(degree) != degree or not (1 <= int(degree) <= MAX_DEGREE):
            raise ValueError(f"SVMClassifier: degree={degree!r} must be an integer in 1..{MAX_DEGREE}")
        if not np.isfinite(float(coef0)):
            raise ValueError(f"SVMClassifier: coef0={coef0!r} is not finite")
        self.kernel, self.C, self.gamma, self.degree, self.coef0, self.class_weight = kernel, float(C), gamma, int(degree), float(coef0), class_weight

    # ---- fitting (host) ----------------------------------------------------------------------------------------------
    def fit(self, X, y) -> "SVMClassifier":
        from sklearn.svm import SVC
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.size or X.shape[0] == 0:
            raise ValueError(f"SVMClassifier.fit: X {X.shape} and y {y.shape} are not n samples of F features")
        if not np.all(np.isfinite(X)):
            raise ValueError("SVMClassifier.fit: X holds NaN or infinite values")
        if X.shape[1] > MAX_FEATURES:
            raise ValueError(f"SVMClassifier.fit: {X.shape[1]} features, the kernels take at most {MAX_FEATURES}")
        _check_classes(np.unique(y), "SVMClassifier.fit")
        offset = X.mean(axis=0)
        std = X.std(axis=0)
        scale = np.where(std > 0.0, 1.0 / np.where(std > 0.0, std, 1.0), 1.0)   # a constant column: scale 1
        svc = SVC(kernel=self.kernel, C=self.C, gamma=self.gamma, degree=self.degree, coef0=self.coef0, class_weight=self.class_weight)
        svc.fit((X - offset) * scale, y)
        return self._take(svc, offset, scale)

    def fit_image(self, features, roi_mask) -> "SVMClassifier":
        """fit() on the rows of the (H, W, F) stack under the non-zero pixels of roi_mask (GaussianClassifier.training_samples)."""
        from .gaussian import GaussianClassifier
        return self.fit(*GaussianClassifier.training_samples(features, roi_mask))

    @classmethod
    def from_sklearn(cls, svc, offset=None, scale=None) -> "SVMClassifier":
        """The model of a fitted sklearn.svm.SVC that was trained on (X - offset) * scale (default: on X itself)."""
        kernel = getattr(svc, "kernel", None)
        if callable(kernel):
            raise ValueError("SVMClassifier.from_sklearn: callable kernels are not supported")
        if kernel in ("sigmoid", "precomputed"):
            raise ValueError(f"SVMClassifier.from_sklearn: the {kernel} kernel is not supported, only {KERNELS}")
        if kernel not in KERNELS:
            raise ValueError(f"SVMClassifier.from_sklearn: kernel {kernel!r} is not supported, only {KERNELS}")
        if not hasattr(svc, "support_vectors_"):
            raise ValueError("SVMClassifier.from_sklearn: the SVC is not fitted")
        if getattr(svc, "_sparse", False):
            raise ValueError("SVMClassifier.from_sklearn: an SVC fitted on sparse samples is not supported")
        _check_classes(np.asarray(svc.classes_), "SVMClassifier.from_sklearn")
        if kernel == "poly" and not (int(svc.degree) == svc.degree and 1 <= int(svc.degree) <= MAX_DEGREE):
            raise ValueError(f"SVMClassifier.from_sklearn: degree={svc.degree!r} is not supported, must be an integer in 1..{MAX_DEGREE}")
        self = cls.__new__(cls)
        self.kernel, self.C, self.gamma, self.degree, self.coef0 = kernel, float(svc.C), svc.gamma, int(svc.degree), float(svc.coef0)
        self.class_weight = svc.class_weight
        F = svc.support_vectors_.shape[1]
        return self._take(svc, np.zeros(F) if offset is None else offset, np.ones(F) if scale is None else scale)

    def _take(self, svc, offset, scale) -> "SVMClassifier":
        k = len(svc.classes_)
        return self._set(svc.support_vectors_, svc._dual_coef_, svc._intercept_, svc._n_support, svc.classes_, np.arange(1, k + 1), offset, scale,
                         float(svc._gamma), None)

    def _set(self, sv, coef, bias, n_support, classes, class_values, offset, scale, gamma, w) -> "SVMClassifier":
        who = "SVMClassifier"
        sv = np.array(sv, dtype=np.float64, ndmin=2, order="C")
        S, F = sv.shape
        ns = np.asarray(n_support).reshape(-1)
        k = ns.size
        P = k * (k - 1) // 2
        coef = np.array(coef, dtype=np.float64, ndmin=2, order="C")
        bias = np.array(bias, dtype=np.float64).reshape(-1)
        offset, scale = np.array(offset, dtype=np.float64).reshape(-1), np.array(scale, dtype=np.float64).reshape(-1)
        classes = np.asarray(classes).reshape(-1).copy()
        cv = np.asarray(class_values).reshape(-1)
        if k < 2:
            raise ValueError(f"{who}: {k} classes, a model needs at least 2")
        if k > MAX_CLASSES:
            raise ValueError(f"{who}: {k} classes, more than {MAX_CLASSES} classes are not supported")
        if F > MAX_FEATURES:
            raise ValueError(f"{who}: {F} features, the kernels take at most {MAX_FEATURES}")
        if not (1 <= S <= MAX_SV):
            raise ValueError(f"{who}: {S} support vectors, the kernels take 1..{MAX_SV}")
        if (coef.shape != (k - 1, S) or bias.size != P or offset.size != F or scale.size != F or classes.size != k or cv.size != k
                or np.any(ns != ns.astype(np.int64)) or np.any(ns < 1) or int(ns.sum()) != S):
            raise ValueError(f"{who}: support vectors {sv.shape}, coefficients {coef.shape}, intercepts {bias.shape}, n_support {ns.tolist()}, "
                             f"offset {offset.shape}, scale {scale.shape}, classes {classes.shape} and class_values {cv.shape} do not describe one model")
        if np.any(cv != cv.astype(np.int64)) or np.any(cv < 1) or np.any(cv > 255) or np.unique(cv).size != k:
            raise ValueError(f"{who}: class_values must be distinct integers in 1..255")
        for name, a in (("support vectors", sv), ("coefficients", coef), ("intercepts", bias), ("offset", offset), ("scale", scale)):
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{who}: the {name} are not finite")
        if np.any(scale == 0.0):
            raise ValueError(f"{who}: a scale of 0")
        if not np.isfinite(gamma) or (self.kernel == "rbf" and not gamma > 0.0):
            raise ValueError(f"{who}: gamma={gamma!r} must be finite" + (" and > 0" if self.kernel == "rbf" else ""))
        self.classes_ = classes
        self.class_values_ = cv.astype(np.uint8)
        self.n_support_ = ns.astype(np.int32)
        self.n_features_in_ = F
        self.support_vectors_, self.dual_coef_, self.intercept_ = sv, coef, bias
        self.offset_, self.scale_, self.gamma_ = offset, scale, float(gamma)
        self.w_ = None
        if self.kernel == "linear":
            self.w_ = fold_linear(sv, self.n_support_, coef) if w is None else np.array(w, dtype=np.float64, order="C").reshape(P, F)
            if not np.all(np.isfinite(self.w_)):
                raise ValueError(f"{who}: the folded weights are not finite")
        return self

    # ---- the model as arrays -------------------------------------------------------------------------------------------
    def _check_fitted(self):
        if not hasattr(self, "support_vectors_"):
            raise ValueError("SVMClassifier: not fitted (fit, fit_image, from_sklearn, from_params or load first)")

    def params(self) -> dict:
        """Everything predict needs: kernel, gamma, coef0, degree, classes, class_values (uint8), offset, scale (F,),
        support_vectors (S, F), dual_coef (k - 1, S), intercept (P,), n_support (k,), w ((P, F) for 'linear', else (0, F))."""
        self._check_fitted()
        w = np.zeros((0, self.n_features_in_)) if self.w_ is None else self.w_.copy()
        return dict(kernel=self.kernel, gamma=self.gamma_, coef0=self.coef0, degree=self.degree, classes=self.classes_.copy(),
                    class_values=self.class_values_.copy(), offset=self.offset_.copy(), scale=self.scale_.copy(),
                    support_vectors=self.support_vectors_.copy(), dual_coef=self.dual_coef_.copy(), intercept=self.intercept_.copy(),
                    n_support=self.n_support_.copy(), w=w)

    @classmethod
    def from_params(cls, kernel, gamma, support_vectors, dual_coef, intercept, n_support, offset=None, scale=None, class_values=None, classes=None,
                    coef0: float = 0.0, degree: int = 3, w=None) -> "SVMClassifier":
        """A model from its arrays (params()' keys).  class_values default to 1..k, classes to class_values, offset / scale to
        0 / 1; w (linear) is folded from the support vectors when it is not given (or empty)."""
        self = cls(kernel=kernel, gamma=float(gamma), degree=int(degree), coef0=float(coef0))
        sv =np.array(support_vectors, dtype=np.float64, ndmin=2)
        F, k = sv.shape[1], np.asarray(n_support).size
        cv = np.arange(1, k + 1) if class_values is None else class_values
        if w is not None and np.asarray(w).size == 0:
            w = None
        return self._set(sv, dual_coef, intercept, n_support, cv if classes is None else classes, cv, np.zeros(F) if offset is None else offset,
                         np.ones(F) if scale is None else scale, float(gamma), w)

    def save(self, path) -> str:
        """The model as an .npz of plain arrays and scalars (no pickled objects)."""
        p = self.params()
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, kernel=np.array(p["kernel"]), gamma=np.float64(p["gamma"]), coef0=np.float64(p["coef0"]), degree=np.int64(p["degree"]),
                 **{key: p[key] for key in ("classes", "class_values", "offset", "scale", "support_vectors", "dual_coef", "intercept", "n_support", "w")})
        return path

    @classmethod
    def load(cls, path) -> "SVMClassifier":
        with np.load(str(path), allow_pickle=False) as z:
            return cls.from_params(str(z["kernel"]), float(z["gamma"]), z["support_vectors"], z["dual_coef"], z["intercept"], z["n_support"],
                                   offset=z["offset"], scale=z["scale"], class_values=z["class_values"], classes=z["classes"],
                                   coef0=float(z["coef0"]), degree=int(z["degree"]), w=z["w"])

    # ---- prediction (GPU) ----------------------------------------------------------------------------------------------
    def _classify(self, ctx, dev, want_margin: bool):
        return ctx.svm_classify(dev, self.offset_, self.scale_, self.support_vectors_, self.n_support_, self.dual_coef_, self.intercept_,
                                self.class_values_, kernel=self.kernel, gamma=self.gamma_, coef0=self.coef0, degree=self.degree, w=self.w_,
                                want_margin=want_margin)

    def _to_classes(self, labels_u8: np.ndarray) -> np.ndarray:
        lut = np.zeros(256, self.classes_.dtype)
        lut[self.class_values_] = self.classes_
        return lut[labels_u8]

    def predict(self, X, ctx=None) -> np.ndarray:
        """Labels of the rows of X (n, F; float32 stays float32, anything else is read as float64) in the dtype of classes_, 0
        for a row with an infinite value.  A NaN feature reads as 0."""
        self._check_fitted()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError(f"SVMClassifier.predict: X {X.shape}, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        dt = np.float32 if X.dtype == np.float32 else np.float64
        dev = [ctx.to_device(np.ascontiguousarray(X[:, f], dtype=dt)) for f in range(X.shape[1])]
        labels, _ = self._classify(ctx, dev, False)
        return self._to_classes(labels.cpu().numpy())

    def predict_image(self, features, mask=None, want_margin: bool = False, ctx=None):
        """The class map of an (H, W, F) array or a list of F (H, W) planes: (H, W) class labels in the dtype of classes_, 0 where
        nothing was classified.  With want_margin: (map, margin), float32 (H, W): the smallest |decision| among the winner's
        pairs.  mask ((H, W), non-zero = valid): only the valid pixels are classified (rsseg.masked: Context.compact_plan /
        compact / expand); label 0 and a NaN margin elsewhere."""
        from .masked import make_plan, planes_to_device
        self._check_fitted()
        if isinstance(features, np.ndarray):
            if features.ndim != 3:
                raise ValueError("features must be a 3-D array (height, width, n_features) or a list of planes")
            planes = [features[:, :, i] for i in range(features.shape[2])]
        else:
            planes = [np.asarray(p) for p in features]
        if len(planes) != self.n_features_in_:
            raise ValueError(f"SVMClassifier.predict_image: {len(planes)} planes, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        dev, _, shape = planes_to_device(ctx, planes)
        if mask is not None:
            plan = make_plan(ctx, mask, dev[0].numel())
            lab_c, m_c = self._classify(ctx, ctx.compact(plan, dev), want_margin)
            labels = ctx.expand(plan, lab_c, 0)
            margin = None if m_c is None else ctx.expand(plan, m_c, float("nan"))
        else:
            labels, margin = self._classify(ctx, dev, want_margin)
        out = self._to_classes(labels.cpu().numpy()).reshape(shape)
        if not want_margin:
            return out
        return out, margin.cpu().numpy().reshape(shape)


def _check_classes(classes, who):
    as_int = classes.astype(np.int64) if classes.dtype.kind in "iufb" else None
    if as_int is None or np.any(as_int != classes):
        raise ValueError(f"{who}: class labels must be integers")
    if classes.size < 2:
        raise ValueError(f"{who}: {classes.size} class, an SVM needs at least 2")
    if classes.size > MAX_CLASSES:
        raise ValueError(f"{who}: {classes.size} classes, more than {MAX_CLASSES} classes are not supported")


# ---- command line ------------------------------------------------------------------------------------------------------------
def _gamma_arg(s: str):
    return s if s in ("scale", "auto") else float(s)


def build_parser():
    import argparse
    from .stages import MASK_NODATA_FROM_TAG
    ap = argparse.ArgumentParser(prog="python -m rsseg.svm",
                                 description="Train and apply a support vector machine on the output directory of an earlier "
                                             "`python -m rsseg.stages image.tif OUTDIR` run (segmentation_results/classification_svm.npy, "
                                             "svm_classification_map.tif, svm_model.npz, svm_margin.npy).")
    ap.add_argument("outdir", metavar="OUTDIR", help="the output directory of that run")
    ap.add_argument("--roi", help="the label raster to train on (.tif; 0 = unlabelled)")
    ap.add_argument("--kernel", choices=KERNELS, default="rbf")
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--gamma", type=_gamma_arg, default="scale", help="'scale', 'auto' or a number")
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--coef0", type=float, default=0.0)
    ap.add_argument("--model", metavar="PATH", help="apply this saved model (svm_model.npz) instead of training one")
    ap.add_argument("--rule-image", action="store_true", help="also write svm_margin.npy")
    def nodata_value(s):   # argparse hands a string `const` to `type` as well
        return s if s == MASK_NODATA_FROM_TAG else float(s)
    nodata_value.__name__ = "float"   # the word argparse's "invalid ... value" message uses
    ap.add_argument("--mask-nodata", nargs="?", type=nodata_value, const=MASK_NODATA_FROM_TAG, default=None, metavar="VALUE",
                    help="classify only the valid pixels: without a value those of the earlier run's feature_outputs/valid_mask.npy, with "
                         "one those where no feature plane holds it (or a NaN)")
    return ap


def main(argv=None) -> int:
    import os
    ap = build_parser()
    a = ap.parse_args(argv)
    if (a.roi is None) == (a.model is None):
        ap.error("give --roi to train a model or --model to apply a saved one")
    fpath = os.path.join(a.outdir, "feature_outputs", "all_features_and_metadata.pkl")
    for path, what in ((fpath, "the feature file of the earlier run"), (a.roi, "the label raster"), (a.model, "the saved model")):
        if path is not None and not os.path.exists(path):
            ap.error(f"{path} not found: {what}")
    from . import stages
    valid = None
    if a.mask_nodata == stages.MASK_NODATA_FROM_TAG:
        vpath = os.path.join(a.outdir, "feature_outputs", "valid_mask.npy")
        if not os.path.exists(vpath):
            ap.error(f"{vpath} not found: the earlier run masked no nodata; name the value: --mask-nodata VALUE")
        valid = np.load(vpath)
    elif a.mask_nodata is not None:
        _, arr, _ = stages._supervised_stack(fpath, os.path.join(a.outdir, "segmentation_results"), "python -m rsseg.svm")
        valid, _ = stages.nodata_valid_mask(_ctx(None), np.moveaxis(arr, -1, 0), float(a.mask_nodata))
    out = stages.run_svm_stage(fpath, os.path.join(a.outdir, "segmentation_results"), labeled_roi_file=a.roi, kernel=a.kernel, C=a.C, gamma=a.gamma,
                               degree=a.degree, coef0=a.coef0, model_path=a.model, rule_image=a.rule_image, valid_mask=valid)
    vals, counts = np.unique(out, return_counts=True)
    print("svm: " + ", ".join(f"class {int(v)}: {int(c)}" for v, c in zip(vals, counts)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
