"""
Neural-network (multi-layer perceptron) classification (K30, csrc/k30_mlp.hip; no counterpart in the reference, whose
supervised_classifiers module has the random forest alone).  Training is scikit-learn's (sklearn.neural_network.MLPClassifier)
on the host, on samples standardised in float32, which keeps the fitted coefs_ in float32; every per-pixel step runs on the
GPU (Context.mlp_classify): the layers' float32 fma chains, the hidden activation, the winner, the margin and the softmax, value
for value what tests/mlp_ref.py restates.

The model is scikit-learn's own: coefs_ and intercepts_ in float32, the hidden activation ('relu', 'identity', 'logistic',
'tanh'); for two classes the output layer has one unit, whose logit stands against +0.
Class labels are any integers; the kernel sees class_values 1..k and the object maps them back, 0 standing for a pixel that
was not classified (an infinite feature value, or outside the mask).

    python -m rsseg.mlp OUTDIR --roi ROI [--hidden 100,100] [--activation relu|identity|logistic|tanh] [--alpha A] [--max-iter N]
                               [--model PATH] [--rule-image] [--mask-nodata [VALUE]]
trains and applies a network on the output directory of an earlier `python -m rsseg.stages image.tif OUTDIR` run
(rsseg.stages.run_mlp_stage); --model PATH applies a saved model instead of training one.
"""
from __future__ import annotations

import numpy as np

ACTIVATIONS = ("relu", "identity", "logistic", "tanh")
MAX_CLASSES = 32        # RSSEG_MLP_MAX_CLASSES
MAX_HIDDEN_LAYERS = 3   # RSSEG_MLP_MAX_HIDDEN_LAYERS
MAX_WIDTH = 128         # RSSEG_MLP_MAX_WIDTH
MAX_FEATURES = 64       # RSSEG_MAX_FEATURES


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .runtime import default_context
    return default_context()


def _hidden(hidden_layer_sizes, who) -> tuple:
    h = (hidden_layer_sizes,) if np.isscalar(hidden_layer_sizes) else tuple(hidden_layer_sizes)
    if not 1 <= len(h) <= MAX_HIDDEN_LAYERS:
        raise ValueError(f"{who}: {len(h)} hidden layers, the kernel takes 1..{MAX_HIDDEN_LAYERS}")
    if any(int(w) != w or not 1 <= int(w) <= MAX_WIDTH for w in h):
        raise ValueError(f"{who}: hidden_layer_sizes {h!r}, every width must be an integer in 1..{MAX_WIDTH}")
    return tuple(int(w) for w in h)


class NeuralNetClassifier:
    """NeuralNetClassifier(hidden_layer_sizes=(100,), activation='relu', alpha=1e-4, max_iter=500, random_state=42,
    solver='adam'): sklearn.neural_network.MLPClassifier's parameters of the same names."""

    def __init__(self, hidden_layer_sizes=(100,), activation: str = "relu", alpha: float = 1e-4, max_iter: int = 500, random_state=42,
                 solver: str = "adam"):
        if activation not in ACTIVATIONS:
            raise ValueError(f"NeuralNetClassifier: activation {activation!r} is not supported, must be one of {ACTIVATIONS}")
        if solver not in ("adam", "lbfgs", "sgd"):
            raise ValueError(f"NeuralNetClassifier: solver {solver!r}, must be 'adam', 'lbfgs' or 'sgd'")
        if not (float(alpha) >= 0.0 and np.isfinite(float(alpha))):
            raise ValueError(f"NeuralNetClassifier: alpha={alpha!r} must be a finite number >= 0")
        if int(max_iter) != max_iter or int(max_iter) < 1:
            raise ValueError(f"NeuralNetClassifier: max_iter={max_iter!r} must be an integer >= 1")
        self.hidden_layer_sizes = _hidden(hidden_layer_sizes, "NeuralNetClassifier")
        self.activation, self.alpha, self.max_iter, self.random_state, self.solver = activation, float(alpha), int(max_iter), random_state, solver

    # ---- fitting (host) ----------------------------------------------------------------------------------------------
    def fit(self, X, y) -> "NeuralNetClassifier":
        import warnings
        from sklearn.exceptions import ConvergenceWarning
        from sklearn.neural_network import MLPClassifier
        X = np.asarray(X, dtype=np.float32)
        y = np.asarray(y).reshape(-1)
        if X.ndim != 2 or X.shape[0] != y.size or X.shape[0] == 0:
            raise ValueError(f"NeuralNetClassifier.fit: X {X.shape} and y {y.shape} are not n samples of F features")
        if not np.all(np.isfinite(X)):
            raise ValueError("NeuralNetClassifier.fit: X holds NaN or infinite values")
        if X.shape[1] > MAX_FEATURES:
            raise ValueError(f"NeuralNetClassifier.fit: {X.shape[1]} features, the kernel takes at most {MAX_FEATURES}")
        _check_classes(np.unique(y), "NeuralNetClassifier.fit")
        offset = X.mean(axis=0, dtype=np.float32)
        std = X.std(axis=0, dtype=np.float32)
        scale = np.where(std > 0, np.float32(1) / np.where(std > 0, std, np.float32(1)), np.float32(1)).astype(np.float32)   # a constant column: scale 1
        mlp = MLPClassifier(hidden_layer_sizes=self.hidden_layer_sizes, activation=self.activation, alpha=self.alpha, max_iter=self.max_iter,
                            random_state=self.random_state, solver=self.solver)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            mlp.fit((X - offset) * scale, y)
        return self._take(mlp, offset, scale)

    def fit_image(self, features, roi_mask) -> "NeuralNetClassifier":
        """fit() on the rows of the (H, W, F) stack under the non-zero pixels of roi_mask (GaussianClassifier.training_samples)."""
        from .gaussian import GaussianClassifier
        return self.fit(*GaussianClassifier.training_samples(features, roi_mask))

    @classmethod
    def from_sklearn(cls, mlp, offset=None, scale=None) -> "NeuralNetClassifier":
        """The model of a fitted sklearn.neural_network.MLPClassifier that was trained on (X - offset) * scale (default: on X
        itself).  A model fitted on float64 samples has float64 coefs_; they are rounded to float32, and labels near a
        decision boundary may then differ from the float64 model's."""
        if not hasattr(mlp, "coefs_"):
            raise ValueError("NeuralNetClassifier.from_sklearn: the MLPClassifier is not fitted")
        if mlp.activation not in ACTIVATIONS:
            raise ValueError(f"NeuralNetClassifier.from_sklearn: activation {mlp.activation!r} is not supported, only {ACTIVATIONS}")
        if getattr(mlp, "out_activation_", None) not in ("softmax", "logistic"):
            raise ValueError("NeuralNetClassifier.from_sklearn: a multilabel or regression network is not supported")
        if mlp.out_activation_ == "logistic" and (len(mlp.classes_) != 2 or mlp.coefs_[-1].shape[1] != 1):
            raise ValueError("NeuralNetClassifier.from_sklearn: a multilabel network is not supported")
        _check_classes(np.asarray(mlp.classes_), "NeuralNetClassifier.from_sklearn")
        self = cls.__new__(cls)
        self.hidden_layer_sizes = _hidden(tuple(c.shape[1] for c in mlp.coefs_[:-1]), "NeuralNetClassifier.from_sklearn")
        self.activation, self.alpha, self.max_iter, self.random_state, self.solver = mlp.activation, float(mlp.alpha), int(mlp.max_iter), mlp.random_state, mlp.solver
        F = mlp.coefs_[0].shape[0]
        return self._take(mlp, np.zeros(F, np.float32) if offset is None else offset, np.ones(F, np.float32) if scale is None else scale)

    def _take(self, mlp, offset, scale) -> "NeuralNetClassifier":
        k = len(mlp.classes_)
        return self._set(mlp.coefs_, mlp.intercepts_, mlp.classes_, np.arange(1, k + 1), offset, scale)

    def _set(self, coefs, intercepts, classes, class_values, offset, scale) -> "NeuralNetClassifier":
        who = "NeuralNetClassifier"
        with np.errstate(over="ignore"):
            coefs = [np.array(c, dtype=np.float32, ndmin=2, order="C") for c in coefs]
            intercepts = [np.array(b, dtype=np.float32).reshape(-1) for b in intercepts]
            offset, scale = np.array(offset, dtype=np.float32).reshape(-1), np.array(scale, dtype=np.float32).reshape(-1)
        classes = np.asarray(classes).reshape(-1).copy()
        cv = np.asarray(class_values).reshape(-1)
        k = classes.size
        if k < 2:
            raise ValueError(f"{who}: {k} classes, a model needs at least 2")
        if k > MAX_CLASSES:
            raise ValueError(f"{who}: {k} classes, more than {MAX_CLASSES} classes are not supported")
        if not 2 <= len(coefs) <= MAX_HIDDEN_LAYERS + 1:
            raise ValueError(f"{who}: {len(coefs) - 1} hidden layers, the kernel takes 1..{MAX_HIDDEN_LAYERS}")
        F = coefs[0].shape[0]
        if F > MAX_FEATURES:
            raise ValueError(f"{who}: {F} features, the kernel takes at most {MAX_FEATURES}")
        widths = [F] + [c.shape[1] for c in coefs]
        if (len(intercepts) != len(coefs) or any(c.shape[0] != w for c, w in zip(coefs, widths)) or any(b.size != w for b, w in zip(intercepts, widths[1:]))
                or widths[-1] != (1 if k == 2 else k) or offset.size != F or scale.size != F or cv.size != k):
            raise ValueError(f"{who}: coefficients {[c.shape for c in coefs]}, intercepts {[b.shape for b in intercepts]}, offset {offset.shape}, "
                             f"scale {scale.shape}, classes {classes.shape} and class_values {cv.shape} do not describe one model")
        if any(not 1 <= w <= MAX_WIDTH for w in widths[1:-1]):
            raise ValueError(f"{who}: hidden widths {widths[1:-1]}, every width must be in 1..{MAX_WIDTH}")
        if np.any(cv != cv.astype(np.int64)) or np.any(cv < 1) or np.any(cv > 255) or np.unique(cv).size != k:
            raise ValueError(f"{who}: class_values must be distinct integers in 1..255")
        for name, arrs in (("coefficients", coefs), ("intercepts", intercepts), ("offset", [offset]), ("scale", [scale])):
            if not all(np.all(np.isfinite(a)) for a in arrs):
                raise ValueError(f"{who}: the {name} are not finite in float32")
        if np.any(scale == 0):
            raise ValueError(f"{who}: a scale of 0")
        self.classes_ = classes
        self.class_values_ = cv.astype(np.uint8)
        self.n_features_in_ = F
        self.coefs_, self.intercepts_, self.offset_, self.scale_ = coefs, intercepts, offset, scale
        self.widths_ = np.array(widths, np.int32)
        self.hidden_layer_sizes = tuple(int(w) for w in widths[1:-1])
        return self

    # ---- the model as arrays -------------------------------------------------------------------------------------------
    def _check_fitted(self):
        if not hasattr(self, "coefs_"):
            raise ValueError("NeuralNetClassifier: not fitted (fit, fit_image, from_sklearn, from_params or load first)")

    def params(self) -> dict:
        """Everything predict needs: activation, widths (int32: F, the hidden widths, the output units), weights (float32: the
        layers' coefficient matrices flattened row-major and concatenated), biases (float32, concatenated), offset, scale
        (float32 (F,)), classes, class_values (uint8)."""
        self._check_fitted()
        return dict(activation=self.activation, widths=self.widths_.copy(), weights=np.concatenate([c.reshape(-1) for c in self.coefs_]),
                    biases=np.concatenate(self.intercepts_), offset=self.offset_.copy(), scale=self.scale_.copy(), classes=self.classes_.copy(),
                    class_values=self.class_values_.copy())

    @classmethod
    def from_params(cls, activation, widths, weights, biases, offset=None, scale=None, class_values=None, classes=None) -> "NeuralNetClassifier":
        """A model from its arrays (params()' keys).  class_values default to 1..k, classes to class_values, offset / scale to
        0 / 1."""
        w = np.asarray(widths).reshape(-1)
        if w.size < 3 or np.any(w != w.astype(np.int64)) or np.any(w < 1):
            raise ValueError(f"NeuralNetClassifier: widths {w.tolist()} are not the widths of an input, 1..{MAX_HIDDEN_LAYERS} hidden layers and an output")
        w = w.astype(np.int64)
        self = cls(hidden_layer_sizes=tuple(int(v) for v in w[1:-1]), activation=str(activation))
        weights, biases = np.asarray(weights).reshape(-1), np.asarray(biases).reshape(-1)
        if weights.size != int((w[:-1] * w[1:]).sum()) or biases.size != int(w[1:].sum()):
            raise ValueError(f"NeuralNetClassifier: {weights.size} weights and {biases.size} biases do not describe layers of widths {w.tolist()}")
        coefs, intercepts, aw, ab = [], [], 0, 0
        for a, b in zip(w[:-1], w[1:]):
            coefs.append(weights[aw:aw + a * b].reshape(a, b))
            intercepts.append(biases[ab:ab + b])
            aw, ab = aw + a * b, ab + b
        F, k = int(w[0]), (2 if w[-1] == 1 else int(w[-1]))
        cv = np.arange(1, k + 1) if class_values is None else class_values
        return self._set(coefs, intercepts, cv if classes is None else classes, cv, np.zeros(F, np.float32) if offset is None else offset,
                         np.ones(F, np.float32) if scale is None else scale)

    def save(self, path) -> str:
        """The model as an .npz of plain arrays (no pickled objects)."""
        p = self.params()
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, activation=np.array(p["activation"]), **{key: p[key] for key in p if key != "activation"})
        return path

    @classmethod
    def load(cls, path) -> "NeuralNetClassifier":
        with np.load(str(path), allow_pickle=False) as z:
            return cls.from_params(str(z["activation"]), z["widths"], z["weights"], z["biases"], offset=z["offset"], scale=z["scale"],
                                   class_values=z["class_values"], classes=z["classes"])

    # ---- prediction (GPU) ----------------------------------------------------------------------------------------------
    def _classify(self, ctx, dev, want_margin=False, want_conf=False, want_proba=False):
        p = self.params()
        return ctx.mlp_classify(dev, p["widths"], p["weights"], p["biases"], p["offset"], p["scale"], self.activation, self.class_values_,
                                want_margin=want_margin, want_conf=want_conf, want_proba=want_proba)

    def _to_classes(self, labels_u8: np.ndarray) -> np.ndarray:
        lut = np.zeros(256, self.classes_.dtype)
        lut[self.class_values_] = self.classes_
        return lut[labels_u8]

    def _rows(self, X, who, ctx):
        """The columns of X as float32 device planes (on ctx, or the default context: asked for only once X has passed)."""
        self._check_fitted()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError(f"NeuralNetClassifier.{who}: X {X.shape}, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        return ctx, [ctx.to_device(np.ascontiguousarray(X[:, f], dtype=np.float32)) for f in range(X.shape[1])]

    def predict(self, X, ctx=None) -> np.ndarray:
        """Labels of the rows of X (n, F), read as float32, in the dtype of classes_; 0 for a row with an infinite value.  A NaN
        feature reads as 0."""
        ctx, dev = self._rows(X, "predict", ctx)
        labels = self._classify(ctx, dev)[0]
        return self._to_classes(labels.cpu().numpy())

    def predict_proba(self, X, ctx=None) -> np.ndarray:
        """(n, k) float32 class probabilities of the rows of X, the columns in the order of classes_; NaN for a row with an
        infinite value."""
        ctx, dev = self._rows(X, "predict_proba", ctx)
        proba = self._classify(ctx, dev, want_proba=True)[3]
        return np.ascontiguousarray(proba.cpu().numpy().T)

    def predict_image(self, features, mask=None, want_margin: bool = False, want_conf: bool = False, want_proba: bool = False, ctx=None):
        """The class map of an (H, W, F) array or a list of F (H, W) planes: (H, W) class labels in the dtype of classes_, 0 where
        nothing was classified.  With any of want_margin / want_conf / want_proba a tuple: the map, then in this order the wanted
        ones of margin (float32 (H, W): the winner's logit minus the runner-up's), confidence (float32 (H, W): the winner's
        probability) and probabilities (float32 (k, H, W)).  mask ((H, W), non-zero = valid): only the valid pixels are
        classified (rsseg.masked: Context.compact_plan / compact / expand); label 0 and NaN elsewhere."""
        from .masked import make_plan, planes_to_device
        self._check_fitted()
        if isinstance(features, np.ndarray):
            if features.ndim != 3:
                raise ValueError("features must be a 3-D array (height, width, n_features) or a list of planes")
            planes = [features[:, :, i] for i in range(features.shape[2])]
        else:
            planes = [np.asarray(p) for p in features]
        if len(planes) != self.n_features_in_:
            raise ValueError(f"NeuralNetClassifier.predict_image: {len(planes)} planes, the model has {self.n_features_in_} features")
        ctx = _ctx(ctx)
        planes = [np.ascontiguousarray(p, dtype=np.float32) for p in planes]
        dev, _, shape = planes_to_device(ctx, planes)
        k = self.classes_.size
        if mask is not None:
            plan = make_plan(ctx, mask, dev[0].numel())
            lab_c, m_c, c_c, p_c = self._classify(ctx, ctx.compact(plan, dev), want_margin, want_conf, want_proba)
            labels = ctx.expand(plan, lab_c, 0)
            nan = float("nan")
            margin = None if m_c is None else ctx.expand(plan, m_c, nan)
            conf = None if c_c is None else ctx.expand(plan, c_c, nan)
            proba = None if p_c is None else [ctx.expand(plan, p_c[j].contiguous(), nan) for j in range(k)]
        else:
            labels, margin, conf, proba = self._classify(ctx, dev, want_margin, want_conf, want_proba)
        out = [self._to_classes(labels.cpu().numpy()).reshape(shape)]
        if want_margin:
            out.append(margin.cpu().numpy().reshape(shape))
        if want_conf:
            out.append(conf.cpu().numpy().reshape(shape))
        if want_proba:
            out.append(np.stack([proba[j].cpu().numpy().reshape(shape) for j in range(k)]))
        return out[0] if len(out) == 1 else tuple(out)


def _check_classes(classes, who):
    as_int = classes.astype(np.int64) if classes.dtype.kind in "iufb" else None
    if as_int is None or np.any(as_int != classes):
        raise ValueError(f"{who}: class labels must be integers")
    if classes.size < 2:
        raise ValueError(f"{who}: {classes.size} class, a network needs at least 2")
    if classes.size > MAX_CLASSES:
        raise ValueError(f"{who}: {classes.size} classes, more than {MAX_CLASSES} classes are not supported")


# ---- command line ------------------------------------------------------------------------------------------------------------
def _hidden_arg(s: str):
    return tuple(int(v) for v in s.split(","))


def build_parser():
    import argparse
    from .stages import MASK_NODATA_FROM_TAG
    ap = argparse.ArgumentParser(prog="python -m rsseg.mlp",
                                 description="Train and apply a neural-network classifier on the output directory of an earlier "
                                             "`python -m rsseg.stages image.tif OUTDIR` run (segmentation_results/classification_mlp.npy, "
                                             "mlp_classification_map.tif, mlp_model.npz, mlp_margin.npy, mlp_confidence.npy).")
    ap.add_argument("outdir", metavar="OUTDIR", help="the output directory of that run")
    ap.add_argument("--roi", help="the label raster to train on (.tif; 0 = unlabelled)")
    ap.add_argument("--hidden", type=_hidden_arg, default=(100,), metavar="W[,W[,W]]", help="the hidden layers' widths, e.g. 100,100")
    ap.add_argument("--activation", choices=ACTIVATIONS, default="relu")
    ap.add_argument("--alpha", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--model", metavar="PATH", help="apply this saved model (mlp_model.npz) instead of training one")
    ap.add_argument("--rule-image", action="store_true", help="also write mlp_margin.npy and mlp_confidence.npy")
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
        _, arr, _ = stages._supervised_stack(fpath, os.path.join(a.outdir, "segmentation_results"), "python -m rsseg.mlp")
        valid, _ = stages.nodata_valid_mask(_ctx(None), np.moveaxis(arr, -1, 0), float(a.mask_nodata))
    out = stages.run_mlp_stage(fpath, os.path.join(a.outdir, "segmentation_results"), labeled_roi_file=a.roi, hidden_layer_sizes=a.hidden,
                               activation=a.activation, alpha=a.alpha, max_iter=a.max_iter, model_path=a.model, rule_image=a.rule_image,
                               valid_mask=valid)
    vals, counts = np.unique(out, return_counts=True)
    print("mlp: " + ", ".join(f"class {int(v)}: {int(c)}" for v, c in zip(vals, counts)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
