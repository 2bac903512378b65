"""
Drop-in counterpart of predict_image of the reference's modules/supervised_classifiers.py:99-115: a
fitted sklearn RandomForestClassifier (or an already flattened forest dict) applied to every pixel of an
(H, W, D) feature array by the K11 forest-walk kernel.  Like the reference, any failure is reported and
answered with an all-zero map (supervised_classifiers.py:113-115) — except a forest beyond the capacity of the
kernels (more than 64 features or classes): that is this library's limit, not a failure the reference would have had,
and raises rsseg.runtime.RssegUnsupported instead of returning an empty map.

prepare_training_samples and train_random_forest_from_samples are the reference's interactive-sample helpers
(supervised_classifiers.py:32-52, 85-97): same names, defaults and print-and-return error behaviour.  The forest is fitted
by K16 on the GPU (rsseg.forest_fit: the same trees scikit-learn grows), or by scikit-learn on the host for an input K16
refuses.  train_random_forest (GridSearchCV) is not mirrored.
"""
from __future__ import annotations

import numpy as np

from rsseg.forest import flatten_forest
from rsseg.runtime import RssegUnsupported
from rsseg.runtime import default_context as _ctx

__all__ = ["prepare_training_samples", "train_random_forest_from_samples", "predict_image", "np"]


def prepare_training_samples(features, roi_array, target_labels):
    """(N, D) samples and (N,) labels: for each label of target_labels in turn, the feature vectors of the pixels of
    roi_array equal to it in row-major order.  On an error: a message and two empty arrays."""
    try:
        h, w, d = features.shape
        X, y = [], []
        for label in target_labels:
            rows, cols = np.nonzero(roi_array == label)
            X.extend(features[r, c] for r, c in zip(rows, cols))
            y.extend([label] * len(rows))
        return np.array(X), np.array(y)
    except Exception as e:  # noqa: BLE001 — reference behaviour
        print("❌ prepare_training_samples 出错:", e)
        return np.array([]), np.array([])


def train_random_forest_from_samples(samples, labels, save_path="output/rf_model.pkl"):
    """RandomForestClassifier(n_estimators=100, max_depth=None, random_state=42) fitted on the samples (on the GPU when
    K16 takes the input), saved with joblib.dump to save_path and returned; on an error a message and None."""
    try:
        import joblib
        from sklearn.ensemble import RandomForestClassifier
        from rsseg.forest_fit import fit
        model = RandomForestClassifier(n_estimators=100, max_depth=None, random_state=42)
        try:
            fit(model, samples, labels)
        except RssegUnsupported:
            model.fit(samples, labels)
        joblib.dump(model, save_path)
        print(f"✅ 交互采样模型训练完成，保存至 {save_path}")
        return model
    except Exception as e:  # noqa: BLE001 — reference behaviour
        print("❌ 交互训练失败:", e)
        return None


def _predict_planes(model, planes):
    forest = model if isinstance(model, dict) else flatten_forest(model)
    ctx = _ctx()
    ctx.forest_load(forest)
    dev = [ctx.to_device(np.ascontiguousarray(p, dtype=np.float32).reshape(-1)) for p in planes]  # _forest.py:640 float32 cast
    out = ctx.forest_predict(dev).cpu().numpy()
    return out.astype(np.asarray(forest["classes"]).dtype, copy=False)


def predict_image(model, features):
    try:
        h, w, d = features.shape
        planes = [features[:, :, i] for i in range(d)]
        return _predict_planes(model, planes).reshape(h, w)
    except RssegUnsupported:
        raise
    except Exception as e:  # noqa: BLE001 — reference behaviour
        print("❌ 预测失败:", e)
        return np.zeros(features.shape[:2], dtype=int)
