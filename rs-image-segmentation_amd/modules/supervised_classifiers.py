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
refuses.  train_random_forest (supervised_classifiers.py:57-83) is the reference's grid search: every fold fit of every
candidate grown in one K16 call and scored by K11 (rsseg.forest_grid.grid_search: GridSearchCV's scores, ranks and best
model), or scikit-learn's GridSearchCV on the host for a search the device path refuses.
"""
from __future__ import annotations

import os

import numpy as np

from rsseg.forest import flatten_forest
from rsseg.runtime import RssegUnsupported
from rsseg.runtime import default_context as _ctx

__all__ = ["prepare_training_samples", "train_random_forest", "train_random_forest_from_samples", "predict_image", "np"]


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


def train_random_forest(X, y, param_grid=None, save_path="output/rf_model.pkl"):
    """GridSearchCV(RandomForestClassifier(), param_grid, cv=3) over (X, y), the default grid being n_estimators 100, max_depth
    10 / 20 / None, random_state 42 (on the GPU when the search is one rsseg.forest_grid takes): the refitted best model,
    saved with joblib.dump to save_path and returned; on an error a message and None."""
    try:
        import joblib
        from sklearn.ensemble import RandomForestClassifier
        from rsseg.forest_grid import grid_search
        if param_grid is None:
            param_grid = {
                'n_estimators': [100],
                'max_depth': [10, 20, None],
                'random_state': [42]
            }
        try:
            best_model = grid_search(RandomForestClassifier(), param_grid, X, y, cv=3).best_estimator_
        except RssegUnsupported:
            from sklearn.model_selection import GridSearchCV
            grid = GridSearchCV(RandomForestClassifier(), param_grid, cv=3, n_jobs=-1)
            grid.fit(X, y)
            best_model = grid.best_estimator_
        os.makedirs(os.path.dirname(save_path), exist_ok=True)
        joblib.dump(best_model, save_path)
        print(f"✅ 模型训练完成，保存至 {save_path}")
        return best_model
    except Exception as e:  # noqa: BLE001 — reference behaviour
        print("❌ 随机森林训练失败:", e)
        return None


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
