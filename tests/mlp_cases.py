"""Seeded cases of the neural-network classifier (K30): models straight from a generator for the kernel's shape sweep, and
networks fitted by scikit-learn on class blobs (gaussian_cases.blobs: correlated Gaussian blobs rounded to float32)."""
import functools
import warnings

import numpy as np

import gaussian_cases as GC

N_TRAIN = 40      # training samples per class
N_TEST = 1025     # test pixels
# (k, F, hidden, activation) of the fitted cases
FITTED = ((2, 3, (8,), "relu"), (3, 8, (32,), "relu"), (8, 19, (100,), "relu"), (8, 19, (64, 32), "relu"), (8, 19, (100,), "tanh"),
          (3, 8, (32,), "logistic"))


def random_model(F: int, hidden, k: int, activation: str, seed: int) -> dict:
    """A model as mlp_ref reads it: weights of both signs with exact zeros among them (scaled so that the sums stay of order 1),
    class values that are not 1..k and descend, an offset and a scale (one of them negative) on every feature."""
    rng = np.random.default_rng(seed)
    widths = [F] + list(hidden) + [1 if k == 2 else k]
    weights, biases = [], []
    for a, b in zip(widths[:-1], widths[1:]):
        W = (rng.standard_normal((a, b)) * (1.5 / np.sqrt(a))).astype(np.float32)
        if a * b >= 4:
            W[rng.random(W.shape) < 0.2] = 0.0
        weights.append(W)
        biases.append((0.3 * rng.standard_normal(b)).astype(np.float32))
    offset = (0.3 * rng.standard_normal(F)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, F).astype(np.float32)
    scale[F // 2] = -scale[F // 2]
    values = np.sort(rng.permutation(254)[:k].astype(np.int64) + 2)[::-1].astype(np.uint8)   # descending: not the class order
    return dict(widths=np.array(widths, np.int32), weights=weights, biases=biases, offset=offset, scale=scale, activation=activation,
                class_values=values)


def pixels(n: int, F: int, seed: int, spread: float = 1.5) -> np.ndarray:
    """n float32 pixels; from 64 pixels on a few NaN entries and two pixels with an infinite one."""
    rng = np.random.default_rng(seed)
    X = (spread * rng.standard_normal((n, F))).astype(np.float32)
    if n >= 64:
        X[rng.random((n, F)) < 0.01] = np.nan
        X[5, F // 2] = np.inf
        X[11, 0] = -np.inf
    return X


def model_args(m: dict) -> dict:
    """The keyword arguments of Context.mlp_classify for a model dict."""
    return dict(widths=m["widths"], weights=np.concatenate([w.reshape(-1) for w in m["weights"]]), biases=np.concatenate(m["biases"]),
                offset=m["offset"], scale=m["scale"], activation=m["activation"], class_values=m["class_values"])


def model_of(clf) -> dict:
    """The model dict of a fitted rsseg.mlp.NeuralNetClassifier."""
    return dict(widths=clf.widths_, weights=clf.coefs_, biases=clf.intercepts_, offset=clf.offset_, scale=clf.scale_, activation=clf.activation,
                class_values=clf.class_values_)


@functools.lru_cache(maxsize=None)
def blobs(k: int, F: int):
    """(X_train float32 (k N_TRAIN, F), y_train, X_test float32 (N_TEST, F), y_test): labels 3, 7, 11, ..."""
    return GC.blobs(F, k, 1.2, 100 * k + F, n_train=N_TRAIN, n_test=N_TEST)


def standardise(X):
    """(offset, scale) float32 of float32 samples: the mean, and 1 / std or 1 where the std is 0."""
    X = np.asarray(X, np.float32)
    offset = X.mean(axis=0, dtype=np.float32)
    std = X.std(axis=0, dtype=np.float32)
    scale = np.where(std > 0, np.float32(1) / np.where(std > 0, std, np.float32(1)), np.float32(1)).astype(np.float32)
    return offset, scale


@functools.lru_cache(maxsize=None)
def fitted(k: int, F: int, hidden: tuple, activation: str):
    """(MLPClassifier trained on the float32 standardised training samples with random_state=0, offset, scale, X_test)."""
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.neural_network import MLPClassifier
    Xtr, ytr, Xte, _ = blobs(k, F)
    offset, scale = standardise(Xtr)
    mlp = MLPClassifier(hidden_layer_sizes=hidden, activation=activation, random_state=0, max_iter=200)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        mlp.fit((Xtr - offset) * scale, ytr)
    return mlp, offset, scale, Xte
