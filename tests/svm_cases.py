"""Seeded cases of the support vector machine (K28): models straight from a generator for the kernel's shape sweep, and models
fitted by scikit-learn on class blobs (gaussian_cases.blobs: correlated Gaussian blobs rounded to float32)."""
import functools

import numpy as np

import gaussian_cases as GC
import svm_ref as R

N_TRAIN = 40      # training samples per class
N_TEST = 1025     # test pixels
# (k, F) of the fitted cases; the separation keeps neighbouring blobs overlapping, so every class pair has support vectors of both
FITTED = ((2, 3), (3, 8), (8, 19))


def random_model(F: int, k: int, S: int, kernel: str, seed: int, degree: int = 3) -> dict:
    """A model as svm_ref reads it: uneven n_support with one class of a single support vector, coefficients of both signs with
    exact zeros among them, class values that are not 1..k, an offset and a scale (one of them negative) on every feature."""
    assert S >= k >= 2
    rng = np.random.default_rng(seed)
    ns = np.ones(k, np.int64)
    one = int(rng.integers(0, k))                     # this class keeps its single support vector
    others = [j for j in range(k) if j != one]
    ns[others] += rng.multinomial(S - k, rng.dirichlet(np.full(len(others), 0.7)))
    assert ns.sum() == S and ns[one] == 1
    sv = rng.standard_normal((S, F))
    coef = rng.standard_normal((k - 1, S))
    coef[rng.random(coef.shape) < 0.2] = 0.0
    offset = 0.3 * rng.standard_normal(F)
    scale = rng.uniform(0.5, 2.0, F)
    scale[F // 2] = -scale[F // 2]
    values = np.sort(rng.permutation(254)[:k].astype(np.int64) + 2)[::-1].astype(np.uint8)   # descending: not the class order
    m = dict(offset=offset, scale=scale, sv=sv, n_support=ns.astype(np.int32), coef=coef, bias=0.1 * rng.standard_normal(k * (k - 1) // 2),
             class_values=values, kernel=kernel, gamma=0.4 / F, coef0=1.0 if kernel == "poly" else 0.0, degree=degree, w=None)
    if kernel == "linear":
        m["w"] = R.fold_linear(sv, m["n_support"], coef)
    return m


def model_args(m: dict) -> dict:
    """The keyword arguments of Context.svm_classify for a model dict."""
    return dict(offset=m["offset"], scale=m["scale"], sv=m["sv"], n_support=m["n_support"], coef=m["coef"], bias=m["bias"],
                class_values=m["class_values"], kernel=m["kernel"], gamma=m["gamma"], coef0=m["coef0"], degree=m["degree"], w=m["w"])


def model_of(clf) -> dict:
    """The model dict of a fitted rsseg.svm.SVMClassifier."""
    p = clf.params()
    return dict(offset=p["offset"], scale=p["scale"], sv=p["support_vectors"], n_support=p["n_support"], coef=p["dual_coef"], bias=p["intercept"],
                class_values=p["class_values"], kernel=p["kernel"], gamma=p["gamma"], coef0=p["coef0"], degree=p["degree"],
                w=p["w"] if p["kernel"] == "linear" else None)


@functools.lru_cache(maxsize=None)
def blobs(k: int, F: int):
    """(X_train float32 (k N_TRAIN, F), y_train, X_test float32 (N_TEST, F), y_test): labels 3, 7, 11, ..."""
    return GC.blobs(F, k, 1.2, 100 * k + F, n_train=N_TRAIN, n_test=N_TEST)


@functools.lru_cache(maxsize=None)
def fitted(k: int, F: int, kernel: str):
    """(SVC trained on the standardised training samples, offset, scale, X_test) with the issue's parameters: poly is degree 3,
    coef0 1."""
    from sklearn.svm import SVC
    Xtr, ytr, Xte, _ = blobs(k, F)
    X = Xtr.astype(np.float64)
    offset = X.mean(axis=0)
    std = X.std(axis=0)
    scale = np.where(std > 0.0, 1.0 / np.where(std > 0.0, std, 1.0), 1.0)
    svc = SVC(kernel=kernel, degree=3, coef0=1.0 if kernel == "poly" else 0.0, decision_function_shape="ovo").fit((X - offset) * scale, ytr)
    return svc, offset, scale, Xte
