"""Seeded cases of the Gaussian classifiers (K22): correlated Gaussian blobs rounded to float32, N_TRAIN training samples per
class and N_TEST test pixels drawn from the same mixture.  Class labels are not 1..k on purpose (the class map carries the
labels themselves)."""
import functools

import numpy as np

N_TRAIN = 4000
N_TEST = 40000

# name -> (F, k, separation of the class means in units of the blobs' spread, seed)
CASES = {
    "f19_k6_separated": (19, 6, 3.0, 11),
    "f19_k6_overlapping": (19, 6, 0.25, 12),
    "f4_k3": (4, 3, 1.5, 13),
    "f32_k16": (32, 16, 1.5, 14),
    "f1_k2": (1, 2, 1.5, 15),
    "f64_k2": (64, 2, 1.0, 16),
}


def class_labels(k: int) -> np.ndarray:
    """k distinct labels in 1..255, ascending, not contiguous: 3, 7, 11, ..."""
    return (3 + 4 * np.arange(k)).astype(np.int64) if k <= 63 else (1 + np.arange(k)).astype(np.int64)


def blobs(F: int, k: int, sep: float, seed: int, n_train: int = N_TRAIN, n_test: int = N_TEST):
    """(X_train float32 (k n_train, F), y_train int64, X_test float32 (n_test, F), y_test int64)."""
    rng = np.random.default_rng(seed)
    labels = class_labels(k)
    means = sep * rng.standard_normal((k, F))
    mix = [rng.standard_normal((F, F)) / np.sqrt(F) + 0.6 * np.eye(F) for _ in range(k)]   # x = mean + A e: covariance A A'
    Xtr = np.concatenate([means[j] + rng.standard_normal((n_train, F)) @ mix[j].T for j in range(k)]).astype(np.float32)
    ytr = np.repeat(labels, n_train)
    which = rng.integers(0, k, n_test)
    e = rng.standard_normal((n_test, F))
    Xte = np.empty((n_test, F))
    for j in range(k):
        s = which == j
        Xte[s] = means[j] + e[s] @ mix[j].T
    perm = rng.permutation(Xtr.shape[0])
    return Xtr[perm], ytr[perm], Xte.astype(np.float32), labels[which]


@functools.lru_cache(maxsize=None)
def case(name: str):
    F, k, sep, seed = CASES[name]
    return blobs(F, k, sep, seed)


def random_model(F: int, k: int, seed: int, spread: float = 1.0):
    """A model straight from a generator, for the kernel's shape sweep: (mean, whiten packed, offset, class_values uint8)."""
    rng = np.random.default_rng(seed)
    mean = spread * rng.standard_normal((k, F))
    W = np.tril(rng.standard_normal((k, F, F)) / np.sqrt(F)) + np.eye(F)
    i, f = np.tril_indices(F)
    offset = rng.standard_normal(k)
    values = rng.permutation(255)[:k].astype(np.uint8) + 1
    return mean, np.ascontiguousarray(W[:, i, f]), offset, values
