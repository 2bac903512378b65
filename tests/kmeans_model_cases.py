"""The seeded cases of the K18 tests (tests/test_kmeans_model_host.py on the CPU, tests/test_gpu_kmeans_model.py on the GPU).

A case is a MODEL, fitted by scikit-learn on the CPU (MinMaxScaler + KMeans(n_init=1, random_state=42) on a training matrix)
and taken over through KMeansModel.from_sklearn, so the sweep is tested independently of the GPU fit, and a SCENE to predict,
drawn separately.  The scene has N_MAX[dtype] pixels (two chunks + 5); every other pixel count of PIXEL_COUNTS is a prefix of
it: every per-pixel result of a prefix is the prefix of the result, which tests/kmeans_model_ref.py computes once per case."""
import functools

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)

# every register-resident width (F <= 8 / 16 / 32), every KMAX step (k <= 8 / 16 / 32 / 64) and the two blocked forms
# (F > 32; float64 with k > 32 and F > 8; (8, 64, f64) is the register-resident neighbour of the latter)
WIDTHS = [(1, 1, F32), (3, 2, F32), (8, 8, F32), (9, 9, F32), (15, 8, F32), (16, 16, F64), (17, 17, F32), (19, 7, F64), (32, 32, F32),
          (33, 33, F32), (55, 7, F32), (64, 64, F32), (8, 64, F64), (9, 64, F64)]

# the seams of the launch geometry: one tile -+ 1, one chunk exactly, one chunk + 3, two chunks + 5
PIXEL_COUNTS = {F32: [1, 3, 1023, 1025, 16384, 16387, 32773], F64: [1, 3, 511, 513, 8192, 8195, 16389]}
N_MAX = {F32: 32773, F64: 16389}
N_TRAIN = 1500

# name -> (F, k, dtype, style).  Styles: blobs; grid (a coarse grid with exact distance ties); nan (2 % NaN); wide (the scene
# spans [-0.5, 1.5] of the fitted range); const (a constant plane in the training matrix: zero range -> scale 1); overflow (one
# pixel of the scene lies beyond the bound of the inertia sum).
CASES = {}
for _F, _k, _dt in WIDTHS:
    CASES[f"blobs-{_F}-{_k}-{_dt.name}"] = (_F, _k, _dt, "blobs")
for _F, _k, _dt, _style in [(3, 2, F32, "grid"), (19, 7, F64, "grid"), (15, 8, F32, "nan"), (16, 16, F64, "nan"), (33, 33, F32, "nan"),
                            (9, 9, F32, "wide"), (55, 7, F32, "wide"), (9, 64, F64, "wide"), (8, 8, F32, "const"), (19, 7, F64, "const"),
                            (3, 2, F32, "overflow")]:
    CASES[f"{_style}-{_F}-{_k}-{_dt.name}"] = (_F, _k, _dt, _style)
NAMES = list(CASES)
OVERFLOW_AT = 777       # the pixel of the overflow scene that lies beyond the bound: inside the pixel counts from 1023 on


def sklearn_exact(name: str) -> bool:
    """Whether the labels of the case must equal scikit-learn's predict: every case but the overflow scene, whose far pixel
    makes ||c||^2 - 2 x.c cancel far beyond the model's range."""
    return CASES[name][3] != "overflow"


def _blobs(rng, n, F, k, dt, spread=0.35):
    cen = rng.uniform(-2, 2, (max(k, 2), F))
    lab = rng.integers(0, max(k, 2), n)
    return (cen[lab] + spread * rng.standard_normal((n, F))).astype(dt)


def _grid(rng, n, F, dt):
    # three levels per feature, 0, 0.5 and 1: every squared distance between grid points is a multiple of 0.25
    return (rng.integers(0, 3, (n, F)) * 0.5).astype(dt)


def _grid_train(rng, n, F, k, dt):
    # k distinct grid points, each repeated equally often, the set closed under x -> 1 - x (pairs, and the middle point when k is
    # odd), the first pair two opposite corners.  Every plane then spans [0, 1] (scale 1, offset 0) with mean exactly 0.5, so
    # the fit's centring and its means are exact and its centres are those points themselves: all the arithmetic of the sweep
    # is exact, and many pixels of a grid scene are EXACTLY as far from two centres.
    corner = rng.integers(0, 2, F).astype(dt)
    half = [corner]
    while len(half) < k // 2:
        p = _grid(rng, 1, F, dt)[0]
        if not any((p == q).all() or (p == 1 - q).all() for q in half) and (p != 0.5).any():
            half.append(p)
    pts = [q for p in half for q in (p, 1 - p)] + ([np.full(F, 0.5, dt)] if k % 2 else [])
    return np.repeat(np.stack(pts), n // k, axis=0)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> dict(F, k, dtype, style, scaler, kmeans (fitted scikit-learn objects), X (N_MAX x F scene), planes (its F columns))."""
    from sklearn.cluster import KMeans
    from sklearn.preprocessing import MinMaxScaler
    F, k, dt, style = CASES[name]
    seed = 1000 + NAMES.index(name)
    rng = np.random.default_rng(seed)
    n = N_MAX[dt]
    if style == "grid":
        train, X = _grid_train(rng, N_TRAIN, F, k, dt), _grid(rng, n, F, dt)
    else:
        both = _blobs(rng, N_TRAIN + n, F, k, dt)
        train, X = both[:N_TRAIN].copy(), both[N_TRAIN:].copy()
    if style == "const":
        train[:, F // 2] = dt.type(0.75)          # the scene keeps its spread in that plane
    scaler = MinMaxScaler().fit(train)
    km = KMeans(n_clusters=k, n_init=1, random_state=42).fit(scaler.transform(train))
    if style == "nan":
        X[rng.random(X.shape) < 0.02] = np.nan
    elif style == "wide":
        lo, hi = train.min(axis=0), train.max(axis=0)
        X = (lo - 0.5 * (hi - lo) + rng.random((n, F)) * 2.0 * (hi - lo)).astype(dt)
    elif style == "overflow":
        lo, hi = train.min(axis=0), train.max(axis=0)
        X[OVERFLOW_AT, 0] = dt.type(lo[0] + 30.0 * (hi[0] - lo[0]))     # scaled value 30: sq ~ 900, beyond float32's 512, below 2^11
    X = np.ascontiguousarray(X)
    return dict(F=F, k=k, dtype=dt, style=style, scaler=scaler, kmeans=km, X=X, planes=[np.ascontiguousarray(X[:, f]) for f in range(F)])


@functools.lru_cache(maxsize=None)
def model(name: str):
    from rsseg.kmeans_model import KMeansModel
    c = case(name)
    return KMeansModel.from_sklearn(c["scaler"], c["kmeans"])


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """tests/kmeans_model_ref.apply on the whole scene, once per case; treat as read-only."""
    import kmeans_model_ref as R
    m = model(name)
    ref = R.apply(case(name)["X"], m.cluster_centers_, m.scale_, m.min_)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def sklearn_labels(name: str):
    """to_sklearn()'s own predict of the scene (NaN -> 0 first, as the pipeline does before the scaler)."""
    sc, km = model(name).to_sklearn()
    X = np.nan_to_num(case(name)["X"], nan=0.0)
    lab = km.predict(sc.transform(X)).astype(np.int32)
    lab.setflags(write=False)
    return lab
