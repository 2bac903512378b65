"""K22 without a GPU: the restatement (tests/gaussian_ref.py) against scikit-learn and a direct float64 evaluation, the exact
rules of the arg-min, the model object (rsseg.gaussian.GaussianClassifier) and the stage driver's argument errors.

The restatement of a seeded case is computed once and shared.  With the fma built from error-free transformations in NumPy
(kmeans_model_ref.fma64) the 40 000 pixels of the two widest cases are 360 and 170 million emulated fmas per method: about
11 s for (F, k) = (32, 16) and 5 s for (64, 2) on eight cores, every other case under 3 s."""
import functools

import numpy as np
import pytest

import gaussian_cases as GC
import gaussian_ref as R

from rsseg.gaussian import GaussianClassifier


@functools.lru_cache(maxsize=None)
def fitted(name: str, method: str):
    Xtr, ytr, Xte, _ = GC.case(name)
    clf = GaussianClassifier(method).fit(Xtr, ytr)
    p = clf.params()
    ref = R.classify(Xte, p["mean"], p["whiten"], p["offset"], p["class_values"], p["max_dist2"])
    return clf, ref


def _independent_ml(name):
    """(g[k][n], labels) of QuadraticDiscriminantAnalysis: its predict, and -2 x its discriminant evaluated in NumPy float64
    from its public fitted attributes (sklearn/discriminant_analysis.py, _decision_function)."""
    from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis
    Xtr, ytr, Xte, _ = GC.case(name)
    q = QuadraticDiscriminantAnalysis().fit(Xtr.astype(np.float64), ytr)
    X = Xte.astype(np.float64)
    g = []
    for c in range(len(q.classes_)):
        X2 = (X - q.means_[c]) @ (q.rotations_[c] * (q.scalings_[c] ** -0.5))
        g.append(np.sum(X2 ** 2, axis=1) + np.sum(np.log(q.scalings_[c])) - 2.0 * np.log(q.priors_[c]))
    return np.array(g), q.predict(X)


def _independent_mindist(name):
    from sklearn.neighbors import NearestCentroid
    Xtr, ytr, Xte, _ = GC.case(name)
    nc = NearestCentroid().fit(Xtr.astype(np.float64), ytr)
    X = Xte.astype(np.float64)
    g = np.array([np.sum((X - c) ** 2, axis=1) for c in nc.centroids_])
    return g, nc.predict(X)


def _independent_mahalanobis(name):
    Xtr, ytr, Xte, _ = GC.case(name)
    Xtr, X = Xtr.astype(np.float64), Xte.astype(np.float64)
    classes = np.unique(ytr)
    F = Xtr.shape[1]
    pooled = np.zeros((F, F))
    for c in classes:
        Xc = Xtr[ytr == c]
        pooled += (Xc.shape[0] - 1) * np.cov(Xc, rowvar=False).reshape(F, F)
    P = np.linalg.inv(pooled / (Xtr.shape[0] - classes.size))
    g = []
    for c in classes:
        D = X - Xtr[ytr == c].mean(0)
        g.append(np.einsum("nf,fg,ng->n", D, P, D))
    g = np.array(g)
    return g, classes[np.argmin(g, axis=0)]


INDEPENDENT = {"ml": _independent_ml, "mindist": _independent_mindist, "mahalanobis": _independent_mahalanobis}


@pytest.mark.parametrize("method", ["ml", "mindist", "mahalanobis"])
@pytest.mark.parametrize("name", list(GC.CASES))
def test_restatement_equals_independent_classifier(name, method):
    """Labels equal at every pixel whose restatement margin exceeds tau = 4 x the largest |g_restatement - g_independent| of
    the case (both evaluations' rounding); at most 0.1 % of the pixels may lie below tau."""
    clf, ref = fitted(name, method)
    g_ind, lab_ind = INDEPENDENT[method](name)
    assert np.all(np.isfinite(ref["g"]))
    tau = 4.0 * float(np.max(np.abs(ref["g"] - g_ind)))
    margin = ref["second"] - ref["best"]
    sure = margin > tau
    excluded = int((~sure).sum())
    print(f"{name} {method}: tau = {tau:.3e}, smallest margin = {margin.min():.3e}, excluded {excluded} of {sure.size}")
    assert tau < 1e-6 * max(1.0, float(np.max(np.abs(g_ind)))), "the two evaluations disagree beyond rounding"
    assert excluded <= sure.size // 1000
    lab_ref = clf._to_classes(ref["labels"])
    assert np.array_equal(lab_ref[sure], lab_ind[sure])
    assert np.all(ref["labels"] != 0)   # no threshold: every pixel is classified


def test_fma_wrapper_equals_exact_fma():
    from kmeans_model_ref import fma_exact
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(200), rng.standard_normal(200)
    c = -(a * b) * (1.0 + rng.integers(-3, 4, 200) * 2.0 ** -52)   # heavy cancellation: the fma's single rounding shows
    got = R.fma(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert np.any(got != a * b + c)
    # non-finite operands take the IEEE value
    assert np.isnan(R.fma(0.0, np.array([np.inf]), 1.0)[0]) and R.fma(2.0, np.array([np.inf]), 1.0)[0] == np.inf


# ---- exact rules, through from_params -----------------------------------------------------------------------------------
def _model(F, k, seed, **kw):
    mean, wh, off, cv = GC.random_model(F, k, seed)
    return GaussianClassifier.from_params(mean, wh, off, cv, **kw)


def _ref(clf, X):
    p = clf.params()
    return R.classify(X, p["mean"], p["whiten"], p["offset"], p["class_values"], p["max_dist2"])


def test_identical_classes_go_to_the_lower_index():
    mean, wh, off, cv = GC.random_model(5, 1, 1)
    clf = GaussianClassifier.from_params(np.repeat(mean, 2, 0), np.repeat(wh, 2, 0), np.repeat(off, 2), [9, 4])
    X = np.random.default_rng(2).standard_normal((500, 5)).astype(np.float32)
    r = _ref(clf, X)
    assert np.all(r["labels"] == 9) and np.all(r["win"] == 0)
    assert np.all(r["margin"] == 0.0)


def test_infinite_g_never_wins_and_all_nonfinite_is_unclassified():
    F = 2
    mean = np.zeros((3, F))
    # at x_0 = 2^180: class 0 has z_0 = 2^511, m = 2^1022 (finite) and g = m + 1.7e308 = +inf; classes 1 and 2 have z_0 = 1,
    # m = 1 and g = 1 and 6
    W = np.stack([np.eye(F) * 2.0 ** 331, np.diag([2.0 ** -180, 1.0]), np.diag([2.0 ** -180, 1.0])])
    clf = GaussianClassifier.from_params(mean, W, [1.7e308, 0.0, 5.0], [1, 2, 3])
    X = np.zeros((4, F))
    X[:, 0] = [2.0 ** 180, 2.0 ** 180, np.inf, -np.inf]
    X[1, 1] = np.nan   # reads as 0
    r = _ref(clf, X)
    assert np.isposinf(r["g"][0, 0]) and np.isfinite(r["m"][0, 0])
    assert list(r["labels"][:2]) == [2, 2] and np.all(r["margin"][:2] == 5.0)
    assert not np.any(np.isfinite(r["g"][:, 2:]))
    assert list(r["labels"][2:]) == [0, 0] and np.all(r["win"][2:] == -1)
    assert np.all(np.isnan(r["dist2"][2:])) and np.all(np.isnan(r["margin"][2:]))
    # +inf alone among the classes: no winner either
    one = GaussianClassifier.from_params(mean[:1], W[:1], [1.7e308], [1])
    r1 = _ref(one, X[:1])
    assert r1["labels"][0] == 0 and np.isnan(r1["dist2"][0]) and np.isnan(r1["margin"][0])


def test_single_class_margin_is_infinite():
    clf = _model(3, 1, 3)
    r = _ref(clf, np.random.default_rng(4).standard_normal((50, 3)))
    assert np.all(np.isposinf(r["margin"])) and np.all(r["labels"] == clf.class_values_[0])
    assert np.all(np.isfinite(r["dist2"]))


def test_threshold_zeroes_the_label_not_dist2():
    X = np.random.default_rng(6).standard_normal((2000, 4)).astype(np.float32)
    free = _ref(_model(4, 3, 7), X)
    cut = float(np.median(free["dist2"]))
    thr = _ref(_model(4, 3, 7, max_dist2=cut), X)
    zeroed = free["m"][free["win"], np.arange(X.shape[0])] > cut
    assert 0 < zeroed.sum() < X.shape[0]
    assert np.all(thr["labels"][zeroed] == 0) and np.array_equal(thr["labels"][~zeroed], free["labels"][~zeroed])
    assert np.array_equal(thr["dist2"], free["dist2"]) and np.array_equal(thr["margin"], free["margin"])


def test_nan_pixels_behave_as_zero():
    rng = np.random.default_rng(8)
    X = rng.standard_normal((3000, 6)).astype(np.float32)
    X[rng.random(X.shape) < 0.02] = np.nan
    assert np.isnan(X).any(axis=1).mean() > 0.02
    clf = _model(6, 4, 9)
    a, b = _ref(clf, X), _ref(clf, np.nan_to_num(X, nan=0.0))
    for key in ("labels", "dist2", "margin"):
        assert np.array_equal(a[key], b[key])


# ---- model object ----------------------------------------------------------------------------------------------------
def _small_scene(seed=21, h=24, w=31, F=5, k=3):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((h, w, F))
    roi = np.zeros((h, w), np.uint8)
    pick = rng.random((h, w)) < 0.5
    roi[pick] = rng.integers(1, k + 1, pick.sum()) * 5
    feats += roi[:, :, None] * 0.1
    feats[3, 4, 1] = np.nan
    roi[3, 4] = 5
    return feats, roi


@pytest.mark.parametrize("method", ["ml", "mahalanobis", "mindist"])
def test_fit_image_equals_fit_on_prepare_training_samples(tmp_path, method):
    from modules.features.extract import prepare_training_samples
    from rsseg.tiff import write_tiff
    feats, roi = _small_scene()
    path = str(tmp_path / "labeled_roi.tif")
    write_tiff(path, roi)
    X, y = prepare_training_samples(feats, path)
    assert X.shape[0] == int((roi != 0).sum())
    a = GaussianClassifier(method).fit(X, y).params()
    b = GaussianClassifier(method).fit_image(feats, roi).params()
    assert list(a["classes"]) == [5, 10, 15]
    for key in ("classes", "class_values", "mean", "whiten", "offset", "priors"):
        assert np.array_equal(a[key], b[key]), key


def test_fit_is_the_textbook_discriminant():
    Xtr, ytr, _, _ = GC.case("f4_k3")
    clf = GaussianClassifier("ml", priors="equal").fit(Xtr, ytr)
    X = Xtr[ytr == clf.classes_[1]].astype(np.float64)
    S = np.cov(X, rowvar=False)
    W = np.zeros((4, 4))
    W[np.tril_indices(4)] = clf.whiten_[1]
    assert np.allclose(W.T @ W, np.linalg.inv(S), rtol=1e-9, atol=1e-12)
    assert np.isclose(clf.offset_[1], np.linalg.slogdet(S)[1] - 2.0 * np.log(1.0 / 3.0), rtol=1e-12)
    assert np.array_equal(clf.mean_[1], X.mean(0))
    thr = GaussianClassifier("ml", threshold=0.99).fit(Xtr, ytr)
    from scipy.stats import chi2
    assert thr.max_dist2_ == chi2.ppf(0.99, 4) and GaussianClassifier("ml").fit(Xtr, ytr).max_dist2_ == np.inf
    md = GaussianClassifier("mindist").fit(Xtr, ytr)
    assert np.array_equal(md.whiten_[0], R.pack_lower(np.eye(4)[None])[0]) and np.all(md.offset_ == 0)
    mh = GaussianClassifier("mahalanobis").fit(Xtr, ytr)
    assert np.all(mh.offset_ == 0) and np.array_equal(mh.whiten_[0], mh.whiten_[2])


def test_save_load_round_trip_is_bit_for_bit(tmp_path):
    Xtr, ytr, _, _ = GC.case("f4_k3")
    clf = GaussianClassifier("ml", threshold=0.95).fit(Xtr, ytr.astype(np.int16))
    path = clf.save(str(tmp_path / "model"))
    assert path.endswith(".npz")
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["class_values", "classes", "max_dist2", "mean", "method", "offset", "priors", "whiten"]
    a, b = clf.params(), GaussianClassifier.load(path).params()
    assert a["method"] == b["method"] and a["max_dist2"] == b["max_dist2"] and a["classes"].dtype == b["classes"].dtype == np.int16
    for key in ("classes", "class_values", "mean", "whiten", "offset", "priors"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_fit_value_errors():
    rng = np.random.default_rng(31)
    X = rng.standard_normal((60, 4))
    y = np.repeat([1, 2, 3], 20)
    with pytest.raises(ValueError, match="1..255"):
        GaussianClassifier().fit(X, np.repeat([0, 1, 2], 20))
    with pytest.raises(ValueError, match="1..255"):
        GaussianClassifier().fit(X, np.repeat([1, 2, 256], 20))
    with pytest.raises(ValueError, match="1..255"):
        GaussianClassifier("mindist").fit(X, np.repeat([1.5, 2, 3], 20))
    few = np.concatenate([np.repeat([1, 2], 28), np.repeat([7], 4)])
    with pytest.raises(ValueError, match="class 7 has 4 samples"):
        GaussianClassifier("ml").fit(X, few)
    GaussianClassifier("mindist").fit(X, few)
    Xs = X.copy()
    Xs[y == 2, 3] = Xs[y == 2, 0] * 2.0   # linearly dependent within class 2 only
    with pytest.raises(ValueError, match="class 2 is not positive definite"):
        GaussianClassifier("ml").fit(Xs, y)
    Xp = X.copy()
    Xp[:, 3] = 1.0
    with pytest.raises(ValueError, match="pooled classes is not positive definite"):
        GaussianClassifier("mahalanobis").fit(Xp, y)
    for bad in ([0.5, 0.5], [0.5, 0.6, -0.1], [0.3, 0.3, 0.3], [np.nan, 0.5, 0.5], "uniform"):
        with pytest.raises(ValueError, match="priors"):
            GaussianClassifier("ml", priors=bad).fit(X, y)
    GaussianClassifier("ml", priors=[0.2, 0.3, 0.5]).fit(X, y)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            GaussianClassifier("ml", threshold=bad)
    with pytest.raises(ValueError, match="not both"):
        GaussianClassifier("ml", threshold=0.9, max_dist2=3.0)
    with pytest.raises(ValueError, match="method"):
        GaussianClassifier("qda")
    with pytest.raises(ValueError, match="not fitted"):
        GaussianClassifier().params()
    with pytest.raises(ValueError, match="distinct integers in 1..255"):
        GaussianClassifier.from_params(np.zeros((2, 1)), np.ones((2, 1)), [0, 0], [3, 3])
    with pytest.raises(ValueError, match="distinct integers in 1..255"):
        GaussianClassifier.from_params(np.zeros((2, 1)), np.ones((2, 1)), [0, 0], [0, 3])


# ---- stage driver ----------------------------------------------------------------------------------------------------
def test_stage_argument_errors(capsys):
    from rsseg import stages as S
    ap = S.build_parser()
    for argv in (["a.tif", "o", "--classify", "kmeans", "--ml-threshold", "0.9"], ["a.tif", "o", "--classify", "random_forest", "--rule-image"],
                 ["a.tif", "o", "--rule-image"], ["a.tif", "o", "--classify", "maximum_likelihood", "--ml-threshold", "1.0"],
                 ["a.tif", "o", "--classify", "quadratic"]):
        with pytest.raises(SystemExit):
            S.parse_args(ap, argv)
    capsys.readouterr()
    for m in S.GAUSS_METHODS:
        a = S.parse_args(ap, ["a.tif", "o", "--classify", m, "--ml-threshold", "0.99", "--rule-image", "--mask-nodata", "0", "--sieve", "4",
                              "--majority", "3", "--evaluate", "roi.npy"])
        assert a.classify == m and a.ml_threshold == 0.99 and a.rule_image
    assert set(S.GAUSS_METHODS) == set(__import__("rsseg.gaussian", fromlist=["x"]).STAGE_METHODS)


def test_unknown_method_still_prints_the_old_message(capsys):
    from rsseg import stages as S
    out, _ = S._classify({"height": 4, "width": 4}, "unused", S.ClassifyRequest(method="quadratic"))
    assert out is None
    assert "错误: 不支持的分割方法 'quadratic'" in capsys.readouterr().out
