"""K30 on the host: the restatement's float32 fma against libm's fmaf, on random operands and on operands built to tie; the
restated network (tests/mlp_ref.py) against scikit-learn's MLPClassifier in labels and probabilities; the model object's class
mapping, round trips and refusals; rsseg_mlp_plan; the parser of python -m rsseg.mlp."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest

import mlp_cases as MC
import mlp_ref as R


def _libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.vectorize(lambda a, b, c: libm.fmaf(float(a), float(b), float(c)), otypes=[np.float32])


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) or bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _tie_operands(n, seed):
    """(a, b, c, sign) float32 whose exact a * b + c lies just beside the midpoint of two float32 values, so close that the
    float64 sum IS the midpoint.  c = m, an integer in [2^23, 2^24): ulp 1, midpoint m + 0.5, whose float64 ulp is 2^-29.
    a * b = 0.5 (1 + 2^-33) from a = 0.5 (1 + 2^-11), b = 1 - 2^-11 + 2^-22 ((1 + x)(1 - x + x^2) = 1 + x^3), or 0.5 (1 - 2^-46)
    from a = 0.5 (1 + 2^-23), b = 1 - 2^-23: both exact in float64 and both dropped by the float64 sum.  Rounding twice resolves
    the tie to even; rounding once goes to the side the small term points to."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1 << 23, 1 << 24, n).astype(np.float32)
    up = rng.random(n) < 0.5
    a = np.where(up, 0.5 * (1 + 2.0 ** -11), 0.5 * (1 + 2.0 ** -23)).astype(np.float32)
    b = np.where(up, 1 - 2.0 ** -11 + 2.0 ** -22, 1 - 2.0 ** -23).astype(np.float32)
    assert np.all(a.astype(np.float64) == np.where(up, 0.5 * (1 + 2.0 ** -11), 0.5 * (1 + 2.0 ** -23)))
    assert np.all(b.astype(np.float64) == np.where(up, 1 - 2.0 ** -11 + 2.0 ** -22, 1 - 2.0 ** -23))
    return a, b, c, np.where(up, 1.0, -1.0)


def test_fma32_equals_fmaf_on_random_operands():
    rng = np.random.default_rng(3001)
    n = 100000
    a = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    c = np.where(rng.random(n) < 0.5, -(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 1e-6),   # cancellation
                 rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))).astype(np.float32)
    assert _same(R.fma32(a, b, c), _libm_fmaf()(a, b, c))


def test_fma32_equals_fmaf_on_ties_and_edges():
    fmaf = _libm_fmaf()
    a, b, c, sign = _tie_operands(2000, 3002)
    got, want = R.fma32(a, b, c), fmaf(a, b, c)
    assert _same(got, want)
    # the operands do tie: the float64 sum is the midpoint exactly, and rounding it again goes wrong on about half of them
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert np.all(s == c.astype(np.float64) + 0.5)
    twice = s.astype(np.float32)
    assert int((twice.view(np.uint32) != want.view(np.uint32)).sum()) > 500
    assert np.all(want == np.where(sign > 0, c + np.float32(1), c))
    # subnormal results, signed zeros, overflow, infinities and NaN
    tiny = np.float32(2.0 ** -149)
    ea = np.array([tiny, 3 * tiny, 2.0 ** -75, 2.0 ** -75, 0.0, -0.0, 3e38, np.inf, np.inf, np.nan, 1.5, 2.0 ** -100], np.float32)
    eb = np.array([0.5, 0.5, 2.0 ** -75, 1.5 * 2.0 ** -74, -1.0, 0.0, 3.0, 0.0, 1.0, 1.0, 2.0 ** -126, 2.0 ** -49], np.float32)
    ec = np.array([0.0, tiny, tiny, -tiny, 0.0, -0.0, -3e38, 1.0, -np.inf, 1.0, 2.0 ** -149, 2.0 ** -149], np.float32)
    assert _same(R.fma32(ea, eb, ec), fmaf(ea, eb, ec))


def _clf(k, F, hidden, activation):
    from rsseg.mlp import NeuralNetClassifier
    mlp, offset, scale, Xte = MC.fitted(k, F, hidden, activation)
    return mlp, NeuralNetClassifier.from_sklearn(mlp, offset, scale), (Xte - offset) * scale, Xte


@pytest.mark.parametrize("k,F,hidden,activation", MC.FITTED)
def test_restatement_equals_scikit_learn(k, F, hidden, activation):
    """Labels equal MLPClassifier.predict wherever the restated margin exceeds 1e-4 max(1, |o_win|); at most 0.1 % of the
    pixels are excluded by that.  The probabilities' largest difference is printed: tests/test_gpu_mlp.py takes its bound from
    the largest over the six cases."""
    mlp, clf, Xs, Xte = _clf(k, F, hidden, activation)
    assert all(c.dtype == np.float32 for c in mlp.coefs_)      # a float32 model already
    ref = R.classify(Xte, MC.model_of(clf))
    o_win = ref["o"][np.arange(Xte.shape[0]), ref["win"]]
    sure = ref["margin"] > 1e-4 * np.maximum(1.0, np.abs(o_win))
    labels = clf._to_classes(ref["labels"])
    differ = int((labels[sure] != mlp.predict(Xs)[sure]).sum())
    perr = float(np.abs(ref["proba"].T.astype(np.float64) - mlp.predict_proba(Xs)).max())
    print(f"k={k} F={F} hidden={hidden} {activation}: {int((~sure).sum())} of {sure.size} pixels excluded, {differ} labels differ, "
          f"worst probability difference {perr:.3g}")
    assert int((~sure).sum()) <= 0.001 * sure.size
    assert differ == 0
    assert perr <= PROBA_RESTATEMENT
    assert not ref["bad"].any() and set(np.unique(labels)) <= set(mlp.classes_.tolist())
    assert np.allclose(ref["proba"].sum(axis=0), 1.0, atol=1e-6) and np.array_equal(ref["conf"], ref["proba"][ref["win"], np.arange(sure.size)])


# the largest |restated probability - MLPClassifier.predict_proba| measured over the six fitted cases on the host (float32
# matrix products summed in BLAS order against the fma chain, then a float32 softmax against the float64 one): 1.19e-07,
# 1.19e-07, 4.77e-07, 7.15e-07, 8.05e-07 and 1.19e-07 in the order of mlp_cases.FITTED.  Twice the largest is allowed, for
# other BLAS builds; tests/test_gpu_mlp.py holds the GPU to the same bound.
PROBA_MEASURED = 8.05e-7
PROBA_RESTATEMENT = 2 * PROBA_MEASURED


def _three_class_samples():
    Xtr, ytr, _, _ = MC.blobs(3, 8)
    return Xtr, np.array([3, 7, 200])[(ytr - 3) // 4]


def test_fit_standardises_in_float32_and_maps_classes():
    from sklearn.neural_network import MLPClassifier
    from rsseg.mlp import NeuralNetClassifier
    X, y = _three_class_samples()
    X = np.concatenate([X, np.full((X.shape[0], 1), 4.5, np.float32)], axis=1)   # a constant column: scale 1
    clf = NeuralNetClassifier(hidden_layer_sizes=(16,), max_iter=60, random_state=3).fit(X, y)
    offset, scale = MC.standardise(X)
    assert clf.offset_.dtype == clf.scale_.dtype == np.float32 and np.array_equal(clf.offset_, offset) and np.array_equal(clf.scale_, scale)
    assert clf.scale_[-1] == 1.0
    assert clf.classes_.tolist() == [3, 7, 200] and clf.class_values_.tolist() == [1, 2, 3] and clf.class_values_.dtype == np.uint8
    assert clf._to_classes(np.array([0, 1, 2, 3, 3, 0], np.uint8)).tolist() == [0, 3, 7, 200, 200, 0]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mlp = MLPClassifier(hidden_layer_sizes=(16,), max_iter=60, random_state=3).fit((X - offset) * scale, y)
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(clf.coefs_ + clf.intercepts_, mlp.coefs_ + mlp.intercepts_))
    assert clf.widths_.tolist() == [9, 16, 3] and clf.hidden_layer_sizes == (16,)
    ref = R.classify(X, MC.model_of(clf))
    assert float((clf._to_classes(ref["labels"]) == y).mean()) > 0.6      # three overlapping classes: chance is 1 / 3


@pytest.mark.parametrize("k", [2, 3])
def test_from_sklearn(k):
    """Two classes: one output unit whose logit stands against +0; a float64 model is rounded to float32."""
    import warnings
    from sklearn.neural_network import MLPClassifier
    from rsseg.mlp import NeuralNetClassifier
    Xtr, ytr, Xte, _ = MC.blobs(k, 3 if k == 2 else 8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mlp = MLPClassifier(hidden_layer_sizes=(8, 4), activation="tanh", max_iter=80, random_state=1).fit(Xtr.astype(np.float64), ytr)
    assert mlp.coefs_[0].dtype == np.float64
    clf = NeuralNetClassifier.from_sklearn(mlp)
    assert clf.widths_.tolist() == [Xtr.shape[1], 8, 4, 1 if k == 2 else k] and clf.activation == "tanh"
    assert all(c.dtype == np.float32 for c in clf.coefs_ + clf.intercepts_) and np.array_equal(clf.coefs_[1], mlp.coefs_[1].astype(np.float32))
    assert np.all(clf.offset_ == 0) and np.all(clf.scale_ == 1) and clf.classes_.tolist() == mlp.classes_.tolist()
    ref = R.classify(Xte, MC.model_of(clf))
    assert ref["proba"].shape == (k, Xte.shape[0])
    want = mlp.predict(Xte.astype(np.float64))
    sure = ref["margin"] > 1e-4
    assert float(sure.mean()) > 0.99 and np.array_equal(clf._to_classes(ref["labels"])[sure], want[sure])
    assert float(np.abs(ref["proba"].T - mlp.predict_proba(Xte.astype(np.float64))).max()) < 1e-4
    if k == 2:
        assert np.array_equal(ref["margin"], np.abs(ref["sums"][-1][:, 0]))


def test_round_trips_are_bit_equal(tmp_path):
    from rsseg.mlp import NeuralNetClassifier
    _, clf, _, _ = _clf(3, 8, (32,), "logistic")
    p = clf.params()
    path = clf.save(str(tmp_path / "model"))
    assert path.endswith("model.npz")
    with np.load(path, allow_pickle=False) as z:   # arrays only
        assert sorted(z.files) == sorted(p.keys())
    for other in (NeuralNetClassifier.load(path), NeuralNetClassifier.from_params(**p)):
        q = other.params()
        assert q.keys() == p.keys() and other.hidden_layer_sizes == (32,) and other.activation == "logistic"
        for key in p:
            a, b = np.asarray(p[key]), np.asarray(q[key])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    assert p["weights"].dtype == p["biases"].dtype == p["offset"].dtype == np.float32 and p["class_values"].dtype == np.uint8
    assert p["widths"].tolist() == [8, 32, 3] and p["weights"].size == 8 * 32 + 32 * 3 and p["biases"].size == 35


def test_refusals():
    import warnings
    from sklearn.neural_network import MLPClassifier
    from rsseg.mlp import NeuralNetClassifier
    X, y = _three_class_samples()
    for kw, word in ((dict(activation="softplus"), "softplus"), (dict(hidden_layer_sizes=()), "hidden layers"), (dict(hidden_layer_sizes=(8, 8, 8, 8)), "hidden layers"),
                     (dict(hidden_layer_sizes=(129,)), "width"), (dict(hidden_layer_sizes=(0,)), "width"), (dict(hidden_layer_sizes=(2.5,)), "width"),
                     (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(max_iter=0), "max_iter"), (dict(solver="newton"), "solver")):
        with pytest.raises(ValueError, match=word):
            NeuralNetClassifier(**kw)
    with pytest.raises(ValueError, match="not fitted"):
        NeuralNetClassifier.from_sklearn(MLPClassifier())
    with pytest.raises(ValueError, match="not fitted"):
        NeuralNetClassifier().params()
    rng = np.random.default_rng(5)
    X33, y33 = rng.standard_normal((330, 3)).astype(np.float32), np.repeat(np.arange(33), 10)
    with pytest.raises(ValueError, match="more than 32 classes"):
        NeuralNetClassifier(max_iter=2).fit(X33, y33)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        wide = MLPClassifier(hidden_layer_sizes=(130,), max_iter=2).fit(X, y)
        multilabel = MLPClassifier(hidden_layer_sizes=(4,), max_iter=2).fit(X, np.stack([y == 3, y == 7], axis=1).astype(int))
    with pytest.raises(ValueError, match="width"):
        NeuralNetClassifier.from_sklearn(wide)
    with pytest.raises(ValueError, match="multilabel"):
        NeuralNetClassifier.from_sklearn(multilabel)
    with pytest.raises(ValueError, match="at least 2"):
        NeuralNetClassifier().fit(X, np.ones(y.size, np.int64))
    with pytest.raises(ValueError, match="integers"):
        NeuralNetClassifier().fit(X, y + 0.5)
    with pytest.raises(ValueError, match="NaN or infinite"):
        NeuralNetClassifier().fit(np.where(np.arange(X.size).reshape(X.shape) == 3, np.nan, X), y)
    with pytest.raises(ValueError, match="n samples"):
        NeuralNetClassifier().fit(X[:-1], y)
    with pytest.raises(ValueError, match="at most 64"):
        NeuralNetClassifier().fit(rng.standard_normal((30, 65)), np.repeat([1, 2], 15))
    p = NeuralNetClassifier(hidden_layer_sizes=(6,), max_iter=5).fit(X, y).params()
    at = lambda a, i, v: np.where(np.arange(a.size) == i, v, a).astype(a.dtype)   # noqa: E731
    for kw, word in ((dict(class_values=[1, 1, 2]), "class_values"), (dict(class_values=[0, 1, 2]), "class_values"), (dict(class_values=[1, 2, 256]), "class_values"),
                     (dict(weights=p["weights"][:-1]), "do not describe"), (dict(biases=p["biases"][:-1]), "do not describe"),
                     (dict(widths=[8, 6]), "widths"), (dict(widths=[8, 6, 4]), "do not describe"), (dict(widths=[8, 0, 3]), "widths"),
                     (dict(offset=p["offset"][:-1]), "one model"), (dict(scale=np.zeros_like(p["scale"])), "scale of 0"),
                     (dict(weights=at(p["weights"], 1, np.inf)), "not finite"), (dict(biases=at(p["biases"], 0, np.nan)), "not finite"),
                     (dict(weights=p["weights"].astype(np.float64) * 1e39), "not finite"), (dict(activation="softplus"), "softplus"),
                     (dict(classes=[1, 2]), "one model")):
        with pytest.raises(ValueError, match=word):
            NeuralNetClassifier.from_params(**{**p, **kw})
    clf = NeuralNetClassifier.from_params(**p)
    with pytest.raises(ValueError, match="features"):
        clf.predict(np.zeros((4, 7)))
    with pytest.raises(ValueError, match="features"):
        clf.predict_proba(np.zeros((4, 7)))
    with pytest.raises(ValueError, match="planes"):
        clf.predict_image(np.zeros((4, 4, 7)))


def test_plan():
    """The limits of include/rsseg.h: the two shapes the contract names fit; the tile shrinks as the model grows."""
    from rsseg import _lib
    lib = _lib.load()

    def plan(widths, k):
        w = np.array(widths, np.int32)
        fits, tile = ctypes.c_int(-1), ctypes.c_int(-1)
        lib.rsseg_mlp_plan(int(w[0]), w.size - 1, w.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), k, ctypes.byref(fits), ctypes.byref(tile))
        return fits.value, tile.value

    assert plan([19, 100, 8], 8) == (1, 256)
    big, deep = plan([64, 128, 128, 32], 32), plan([19, 64, 64, 64, 16], 16)
    assert big[0] == 1 and deep[0] == 1 and 16 <= big[1] <= deep[1] <= 256 and big[1] % 16 == 0 and deep[1] % 16 == 0
    assert plan([3, 8, 1], 2) == (1, 256)
    for widths, k in (([64, 128, 128, 128, 32], 32), ([65, 8, 3], 3), ([3, 129, 3], 3), ([3, 8, 33], 33), ([3, 8, 8, 8, 8, 3], 3), ([3, 3], 3),
                      ([3, 8, 2], 2), ([3, 8, 4], 3), ([3, 0, 3], 3)):
        assert plan(widths, k) == (0, 0), widths
    lib.rsseg_mlp_plan(3, 2, None, 3, None, None)      # null pointers are taken


def test_parser_of_the_command(tmp_path, capsys):
    from rsseg import mlp, stages
    ap = mlp.build_parser()
    a = ap.parse_args(["out", "--roi", "roi.tif"])
    assert (a.outdir, a.roi, a.hidden, a.activation, a.alpha, a.max_iter, a.model, a.rule_image, a.mask_nodata) == \
        ("out", "roi.tif", (100,), "relu", 1e-4, 500, None, False, None)
    a = ap.parse_args(["out", "--model", "m.npz", "--hidden", "100,50", "--activation", "tanh", "--alpha", "0.01", "--max-iter", "50", "--rule-image",
                       "--mask-nodata"])
    assert (a.hidden, a.activation, a.alpha, a.max_iter, a.model, a.rule_image, a.mask_nodata) == \
        ((100, 50), "tanh", 0.01, 50, "m.npz", True, stages.MASK_NODATA_FROM_TAG)
    assert ap.parse_args(["out", "--roi", "r", "--mask-nodata", "-9999"]).mask_nodata == -9999.0
    for argv in (["out", "--roi", "r", "--activation", "softplus"], ["out", "--roi", "r", "--hidden", "wide"], ["--roi", "r"],
                 ["out"], ["out", "--roi", "r", "--model", "m"], [str(tmp_path), "--roi", "r"]):
        with pytest.raises(SystemExit) as e:
            mlp.main(argv)
        assert e.value.code == 2
    assert "feature_outputs" in capsys.readouterr().err
    import inspect
    sig = inspect.signature(stages.run_mlp_stage).parameters
    assert {n: p.default for n, p in sig.items() if p.default is not inspect.Parameter.empty} == dict(
        labeled_roi_file="labeled_roi.tif", hidden_layer_sizes=(100,), activation="relu", alpha=1e-4, max_iter=500, random_state=42, model_path=None,
        rule_image=False, valid_mask=None, ctx=None)
    assert os.path.basename(mlp.__file__) == "mlp.py"
