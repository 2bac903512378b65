"""K28 on the host: svm_exp against np.exp; the restatement (tests/svm_ref.py) against scikit-learn's SVC in decisions and
labels; the folded linear weights; the model object's class mapping, class_weight, round trips and refusals; the parser of
python -m rsseg.svm."""
import os

import numpy as np
import pytest

import svm_cases as SC
import svm_ref as R

KERNELS = ("rbf", "poly", "linear")


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(want)


def test_svm_exp_is_within_two_ulp_of_numpy():
    """1 ulp was measured (8 % of the arguments); the second is margin for another libm."""
    rng = np.random.default_rng(2801)
    t = np.concatenate([-708.0 * rng.random(200000), -np.exp(rng.uniform(np.log(1e-12), np.log(708.0), 200000)),
                        [0.0, -0.0, -708.0, -1e-12, -1.0, -0.5 * np.log(2.0), -np.log(2.0), -707.999]])
    got = R.svm_exp(t)
    worst = float(_ulps(got, np.exp(t)).max())
    print(f"svm_exp: worst {worst} ulp over {t.size} arguments, {float((got != np.exp(t)).mean()):.3f} of them differ")
    assert worst <= 2.0
    assert R.svm_exp(0.0) == 1.0 and R.svm_exp(-0.0) == 1.0
    assert R.svm_exp(-708.0) > 0.0 and np.isfinite(R.svm_exp(-708.0))
    below = R.svm_exp(np.array([np.nextafter(-708.0, -np.inf), -1e4, -1e308, -np.inf]))
    assert np.all(below == 0.0) and not np.any(np.signbit(below))


def test_svm_exp_is_monotone():
    rng = np.random.default_rng(2802)
    t = np.sort(np.concatenate([-708.0 * rng.random(100000), -np.exp(rng.uniform(np.log(1e-12), np.log(708.0), 100000)),
                                -np.log(2.0) * (np.arange(0, 1021) + 0.5), [0.0, -708.0]]))   # the last: where n steps
    e = R.svm_exp(t)
    assert np.all(np.diff(e) >= 0.0)
    assert e[0] > 0.0 and e[-1] == 1.0


def _fitted_model(k, F, kernel):
    from rsseg.svm import SVMClassifier
    svc, offset, scale, Xte = SC.fitted(k, F, kernel)
    clf = SVMClassifier.from_sklearn(svc, offset, scale)
    return svc, clf, (Xte.astype(np.float64) - offset) * scale, Xte


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,F", SC.FITTED)
def test_restatement_equals_scikit_learn(k, F, kernel):
    """decisions within 1e-10 max(1, |d|) of SVC.decision_function (ovo; its sign flipped for two classes); labels equal
    SVC.predict wherever every |d_p| exceeds 1e-9 max(1, |d_p|), and at most 0.1 % of the pixels are excluded by that."""
    svc, clf, Xs, Xte = _fitted_model(k, F, kernel)
    ref = R.classify(Xte, SC.model_of(clf))
    want = svc.decision_function(Xs)
    want = -want.reshape(-1, 1) if k == 2 else want
    d = ref["d"].T
    err = np.abs(d - want) / np.maximum(1.0, np.abs(want))
    sure = np.all(np.abs(d) > 1e-9 * np.maximum(1.0, np.abs(d)), axis=1)
    labels = clf._to_classes(ref["labels"])
    differ = int((labels[sure] != svc.predict(Xs)[sure]).sum())
    print(f"{kernel} k={k} F={F}: S={clf.support_vectors_.shape[0]}, worst decision error {float(err.max()):.3g}, "
          f"{int((~sure).sum())} of {sure.size} pixels excluded, {differ} labels differ")
    assert float(err.max()) <= 1e-10
    assert int((~sure).sum()) <= 0.001 * sure.size
    assert differ == 0
    assert not ref["bad"].any() and set(np.unique(labels)) <= set(svc.classes_.tolist())


@pytest.mark.parametrize("k,F", SC.FITTED)
def test_folded_linear_weights(k, F):
    svc, clf, _, _ = _fitted_model(k, F, "linear")
    w = clf.w_
    assert w.shape == (k * (k - 1) // 2, F)
    assert np.array_equal(w, R.fold_linear(clf.support_vectors_, clf.n_support_, clf.dual_coef_))   # the library's fold, bit for bit
    want = -svc.coef_ if k == 2 else svc.coef_
    assert float((np.abs(w - want) / np.maximum(1.0, np.abs(want))).max()) <= 1e-10
    assert SC.fitted(k, F, "rbf")[0] is not None and _fitted_model(k, F, "rbf")[1].w_ is None


def _three_class_samples():
    Xtr, ytr, _, _ = SC.blobs(3, 8)
    return Xtr, np.array([3, 7, 200])[(ytr - 3) // 4]


def test_class_mapping():
    from rsseg.svm import SVMClassifier
    X, y = _three_class_samples()
    clf = SVMClassifier().fit(X, y)
    assert clf.classes_.tolist() == [3, 7, 200] and clf.class_values_.tolist() == [1, 2, 3] and clf.class_values_.dtype == np.uint8
    assert clf._to_classes(np.array([0, 1, 2, 3, 3, 0], np.uint8)).tolist() == [0, 3, 7, 200, 200, 0]
    assert clf.n_support_.shape == (3,) and int(clf.n_support_.sum()) == clf.support_vectors_.shape[0]
    ref = R.classify(X, SC.model_of(clf))
    assert float((clf._to_classes(ref["labels"]) == y).mean()) > 0.8
    # negative and large labels pass through the same table
    far = SVMClassifier("linear").fit(X, np.array([-5, 0, 100000])[(y == 7) + 2 * (y == 200)])
    assert far.classes_.tolist() == [-5, 0, 100000] and far._to_classes(np.array([1, 2, 3], np.uint8)).tolist() == [-5, 0, 100000]


def test_fit_standardises_and_class_weight():
    from sklearn.svm import SVC
    from rsseg.svm import SVMClassifier
    X, y = _three_class_samples()
    X = np.concatenate([X.astype(np.float64), np.full((X.shape[0], 1), 4.5)], axis=1)   # a constant column: scale 1
    cw = {3: 1.0, 7: 5.0, 200: 0.5}
    clf = SVMClassifier("rbf", C=2.0, class_weight=cw).fit(X, y)
    assert np.array_equal(clf.offset_, X.mean(axis=0)) and clf.scale_[-1] == 1.0 and np.array_equal(clf.scale_[:-1], 1.0 / X.std(axis=0)[:-1])
    Xs = (X - clf.offset_) * clf.scale_
    svc = SVC(kernel="rbf", C=2.0, class_weight=cw).fit(Xs, y)
    assert np.array_equal(clf.support_vectors_, svc.support_vectors_) and np.array_equal(clf.dual_coef_, svc._dual_coef_)
    assert np.array_equal(clf.intercept_, svc._intercept_) and np.array_equal(clf.n_support_, svc._n_support) and clf.gamma_ == svc._gamma
    plain = SVMClassifier("rbf", C=2.0).fit(X, y)
    assert not np.array_equal(plain.n_support_, clf.n_support_) or not np.array_equal(plain.dual_coef_, clf.dual_coef_)
    assert np.abs(clf.dual_coef_).max() <= 2.0 * 5.0 + 1e-12 and np.abs(plain.dual_coef_).max() <= 2.0 + 1e-12


@pytest.mark.parametrize("kernel", KERNELS)
def test_round_trips_are_bit_equal(kernel, tmp_path):
    from rsseg.svm import SVMClassifier
    X, y = _three_class_samples()
    clf = SVMClassifier(kernel, gamma=0.05, degree=2, coef0=0.5).fit(X, y)
    p = clf.params()
    path = clf.save(str(tmp_path / "model"))
    assert path.endswith("model.npz")
    with np.load(path, allow_pickle=False) as z:   # arrays and scalars only
        assert sorted(z.files) == sorted(p.keys())
    for other in (SVMClassifier.load(path), SVMClassifier.from_params(**p)):
        q = other.params()
        assert q.keys() == p.keys()
        for key in p:
            a, b = np.asarray(p[key]), np.asarray(q[key])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    assert (p["w"].shape == (3, 8)) == (kernel == "linear") and p["class_values"].dtype == np.uint8


def test_refusals():
    from sklearn.svm import SVC
    from rsseg.svm import SVMClassifier
    X, y = _three_class_samples()
    X = X.astype(np.float64)
    for kw, word in ((dict(kernel="sigmoid"), "sigmoid"), (dict(kernel="precomputed"), "precomputed"), (dict(kernel=lambda a, b: a @ b.T), "callable"),
                     (dict(gamma="big"), "gamma"), (dict(gamma=0.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(C=0.0), "C="),
                     (dict(degree=9), "degree"), (dict(degree=0), "degree"), (dict(degree=2.5), "degree"), (dict(coef0=float("inf")), "coef0")):
        with pytest.raises(ValueError, match=word):
            SVMClassifier(**kw)
    for kernel, word in (("sigmoid", "sigmoid"), ("precomputed", "precomputed"), (lambda a, b: a @ b.T, "callable")):
        Xf = X @ X.T if kernel == "precomputed" else X
        with pytest.raises(ValueError, match=word):
            SVMClassifier.from_sklearn(SVC(kernel=kernel).fit(Xf, y))
    with pytest.raises(ValueError, match="not fitted"):
        SVMClassifier.from_sklearn(SVC())
    with pytest.raises(ValueError, match="degree"):
        SVMClassifier.from_sklearn(SVC(kernel="poly", degree=9).fit(X, y))
    rng = np.random.default_rng(5)
    X17, y17 = rng.standard_normal((170, 3)), np.repeat(np.arange(17), 10)
    with pytest.raises(ValueError, match="more than 16 classes"):
        SVMClassifier.from_sklearn(SVC(kernel="linear").fit(X17, y17))
    with pytest.raises(ValueError, match="more than 16 classes"):
        SVMClassifier("linear").fit(X17, y17)
    with pytest.raises(ValueError, match="at least 2"):
        SVMClassifier().fit(X, np.ones(y.size, np.int64))
    with pytest.raises(ValueError, match="integers"):
        SVMClassifier().fit(X, y + 0.5)
    with pytest.raises(ValueError, match="NaN or infinite"):
        SVMClassifier().fit(np.where(np.arange(X.size).reshape(X.shape) == 3, np.nan, X), y)
    with pytest.raises(ValueError, match="n samples"):
        SVMClassifier().fit(X[:-1], y)
    with pytest.raises(ValueError, match="at most 64"):
        SVMClassifier().fit(rng.standard_normal((30, 65)), np.repeat([1, 2], 15))
    with pytest.raises(ValueError, match="not fitted"):
        SVMClassifier().params()
    p = SVMClassifier("rbf").fit(X, y).params()
    for kw, word in ((dict(class_values=[1, 1, 2]), "class_values"), (dict(class_values=[0, 1, 2]), "class_values"), (dict(class_values=[1, 2, 256]), "class_values"),
                     (dict(n_support=p["n_support"] + 1), "one model"), (dict(n_support=np.array([0, 1, p["n_support"].sum() - 1])), "one model"),
                     (dict(dual_coef=p["dual_coef"][:1]), "one model"), (dict(intercept=p["intercept"][:2]), "one model"),
                     (dict(offset=p["offset"][:-1]), "one model"), (dict(scale=np.zeros_like(p["scale"])), "scale of 0"),
                     (dict(support_vectors=np.where(np.arange(p["support_vectors"].size).reshape(p["support_vectors"].shape) == 1, np.inf, p["support_vectors"])),
                      "not finite"), (dict(gamma=-1.0), "gamma"), (dict(kernel="sigmoid"), "sigmoid")):
        with pytest.raises(ValueError, match=word):
            SVMClassifier.from_params(**{**p, **kw})
    clf = SVMClassifier.from_params(**p)
    with pytest.raises(ValueError, match="features"):
        clf.predict(np.zeros((4, 7)))
    with pytest.raises(ValueError, match="planes"):
        clf.predict_image(np.zeros((4, 4, 7)))


def test_parser_of_the_command(tmp_path, capsys):
    from rsseg import stages, svm
    ap = svm.build_parser()
    a = ap.parse_args(["out", "--roi", "roi.tif"])
    assert (a.outdir, a.roi, a.kernel, a.C, a.gamma, a.degree, a.coef0, a.model, a.rule_image, a.mask_nodata) == \
        ("out", "roi.tif", "rbf", 1.0, "scale", 3, 0.0, None, False, None)
    a = ap.parse_args(["out", "--model", "m.npz", "--kernel", "poly", "--C", "10", "--gamma", "0.25", "--degree", "2", "--coef0", "1.5", "--rule-image",
                       "--mask-nodata"])
    assert (a.kernel, a.C, a.gamma, a.degree, a.coef0, a.model, a.rule_image, a.mask_nodata) == \
        ("poly", 10.0, 0.25, 2, 1.5, "m.npz", True, stages.MASK_NODATA_FROM_TAG)
    assert ap.parse_args(["out", "--roi", "r", "--gamma", "auto"]).gamma == "auto"
    assert ap.parse_args(["out", "--roi", "r", "--mask-nodata", "-9999"]).mask_nodata == -9999.0
    for argv in (["out", "--roi", "r", "--kernel", "sigmoid"], ["out", "--roi", "r", "--gamma", "wide"], ["--roi", "r"],
                 ["out"], ["out", "--roi", "r", "--model", "m"], [str(tmp_path), "--roi", "r"]):
        with pytest.raises(SystemExit) as e:
            svm.main(argv)
        assert e.value.code == 2
    assert "feature_outputs" in capsys.readouterr().err
    # the stage function is rsseg.stages', with the issue's defaults
    import inspect
    sig = inspect.signature(stages.run_svm_stage).parameters
    assert {n: p.default for n, p in sig.items() if p.default is not inspect.Parameter.empty} == dict(
        labeled_roi_file="labeled_roi.tif", kernel="rbf", C=1.0, gamma="scale", degree=3, coef0=0.0, model_path=None, rule_image=False,
        valid_mask=None, ctx=None)
    assert os.path.basename(svm.__file__) == "svm.py"
