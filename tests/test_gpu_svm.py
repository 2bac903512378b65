"""K28 on the GPU: rsseg_svm_classify equals the restatement (tests/svm_ref.py) bit for bit in labels and margin over the
widths, class counts (registers up to 8 classes, LDS beyond), kernels, plane types, alignments, pixel counts, the exp range,
the support-vector seam and overflowed decisions; the model object, the stage and the command; the error codes."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import svm_cases as SC
import svm_ref as R

pytestmark = pytest.mark.gpu

SV_CHUNK = 2      # SV_UNROLL of csrc/k28_svm.hip: the support vectors of one class the kernel evaluates together
SHAPES = [(1, 2), (3, 2), (8, 3), (9, 3), (19, 8), (19, 9), (32, 4), (33, 4), (64, 2), (19, 16)]
KERNELS = [("rbf", 3), ("poly", 2), ("poly", 3), ("linear", 3)]
N_SHAPE = 1025    # more than one workgroup of every form (512, 256 and 64 pixels), an odd last pixel


def _torch():
    import torch
    return torch


def _pixels(n, F, seed, spread=1.5):
    """(X32, X64): n pixels whose float64 form holds values no float32 has; a few NaN and +-inf entries."""
    rng = np.random.default_rng(seed)
    X64 = spread * rng.standard_normal((n, F))
    if n >= 64:
        X64[rng.random((n, F)) < 0.01] = np.nan
        X64[5, F // 2] = np.inf
        X64[11, 0] = -np.inf
    return X64.astype(np.float32), X64


def _both(model, X32, X64):
    """The restatement of both plane types in one pass: {dtype: dict(labels, margin, d, K, bad)}."""
    n = X32.shape[0]
    ref = R.classify(np.concatenate([X32.astype(np.float64), X64]), model)
    cut = lambda a, s: None if a is None else a[..., s]   # noqa: E731
    return {dt: {key: cut(ref[key], s) for key in ("labels", "margin", "d", "K", "bad")}
            for dt, s in (("float32", slice(0, n)), ("float64", slice(n, 2 * n)))}


@functools.lru_cache(maxsize=None)
def shape_case(F, k, kernel, degree, n=N_SHAPE, S=None):
    S = (64 if k == 16 else 41) if S is None else S
    model = SC.random_model(F, k, S, kernel, 1000 * F + 10 * k + degree, degree=degree)
    X32, X64 = _pixels(n, F, 7 * F + k)
    return dict(model=model, X={"float32": X32, "float64": X64}, ref=_both(model, X32, X64))


def _planes(ctx, X, shift=0):
    """Flat device planes of the columns of X; shift: every plane starts `shift` elements off its allocation (which is
    256-byte aligned), so one element off 16-byte alignment for shift = 1."""
    torch = _torch()
    out = []
    for f in range(X.shape[1]):
        t = torch.empty(X.shape[0] + shift, dtype=torch.float32 if X.dtype == np.float32 else torch.float64, device=ctx.device)
        t[shift:] = torch.from_numpy(np.ascontiguousarray(X[:, f])).to(ctx.device)
        out.append(t[shift:])
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(ctx, c, dt, shift=0, want_margin=True):
    ref = c["ref"][dt]
    lab, mg = ctx.svm_classify(_planes(ctx, c["X"][dt], shift), want_margin=want_margin, **SC.model_args(c["model"]))
    assert np.array_equal(lab.cpu().numpy(), ref["labels"])
    assert (mg is None) == (not want_margin)
    if want_margin:
        assert np.array_equal(_bits(mg.cpu().numpy()), _bits(ref["margin"]))
    return ref


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("kernel,degree", KERNELS)
@pytest.mark.parametrize("F,k", SHAPES)
def test_kernel_equals_the_restatement(ctx, F, k, kernel, degree, dt):
    c = shape_case(F, k, kernel, degree)
    ref = _check(ctx, c, dt)
    _check(ctx, c, dt, want_margin=False)
    _check(ctx, c, dt, shift=1)      # planes one element off 16-byte alignment
    # the case is worth its name: the refused pixels, the single-vector class and the zeros took part
    bad = ref["bad"]
    assert int(bad.sum()) == 2 and np.all(ref["labels"][bad] == 0) and np.all(np.isnan(ref["margin"][bad]))
    assert np.all(ref["labels"][~bad] != 0) and np.all(np.isfinite(ref["margin"][~bad]))
    m = c["model"]
    assert int(m["n_support"].min()) == 1 and np.unique(m["n_support"]).size > 1 and bool((m["coef"] == 0).any())
    assert bool((m["coef"] > 0).any()) and bool((m["coef"] < 0).any()) and not np.array_equal(np.sort(m["class_values"]), np.arange(1, k + 1))


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("kernel,degree", [("rbf", 3), ("poly", 3), ("linear", 3)])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023])
def test_pixel_counts(ctx, n, kernel, degree, dt):
    c = shape_case(19, 8, kernel, degree, n)
    _check(ctx, c, dt)
    _check(ctx, c, dt, shift=1, want_margin=False)


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_outputs_at_any_element_alignment(ctx, dt):
    """Output planes that start one element off their vector alignment: nothing outside [0, n) of either is written."""
    torch = _torch()
    n = 1023
    c = shape_case(9, 3, "rbf", 3, n)
    m, ref = c["model"], c["ref"][dt]
    lab = torch.full((n + 9,), 77, dtype=torch.uint8, device=ctx.device)
    mg = torch.full((n + 9,), -5.0, dtype=torch.float32, device=ctx.device)
    assert _raw(ctx, dict(planes=_planes(ctx, c["X"][dt]), F=9, n=n, labels=lab[1:], margin=mg[3:], **_model_kw(m))) == 0
    ctx.sync()
    lab, mg = lab.cpu().numpy(), mg.cpu().numpy()
    assert np.array_equal(lab[1:n + 1], ref["labels"]) and lab[0] == 77 and np.all(lab[n + 1:] == 77)
    assert np.array_equal(_bits(mg[3:n + 3]), _bits(ref["margin"])) and np.all(mg[:3] == -5.0) and np.all(mg[n + 3:] == -5.0)


def test_the_exp_range(ctx):
    """RBF whose gamma * q runs from 0 (a pixel on a support vector: K = 1) to beyond 708 (K = +0)."""
    F, k, S, n = 5, 3, 12, 513
    m = SC.random_model(F, k, S, "rbf", 31)
    m.update(offset=np.zeros(F), scale=np.ones(F), gamma=1.0)
    rng = np.random.default_rng(32)
    X = np.empty((n, F))
    step = np.geomspace(1e-6, 60.0, n - S)      # distance from a support vector
    for i in range(n - S):
        u = rng.standard_normal(F)
        X[i] = m["sv"][i % S] + step[i] * u / np.linalg.norm(u)
    X[n - S:] = m["sv"]
    ref = _both(m, X.astype(np.float32), X)
    for dt, Xv in (("float32", X.astype(np.float32)), ("float64", X)):
        _check(ctx, dict(model=m, X={dt: Xv}, ref=ref), dt)
    K = ref["float64"]["K"]
    assert int((K == 1.0).sum()) >= S and int((K == 0.0).sum()) > 0 and int(((K > 0.0) & (K < 1e-100)).sum()) > 0
    assert int(((K > 0.0) & (K < 1.0)).sum()) > n


@pytest.mark.parametrize("kernel", ["rbf", "poly"])
@pytest.mark.parametrize("S", [SV_CHUNK + 1, 2 * SV_CHUNK + 1])
def test_support_vector_seam(ctx, S, kernel):
    c = shape_case(4, 2, kernel, 3, 257, S)
    assert sorted(c["model"]["n_support"].tolist()) == [1, S - 1]   # one whole chunk (or two) and a single vector
    for dt in ("float32", "float64"):
        _check(ctx, c, dt)


@pytest.mark.parametrize("k", [3, 9])
def test_overflowed_poly_decisions_vote_as_the_restatement(ctx, k):
    """degree 8 at gamma 1e10 over pixels of three magnitudes: kernel values of 1e80, 1e160 and +inf, so decisions that are
    +-inf and NaN (inf - inf, 0 * inf).  A NaN decision votes for the pair's second class."""
    F, S, n = 6, 14, 300
    m = SC.random_model(F, k, S, "poly", 41, degree=8)
    m.update(gamma=1e10)
    rng = np.random.default_rng(42)
    X = rng.standard_normal((n, F)) * np.repeat([1.0, 1e10, 1e30], n // 3)[:, None]
    ref = _both(m, X.astype(np.float32), X)
    for dt, Xv in (("float32", X.astype(np.float32)), ("float64", X)):
        _check(ctx, dict(model=m, X={dt: Xv}, ref=ref), dt)
        d = ref[dt]["d"]
        assert bool(np.isnan(d).any()) and bool(np.isfinite(d).any()) and bool(np.isinf(ref[dt]["K"]).any())
        assert np.all(np.isinf(ref[dt]["margin"][np.isnan(d).all(axis=0)]))


def test_predict_image_with_a_mask(ctx):
    from rsseg.svm import SVMClassifier
    Xtr, ytr, _, _ = SC.blobs(3, 8)
    rng = np.random.default_rng(91)
    h, w = 67, 131          # more than two compaction tiles
    feats = (1.5 * rng.standard_normal((h, w, 8))).astype(np.float32)
    mask = rng.random((h, w)) < 0.6
    mask[:9] = False
    for kernel in ("rbf", "poly", "linear"):
        clf = SVMClassifier(kernel, degree=2, coef0=1.0).fit(Xtr, ytr)
        got, mg = clf.predict_image(feats, mask=mask, want_margin=True, ctx=ctx)
        assert got.shape == (h, w) and got.dtype == clf.classes_.dtype and mg.dtype == np.float32 and mg.shape == (h, w)
        want = np.zeros((h, w), np.int64)
        want[mask] = clf.predict(feats[mask], ctx=ctx)      # the host-compacted pixels
        assert np.array_equal(got, want) and set(np.unique(got[mask])) <= set(clf.classes_.tolist())
        ref = R.classify(feats[mask], SC.model_of(clf))
        assert np.array_equal(got[mask], clf._to_classes(ref["labels"])) and np.all(got[~mask] == 0)
        assert np.array_equal(_bits(mg[mask]), _bits(ref["margin"])) and np.all(np.isnan(mg[~mask]))
        plain = clf.predict_image([feats[:, :, i] for i in range(8)], ctx=ctx)      # unmasked, from a list of planes, labels only
        assert np.array_equal(plain[mask], got[mask])
        assert np.array_equal(plain.reshape(-1), clf.predict(feats.reshape(-1, 8), ctx=ctx))


@pytest.mark.parametrize("kernel", ["rbf", "poly", "linear"])
@pytest.mark.parametrize("k,F", SC.FITTED)
def test_fitted_model_reproduces_scikit_learn(ctx, k, F, kernel):
    """Labels equal SVC.predict wherever every |d_p| exceeds 1e-9 max(1, |d_p|); at most 0.1 % of the pixels are excluded."""
    from rsseg.svm import SVMClassifier
    svc, offset, scale, Xte = SC.fitted(k, F, kernel)
    clf = SVMClassifier.from_sklearn(svc, offset, scale)
    got = clf.predict(Xte, ctx=ctx)
    d = R.classify(Xte, SC.model_of(clf))["d"].T
    sure = np.all(np.abs(d) > 1e-9 * np.maximum(1.0, np.abs(d)), axis=1)
    assert int((~sure).sum()) <= 0.001 * sure.size
    assert np.array_equal(got[sure], svc.predict((Xte.astype(np.float64) - offset) * scale)[sure])


def test_stage_and_command(ctx, golden_dir, tmp_path):
    """python -m rsseg.svm on the directory of an earlier stages run: the four files, equal to the model object called
    directly; every earlier file byte-identical; --model reproduces the map.  run_svm_stage with a valid mask."""
    from rsseg import stages, svm
    from rsseg.svm import SVMClassifier
    from rsseg.tiff import read_tiff, write_tiff
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    bands = np.ascontiguousarray(crop["bands"])
    image, out = str(tmp_path / "in.tif"), tmp_path / "run"
    write_tiff(image, bands, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    roi = np.zeros((96, 96), np.uint8)
    roi[4:60:2, 4:60:2] = (crop["kmeans_stack19_k6"][4:60:2, 4:60:2] % 3 + 1).astype(np.uint8) * 4
    write_tiff(str(tmp_path / "roi.tif"), roi)
    assert stages.main([image, str(out), "--classify", "rule_based"]) == 0

    def snapshot():
        return {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}

    before = snapshot()
    assert svm.main([str(out), "--roi", str(tmp_path / "roi.tif"), "--rule-image"]) == 0
    after = snapshot()
    new = {os.path.join("segmentation_results", f) for f in ("classification_svm.npy", "svm_classification_map.tif", "svm_model.npz", "svm_margin.npy")}
    assert set(after) - set(before) == new
    assert all(after[f] == before[f] for f in before)
    sdir = out / "segmentation_results"
    allf = np.load(out / "feature_outputs" / "all_hierarchical_features.npy")
    clf = SVMClassifier().fit_image(allf, roi)
    want, mg = clf.predict_image(allf, want_margin=True, ctx=ctx)
    got = np.load(sdir / "classification_svm.npy")
    assert got.dtype == np.uint8 and np.array_equal(got, want) and set(np.unique(got)) <= {4, 8, 12}
    assert np.array_equal(read_tiff(str(sdir / "svm_classification_map.tif"))[0], want)
    assert np.array_equal(_bits(np.load(sdir / "svm_margin.npy")), _bits(mg))
    a, b = clf.params(), SVMClassifier.load(str(sdir / "svm_model.npz")).params()
    assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)
    assert float((got[roi != 0] == roi[roi != 0]).mean()) > 0.5
    # --model: the saved model, applied to a directory that has no SVM files yet
    model = str(tmp_path / "kept_model.npz")
    shutil.copy(sdir / "svm_model.npz", model)
    for f in new:
        os.remove(out / f)
    assert svm.main([str(out), "--model", model]) == 0
    assert np.array_equal(np.load(sdir / "classification_svm.npy"), want) and not os.path.exists(sdir / "svm_margin.npy")
    assert all(np.asarray(a[key]).tobytes() == np.asarray(v).tobytes() for key, v in SVMClassifier.load(str(sdir / "svm_model.npz")).params().items())
    # the stage function, linear, under a valid mask
    valid = np.ones((96, 96), np.uint8)
    valid[:, 70:] = 0
    lin = stages.run_svm_stage(str(out / "feature_outputs" / "all_features_and_metadata.pkl"), str(tmp_path / "lin"),
                               labeled_roi_file=str(tmp_path / "roi.tif"), kernel="linear", C=0.5, valid_mask=valid, ctx=ctx)
    want_lin = SVMClassifier("linear", C=0.5).fit_image(allf, roi).predict_image(allf, mask=valid, ctx=ctx)
    assert np.array_equal(lin, want_lin) and np.all(lin[:, 70:] == 0) and np.all(lin[:, :70] != 0)
    assert sorted(os.listdir(tmp_path / "lin")) == ["classification_svm.npy", "svm_classification_map.tif", "svm_model.npz"]


def _model_kw(m):
    return dict(k=len(m["n_support"]), S=m["sv"].shape[0], offset=m["offset"], scale=m["scale"], sv=m["sv"], n_support=m["n_support"], coef=m["coef"],
                bias=m["bias"], cv=m["class_values"], kernel={"rbf": 0, "poly": 1, "linear": 2}[m["kernel"]], gamma=m["gamma"], coef0=m["coef0"],
                degree=m["degree"], w=m["w"])


def _raw(ctx, a):
    from rsseg import _lib as L
    torch = _torch()
    dp = C.POINTER(C.c_double)
    f64 = lambda v: None if v is None else np.ascontiguousarray(v, np.float64)   # noqa: E731
    keep = {key: f64(a[key]) for key in ("offset", "scale", "sv", "coef", "bias", "w")}
    ns = None if a["n_support"] is None else np.ascontiguousarray(a["n_support"], np.int32)
    cv = None if a["cv"] is None else np.ascontiguousarray(a["cv"], np.uint8)
    planes = a["planes"]
    dtype = a.get("dtype")
    if dtype is None:
        dtype = L.F64 if planes and planes[0] is not None and planes[0].dtype == torch.float64 else L.F32
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    d = lambda key: None if keep[key] is None else keep[key].ctypes.data_as(dp)   # noqa: E731
    return ctx.lib.rsseg_svm_classify(ctx.h, ctx._pp(planes), a["F"], dtype, a["n"], a["k"], a["S"], d("offset"), d("scale"), d("sv"),
                                      None if ns is None else ns.ctypes.data_as(C.POINTER(C.c_int)), d("coef"), d("bias"),
                                      None if cv is None else cv.ctypes.data_as(C.POINTER(C.c_uint8)), a["kernel"], C.c_double(a["gamma"]),
                                      C.c_double(a["coef0"]), a["degree"], d("w"), ptr(a["labels"]), ptr(a["margin"]))


def test_error_codes(ctx):
    from rsseg.runtime import RssegUnsupported
    torch = _torch()
    F, k, S, n = 3, 3, 7, 10
    m = SC.random_model(F, k, S, "rbf", 5)
    lin = SC.random_model(F, k, S, "linear", 5)
    pl = _planes(ctx, np.zeros((n, F), np.float32))
    lab = torch.full((n,), 9, dtype=torch.uint8, device=ctx.device)
    ok = dict(planes=pl, F=F, n=n, labels=lab, margin=None, **_model_kw(m))

    def call(**kw):
        rc = _raw(ctx, {**ok, **kw})
        return rc, ctx.lib.rsseg_last_error(ctx.h).decode()

    assert call()[0] == 0 and call(**_model_kw(lin))[0] == 0
    INVALID, UNSUPPORTED = -1, -5
    at = lambda a, i, v: np.where(np.arange(a.size).reshape(a.shape) == i, v, a)   # noqa: E731
    for kw, code, word in (
            (dict(planes=[pl[0], None, pl[2]]), INVALID, "d_planes[1] is null"),
            (dict(F=0), INVALID, "d_planes"),
            (dict(F=65), UNSUPPORTED, "F=65"),
            (dict(k=1), INVALID, "k=1"),
            (dict(k=17), UNSUPPORTED, "k=17"),
            (dict(S=0), INVALID, "S=0"),
            (dict(S=16385), UNSUPPORTED, "S=16385"),
            (dict(dtype=3), INVALID, "dtype"),
            (dict(n=-1), INVALID, "n=-1"),
            (dict(kernel=3), UNSUPPORTED, "kernel=3"),
            (dict(sv=None), INVALID, "model"),
            (dict(n_support=None), INVALID, "model"),
            (dict(**{**_model_kw(lin), "w": None}), INVALID, "folded weights"),
            (dict(offset=at(m["offset"], 1, np.nan)), INVALID, "offset[1]"),
            (dict(scale=at(m["scale"], 2, np.inf)), INVALID, "scale[2]"),
            (dict(scale=at(m["scale"], 0, 0.0)), INVALID, "scale[0] is 0"),
            (dict(sv=at(m["sv"], 4, np.nan)), INVALID, "sv[4]"),
            (dict(coef=at(m["coef"], 8, -np.inf)), INVALID, "coef[8]"),
            (dict(bias=at(m["bias"], 2, np.nan)), INVALID, "bias[2]"),
            (dict(**{**_model_kw(lin), "w": at(lin["w"], 5, np.nan)}), INVALID, "w[5]"),
            (dict(n_support=np.array([7, 0, 0], np.int32)), INVALID, "n_support[1]=0"),
            (dict(n_support=np.array([1, 1, 1], np.int32)), INVALID, "n_support sums to 3"),
            (dict(cv=np.array([3, 0, 4], np.uint8)), INVALID, "class_values[1] is 0"),
            (dict(cv=np.array([3, 4, 3], np.uint8)), INVALID, "class_values[2]=3 occurs twice"),
            (dict(gamma=0.0), INVALID, "gamma"),
            (dict(gamma=-1.0), INVALID, "gamma"),
            (dict(gamma=float("nan")), INVALID, "gamma"),
            (dict(kernel=1, gamma=float("inf")), INVALID, "gamma"),
            (dict(kernel=1, coef0=float("nan")), INVALID, "coef0"),
            (dict(kernel=1, degree=0), INVALID, "degree=0"),
            (dict(kernel=1, degree=9), UNSUPPORTED, "degree=9"),
            (dict(labels=None), INVALID, "d_labels")):
        rc, msg = call(**kw)
        assert rc == code and word in msg and msg.startswith("svm_classify: "), (list(kw), rc, msg)
    # n == 0 touches nothing, whatever the planes
    assert call(**{**_model_kw(lin), "gamma": 0.0})[0] == 0      # gamma is the RBF's and the polynomial's alone
    ctx.sync()
    lab.fill_(9)
    assert call(n=0, planes=[None] * F, labels=None)[0] == 0
    ctx.sync()
    assert bool((lab == 9).all().item())
    # the Python side
    args = SC.model_args(m)
    with pytest.raises(ValueError, match="class_values"):
        ctx.svm_classify(pl, **{**args, "class_values": [1, 2, 256]})
    with pytest.raises(ValueError, match="is 0"):
        ctx.svm_classify(pl, **{**args, "class_values": [1, 0, 2]})
    with pytest.raises(ValueError, match="shapes"):
        ctx.svm_classify(pl, **{**args, "sv": m["sv"][:, :2]})
    with pytest.raises(ValueError, match="kernel"):
        ctx.svm_classify(pl, **{**args, "kernel": "sigmoid"})
    with pytest.raises(ValueError, match="float32 or all float64"):
        ctx.svm_classify([pl[0], pl[1], pl[2].double()], **args)
    with pytest.raises(RssegUnsupported):
        ctx.svm_classify(_planes(ctx, np.zeros((4, 65), np.float32)), **SC.model_args(SC.random_model(65, 2, 5, "rbf", 6)))
    lab0, m0 = ctx.svm_classify(_planes(ctx, np.zeros((0, F), np.float32)), want_margin=True, **args)
    assert lab0.numel() == m0.numel() == 0


def test_profiler_name(ctx):
    c = shape_case(3, 2, "rbf", 3, 3, 5)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _check(ctx, c, "float32")
        _, calls = ctx.prof_get("svm_classify")
    finally:
        ctx.prof_enable(False)
    assert calls == 1
