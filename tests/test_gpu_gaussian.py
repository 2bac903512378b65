"""K22 on the GPU: rsseg_gauss_classify equals the restatement (tests/gaussian_ref.py) bit for bit in labels, dist2 and margin
over the widths, class counts, plane types, output combinations, alignments and special values; the model object's masked
prediction, the three stage methods and the error codes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import gaussian_cases as GC
import gaussian_ref as R

pytestmark = pytest.mark.gpu

INF = float("inf")
SHAPES = sorted({(F, 8) for F in (1, 2, 8, 9, 19, 32, 33, 64)} | {(19, k) for k in (1, 2, 8, 9, 64)})
N_SHAPE = 1025   # more than one workgroup of every form (tiles of 1024, 512 and 256 pixels), a ragged last vector


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


@functools.lru_cache(maxsize=None)
def shape_case(F, k, n=N_SHAPE):
    """The model, the pixels and the restatement's m of both plane types: computed once per shape."""
    mean, wh, off, cv = GC.random_model(F, k, 1000 * F + k)
    X32, X64 = _pixels(n, F, 7 * F + k)
    m = R.quadratic_forms(np.concatenate([X32.astype(np.float64), X64]), mean, wh)
    return dict(mean=mean, whiten=wh, offset=off, values=cv, X={"float32": X32, "float64": X64}, m={"float32": m[:, :n], "float64": m[:, n:]})


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


def _check(ctx, c, dt, max_dist2, want_dist2, want_margin, shift=0):
    ref = R.decide(c["m"][dt], c["offset"], c["values"], max_dist2)
    lab, d2, mg = ctx.gauss_classify(_planes(ctx, c["X"][dt], shift), c["mean"], c["whiten"], c["offset"], c["values"], max_dist2,
                                     want_dist2=want_dist2, want_margin=want_margin)
    assert np.array_equal(lab.cpu().numpy(), ref["labels"])
    assert (d2 is None) == (not want_dist2) and (mg is None) == (not want_margin)
    if want_dist2:
        assert np.array_equal(_bits(d2.cpu().numpy()), _bits(ref["dist2"]))
    if want_margin:
        assert np.array_equal(_bits(mg.cpu().numpy()), _bits(ref["margin"]))
    return ref


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("F,k", SHAPES)
def test_kernel_equals_the_restatement(ctx, F, k, dt):
    c = shape_case(F, k)
    free = R.decide(c["m"][dt], c["offset"], c["values"])
    cut = float(np.nanmedian(free["dist2"]))
    for max_dist2 in (INF, cut):
        for want_dist2, want_margin in ((False, False), (True, False), (False, True), (True, True)):
            ref = _check(ctx, c, dt, max_dist2, want_dist2, want_margin)
    assert 0 < int((ref["labels"] == 0).sum()) < N_SHAPE          # the threshold bit, and did not take everything
    assert int(np.isnan(free["dist2"]).sum()) >= 2                 # the +-inf pixels have no winner
    if k == 1:
        assert np.all(np.isposinf(free["margin"][~np.isnan(free["dist2"])]))
    # planes one element off 16-byte alignment
    _check(ctx, c, dt, cut, True, True, shift=1)


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 32773])
@pytest.mark.parametrize("F,k", [(2, 2), (9, 3)])
def test_pixel_counts(ctx, F, k, n, dt):
    c = shape_case(F, k, n)
    _check(ctx, c, dt, INF, True, True)
    _check(ctx, c, dt, 2.0, False, False, shift=1)


def _raw(ctx, planes, F, n, k, mean, wh, off, cv, max_dist2, labels, dist2, margin, dtype=None):
    from rsseg import _lib as L
    torch = _torch()
    dp = C.POINTER(C.c_double)
    keep = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (mean, wh, off)]
    cvv = None if cv is None else np.ascontiguousarray(cv, np.uint8)
    if dtype is None:
        dtype = L.F64 if planes and planes[0] is not None and planes[0].dtype == torch.float64 else L.F32
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    return ctx.lib.rsseg_gauss_classify(ctx.h, ctx._pp(planes), F, dtype, n, k, *[None if a is None else a.ctypes.data_as(dp) for a in keep],
                                        None if cvv is None else cvv.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_double(max_dist2), ptr(labels),
                                        ptr(dist2), ptr(margin))


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_outputs_at_any_element_alignment(ctx, dt):
    """Output planes that start one element off their vector alignment: the kernel's element stores, and nothing outside
    [0, n) of any output is written."""
    torch = _torch()
    c = shape_case(9, 3, 1023)
    n = 1023
    ref = R.decide(c["m"][dt], c["offset"], c["values"], 2.0)
    lab = torch.full((n + 9,), 77, dtype=torch.uint8, device=ctx.device)
    d2 = torch.full((n + 9,), -5.0, dtype=torch.float32, device=ctx.device)
    mg = torch.full((n + 9,), -5.0, dtype=torch.float32, device=ctx.device)
    rc = _raw(ctx, _planes(ctx, c["X"][dt]), 9, n, 3, c["mean"], c["whiten"], c["offset"], c["values"], 2.0, lab[1:], d2[1:], mg[3:])
    assert rc == 0
    ctx.sync()
    lab, d2, mg = lab.cpu().numpy(), d2.cpu().numpy(), mg.cpu().numpy()
    assert np.array_equal(lab[1:n + 1], ref["labels"]) and lab[0] == 77 and np.all(lab[n + 1:] == 77)
    assert np.array_equal(_bits(d2[1:n + 1]), _bits(ref["dist2"])) and d2[0] == -5.0 and np.all(d2[n + 1:] == -5.0)
    assert np.array_equal(_bits(mg[3:n + 3]), _bits(ref["margin"])) and np.all(mg[:3] == -5.0) and np.all(mg[n + 3:] == -5.0)


def test_ties_nan_and_infinite_planes(ctx):
    """Two classes with identical parameters: the lower index everywhere; NaN pixels read as 0; +-inf planes leave a pixel
    unclassified with NaN outputs; a class whose g is +inf never wins."""
    from rsseg.gaussian import GaussianClassifier
    mean, wh, off, cv = GC.random_model(5, 2, 77)
    mean, wh, off = np.repeat(mean[:1], 3, 0), np.repeat(wh[:1], 3, 0), np.array([off[0], off[0], off[0] + 1.0])
    clf = GaussianClassifier.from_params(mean, wh, off, [200, 3, 9])
    rng = np.random.default_rng(78)
    X = rng.standard_normal((4099, 5)).astype(np.float32)
    X[rng.random(X.shape) < 0.02] = np.nan
    X[17, 2], X[18, 4], X[4098, 0] = np.inf, -np.inf, np.inf
    ref = R.classify(X, mean, wh, off, clf.class_values_)
    for Xv in (X, X.astype(np.float64)):
        lab, d2, mg = ctx.gauss_classify(_planes(ctx, Xv), mean, wh, off, clf.class_values_, want_dist2=True, want_margin=True)
        lab, d2, mg = lab.cpu().numpy(), d2.cpu().numpy(), mg.cpu().numpy()
        assert np.array_equal(lab, ref["labels"]) and np.array_equal(_bits(d2), _bits(ref["dist2"])) and np.array_equal(_bits(mg), _bits(ref["margin"]))
        bad = np.array([17, 18, 4098])
        ok = np.setdiff1d(np.arange(4099), bad)
        assert np.all(lab[ok] == 200) and np.all(mg[ok] == 0.0)
        assert np.all(lab[bad] == 0) and np.all(np.isnan(d2[bad])) and np.all(np.isnan(mg[bad]))
        assert np.array_equal(clf.predict(Xv, ctx=ctx), np.where(lab == 0, 0, 200))
        lab0, _, _ = ctx.gauss_classify(_planes(ctx, np.where(np.isnan(Xv), 0, Xv).astype(Xv.dtype)), mean, wh, off, clf.class_values_)
        assert np.array_equal(lab0.cpu().numpy(), lab)
    # g = +inf through the offset (tests/test_gaussian_host.py has the arithmetic): never the winner, not even alone
    W = np.stack([np.eye(2) * 2.0 ** 331, np.diag([2.0 ** -180, 1.0]), np.diag([2.0 ** -180, 1.0])])
    big = GaussianClassifier.from_params(np.zeros((3, 2)), W, [1.7e308, 0.0, 5.0], [1, 2, 3])
    Xb = np.zeros((3, 2))
    Xb[:, 0] = 2.0 ** 180
    lab, d2, mg = ctx.gauss_classify(_planes(ctx, Xb), big.mean_, big.whiten_, big.offset_, big.class_values_, want_dist2=True, want_margin=True)
    assert lab.cpu().tolist() == [2, 2, 2] and d2.cpu().tolist() == [1.0] * 3 and mg.cpu().tolist() == [5.0] * 3
    lab, d2, mg = ctx.gauss_classify(_planes(ctx, Xb), big.mean_[:1], big.whiten_[:1], big.offset_[:1], [1], want_dist2=True, want_margin=True)
    assert lab.cpu().tolist() == [0, 0, 0] and np.all(np.isnan(d2.cpu().numpy())) and np.all(np.isnan(mg.cpu().numpy()))


def test_predict_image_with_a_mask(ctx):
    from rsseg.gaussian import GaussianClassifier
    Xtr, ytr, _, _ = GC.case("f4_k3")
    rng = np.random.default_rng(91)
    h, w = 67, 131          # more than two compaction tiles
    feats = (1.5 * rng.standard_normal((h, w, 4))).astype(np.float32)
    mask = rng.random((h, w)) < 0.6
    mask[:9] = False
    for method, thr in (("ml", 0.9), ("mahalanobis", None), ("mindist", None)):
        clf = GaussianClassifier(method, threshold=thr).fit(Xtr, ytr)
        got, d2, mg = clf.predict_image(feats, mask=mask, want_dist2=True, want_margin=True, ctx=ctx)
        assert got.dtype == np.uint8 and got.shape == (h, w) and d2.dtype == mg.dtype == np.float32
        want = np.zeros((h, w), np.int64)
        want[mask] = clf.predict(feats[mask], ctx=ctx)
        assert np.array_equal(got, want)
        p = clf.params()
        ref = R.classify(feats[mask], p["mean"], p["whiten"], p["offset"], p["class_values"], p["max_dist2"])
        assert np.array_equal(got[mask], ref["labels"]) and np.all(got[~mask] == 0)
        assert np.array_equal(_bits(d2[mask]), _bits(ref["dist2"])) and np.all(np.isnan(d2[~mask]))
        assert np.array_equal(_bits(mg[mask]), _bits(ref["margin"])) and np.all(np.isnan(mg[~mask]))
        if thr is not None:
            assert 0 < int((got[mask] == 0).sum()) < int(mask.sum())
        # unmasked, from a list of planes, labels only
        plain = clf.predict_image([feats[:, :, i] for i in range(4)], ctx=ctx)
        assert np.array_equal(plain[mask], got[mask])
        counts = clf.class_counts(plain, ctx=ctx)
        assert counts == {0: int((plain == 0).sum()), **{int(v): int((plain == v).sum()) for v in clf.class_values_}}


def test_the_three_stage_methods(ctx, golden_dir, tmp_path, monkeypatch):
    """maximum_likelihood, mahalanobis and minimum_distance on crop96 with a synthetic ROI: the files are written and equal
    GaussianClassifier called directly; the command line composes with --ml-threshold, --rule-image, --mask-nodata, --sieve."""
    from rsseg import stages
    from rsseg.gaussian import GaussianClassifier
    from rsseg.tiff import read_tiff, write_tiff
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    bands = crop["bands"]
    fd, hier = stages.run_feature_extraction_stage(list(bands), ctx=ctx)
    paths = stages.save_feature_outputs(str(tmp_path / "features"), fd, hier, 96, 96, (30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), "EPSG:32649")
    roi = np.zeros((96, 96), np.uint8)
    roi[4:60, 4:60] = (crop["kmeans_stack19_k6"][4:60, 4:60] % 3 + 1).astype(np.uint8) * 4
    write_tiff(str(tmp_path / "labeled_roi.tif"), roi)
    arr = hier["all"]
    for method, short in (("maximum_likelihood", "ml"), ("mahalanobis", "mahalanobis"), ("minimum_distance", "mindist")):
        out = tmp_path / method
        got = stages.run_classification_stage(paths["pkl"], method, str(out), labeled_roi_file=str(tmp_path / "labeled_roi.tif"), ctx=ctx)
        assert sorted(os.listdir(out)) == [f"classification_{method}.npy", f"{method}_classification_map.tif", f"{method}_model.npz"]
        clf = GaussianClassifier(short).fit_image(arr, roi)
        want = clf.predict_image(arr, ctx=ctx)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and set(np.unique(got)) <= {4, 8, 12}
        assert np.array_equal(np.load(out / f"classification_{method}.npy"), want)
        assert np.array_equal(read_tiff(str(out / f"{method}_classification_map.tif"))[0], want)
        a, b = clf.params(), GaussianClassifier.load(str(out / f"{method}_model.npz")).params()
        for key in ("classes", "class_values", "mean", "whiten", "offset"):
            assert np.array_equal(a[key], b[key]), key
        assert float((got[roi != 0] == roi[roi != 0]).mean()) > 0.5
    # the command line: the label raster is ./labeled_roi.tif as for the forest
    monkeypatch.chdir(tmp_path)
    dn = np.ascontiguousarray(bands)
    image = str(tmp_path / "in.tif")
    write_tiff(image, dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    assert stages.main([image, str(tmp_path / "cli"), "--classify", "maximum_likelihood", "--ml-threshold", "0.999", "--rule-image", "--sieve", "4",
                        "--evaluate", str(tmp_path / "labeled_roi.tif")]) == 0
    sdir = tmp_path / "cli" / "segmentation_results"
    assert {"classification_maximum_likelihood.npy", "maximum_likelihood_classification_map.tif", "maximum_likelihood_model.npz",
            "maximum_likelihood_dist2.npy", "maximum_likelihood_margin.npy", "classification_maximum_likelihood_clean.npy"} <= set(os.listdir(sdir))
    allf = np.load(tmp_path / "cli" / "feature_outputs" / "all_hierarchical_features.npy")
    clf = GaussianClassifier("ml", threshold=0.999).fit_image(allf, roi)
    want, d2, mg = clf.predict_image(allf, want_dist2=True, want_margin=True, ctx=ctx)
    assert np.array_equal(np.load(sdir / "classification_maximum_likelihood.npy"), want)
    assert np.array_equal(_bits(np.load(sdir / "maximum_likelihood_dist2.npy")), _bits(d2))
    assert np.array_equal(_bits(np.load(sdir / "maximum_likelihood_margin.npy")), _bits(mg))
    assert os.path.exists(tmp_path / "cli" / "evaluation_results")


def test_error_codes(ctx):
    from rsseg.runtime import RssegUnsupported
    torch = _torch()
    F, k, n = 3, 2, 10
    mean, wh, off, cv = GC.random_model(F, k, 5)
    X = np.zeros((n, F), np.float32)
    pl = _planes(ctx, X)
    lab = torch.full((n,), 9, dtype=torch.uint8, device=ctx.device)
    ok = dict(planes=pl, F=F, n=n, k=k, mean=mean, wh=wh, off=off, cv=cv, max_dist2=INF, labels=lab, dist2=None, margin=None)

    def call(**kw):
        a = {**ok, **kw}
        rc = _raw(ctx, a["planes"], a["F"], a["n"], a["k"], a["mean"], a["wh"], a["off"], a["cv"], a["max_dist2"], a["labels"], a["dist2"], a["margin"],
                  a.get("dtype"))
        return rc, ctx.lib.rsseg_last_error(ctx.h).decode()

    assert call()[0] == 0
    INVALID, UNSUPPORTED = -1, -5
    for kw, code, word in (
            (dict(planes=[pl[0], None, pl[2]]), INVALID, "d_planes[1] is null"),
            (dict(mean=np.where(np.arange(k * F).reshape(k, F) == 4, np.nan, mean)), INVALID, "mean[4]"),
            (dict(wh=np.where(np.arange(wh.size).reshape(wh.shape) == 7, np.inf, wh)), INVALID, "whiten[7]"),
            (dict(off=np.array([0.0, -np.inf])), INVALID, "offset[1]"),
            (dict(cv=np.array([3, 0], np.uint8)), INVALID, "class_values[1] is 0"),
            (dict(cv=np.array([3, 3], np.uint8)), INVALID, "class_values[1]=3 occurs twice"),
            (dict(max_dist2=float("nan")), INVALID, "max_dist2 is NaN"),
            (dict(labels=None), INVALID, "d_labels"),
            (dict(n=-1), INVALID, "n=-1"),
            (dict(k=0), INVALID, "k=0"),
            (dict(F=0), INVALID, "d_planes"),
            (dict(dtype=3), INVALID, "dtype"),
            (dict(mean=None), INVALID, "model"),
            (dict(F=65), UNSUPPORTED, "F=65"),
            (dict(k=65), UNSUPPORTED, "k=65")):
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw.keys(), rc, msg)
    # n == 0 touches nothing, whatever the planes
    lab.fill_(9)
    assert call(n=0, planes=[None] * F, labels=None)[0] == 0
    ctx.sync()
    assert bool((lab == 9).all().item())
    # the Python side
    with pytest.raises(ValueError, match="class_values"):
        ctx.gauss_classify(pl, mean, wh, off, [1, 256])
    with pytest.raises(ValueError, match="is 0"):
        ctx.gauss_classify(pl, mean, wh, off, [1, 0])
    with pytest.raises(ValueError, match="shapes"):
        ctx.gauss_classify(pl, mean[:, :2], wh, off, cv)
    with pytest.raises(ValueError, match="float32 or all float64"):
        ctx.gauss_classify([pl[0], pl[1], pl[2].double()], mean, wh, off, cv)
    with pytest.raises(RssegUnsupported):
        m65, w65, o65, c65 = GC.random_model(65, 2, 6)
        ctx.gauss_classify(_planes(ctx, np.zeros((4, 65), np.float32)), m65, w65, o65, c65)
    lab0, d0, m0 = ctx.gauss_classify(_planes(ctx, np.zeros((0, F), np.float32)), mean, wh, off, cv, want_dist2=True, want_margin=True)
    assert lab0.numel() == d0.numel() == m0.numel() == 0


def test_profiler_name(ctx):
    c = shape_case(2, 2, 3)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _check(ctx, c, "float32", INF, False, False)
        _, calls = ctx.prof_get("gauss_classify")
    finally:
        ctx.prof_enable(False)
    assert calls == 1
