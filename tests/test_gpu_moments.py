"""K24 on the GPU: rsseg_class_moments equals the restatement (tests/moments_ref.py) bit for bit over the widths, class counts,
plane and label types, pixel counts around the tile seams and both paths; the inputs that stress the contract; stripe-wise
merging; the error codes; the model fitted on the device and the stage driver's two flags."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import moments_ref as M

pytestmark = pytest.mark.gpu

FS = (1, 2, 8, 9, 19, 33, 64)
KS = (1, 2, 8, 9, 64, 256)
F32, U8, I32 = 0, 3, 6


def _torch():
    import torch
    return torch


def _plan(F, k, u8=False):
    from rsseg import _lib as L
    path, tile = C.c_int(0), C.c_int(0)
    L.load().rsseg_class_moments_plan(F, k, U8 if u8 else F32, C.byref(path), C.byref(tile))
    return path.value, tile.value


def _dev(ctx, a, shift=0):
    """A flat device tensor holding `a` that starts `shift` elements off its (256-byte aligned) allocation."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    t = torch.empty(a.size + shift, dtype=torch.from_numpy(a[:0].copy()).dtype, device=ctx.device)
    t[shift:] = torch.from_numpy(a.reshape(-1)).to(ctx.device)
    return t[shift:]


def _exp_of(x):
    from rsseg.signatures import exponent_for
    x = np.where(np.isfinite(x), x, 0.0)
    return np.array([exponent_for(np.abs(x[f]).max()) for f in range(x.shape[0])], np.int64)


def _run(ctx, planes, labels, k, pe, Q, ignore=-1, mask=None, shift=0):
    dp = [_dev(ctx, planes[f], shift) for f in range(planes.shape[0])]
    table, left = ctx.class_moments(dp, _dev(ctx, labels, shift), k, pe, Q, ignore=ignore, mask=None if mask is None else _dev(ctx, mask, shift))
    return table.cpu().numpy(), left


def _same(ctx, planes, labels, k, pe, Q, ignore=-1, mask=None, shift=0, label_types=(np.uint8, np.int32)):
    want, wleft = M.moments_table(planes, labels, k, pe, Q, ignore=ignore, mask=mask)
    for lt in label_types:
        got, left = _run(ctx, planes, labels.astype(lt), k, pe, Q, ignore, mask, shift)
        assert got.dtype == np.int64 and got.shape == want.shape
        assert np.array_equal(got, want), (lt, np.argwhere(got != want)[:5])
        assert left == wleft
    return want, wleft


@functools.lru_cache(maxsize=None)
def sweep_data(F, k, tile):
    """planes of scales 2^-7 ... 2^6 (float32, negative values included), their uint8 twins, labels over all k classes"""
    n = 3 * tile + 5
    rng = np.random.default_rng(100 * F + k)
    x = (rng.standard_normal((F, n)) * 2.0 ** rng.integers(-7, 7, (F, 1))).astype(np.float32)
    q = rng.integers(0, 256, (F, n)).astype(np.uint8)
    lab = rng.integers(0, k, n)
    lab[:min(k, n)] = np.arange(k)[:n]   # every class occurs
    return x, q, lab


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("F", FS)
def test_table_equals_the_restatement(ctx, F, k):
    path, tile = _plan(F, k)
    assert path in (0, 1) and tile in (256, 512) and _plan(F, k, True) == (path, tile)
    x, q, lab = sweep_data(F, k, tile)
    pe = _exp_of(x)
    for n in (1, 3, tile - 1, tile + 1, 3 * tile + 5):
        # uint8 labels with no label ignored, int32 labels with label 0 ignored
        _same(ctx, x[:, :n], lab[:n], k, pe, 44, ignore=-1, label_types=(np.uint8,))
        _same(ctx, x[:, :n], lab[:n], k, pe, 44, ignore=0, label_types=(np.int32,))
        _same(ctx, q[:, :n], lab[:n], k, None, 0, ignore=-1, label_types=(np.int32,))
        _same(ctx, q[:, :n], lab[:n], k, None, 0, ignore=0, label_types=(np.uint8,))


def test_both_paths_are_in_the_sweep():
    paths = {(F, k): _plan(F, k)[0] for F in FS for k in KS}
    assert set(paths.values()) == {0, 1}
    assert paths[(19, 8)] == 0 and paths[(64, 1)] == 0 and paths[(64, 2)] == 1 and paths[(19, 64)] == 1 and paths[(1, 256)] == 0
    # both sides of the switch at F = 19: the last class count whose table fits, and the next
    ks = [k for k in range(1, 257) if _plan(19, k)[0] == 0]
    assert ks == list(range(1, ks[-1] + 1)) and 8 <= ks[-1] < 64
    assert _plan(65, 2) == (-1, 0) and _plan(2, 257) == (-1, 0) and _plan(0, 2) == (-1, 0)


@pytest.mark.parametrize("F,k", [(5, 4), (19, "last in LDS"), (19, "first global"), (64, 3)])
def test_inputs_that_stress_the_contract(ctx, F, k):
    if isinstance(k, str):   # the two class counts on either side of the path switch at this width
        last = max(c for c in range(1, 257) if _plan(F, c)[0] == 0)
        k = last if k == "last in LDS" else last + 1
        assert _plan(F, k)[0] == (0 if k == last else 1)
    path, tile = _plan(F, k)
    n = 2 * tile + 77
    rng = np.random.default_rng(7 * F + k)
    x = (rng.standard_normal((F, n)) * 2.0 ** rng.integers(-3, 4, (F, 1))).astype(np.float32)
    lab = rng.integers(0, k, n)
    pe = _exp_of(x)
    mask = (rng.random(n) < 0.7).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    # one element off 16-byte alignment, with and without a mask and an ignored label
    _same(ctx, x, lab, k, pe, 40, ignore=-1, shift=1)
    _same(ctx, x, lab, k, pe, 40, ignore=1 % k, mask=mask, shift=1)
    _same(ctx, x, lab, k, pe, 40, ignore=0, mask=mask, shift=3)
    # every label ignored; every pixel masked
    want, _ = _same(ctx, x, np.full(n, k - 1), k, pe, 40, ignore=k - 1)
    assert not want.any()
    want, _ = _same(ctx, x, lab, k, pe, 40, mask=np.zeros(n, np.uint8))
    assert not want.any()
    # one counted pixel, in the last tile
    one = np.full(n, 0)
    one[n - 2] = k - 1
    want, _ = _same(ctx, x, one, k, pe, 40, ignore=0)
    assert want[:, 0].sum() == (1 if k > 1 else 0)
    # all pixels in one class
    want, _ = _same(ctx, x, np.full(n, k - 1), k, pe, 40)
    assert want[k - 1, 0] == n and want[:, 0].sum() == n
    # NaN reads as 0; +-inf and values beyond the stated range leave the pixel out
    y = x.copy()
    y[rng.random(y.shape) < 0.02] = np.nan
    y[0, 5], y[F - 1, 9], y[F // 2, n - 1] = np.inf, -np.inf, np.inf
    tight = pe.copy()
    tight[0] += 2          # plane 0 is stated four times narrower than it is
    want, left = _same(ctx, y, lab, k, tight, 40)
    assert 3 <= left < n and want[:, 0].sum() == n - left
    want0, left0 = M.moments_table(np.nan_to_num(y, nan=0.0, posinf=np.inf, neginf=-np.inf), lab, k, tight, 40)
    assert np.array_equal(want, want0) and left == left0
    # Q at 0 and at its cap
    _same(ctx, x, lab, k, pe, 0)
    _same(ctx, x, lab, k, pe, 50)
    # rounding ties: multiples of 1/16 at Q = 3 put u 2^Q and u_a 2^Q u_b on halves
    t = (rng.integers(-16, 17, (F, n)) / 16.0).astype(np.float32)
    prod = t[0] * 8.0 * t[F - 1]
    assert int((np.abs(prod - np.trunc(prod)) == 0.5).sum()) > 10 and int((np.abs(t[0] * 8 % 1) == 0.5).sum()) > 10
    for Q in (0, 1, 3):
        _same(ctx, t, lab, k, np.zeros(F, np.int64), Q)
    # uint8 planes, misaligned, masked
    q = rng.integers(0, 256, (F, n)).astype(np.uint8)
    q[:, :3] = 255
    _same(ctx, q, lab, k, None, 0, ignore=0, mask=mask, shift=1)


@pytest.mark.parametrize("F,k", [(5, 4), (19, 32), (64, 2)])
def test_several_workgroups(ctx, F, k):
    """More pixels than three workgroups take at a time (a workgroup walks spans of at most 4096 pixels), on both paths, with
    spans that hold no counted pixel between spans that do."""
    n = 3 * 4096 + 5
    rng = np.random.default_rng(31 * F + k)
    x = (rng.standard_normal((F, n)) * 2.0 ** rng.integers(-3, 4, (F, 1))).astype(np.float32)
    lab = rng.integers(0, k, n)
    _same(ctx, x, lab, k, _exp_of(x), 44, ignore=-1, label_types=(np.uint8,))
    lab[4096:8192] = 0
    mask = np.ones(n, np.uint8)
    mask[8192:8192 + 4096] = 0
    mask[n - 3] = 1
    want, _ = _same(ctx, x, lab, k, _exp_of(x), 44, ignore=0, mask=mask, label_types=(np.int32,))
    assert want[:, 0].sum() == int(((lab != 0) & (mask != 0)).sum()) > 0


def test_empty_raster_writes_zeros(ctx):
    torch = _torch()
    planes = [torch.empty(0, dtype=torch.float32, device=ctx.device) for _ in range(3)]
    table, left = ctx.class_moments(planes, torch.empty(0, dtype=torch.uint8, device=ctx.device), 4, [0, 0, 0], 44)
    assert table.shape == (4, 10) and not table.cpu().numpy().any() and left == 0


def test_stripes_merge_to_the_single_call(ctx):
    """Geometry independence at the public interface: row stripes taken with the whole raster's ranges and pixel count merge
    to the table of one call, and to the restatement."""
    from rsseg.signatures import class_moments
    rng = np.random.default_rng(2410)
    H, W, F = 61, 53, 7
    feats = (rng.standard_normal((H, W, F)) * np.array([1e-3, 0.1, 1, 5, 40, 200, 3])).astype(np.float32)
    feats[rng.random(feats.shape) < 0.01] = np.nan
    lab = rng.integers(0, 6, (H, W)).astype(np.uint8)
    lab[3, 4] = 1
    mask = rng.random((H, W)) < 0.8
    whole = class_moments(feats, lab, mask=mask, ctx=ctx)
    assert whole.Q == 44 and whole.n_left_out == 0 and whole.classes.tolist() == [1, 2, 3, 4, 5]
    want, _ = M.moments_table(np.moveaxis(feats, -1, 0).reshape(F, -1), lab.reshape(-1), 6, whole.plane_exp, whole.Q, ignore=0, mask=mask.reshape(-1))
    assert np.array_equal(whole.table, want)
    ranges = np.nanmax(np.abs(feats.reshape(-1, F)), axis=0)
    acc = None
    for r0, r1 in ((0, 1), (1, 20), (20, 21), (21, 61)):
        part = class_moments(feats[r0:r1], lab[r0:r1], mask=mask[r0:r1], ranges=ranges, n_total=H * W, ctx=ctx)
        acc = part if acc is None else acc.merge(part)
    assert np.array_equal(acc.table, whole.table) and np.array_equal(acc.plane_exp, whole.plane_exp) and acc.Q == whole.Q
    # device planes and int32 device labels give the same table; the extrema pass ignores NaN and infinite values
    dev = [ctx.to_device(np.ascontiguousarray(feats[:, :, f]).reshape(-1)) for f in range(F)]
    again = class_moments(dev, ctx.to_device(lab.reshape(-1).astype(np.int32)), mask=mask, ctx=ctx)
    assert np.array_equal(again.table, whole.table)
    feats[3, 4, 2] = np.inf
    with_inf = class_moments(feats, lab, ctx=ctx)
    assert np.array_equal(with_inf.plane_exp, whole.plane_exp) and with_inf.n_left_out == 1
    # uint8 planes
    q = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    m8 = class_moments(q, lab, ctx=ctx)
    want8, _ = M.moments_table(np.moveaxis(q, -1, 0).reshape(3, -1), lab.reshape(-1), 6, None, 0, ignore=0)
    assert m8.Q == 0 and np.array_equal(m8.table, want8)


@pytest.mark.parametrize("F,k", [(6, 5), (64, 256)])
def test_sum_over_ranks_through_the_hook(F, k):
    """With a communication hook installed the table and n_left_out go through it as int64 SUM.  The hook here stands for
    two ranks that hold the same stripe (it doubles what it is given), so the result is twice the restatement's; the
    4.4 MB table of F = 64 with 256 labels passes the 4 MiB communication buffer in two pieces."""
    from rsseg import _lib as L
    from rsseg.runtime import Context
    n = 300
    rng = np.random.default_rng(5 * F + k)
    x = rng.standard_normal((F, n)).astype(np.float32)
    x[0, 7] = np.inf
    lab = rng.integers(0, k, n)
    pe = _exp_of(x)
    want, wleft = M.moments_table(x, lab, k, pe, 44)
    seen = []

    def twice(buf, offset, count, dtype, op):
        assert dtype == L.I64 and op == L.SUM and offset + 8 * count <= buf.numel()
        seen.append(count)
        buf[offset:offset + 8 * count].view(_torch().int64).mul_(2)

    c = Context(0, use_dist=False)
    try:
        c.install_comm_hook(0, 1, twice)
        got, left = _run(c, x, lab.astype(np.int32), k, pe, 44)
    finally:
        c.close()
    assert wleft == 1 and left == 2 * wleft and np.array_equal(got, 2 * want)
    assert sum(seen) == want.size + 1 and len(seen) == (1 if 8 * (want.size + 1) <= (1 << 22) else 2)


def _raw(ctx, planes, F, dtype, n, labels, label_dtype, k, ignore, mask, pe, Q, out, left=True):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    pe_arr = None if pe is None else (C.c_int * len(pe))(*pe)
    nl = C.c_int64(-7)
    rc = ctx.lib.rsseg_class_moments(ctx.h, None if planes is None else ctx._pp(planes), F, dtype, n, ptr(labels), label_dtype, k, ignore, ptr(mask),
                                     pe_arr, Q, ptr(out), C.byref(nl) if left else None)
    return rc, ctx.lib.rsseg_last_error(ctx.h).decode()


def test_error_codes(ctx):
    from rsseg.runtime import RssegUnsupported
    torch = _torch()
    F, k, n = 3, 4, 10
    pl = [torch.zeros(n + 1, dtype=torch.float32, device=ctx.device) for _ in range(F)]
    pu = [torch.zeros(n, dtype=torch.uint8, device=ctx.device) for _ in range(F)]
    lab8 = torch.ones(n, dtype=torch.uint8, device=ctx.device)
    lab32 = torch.ones(n + 1, dtype=torch.int32, device=ctx.device)
    out = torch.zeros(64, dtype=torch.int64, device=ctx.device)   # room for the 5-class call below
    ok = dict(planes=[p[:n] for p in pl], F=F, dtype=F32, n=n, labels=lab8, label_dtype=U8, k=k, ignore=-1, mask=None, pe=[0, 0, 0], Q=44, out=out)

    def call(**kw):
        a = {**ok, **kw}
        return _raw(ctx, a["planes"], a["F"], a["dtype"], a["n"], a["labels"], a["label_dtype"], a["k"], a["ignore"], a["mask"], a["pe"], a["Q"], a["out"],
                    a.get("left", True))

    assert call()[0] == 0
    INVALID, UNSUPPORTED = -1, -5
    bad8 = lab8.clone()
    bad8[7] = k
    neg32 = lab32[:n].clone()
    neg32[2] = -1
    for kw, code, word in (
            (dict(F=0), INVALID, "F=0"),
            (dict(planes=None), INVALID, "d_planes"),
            (dict(F=65), UNSUPPORTED, "F=65"),
            (dict(k=0), INVALID, "n_classes=0"),
            (dict(k=257), UNSUPPORTED, "n_classes=257"),
            (dict(Q=-1), INVALID, "Q=-1"),
            (dict(Q=51), INVALID, "Q=51"),
            (dict(n=1 << 20, Q=42), INVALID, "2^62"),
            (dict(n=-1), INVALID, "n_local=-1"),
            (dict(dtype=1), INVALID, "dtype"),
            (dict(label_dtype=F32), INVALID, "label_dtype"),
            (dict(pe=None), INVALID, "plane_exp"),
            (dict(pe=[0, 301, 0]), INVALID, "plane_exp[1]=301"),
            (dict(planes=pu, dtype=U8), INVALID, "plane_exp = NULL and Q = 0"),
            (dict(planes=pu, dtype=U8, pe=None, Q=1), INVALID, "plane_exp = NULL and Q = 0"),
            (dict(planes=[pl[0][:n], None, pl[2][:n]]), INVALID, "d_planes[1]"),
            (dict(labels=None), INVALID, "d_labels"),
            (dict(out=None), INVALID, "d_out"),
            (dict(left=False), INVALID, "n_left_out"),
            (dict(labels=bad8), INVALID, "label outside 0 ... 3"),
            (dict(labels=neg32, label_dtype=I32), INVALID, "label outside 0 ... 3"),
            (dict(labels=bad8, k=5, ignore=4, pe=[0, 0, 0]), 0, "")):
        rc, msg = call(**kw)
        assert rc == code and (code == 0 or word in msg), (list(kw), rc, msg)
    # a bad label under the mask, or equal to `ignore`, is not counted and not an error
    m = torch.ones(n, dtype=torch.uint8, device=ctx.device)
    m[7] = 0
    assert call(labels=bad8, mask=m)[0] == 0 and call(labels=bad8, ignore=k)[0] == 0
    # the Python side
    with pytest.raises(ValueError, match="float32 or all uint8"):
        ctx.class_moments([pl[0][:n], pu[1], pl[2][:n]], lab8, k, [0, 0, 0], 44)
    with pytest.raises(ValueError, match="uint8 or int32"):
        ctx.class_moments(ok["planes"], lab8.long(), k, [0, 0, 0], 44)
    with pytest.raises(ValueError, match="plane exponents"):
        ctx.class_moments(ok["planes"], lab8, k, [0, 0], 44)
    with pytest.raises(RssegUnsupported):
        ctx.class_moments(ok["planes"], lab8, 257, [0, 0, 0], 44)
    # planes and labels at any element alignment (one element off their allocation) are taken
    assert call(planes=[p[1:] for p in pl], labels=lab32[1:], label_dtype=I32)[0] == 0


def test_profiler_name(ctx):
    x = np.zeros((2, 3), np.float32)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _run(ctx, x, np.zeros(3, np.uint8), 1, [0, 0], 44)
        _, calls = ctx.prof_get("class_moments")
    finally:
        ctx.prof_enable(False)
    assert calls == 1


# ---- the model and the stage on the 96 x 96 golden crop ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crop(golden_dir):
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    roi = np.zeros((96, 96), np.uint8)
    roi[4:60, 4:60] = (crop["kmeans_stack19_k6"][4:60, 4:60] % 3 + 1).astype(np.uint8) * 4
    return crop["bands"], roi


def test_fit_image_on_the_device(ctx, golden_dir, tmp_path):
    """fit_image(..., device=True) against the default fit on the same float32 stack: the labels of every pixel whose margin
    under the default model exceeds 1e-6 (asserted for all of them first) are identical, for the three methods."""
    import gaussian_ref as R
    from rsseg import stages
    from rsseg.gaussian import GaussianClassifier
    bands, roi = _crop(golden_dir)
    _, hier = stages.run_feature_extraction_stage(list(bands), ctx=ctx)
    arr = hier["all"].astype(np.float32)
    X = arr.reshape(-1, arr.shape[2])
    for method in ("ml", "mahalanobis", "mindist"):
        a = GaussianClassifier(method).fit_image(arr, roi)
        b = GaussianClassifier(method).fit_image(arr, roi, device=True, ctx=ctx)
        assert np.array_equal(a.classes_, b.classes_) and np.array_equal(a.class_counts_, b.class_counts_)
        # half a unit of 2^-Q 2^-e_f <= 2^-44 max|x_f| on one side, the float64 rounding of the host mean (n eps max|x_f|) on the other
        assert np.all(np.abs(a.mean_ - b.mean_) <= (2.0 ** -44 + X.shape[0] * np.finfo(np.float64).eps) * np.abs(X).max(0))
        pa = a.params()
        ra = R.classify(X, pa["mean"], pa["whiten"], pa["offset"], pa["class_values"], pa["max_dist2"])
        margin = ra["second"] - ra["best"]
        print(method, "smallest margin", float(margin.min()))
        assert np.all(margin > 1e-6)
        got = b.predict_image(arr, ctx=ctx)
        assert np.array_equal(got.reshape(-1), ra["labels"])
        assert np.array_equal(got, a.predict_image(arr, ctx=ctx))


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def test_signatures_and_fit_on_device_flags(ctx, golden_dir, tmp_path, monkeypatch):
    """--signatures with and without an ROI and --fit-on-device on crop96: the two files are written, their counts are
    np.bincount's and their means NumPy's; every file a run without the flags writes is there with the same bytes."""
    import json
    from rsseg import stages
    from rsseg.signatures import ClassMoments
    from rsseg.tiff import write_tiff
    bands, roi = _crop(golden_dir)
    monkeypatch.chdir(tmp_path)
    write_tiff(str(tmp_path / "labeled_roi.tif"), roi)
    image = str(tmp_path / "in.tif")
    write_tiff(image, np.ascontiguousarray(bands), transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)

    def check(sdir, method, labels, valid=None):
        allf = np.load(os.path.join(os.path.dirname(sdir), "feature_outputs", "all_hierarchical_features.npy")).astype(np.float32)
        mom = ClassMoments.load(os.path.join(sdir, f"signatures_{method}.npz"))
        with open(os.path.join(sdir, f"separability_{method}.json")) as f:
            rep = json.load(f)
        lab = np.where(valid, labels, 0) if valid is not None else labels
        counts = np.bincount(lab.reshape(-1), minlength=mom.table.shape[0])
        counts[0] = 0
        assert np.array_equal(mom.counts, counts) and mom.n_left_out == 0
        assert rep["classes"] == np.flatnonzero(counts).tolist() and [p["count"] for p in rep["per_class"]] == counts[counts > 0].tolist()
        X = allf.reshape(-1, allf.shape[2]).astype(np.float64)
        unit = 2.0 ** (-mom.Q - mom.plane_exp.astype(np.float64))
        for j, c in enumerate(mom.classes):
            want = np.nan_to_num(X[lab.reshape(-1) == c], nan=0.0).mean(0)
            assert np.all(np.abs(mom.mean()[j] - want) <= unit + X.shape[0] * np.finfo(np.float64).eps * np.abs(X).max(0))
            assert np.allclose(rep["per_class"][j]["mean"], mom.mean()[j], rtol=0, atol=0)
        assert ("jm" in rep and "td" in rep) or "error" in rep
        return rep

    # the raw k-means map's signatures; the plain run's files are all there, byte for byte
    assert stages.main([image, str(tmp_path / "plain"), "--classify", "kmeans", "--n-clusters", "4"]) == 0
    assert stages.main([image, str(tmp_path / "sig"), "--classify", "kmeans", "--n-clusters", "4", "--signatures"]) == 0
    plain, sig = _tree(tmp_path / "plain"), _tree(tmp_path / "sig")
    new = {os.path.join("segmentation_results", "signatures_kmeans.npz"), os.path.join("segmentation_results", "separability_kmeans.json")}
    assert set(sig) - set(plain) == new and set(plain) <= set(sig)
    assert all(sig[k] == plain[k] for k in plain), [k for k in plain if sig[k] != plain[k]]
    kmap = np.load(tmp_path / "sig" / "segmentation_results" / "classification_kmeans.npy")
    check(str(tmp_path / "sig" / "segmentation_results"), "kmeans", kmap)

    # the ROI's training classes, the model fitted on the device, under a nodata mask
    assert stages.main([image, str(tmp_path / "mlp"), "--classify", "maximum_likelihood", "--mask-nodata", "0"]) == 0
    assert stages.main([image, str(tmp_path / "ml"), "--classify", "maximum_likelihood", "--mask-nodata", "0", "--fit-on-device",
                        "--signatures", str(tmp_path / "labeled_roi.tif")]) == 0
    mdir = tmp_path / "ml" / "segmentation_results"
    valid = np.load(tmp_path / "ml" / "feature_outputs" / "valid_mask.npy") != 0
    rep = check(str(mdir), "maximum_likelihood", roi, valid)
    assert rep["classes"] == [4, 8, 12] and "error" not in rep and len(rep["jm"]["matrix"]) == 3
    got = np.load(mdir / "classification_maximum_likelihood.npy")
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 4, 8, 12}
    assert float((got[(roi != 0) & valid] == roi[(roi != 0) & valid]).mean()) > 0.5
    # the flags leave the feature files of the same command alone
    p2, m2 = _tree(tmp_path / "mlp"), _tree(tmp_path / "ml")
    same = [k for k in p2 if "maximum_likelihood" not in k]     # the feature files; the model and its map come from another fit
    assert same and all(m2[k] == p2[k] for k in same)
