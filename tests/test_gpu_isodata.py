"""K26 on the GPU: rsseg_isodata_sweep equals the restatement (tests/isodata_ref.py) bit for bit over the widths, cluster
counts, plane types, pixel counts around the tile seams and both paths; the inputs that stress the contract; whole isodata()
runs against the runs on the restatement; the stage's command line; the error codes."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import isodata_ref as R

pytestmark = pytest.mark.gpu

FS = (1, 7, 15, 19, 33, 64)
KS = (1, 2, 8, 33, 64)


def _torch():
    import torch
    return torch


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


def _same(ctx, planes, mask, pe, Q, weight, centers, labels_in, shift=0):
    """The sweep with a table and the labels-only sweep against the restatement: labels, table, n_changed, n_left_out."""
    want = R.sweep_ref(planes, mask, pe, Q, weight, centers, labels_in)
    dp = [_dev(ctx, planes[f], shift) for f in range(planes.shape[0])]
    dm = None if mask is None else _dev(ctx, mask, shift)
    for want_table in (True, False):
        lab = _dev(ctx, labels_in, shift)
        table, changed, left = ctx.isodata_sweep(dp, lab, centers, weight, pe, Q, mask=dm, want_table=want_table)
        got = lab.cpu().numpy()
        assert np.array_equal(got, want[0]), (want_table, np.flatnonzero(got != want[0])[:5])
        assert (changed, left) == (want[2], want[3]), (want_table, changed, left, want[2], want[3])
        if want_table:
            t = table.cpu().numpy()
            assert t.dtype == np.int64 and np.array_equal(t, R.table_array(want[1])), np.argwhere(t != R.table_array(want[1]))[:5]
        else:
            assert table is None
    return want


@functools.lru_cache(maxsize=None)
def sweep_data(F, k, n):
    """planes of scales 2^-7 ... 2^6 (float32, negative values included), their uint8 twins, weights, centres among the pixels
    (in weighted units), labels over 0 ... k - 1 and 255"""
    rng = np.random.default_rng(100 * F + k)
    x = (rng.standard_normal((F, n)) * 2.0 ** rng.integers(-7, 7, (F, 1))).astype(np.float32)
    q = rng.integers(0, 256, (F, n)).astype(np.uint8)
    pe = _exp_of(x)
    w = rng.uniform(0.25, 4.0, F)
    pick = rng.integers(0, n, k)
    cx = np.ldexp(x[:, pick].astype(np.float64), pe.reshape(F, 1)).T * w + 0.01 * rng.standard_normal((k, F))
    wq = rng.uniform(0.25, 4.0, F) / 255.0
    cq = q[:, pick].astype(np.float64).T * wq + 0.01 * rng.standard_normal((k, F))
    lab = np.where(rng.random(n) < 0.2, 255, rng.integers(0, k, n)).astype(np.uint8)
    return x, pe, w, cx, q, wq, cq, lab


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("F", FS)
def test_sweep_equals_the_restatement(ctx, F, k):
    path, tile = ctx.isodata_plan(F, k)
    assert path in (0, 1) and tile == 256 and ctx.isodata_plan(F, k, True) == (path, tile)
    x, pe, w, cx, q, wq, cq, lab = sweep_data(F, k, 3 * tile + 5)
    for n in (0, 1, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile + 5):
        want = _same(ctx, x[:, :n], None, pe, 44, w, cx, lab[:n])
        assert sum(row[0] for row in want[1]) == n
        _same(ctx, q[:, :n], None, None, 0, wq, cq, lab[:n])


def test_both_paths_are_in_the_sweep(ctx):
    paths = {(F, k): ctx.isodata_plan(F, k)[0] for F in FS for k in KS}
    assert set(paths.values()) == {0, 1} and paths[(19, 8)] == 0 and paths[(64, 33)] == 0 and paths[(64, 64)] == 1
    ks = [k for k in range(1, 65) if ctx.isodata_plan(64, k)[0] == 0]
    assert ks == list(range(1, ks[-1] + 1)) and 33 <= ks[-1] < 64
    assert ctx.isodata_plan(65, 2) == (-1, 0) and ctx.isodata_plan(2, 65) == (-1, 0) and ctx.isodata_plan(0, 2) == (-1, 0)


@pytest.mark.parametrize("F,k", [(5, 4), (19, 8), (64, "last in LDS"), (64, "first global")])
def test_inputs_that_stress_the_contract(ctx, F, k):
    if isinstance(k, str):   # the two cluster counts on either side of the path switch at this width
        last = max(c for c in range(1, 65) if ctx.isodata_plan(F, c)[0] == 0)
        k = last if k == "last in LDS" else last + 1
        assert ctx.isodata_plan(F, k)[0] == (0 if k == last else 1)
    n = 4000 + 77
    x, pe, w, cx, q, wq, cq, lab = sweep_data(F, k, n)
    rng = np.random.default_rng(7 * F + k)
    sparse = (rng.random(n) < 0.01).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)   # a sparse ROI: whole tiles without a pixel
    collar = np.ones(n, np.uint8)
    collar[:700], collar[-900:] = 0, 0
    # one element off 16-byte alignment, with and without a mask
    _same(ctx, x, None, pe, 40, w, cx, lab, shift=1)
    _same(ctx, x, sparse, pe, 40, w, cx, lab, shift=1)
    _same(ctx, x, collar, pe, 40, w, cx, lab, shift=3)
    _same(ctx, q, sparse, None, 0, wq, cq, lab, shift=1)
    _same(ctx, q, collar, None, 0, wq, cq, lab, shift=3)
    # every pixel masked
    want = _same(ctx, x, np.zeros(n, np.uint8), pe, 40, w, cx, lab)
    assert np.all(want[0] == 255) and want[2] == 0 and not R.table_array(want[1]).any()
    # NaN reads as 0; +-inf and values beyond the stated range leave the pixel out, with label 255
    y = x.copy()
    y[rng.random(y.shape) < 0.02] = np.nan
    y[0, 5], y[F - 1, 9], y[F // 2, n - 1] = np.inf, -np.inf, np.inf
    tight = pe.copy()
    tight[0] += 2          # plane 0 is stated four times narrower than it is
    want = _same(ctx, y, None, tight, 40, w, cx, lab)
    assert 3 <= want[3] < n and int((want[0] == 255).sum()) == want[3] and sum(row[0] for row in want[1]) == n - want[3]
    _same(ctx, y, collar, tight, 40, w, cx, lab, shift=1)
    # Q at 0 and at its cap; labels_in equal to the answer: nothing changes
    _same(ctx, x, None, pe, 0, w, cx, lab)
    _same(ctx, x, None, pe, 50, w, cx, lab)
    again = _same(ctx, x, None, pe, 40, w, cx, R.sweep_ref(x, None, pe, 40, w, cx, lab)[0])
    assert again[2] == 0
    # weights of zero and centres far away
    w0 = w.copy()
    w0[::2] = 0.0
    _same(ctx, x, sparse, pe, 40, w0, cx * 1e3, lab)


def test_ties_go_to_the_lowest_index_and_run_lengths_do_not_matter(ctx):
    n = 3 * 256 + 17
    g = (np.arange(n) % 5).astype(np.float32) / 4.0                  # a coarse grid: 0, 1/4, ... 1
    x = np.stack([g, np.zeros(n, np.float32)])
    pe, w = np.array([0, 0]), np.array([1.0, 1.0])
    c = np.array([[0.75, 0.0], [0.25, 0.0], [0.75, 0.0], [0.25, 0.0]])  # 0.5 is equidistant from all four; 2 and 3 never win
    want = _same(ctx, x, None, pe, 30, w, c, np.zeros(n, np.uint8))
    assert [row[0] for row in want[1]][2:] == [0, 0] and want[0][:5].tolist() == [1, 1, 0, 0, 0]
    # labels alternating per pixel (runs of one) against blocky (runs of a tile and more)
    rng = np.random.default_rng(5)
    n = 8 * 256
    alt = np.where(np.arange(n) % 2 == 0, 0.1, 0.9).astype(np.float32)
    blocky = np.where((np.arange(n) // 600) % 2 == 0, 0.1, 0.9).astype(np.float32)
    noise = (0.01 * rng.standard_normal((2, n))).astype(np.float32)
    c2 = np.array([[0.1, 0.0], [0.9, 0.0]])
    for first in (alt, blocky):
        want = _same(ctx, np.stack([first, np.zeros(n, np.float32)]) + noise, None, pe - 1, 40, w * 2, c2 * 1.0, np.full(n, 255, np.uint8))
        assert [row[0] for row in want[1]] == [int((first < 0.5).sum()), int((first > 0.5).sum())] and want[2] == n


def test_more_tiles_than_workgroups(ctx):
    """past 2048 tiles a workgroup takes several: its table in LDS gathers them all before it is added to the global one"""
    n = 2048 * 256 * 2 + 300
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (3, n)).astype(np.float32)
    mask = (rng.random(n) < 0.9).astype(np.uint8)
    c = rng.uniform(-1, 1, (6, 3))
    want = _same(ctx, x, mask, np.zeros(3, np.int64), 40, np.ones(3), c, np.full(n, 255, np.uint8))
    assert want[2] == int(mask.sum())


def test_labels_only_leaves_a_table_untouched(ctx):
    torch = _torch()
    x, pe, w, cx, *_ = sweep_data(7, 8, 4077)
    lab = _dev(ctx, np.full(4077, 255, np.uint8))
    table = torch.full((8 * 15,), -7, dtype=torch.int64, device=ctx.device)
    from rsseg import _lib as L
    dp = [_dev(ctx, x[f]) for f in range(7)]
    changed, left = C.c_int64(-1), C.c_int64(-1)
    pe32 = pe.astype(np.int32)
    rc = ctx.lib.rsseg_isodata_sweep(ctx.h, ctx._pp(dp), 7, L.F32, 4077, None, pe32.ctypes.data_as(C.POINTER(C.c_int)), 44,
                                     w.ctypes.data_as(C.POINTER(C.c_double)), 8, np.ascontiguousarray(cx).ctypes.data_as(C.POINTER(C.c_double)),
                                     C.c_void_p(lab.data_ptr()), None, C.byref(changed), C.byref(left))
    assert rc == 0 and (changed.value, left.value) == (4077, 0)
    assert bool((table == -7).all())
    assert np.array_equal(lab.cpu().numpy(), R.sweep_ref(x, None, pe, 44, w, cx, np.full(4077, 255, np.uint8))[0])


# ---- whole runs ---------------------------------------------------------------------------------------------------------
def _same_run(a, b):
    la = a.labels.cpu().numpy() if hasattr(a.labels, "cpu") else a.labels
    assert np.array_equal(la, b.labels)
    assert a.model.centers.tobytes() == b.model.centers.tobytes() and a.model.centers.shape == b.model.centers.shape
    assert np.array_equal(a.counts, b.counts) and a.history == b.history and a.n_left_out == b.n_left_out
    assert np.array_equal(a.model.weight, b.model.weight) and np.array_equal(a.model.plane_exp, b.model.plane_exp) and a.model.Q == b.model.Q


@pytest.mark.parametrize("k_init", (1, 12))
def test_whole_runs_equal_the_runs_on_the_restatement(ctx, k_init):
    from rsseg import isodata as ISO
    from test_isodata_host import blob_run, blobs
    got = blob_run(k_init, sweep=None, ctx=ctx)
    _same_run(got, blob_run(k_init))
    assert got.model.n_clusters == 5
    X, _ = blobs()
    assert np.array_equal(got.model.predict(X, ctx=ctx), got.labels)
    # device planes in, a device plane out; the default ranges come from the planes' extrema on either side
    dev = [ctx.to_device(X[f]) for f in range(4)]
    got = ISO.isodata(dev, k_target=5, k_init=k_init, min_size=50, ctx=ctx)
    assert hasattr(got.labels, "data_ptr") and got.labels.dtype == _torch().uint8
    _same_run(got, ISO.isodata(X, k_target=5, k_init=k_init, min_size=50, sweep=R.ref_sweep))


def test_a_whole_run_on_masked_uint8_planes(ctx):
    from rsseg import isodata as ISO
    rng = np.random.default_rng(21)
    H, W = 72, 90
    cls = (np.arange(H)[:, None] // 24) * 2 + (np.arange(W)[None, :] // 45)          # six fields
    lev = rng.integers(30, 226, (6, 7))
    img = np.clip(lev[cls].transpose(2, 0, 1) + rng.integers(-6, 7, (7, H, W)), 0, 255).astype(np.uint8)
    mask = np.ones((H, W), np.uint8)
    mask[:5], mask[:, -7:] = 0, 0
    kw = dict(k_target=6, k_init=3, min_size=30, max_std=0.05, min_dist=0.08, mask=mask)
    got = ISO.isodata(img, ctx=ctx, **kw)
    _same_run(got, ISO.isodata(img, sweep=R.ref_sweep, **kw))
    assert got.labels.shape == (H, W) and np.all(got.labels[mask == 0] == 255) and got.counts.sum() == int(mask.sum())
    assert got.model.dtype == "uint8" and np.array_equal(got.model.predict(img, mask=mask, ctx=ctx), got.labels)


# ---- the stage ------------------------------------------------------------------------------------------------------------
def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def test_cli_end_to_end(ctx, golden_dir, tmp_path):
    from rsseg import isodata as ISO
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    image = str(tmp_path / "in.tif")
    geo = dict(transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    write_tiff(image, np.ascontiguousarray(crop["bands"]), **geo)
    assert stages.main([image, str(tmp_path / "before"), "--classify", "kmeans", "--n-clusters", "5"]) == 0
    out = tmp_path / "iso"
    assert stages.main([image, str(out), "--classify", "isodata", "--n-clusters", "5", "--isodata-init-clusters", "3", "--isodata-min-size", "40",
                        "--isodata-iterations", "8", "--sieve", "4", "--signatures"]) == 0
    sdir = out / "segmentation_results"
    for f in ("classification_isodata.npy", "isodata_classification_map.tif", "isodata_model.npz", "isodata_history.json", "classification_isodata_clean.npy",
              "signatures_isodata.npz", "separability_isodata.json"):
        assert (sdir / f).exists(), f
    cm = np.load(sdir / "classification_isodata.npy")
    feats = stages._load_normalised(str(out / "feature_outputs" / "all_features_and_metadata.pkl"), str(tmp_path / "scratch"))
    planes, names = stages.isodata_planes(feats)
    res = ISO.isodata(planes, k_target=5, k_init=3, min_size=40, max_iter=8, ctx=ctx)
    assert cm.dtype == np.uint8 and cm.shape == res.labels.shape and np.array_equal(cm, res.labels + 1) and cm.min() >= 1
    assert np.array_equal(read_tiff(str(sdir / "isodata_classification_map.tif"))[0], cm)
    hist = json.load(open(sdir / "isodata_history.json"))
    assert hist["history"] == res.history and hist["counts"] == res.counts.tolist() and hist["n_clusters"] == res.model.n_clusters
    model = ISO.IsodataModel.load(sdir / "isodata_model.npz")
    assert model.centers.tobytes() == res.model.centers.tobytes() and model.feature_names == list(names)
    # the saved model applied by the command line gives the same map
    assert stages.main([image, str(tmp_path / "applied"), "--classify", "isodata", "--isodata-model", str(sdir / "isodata_model.npz")]) == 0
    assert np.array_equal(np.load(tmp_path / "applied" / "segmentation_results" / "classification_isodata.npy"), cm)
    # --mask-nodata: the mask goes to the sweep, class 0 outside it
    nod = crop["bands"].astype(np.float32).copy()
    nod[:, :9, :] = -9999.0
    write_tiff(str(tmp_path / "nod.tif"), nod, **geo)
    assert stages.main([str(tmp_path / "nod.tif"), str(tmp_path / "masked"), "--classify", "isodata", "--n-clusters", "4", "--mask-nodata", "-9999"]) == 0
    mm = np.load(tmp_path / "masked" / "segmentation_results" / "classification_isodata.npy")
    assert np.all(mm[:9] == 0) and np.all(mm[9:] >= 1)
    # the k-means command writes what it wrote before
    assert stages.main([image, str(tmp_path / "after"), "--classify", "kmeans", "--n-clusters", "5"]) == 0
    for sub in ("segmentation_results", "feature_outputs"):
        a, b = _files(tmp_path / "before" / sub), _files(tmp_path / "after" / sub)
        assert list(a) == list(b) and [f for f in a if a[f] != b[f]] == [], sub


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_error_codes_name_the_argument(ctx):
    from rsseg import _lib as L
    from rsseg.runtime import RssegUnsupported
    torch = _torch()
    n = 300
    x = [_dev(ctx, np.zeros(n, np.float32)) for _ in range(2)]
    lab = _dev(ctx, np.zeros(n, np.uint8))
    table = torch.zeros(4 * 5 + 1, dtype=torch.int64, device=ctx.device)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def call(planes=x, F=2, dtype=L.F32, n=n, pe=(0, 0), Q=40, w=(1.0, 1.0), k=4, cen=None, labels=lab, tab=table.data_ptr(), chg=True, left=True):
        pe_a = None if pe is None else np.array(pe, np.int32)
        w_a = None if w is None else np.array(w, np.float64)
        c_a = np.zeros(max(k, 1) * max(F, 1)) if cen is None else np.array(cen, np.float64)
        a, b = C.c_int64(0), C.c_int64(0)
        rc = ctx.lib.rsseg_isodata_sweep(ctx.h, ctx._pp(planes) if planes is not None else None, F, dtype, n, None,
                                         None if pe_a is None else pe_a.ctypes.data_as(ip), Q, None if w_a is None else w_a.ctypes.data_as(dp), k,
                                         None if cen is False else c_a.ctypes.data_as(dp), None if labels is None else C.c_void_p(labels.data_ptr()),
                                         None if tab is None else C.c_void_p(tab), C.byref(a) if chg else None, C.byref(b) if left else None)
        return rc, ctx.lib.rsseg_last_error(ctx.h).decode()

    assert call()[0] == 0
    for kw, code, word in [(dict(planes=None), -1, "d_planes"), (dict(F=0), -1, "d_planes"), (dict(k=0), -1, "k="), (dict(dtype=L.F64), -1, "dtype"),
                           (dict(n=-1), -1, "n_local"), (dict(Q=-1), -1, "Q="), (dict(Q=51), -1, "Q="), (dict(n=1 << 40, Q=30), -1, "n_local"),
                           (dict(pe=None), -1, "plane_exp"), (dict(pe=(0, 301)), -1, "plane_exp[1]"), (dict(dtype=L.U8), -1, "RSSEG_U8"),
                           (dict(dtype=L.U8, pe=None), -1, "RSSEG_U8"), (dict(w=None), -1, "weight"), (dict(w=(1.0, float("inf"))), -1, "weight[1]"),
                           (dict(cen=False), -1, "centers"), (dict(cen=[0, 0, 0, 0, 0, float("nan"), 0, 0]), -1, "centers[2][1]"),
                           (dict(labels=None), -1, "d_labels"), (dict(tab=table.data_ptr() + 4), -1, "d_table"), (dict(chg=False), -1, "n_changed"),
                           (dict(left=False), -1, "n_left_out"), (dict(planes=[x[0], None]), -1, "d_planes[1]"),
                           (dict(planes=[x[0], _dev(ctx, np.zeros(2 * n, np.float32)).view(torch.uint8)[2:]]), -1, "d_planes[1]"),
                           (dict(F=65), -5, "F=65"), (dict(k=65), -5, "k=65")]:
        rc, msg = call(**kw)
        assert rc == code and msg.startswith("isodata_sweep:") and word in msg, (kw, rc, msg)
    # the Python layer: ValueError and RssegUnsupported
    with pytest.raises(ValueError):
        ctx.isodata_sweep(x, lab, np.zeros((4, 3)), np.ones(2), [0, 0], 40)
    with pytest.raises(ValueError):
        ctx.isodata_sweep(x, lab[:-1], np.zeros((4, 2)), np.ones(2), [0, 0], 40)
    with pytest.raises(ValueError):
        ctx.isodata_sweep(x, lab, np.zeros((4, 2)), np.ones(2), None, 40)
    with pytest.raises(RssegUnsupported):
        ctx.isodata_sweep(x, lab, np.zeros((65, 2)), np.ones(2), [0, 0], 40)
    # n_local = 0 with null planes: zeros
    table.fill_(-1)
    rc, _ = call(planes=[None, None], n=0, labels=None)
    assert rc == 0 and bool((table[:20] == 0).all()) and int(table[20]) == -1
