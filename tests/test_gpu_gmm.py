"""K29 on the GPU: rsseg_gmm_sweep equals the restatement (tests/gmm_ref.py) bit for bit over the register widths, component
counts, plane types, both covariance forms, both paths and the pixel counts around the tile seams; the inputs that stress the
contract; the labels against K22's; whole fits against the fits on the restatement; the error codes."""
import functools

import numpy as np
import pytest

import gmm_ref as R

from rsseg import gmm as G

pytestmark = pytest.mark.gpu

FS = (1, 3, 8, 9, 19, 24, 25, 33, 64)
KS = (1, 2, 8, 9, 32)
# every width at two components, every component count at nine planes, two wider pairs on Path A, and the pairs whose full
# table does not fit in LDS (Path B) at each of the register widths 24, 32 and 64 (twice at 32); at 64 planes five components
# are enough for that.  (64, 32) is the one pair whose DIAG table does not fit: it runs in that form alone, its full form
# would cost the restatement ten seconds per plane type and launches the kernels that (64, 5) launches.
PATH_B = ((24, 32), (25, 32), (33, 32), (64, 5))
DIAG_PATH_B = (64, 32)
PAIRS = sorted({(F, 2) for F in FS} | {(9, k) for k in KS} | {(25, 8), (24, 9), DIAG_PATH_B} | set(PATH_B))


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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(ctx, planes, mask, pe, Q, mean, whiten, offset, diag, shift=0, want=None):
    """The sweep with a table and every output, and the sweep without a table, against the restatement."""
    if want is None:
        want = R.sweep_ref(planes, mask, pe, Q, mean, whiten, offset, diag)
    F, k = planes.shape[0], mean.shape[0]
    dp = [_dev(ctx, planes[f], shift) for f in range(F)]
    dm = None if mask is None else _dev(ctx, mask, shift)
    km = dict(mean=mean, whiten=whiten, offset=offset, plane_exp=pe, Q=Q, diag=diag)
    for want_table in (True, False):
        o = ctx.gmm_sweep(dp, km, mask=dm, want_table=want_table, want_labels=True, want_posterior=True, want_loglik=True, want_proba=True)
        for key in ("n_counted", "n_left_out", "n_far", "ll_sum"):
            assert o[key] == want[key], (want_table, key, o[key], want[key])
        assert np.array_equal(o["labels"].cpu().numpy(), want["labels"]), want_table
        for key in ("posterior", "loglik", "proba"):
            got = o[key].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want[key])), (want_table, key, np.argwhere(_bits(got) != _bits(want[key]))[:5])
        if want_table:
            t = o["table"].cpu().numpy()
            ref = R.table_array(want["table"])
            assert t.dtype == np.int64 and t.shape == (k, R.n_columns(F, diag)) and np.array_equal(t, ref), np.argwhere(t != ref)[:5]
        else:
            assert o["table"] is None
    o = ctx.gmm_sweep(dp, km, mask=dm, want_table=False, want_labels=True)   # the outputs are optional one by one
    assert o["posterior"] is None and o["proba"] is None and np.array_equal(o["labels"].cpu().numpy(), want["labels"])
    return want


@functools.lru_cache(maxsize=None)
def sweep_data(F, k, n, seed=0):
    """float32 planes of scales 2^-7 ... 2^6 with their exponents, their uint8 twins, and a model in u units for each: means
    among the pixels, lower-triangular W with a dominant diagonal, offsets around 0"""
    rng = np.random.default_rng(1000 * F + k + seed)
    x = (rng.uniform(-1, 1, (F, n)) * 2.0 ** rng.integers(-7, 7, (F, 1))).astype(np.float32)
    b = rng.integers(0, 256, (F, n)).astype(np.uint8)
    pe = _exp_of(x)
    pick = rng.integers(0, n, k)
    W = np.tril(rng.normal(size=(k, F, F)) * 0.4 / np.sqrt(F)) + np.eye(F) * rng.uniform(0.7, 1.6, (k, F, 1))
    mean = np.ldexp(x[:, pick].astype(np.float64), pe.reshape(F, 1)).T + 0.05 * rng.standard_normal((k, F))
    mean_b = b[:, pick].astype(np.float64).T + 8.0 * rng.standard_normal((k, F))
    offset = rng.normal(size=k)
    return x, pe, mean, R.pack_lower(W), offset, b, mean_b, R.pack_lower(W / 48.0)


def test_both_paths_are_reached(ctx):
    plans = {(F, k, d): ctx.gmm_plan(F, k, diag=d) for F, k in PAIRS for d in (False, True)}
    assert all(tile == 256 and path in (0, 1) for path, tile in plans.values())
    assert all(plans[(F, k, False)][0] == (1 if (F, k) in PATH_B + (DIAG_PATH_B,) else 0) for F, k in PAIRS)
    assert all(plans[(F, k, True)][0] == (1 if (F, k) == DIAG_PATH_B else 0) for F, k in PAIRS)
    assert ctx.gmm_plan(64, 4)[0] == 0
    assert all(ctx.gmm_plan(F, k, u8=True, diag=d) == plans[(F, k, d)] for F, k, d in plans)
    assert ctx.gmm_plan(65, 2)[0] == -1 and ctx.gmm_plan(8, 33)[0] == -1 and ctx.gmm_plan(9, 8, u8=True) == ctx.gmm_plan(9, 8)


@pytest.mark.parametrize("F,k", PAIRS)
def test_sweep_equals_the_restatement(ctx, F, k):
    n = 257   # two workgroups
    x, pe, mean, wh, off, b, mean_b, wh_b = sweep_data(F, k, n)
    if (F, k) != DIAG_PATH_B:
        want = _same(ctx, x, None, pe, 20, mean, wh, off, False)
        assert want["n_counted"] == n and (np.asarray(want["q"]) != 0).sum(axis=0).max() >= min(k, 2)   # soft: pixels with two components
        _same(ctx, b, None, None, 20, mean_b, wh_b, off, False)
    _same(ctx, x, None, pe, 20, mean, wh, off, True)
    _same(ctx, b, None, None, 20, mean_b, wh_b, off, True)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5])
def test_pixel_counts_at_the_seams(ctx, n):
    x, pe, mean, wh, off, b, mean_b, wh_b = sweep_data(3, 3, n)
    mask = (np.arange(n) % 5 != 1).astype(np.uint8)
    _same(ctx, x, None, pe, G.q_for(n), mean, wh, off, False, shift=1)   # plane starts 4 bytes off the alignment
    _same(ctx, x, mask, pe, G.q_for(n), mean, wh, off, True, shift=3)
    _same(ctx, b, mask, None, G.q_for(n), mean_b, wh_b, off, False, shift=1)


def test_inputs_that_stress_the_contract(ctx):
    F, k, n = 4, 3, 700
    x, pe, mean, wh, off, *_ = sweep_data(F, k, n, seed=1)
    x = x.copy()
    pe = _exp_of(x)
    x[1, 5] = np.nan                      # read as +0
    x[2, 300] = np.nan
    x[0, 7] = 2.0 ** (1 - pe[0])          # |u| = 2: left out
    x[3, 8] = np.inf                      # left out
    x[1, 9] = -np.inf
    x[:, 256:300] = 0.0                   # a run of identical pixels
    mask = np.ones(n, np.uint8)
    mask[10:20] = 0
    mask[512:] = 0                        # a whole tile without a counted pixel
    mask[600] = 1
    off = off.copy()
    off[2] = 1.0e4                        # a component so far away that every q is 0
    want = _same(ctx, x, mask, pe, 20, mean, wh, off, False)
    assert want["n_left_out"] == 3 and want["n_counted"] == 512 - 10 - 3 + 1
    assert want["table"][2] == [0] * R.n_columns(F, False) and not np.any(want["q"][2])
    assert want["labels"][7] == want["labels"][8] == want["labels"][9] == want["labels"][15] == 0 and want["labels"][5] > 0
    _same(ctx, x, mask, pe, 20, mean, wh, off, True)
    # two components with the same parameters: the lowest wins and each takes q = 2^19
    mean2, wh2, off2 = np.stack([mean[0], mean[0]]), np.stack([wh[0], wh[0]]), np.array([off[0], off[0]])
    want = _same(ctx, x, mask, pe, 20, mean2, wh2, off2, False)
    assert np.all(want["q"] == 2 ** 19) and np.all(want["labels"][want["keep"]] == 1) and want["table"][0] == want["table"][1]
    assert np.all(want["posterior"][want["keep"]] == np.float32(0.5))
    # a pixel far from every component: ll is far below zero but finite, nothing is lost
    want = _same(ctx, x, None, pe, 20, mean, wh * 300.0, off, False)
    assert want["n_far"] == 0 and np.nanmin(want["loglik"]) < -1000.0
    want = _same(ctx, x, None, pe, 20, mean, wh * 3.0e4, off, False)
    assert want["n_far"] > 0


def test_labels_equal_the_gaussian_classifier(ctx):
    F, k, n = 6, 5, 3000
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (F, n)).astype(np.float32)
    pe = _exp_of(x)
    assert not pe.any()
    W = np.tril(rng.normal(size=(k, F, F)) * 0.3) + np.eye(F) * 1.2
    mean, off = rng.uniform(-0.6, 0.6, (k, F)), rng.normal(size=k)
    dp = [_dev(ctx, x[f]) for f in range(F)]
    o = ctx.gmm_sweep(dp, dict(mean=mean, whiten=R.pack_lower(W), offset=off, plane_exp=pe, Q=20, diag=False), want_table=False, want_labels=True)
    lab, _, _ = ctx.gauss_classify(dp, mean, R.pack_lower(W), off, np.arange(1, k + 1))
    assert np.array_equal(o["labels"].cpu().numpy(), lab.cpu().numpy()) and len(np.unique(lab.cpu().numpy())) == k
    # the same through the public classes: the mixture's weights as the priors of an 'ml' model
    cov = np.stack([np.linalg.inv(w.T @ w) for w in W])
    wts = np.full(k, 1.0 / k)
    m = G.GaussianMixtureModel.from_params(wts, mean, cov, "full", plane_exp=pe)
    got = m.predict(dp, ctx=ctx).cpu().numpy()
    gc = m.to_gaussian_classifier()
    lab2, _, _ = ctx.gauss_classify(dp, gc.mean_, gc.whiten_, gc.offset_, gc.class_values_)
    assert np.array_equal(got, lab2.cpu().numpy())


def _blobs():
    import test_gmm_host as H
    return np.array(H.overlapping()[0][:, :48 * 40]), H.start()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ct", ["full", "diag"])
def test_fit_equals_the_fit_on_the_restatement(ctx, ct, masked):
    P, (w0, mu0, cov0) = _blobs()
    perm = np.random.default_rng(2).permutation(P.shape[1])
    P = np.ascontiguousarray(P[:, perm])
    mask = (np.arange(P.shape[1]) % 7 != 0).astype(np.uint8).reshape(48, 40) if masked else None
    cov = cov0 if ct == "full" else np.stack([np.diag(c) for c in cov0])
    fits = []
    for sweep in (None, R.ref_sweep):
        m = G.GaussianMixtureModel(3, ct, tol=1e-3, reg_covar=1e-6, max_iter=12, init=(w0, mu0, cov))
        res = m.fit(P.reshape(5, 48, 40), mask=mask, ctx=ctx if sweep is None else None, sweep=sweep, keep_tables=True)
        fits.append((m, res))
    (a, ra), (b, rb) = fits
    assert a.n_iter_ == b.n_iter_ >= 3 and a.converged_ == b.converged_
    assert a.tables_ == b.tables_
    assert np.array_equal(a.weights_, b.weights_) and np.array_equal(a.means_, b.means_) and np.array_equal(a.covariances_, b.covariances_)
    assert ra.labels.shape == (48, 40) and np.array_equal(ra.labels, rb.labels) and ra.n_left_out == rb.n_left_out == 0
    assert ra.history == rb.history
    assert a.score(P, ctx=ctx) == b.score(P, sweep=R.ref_sweep)


def test_fit_from_a_kmeans_start_and_the_selection(ctx):
    P, _ = _blobs()
    m = G.GaussianMixtureModel(3, "full", max_iter=25, init="kmeans", random_state=3)
    res = m.fit(P.reshape(5, 48, 40), ctx=ctx)
    again = G.GaussianMixtureModel(3, "full", max_iter=25, init="kmeans", random_state=3).fit(P.reshape(5, 48, 40), ctx=ctx)
    assert np.array_equal(res.labels, again.labels) and np.array_equal(res.model.means_, again.model.means_)   # no other random number
    assert res.labels.dtype == np.uint8 and set(np.unique(res.labels)) == {1, 2, 3} and abs(res.weights.sum() - 1.0) < 1e-12
    lb = [h["lower_bound"] for h in res.history]
    assert all(y >= x - 1e-6 for x, y in zip(lb, lb[1:]))
    table, best = G.select_components(P, (1, 3), ctx=ctx, covariance_type="diag", max_iter=10, init="kmeans", random_state=0)
    assert [r["k"] for r in table] == [1, 3] and table[1]["bic"] < table[0]["bic"] and best.n_components == 3
    proba = m.predict_proba(P.reshape(5, 48, 40), ctx=ctx)
    assert proba.shape == (3, 48, 40) and np.allclose(proba.sum(axis=0), 1.0, atol=1e-6)
    assert np.array_equal(proba.argmax(axis=0) + 1, res.labels) or (np.sort(proba, axis=0)[-1] - np.sort(proba, axis=0)[-2]).min() == 0


def test_fit_from_an_isodata_start(ctx):
    P, _ = _blobs()
    from rsseg import isodata as ISO
    m = G.GaussianMixtureModel(3, "diag", max_iter=10, init="isodata")
    res = m.fit(P.reshape(5, 48, 40), ctx=ctx)
    iso = ISO.isodata([ctx.to_device(np.ascontiguousarray(p)) for p in P], k_target=3, k_max=3, ctx=ctx)
    k_iso = iso.model.n_clusters
    assert 1 <= k_iso <= 3   # k_max = n_components: never more clusters than components
    # a component ISODATA gave no cluster is dropped in the first iteration's record; nothing else is
    assert len(res.history[0]["dropped"]) >= 3 - k_iso and m.n_components <= k_iso and len(res.weights) == m.n_components
    assert res.labels.max() <= m.n_components and res.labels.min() >= 1 and abs(res.weights.sum() - 1.0) < 1e-12
    again = G.GaussianMixtureModel(3, "diag", max_iter=10, init="isodata").fit(P.reshape(5, 48, 40), ctx=ctx)
    assert np.array_equal(again.labels, res.labels)


def test_error_codes(ctx):
    x, pe, mean, wh, off, *_ = sweep_data(3, 3, 4097)
    dp = [_dev(ctx, x[f]) for f in range(3)]
    km = dict(mean=mean, whiten=wh, offset=off, plane_exp=pe, Q=20, diag=False)
    with pytest.raises(ValueError, match="Q=31"):
        ctx.gmm_sweep(dp, dict(km, Q=31))
    with pytest.raises(ValueError, match="passes 2\\^62"):
        ctx.gmm_sweep(dp, dict(km, Q=30))   # 4097 pixels: Q <= 29
    with pytest.raises(RuntimeError, match="at most 32"):
        ctx.gmm_sweep(dp, dict(km, mean=np.zeros((33, 3)), whiten=np.zeros((33, 6)), offset=np.zeros(33)))
    with pytest.raises(RuntimeError, match="at most 64"):
        ctx.gmm_sweep(dp[:1] * 65, dict(km, mean=np.zeros((1, 65)), whiten=np.zeros((1, 65 * 33)), offset=np.zeros(1), plane_exp=np.zeros(65, int)))
    with pytest.raises(ValueError, match="not finite"):
        ctx.gmm_sweep(dp, dict(km, offset=np.array([0.0, np.nan, 0.0])))
    with pytest.raises(ValueError, match="plane_exp is null"):
        ctx.gmm_sweep(dp, dict(km, plane_exp=None))
    with pytest.raises(ValueError, match="all be float32 or all uint8"):
        ctx.gmm_sweep([dp[0], dp[1], _dev(ctx, np.zeros(4097, np.uint8))], km)
    with pytest.raises(ValueError, match="do not describe"):
        ctx.gmm_sweep(dp, dict(km, whiten=wh[:, :5]))
    o = ctx.gmm_sweep(dp, km)   # the context is usable after a refusal
    assert o["n_counted"] == 4097


# ---- the stage ------------------------------------------------------------------------------------------------------------
def _files(d):
    import os
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def test_cli_end_to_end(ctx, golden_dir, tmp_path):
    import json
    import os
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    image = str(tmp_path / "in.tif")
    geo = dict(transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    write_tiff(image, np.ascontiguousarray(crop["bands"]), **geo)
    assert stages.main([image, str(tmp_path / "before"), "--classify", "kmeans", "--n-clusters", "5"]) == 0
    out = tmp_path / "gmm"
    assert stages.main([image, str(out), "--classify", "gmm", "--n-clusters", "4", "--gmm-covariance", "diag", "--gmm-iterations", "6", "--gmm-tol", "0",
                        "--gmm-posterior", "--sieve", "4", "--signatures"]) == 0
    sdir = out / "segmentation_results"
    for f in ("classification_gmm.npy", "gmm_classification_map.tif", "gmm_model.npz", "gmm_history.json", "gmm_posterior.npy", "gmm_loglik.npy",
              "classification_gmm_clean.npy", "signatures_gmm.npz", "separability_gmm.json"):
        assert (sdir / f).exists(), f
    cm = np.load(sdir / "classification_gmm.npy")
    feats = stages._load_normalised(str(out / "feature_outputs" / "all_features_and_metadata.pkl"), str(tmp_path / "scratch"))
    planes, names = stages.isodata_planes(feats)
    m = G.GaussianMixtureModel(4, "diag", tol=0.0, max_iter=6, init="kmeans", random_state=42)
    res = m.fit(planes, ctx=ctx)
    assert cm.dtype == np.uint8 and cm.shape == (96, 96) and np.array_equal(cm, res.labels) and cm.min() >= 1 and cm.max() <= 4
    assert np.array_equal(read_tiff(str(sdir / "gmm_classification_map.tif"))[0], cm)
    hist = json.load(open(sdir / "gmm_history.json"))
    assert hist["history"] == res.history and hist["n_iter"] == 6 and hist["covariance"] == "diag" and hist["feature_names"] == list(names)
    assert sum(hist["counts"]) == cm.size and hist["n_left_out"] == 0
    saved = G.GaussianMixtureModel.load(sdir / "gmm_model.npz")
    assert saved.means_.tobytes() == m.means_.tobytes() and saved.covariances_.tobytes() == m.covariances_.tobytes()
    post, ll = np.load(sdir / "gmm_posterior.npy"), np.load(sdir / "gmm_loglik.npy")
    assert post.dtype == ll.dtype == np.float32 and post.shape == ll.shape == cm.shape and post.min() >= 1.0 / 4 - 1e-6 and post.max() <= 1.0
    assert np.all(np.isfinite(ll))
    # the saved model applied by the command line gives the same map
    assert stages.main([image, str(tmp_path / "applied"), "--classify", "gmm", "--gmm-model", str(sdir / "gmm_model.npz")]) == 0
    assert np.array_equal(np.load(tmp_path / "applied" / "segmentation_results" / "classification_gmm.npy"), cm)
    assert not (tmp_path / "applied" / "segmentation_results" / "gmm_posterior.npy").exists()
    applied = json.load(open(tmp_path / "applied" / "segmentation_results" / "gmm_history.json"))
    assert applied["n_clusters"] == applied["n_components"] == 4 and applied["fitted"] is False   # the model's count, not --n-clusters' default
    # --mask-nodata: the mask goes to the sweep, class 0 outside it
    nod = crop["bands"].astype(np.float32).copy()
    nod[:, :9, :] = -9999.0
    write_tiff(str(tmp_path / "nod.tif"), nod, **geo)
    assert stages.main([str(tmp_path / "nod.tif"), str(tmp_path / "masked"), "--classify", "gmm", "--n-clusters", "3", "--gmm-covariance", "spherical",
                        "--gmm-iterations", "4", "--mask-nodata", "-9999", "--gmm-posterior"]) == 0
    mm = np.load(tmp_path / "masked" / "segmentation_results" / "classification_gmm.npy")
    assert np.all(mm[:9] == 0) and np.all(mm[9:] >= 1)
    assert np.all(np.isnan(np.load(tmp_path / "masked" / "segmentation_results" / "gmm_posterior.npy")[:9]))
    # the k-means command writes what it wrote before
    assert stages.main([image, str(tmp_path / "after"), "--classify", "kmeans", "--n-clusters", "5"]) == 0
    for sub in ("segmentation_results", "feature_outputs"):
        a, b = _files(tmp_path / "before" / sub), _files(tmp_path / "after" / sub)
        assert list(a) == list(b) and [f for f in a if a[f] != b[f]] == [], sub
