"""K26 without a GPU: rsseg.isodata on the restatement of the sweep (tests/isodata_ref.py supplies what the kernel would):
the driver recovers blobs from several starts, splits, merges and drops where it should, the model predicts, saves and
loads, the restated table agrees with K24's restatement and adds over stripes; the argument errors."""
import functools
import os

import numpy as np
import pytest

import isodata_ref as R
import moments_ref as M

from rsseg import isodata as ISO
from rsseg import signatures as SIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def blobs():
    """five blobs of sigma 0.03 in [0, 1]^4, 3000 / 2500 / 2000 / 1500 / 1000 pixels, shuffled -> ((4, n) float32, blob of every pixel)"""
    rng = np.random.default_rng(7)
    cen = rng.uniform(0.15, 0.85, (5, 4))
    sizes = [3000, 2500, 2000, 1500, 1000]
    X = np.vstack([c + 0.03 * rng.standard_normal((s, 4)) for c, s in zip(cen, sizes)]).astype(np.float32)
    y = np.repeat(np.arange(5), sizes)
    perm = rng.permutation(y.size)
    X, y = X[perm], y[perm]
    X.setflags(write=False)
    return np.ascontiguousarray(X.T), y


def blob_run(k_init, sweep=R.ref_sweep, **kw):
    X, _ = blobs()
    return ISO.isodata(X, k_target=5, k_init=k_init, min_size=50, max_std=0.06, min_dist=0.1, ranges=[(0, 1)] * 4, sweep=sweep, **kw)


def test_header_symbols_are_exported():
    lib_path = os.path.join(ROOT, "rs-image-segmentation_amd", "librsseg_hip.so")
    if not os.path.exists(lib_path):
        pytest.skip("librsseg_hip.so is not built")
    import ctypes as C
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    lib = C.CDLL(lib_path)
    for name in ("rsseg_isodata_sweep", "rsseg_isodata_plan"):
        assert name + "(" in hdr and hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rsseg_isodata_sweep"][1]) == 15 and _lib.SIGNATURES["rsseg_isodata_plan"][0] is None


@pytest.mark.parametrize("k_init", (1, 2, 5, 12))
def test_blobs_are_recovered_from_every_start(k_init):
    _, y = blobs()
    res = blob_run(k_init)
    assert res.model.n_clusters == 5 and len(res.history) <= 5 and res.n_left_out == 0
    assert [len(set(y[res.labels == j].tolist())) for j in range(5)] == [1] * 5
    assert sorted(res.counts.tolist()) == [1000, 1500, 2000, 2500, 3000]
    assert set(res.history[0]) == {"k", "dropped", "split", "merged", "n_changed"} and res.history[0]["n_changed"] == y.size


def test_the_starts_exercise_drop_split_and_merge():
    h = [e for k_init in (1, 2, 5, 12) for e in blob_run(k_init).history]
    assert sum(e["dropped"] for e in h) > 0 and sum(e["split"] for e in h) > 0 and sum(e["merged"] for e in h) > 0


def test_an_elongated_cluster_is_split_along_its_widest_plane():
    rng = np.random.default_rng(11)
    X = np.stack([0.5 + 0.01 * rng.standard_normal(4000), rng.uniform(0.1, 0.9, 4000), 0.5 + 0.01 * rng.standard_normal(4000)]).astype(np.float32)
    res = ISO.isodata(X, k_target=2, k_init=1, min_size=10, max_std=0.06, min_dist=0.05, max_iter=2, ranges=[(0, 1)] * 3, sweep=R.ref_sweep)
    assert res.history[0]["split"] == 1 and res.model.n_clusters == 2
    c = res.model.centers_in_feature_units()
    assert abs(c[0, 1] - c[1, 1]) > 0.2 and abs(c[0, 0] - c[1, 0]) < 0.01 and abs(c[0, 2] - c[1, 2]) < 0.01
    assert c[0, 1] < c[1, 1]   # c_j - gamma sigma stays at j, c_j + gamma sigma is appended


def test_two_close_blobs_are_merged():
    rng = np.random.default_rng(12)
    cen = np.array([[0.30, 0.30], [0.34, 0.30], [0.80, 0.80]])
    X = np.vstack([c + 0.01 * rng.standard_normal((1500, 2)) for c in cen]).astype(np.float32)
    res = ISO.isodata(np.ascontiguousarray(X.T), k_target=3, min_size=10, max_std=0.06, min_dist=0.1, init=cen, ranges=[(0, 1)] * 2, sweep=R.ref_sweep)
    assert res.model.n_clusters == 2 and sum(e["merged"] for e in res.history) == 1 and sorted(res.counts.tolist()) == [1500, 3000]


def test_a_cluster_below_min_size_disappears():
    rng = np.random.default_rng(13)
    cen = np.array([[0.2, 0.2], [0.8, 0.8], [0.2, 0.8]])
    X = np.vstack([c + 0.01 * rng.standard_normal((s, 2)) for c, s in zip(cen, (2000, 2000, 30))]).astype(np.float32)
    res = ISO.isodata(np.ascontiguousarray(X.T), k_target=3, min_size=50, max_std=0.5, min_dist=0.01, init=cen, ranges=[(0, 1)] * 2, sweep=R.ref_sweep)
    assert res.history[0]["dropped"] == 1 and res.model.n_clusters == 2 and res.counts.sum() == 4030


def test_a_constant_plane_has_weight_zero():
    X, _ = blobs()
    Xc = np.vstack([X[:2], np.full((1, X.shape[1]), 3.25, np.float32), X[2:]])
    res = ISO.isodata(Xc, k_target=5, min_size=50, sweep=R.ref_sweep)
    assert res.model.weight[2] == 0.0 and np.all(res.model.weight[[0, 1, 3, 4]] > 0)
    assert np.all(res.model.centers[:, 2] == 0.0) and np.all(res.model.centers_in_feature_units()[:, 2] == 3.25)
    assert np.array_equal(res.model.ranges[2], [3.25, 3.25])


def test_one_iteration_splits_and_merges_nothing():
    for k_init in (1, 12):
        res = blob_run(k_init, max_iter=1)
        assert len(res.history) == 1 and res.history[0]["split"] == 0 and res.history[0]["merged"] == 0


def test_predict_equals_the_returned_labels_and_the_model_survives_a_file(tmp_path):
    X, _ = blobs()
    mask = (np.arange(X.shape[1]) % 7 != 0).astype(np.uint8)
    res = blob_run(2, mask=mask)
    assert np.all(res.labels[mask == 0] == 255) and np.all(res.labels[mask != 0] < res.model.n_clusters)
    assert np.array_equal(res.model.predict(X, mask=mask, sweep=R.ref_sweep), res.labels)
    assert np.array_equal(np.bincount(res.labels[mask != 0], minlength=res.model.n_clusters), res.counts)
    res.model.feature_names = ["a", "b", "c", "d"]
    m2 = ISO.IsodataModel.load(res.model.save(tmp_path / "model"))
    for name in ("centers", "weight", "plane_exp", "ranges"):
        assert np.array_equal(getattr(m2, name), getattr(res.model, name)) and getattr(m2, name).dtype == getattr(res.model, name).dtype
    assert (m2.Q, m2.dtype, m2.feature_names) == (res.model.Q, "float32", ["a", "b", "c", "d"])
    assert np.array_equal(m2.predict(X, mask=mask, sweep=R.ref_sweep), res.labels)
    with pytest.raises(ValueError):
        m2.predict(X[:3], sweep=R.ref_sweep)
    with pytest.raises(ValueError):
        m2.predict((X * 255).astype(np.uint8), sweep=R.ref_sweep)


def test_two_calls_give_identical_results():
    a, b = blob_run(12), blob_run(12)
    assert np.array_equal(a.labels, b.labels) and a.model.centers.tobytes() == b.model.centers.tobytes()
    assert a.history == b.history and np.array_equal(a.counts, b.counts)


def test_uint8_planes_and_an_image_shaped_stack():
    rng = np.random.default_rng(14)
    img = np.zeros((3, 40, 50), np.uint8)
    img[:, :, :25] = np.array([40, 200, 90], np.uint8)[:, None, None]
    img[:, :, 25:] = np.array([180, 60, 90], np.uint8)[:, None, None]
    img = (img + rng.integers(0, 6, img.shape)).astype(np.uint8)
    res = ISO.isodata(img, k_target=2, min_size=10, ranges=[(0, 255)] * 3, sweep=R.ref_sweep)   # the noise is small against 255
    assert res.labels.shape == (40, 50) and res.model.dtype == "uint8" and res.model.Q == 0 and not res.model.plane_exp.any()
    assert res.model.n_clusters == 2 and len(set(res.labels[:, :25].ravel().tolist())) == 1 and res.labels[0, 0] != res.labels[0, 49]
    assert np.allclose(res.model.centers_in_feature_units()[res.labels[0, 0]], [42.5, 202.5, 92.5], atol=0.5)


def sweep_case(F=5, k=4, n=1500, seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((F, n)) * 2.0 ** rng.integers(-5, 5, (F, 1))).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    x[0, 7], x[F - 1, 11] = np.inf, -np.inf
    pe = np.array([SIG.exponent_for(np.abs(np.where(np.isfinite(x[f]), x[f], 0)).max()) for f in range(F)])
    pe[1] += 1   # plane 1 is stated twice narrower than it is: pixels are left out
    weight = rng.uniform(0.5, 2.0, F)
    centers = rng.uniform(-0.5, 0.5, (k, F)) * weight
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    return x, mask, pe, weight, centers, rng.integers(0, k, n).astype(np.uint8)


def test_the_restated_table_is_k24s_in_the_columns_they_share():
    x, mask, pe, weight, centers, lab_in = sweep_case()
    F, k = x.shape[0], centers.shape[0]
    lab, table, changed, left = R.sweep_ref(x, mask, pe, 40, weight, centers, lab_in)
    assert left > 2 and np.all(lab[mask == 0] == 255) and int((lab == 255).sum()) == int((mask == 0).sum()) + left
    assert changed == int(((lab != lab_in) & (lab != 255)).sum()) and 0 < changed < x.shape[1]
    want, wleft = M.moments_table(x, lab, k, pe, 40, ignore=255, mask=mask)
    # K24 counts the left-out pixels by their label; here they carry 255 and are ignored: the tables then agree
    diag = [1 + F + int(np.flatnonzero((np.triu_indices(F)[0] == f) & (np.triu_indices(F)[1] == f))[0]) for f in range(F)]
    assert np.array_equal(R.table_array(table), want[:, [0] + list(range(1, 1 + F)) + diag])
    assert wleft == 0


def test_tables_of_two_stripes_add_to_the_whole():
    x, mask, pe, weight, centers, lab_in = sweep_case(F=3, k=5, n=2001, seed=4)
    whole = R.sweep_ref(x, mask, pe, 38, weight, centers, lab_in)
    cut = 777
    a = R.sweep_ref(x[:, :cut], mask[:cut], pe, 38, weight, centers, lab_in[:cut])
    b = R.sweep_ref(x[:, cut:], mask[cut:], pe, 38, weight, centers, lab_in[cut:])
    assert np.array_equal(R.table_array(a[1]) + R.table_array(b[1]), R.table_array(whole[1]))
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0]) and a[2] + b[2] == whole[2] and a[3] + b[3] == whole[3]


def test_ties_go_to_the_lowest_index():
    x = np.array([[0.0, 0.25, 0.5, 0.75, 1.0]], np.float32)
    lab, table, _, _ = R.sweep_ref(x, None, np.array([0]), 10, np.array([1.0]), np.array([[0.75], [0.25], [0.75]]), np.zeros(5, np.uint8))
    assert lab.tolist() == [1, 1, 0, 0, 0] and [row[0] for row in table] == [3, 2, 0]


@pytest.mark.parametrize("kw", [dict(k_target=0), dict(k_target=65), dict(k_init=0), dict(k_init=65), dict(k_max=3, k_init=5), dict(k_max=65),
                                dict(min_size=0), dict(max_iter=0), dict(max_pairs=-1), dict(max_std=-1.0), dict(min_dist=float("nan")),
                                dict(change=float("inf")), dict(gamma=-0.5), dict(init="random"), dict(init=np.zeros((2, 3))),
                                dict(init=np.full((2, 4), np.nan)), dict(init=np.zeros((3, 4)), k_init=2), dict(ranges=[(0, 1)] * 3),
                                dict(ranges=[(1, 0)] * 4), dict(mask=np.ones(5, np.uint8))])
def test_bad_arguments_raise_value_error(kw):
    X, _ = blobs()
    with pytest.raises(ValueError):
        ISO.isodata(X[:, :200], sweep=R.ref_sweep, **{"k_target": 3, **kw})


def test_bad_features_and_models_raise_value_error():
    with pytest.raises(ValueError):
        ISO.isodata([], sweep=R.ref_sweep)
    with pytest.raises(ValueError):
        ISO.isodata(np.zeros(10, np.float32), sweep=R.ref_sweep)
    with pytest.raises(ValueError):
        ISO.isodata([np.zeros(10, np.float32), np.zeros(11, np.float32)], sweep=R.ref_sweep)
    with pytest.raises(ValueError):
        ISO.isodata(np.zeros((2, 10), np.int32), sweep=R.ref_sweep)
    with pytest.raises(ValueError):
        ISO.IsodataModel(np.zeros((2, 3)), np.ones(2), np.zeros(3), 0, np.zeros((3, 2)), "float32")
    with pytest.raises(ValueError):
        ISO.IsodataModel(np.zeros((2, 3)), np.ones(3), np.zeros(3), 0, np.zeros((3, 2)), "float64")
    with pytest.raises(ValueError):
        ISO.IsodataModel(np.zeros((65, 3)), np.ones(3), np.zeros(3), 0, np.zeros((3, 2)), "uint8")


def test_stage_flags():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["x.tif", "out", "--classify", "isodata", "--n-clusters", "5", "--isodata-init-clusters", "2", "--isodata-max-std", "0.05",
                               "--isodata-min-dist", "0.2", "--isodata-min-size", "40", "--isodata-iterations", "9", "--isodata-change", "0.01",
                               "--mask-nodata", "0", "--sieve", "4", "--signatures", "--segment", "8"])
    assert (a.classify, a.n_clusters, a.isodata_init_clusters, a.isodata_max_std, a.isodata_min_dist, a.isodata_min_size, a.isodata_iterations,
            a.isodata_change, a.isodata_model) == ("isodata", 5, 2, 0.05, 0.2, 40, 9, 0.01, None)
    a = stages.parse_args(ap, ["x.tif", "out", "--classify", "isodata", "--isodata-model", "m.npz"])
    assert a.isodata_model == "m.npz" and a.isodata_max_std is None
    a = stages.parse_args(ap, ["x.tif", "out", "--classify", "kmeans"])
    assert a.isodata_model is None and a.isodata_iterations is None
    for argv in (["x.tif", "out", "--classify", "kmeans", "--isodata-max-std", "0.1"], ["x.tif", "out", "--isodata-model", "m.npz"],
                 ["x.tif", "out", "--classify", "isodata", "--n-clusters", "65"], ["x.tif", "out", "--classify", "isodata", "--isodata-min-size", "0"],
                 ["x.tif", "out", "--classify", "isodata", "--isodata-iterations", "0"], ["x.tif", "out", "--classify", "isodata", "--isodata-change", "-1"],
                 ["x.tif", "out", "--classify", "isodata", "--isodata-init-clusters", "0"]):
        with pytest.raises(SystemExit):
            stages.parse_args(ap, argv)
