"""K18 on the GPU (rsseg_kmeans_predict, Context.kmeans_predict, rsseg.kmeans_model, the stage and its options): every case of
tests/kmeans_model_cases.py at every pixel count against the NumPy restatement (tests/kmeans_model_ref.py), bit for bit, and
against scikit-learn's own predict."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kmeans_model_cases as K
import kmeans_model_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    """The scene of a case on the device, uploaded once: name -> list of F flat planes of N_MAX pixels."""
    cache = {}

    def get(ctx, name):
        if name not in cache:
            cache[name] = [ctx.to_device(p) for p in K.case(name)["planes"]]
        return cache[name]
    return get


def _args(name):
    m = K.model(name)
    return m.cluster_centers_.astype(np.float64), m.scale_.astype(np.float64), m.min_.astype(np.float64)


PARAMS = [(name, n) for name in K.NAMES for n in K.PIXEL_COUNTS[K.CASES[name][2]]]


@pytest.mark.parametrize("name,n", PARAMS, ids=[f"{a}-n{b}" for a, b in PARAMS])
def test_sweep_equals_the_restatement(ctx, dev, name, n):
    c, ref = K.case(name), K.reference(name)
    planes = [p[:n] for p in dev(ctx, name)]
    want = R.summary(ref, n, c["k"])
    labels, dist, s = ctx.kmeans_predict(planes, *_args(name), want_distance=True, want_summary=True)
    labels, dist = labels.cpu().numpy(), dist.cpu().numpy()
    assert labels.dtype == np.int32 and dist.dtype == c["dtype"] and labels.shape == dist.shape == (n,)
    assert np.array_equal(labels, ref["labels"][:n])
    assert dist.tobytes() == ref["dist"][:n].tobytes()
    assert s["counts"].dtype == np.int64 and np.array_equal(s["counts"], want["counts"])
    assert s["overflow"] == want["overflow"]
    assert s["inertia"] == want["inertia"], (s["inertia"].hex(), want["inertia"].hex())
    if K.sklearn_exact(name):
        assert np.array_equal(labels, K.sklearn_labels(name)[:n])
    elif n > K.OVERFLOW_AT:
        assert s["overflow"] and s["inertia"] == float("inf") and s["counts"].sum() == n
    # the three forms of the sweep (and the summary without the distance plane) give the same labels and the same summary
    only, none_d, none_s = ctx.kmeans_predict(planes, *_args(name))
    assert none_d is None and none_s is None and np.array_equal(only.cpu().numpy(), labels)
    l1, d1, s1 = ctx.kmeans_predict(planes, *_args(name), want_distance=True)
    assert s1 is None and np.array_equal(l1.cpu().numpy(), labels) and d1.cpu().numpy().tobytes() == dist.tobytes()
    l2, d2, s2 = ctx.kmeans_predict(planes, *_args(name), want_summary=True)
    assert d2 is None and np.array_equal(l2.cpu().numpy(), labels)
    assert np.array_equal(s2["counts"], s["counts"]) and s2["inertia"] == s["inertia"] and s2["overflow"] == s["overflow"]


def test_unaligned_planes_and_outputs(ctx):
    """A plane one element off a 16-byte boundary is refused by name, as kmeans_fit_predict refuses it; output planes off the
    boundary are written element by element."""
    import torch
    name = "blobs-9-9-float32"
    c, ref = K.case(name), K.reference(name)
    n = 3001
    buf = [ctx.to_device(np.concatenate([np.zeros(1, np.float32), p[:n]])) for p in c["planes"]]
    off = [b[1:] for b in buf]
    assert off[0].data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="plane 0 null or not 16-byte aligned"):
        ctx.kmeans_fit_predict(off, 9)
    with pytest.raises(ValueError, match="plane 0 null or not 16-byte aligned"):
        ctx.kmeans_predict(off, *_args(name))
    # the library's own entry point with output planes one element off
    planes = [b[:n].clone() for b in off]
    labels = torch.full((n + 2,), -7, dtype=torch.int32, device=planes[0].device)
    dist = torch.full((n + 2,), -7.0, dtype=torch.float32, device=planes[0].device)
    cen, sc, mn = _args(name)
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx.lib.rsseg_kmeans_predict(ctx.h, ctx._pp(planes), 9, 0, n, 9, cen.ctypes.data_as(dp), sc.ctypes.data_as(dp), mn.ctypes.data_as(dp),
                                          C.c_void_p(labels.data_ptr() + 4), C.c_void_p(dist.data_ptr() + 4), None))
    labels, dist = labels.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(labels[1:n + 1], ref["labels"][:n]) and dist[1:n + 1].tobytes() == ref["dist"][:n].tobytes()
    assert labels[0] == labels[-1] == -7 and dist[0] == dist[-1] == -7


def test_refusals_and_the_empty_stripe(ctx):
    import torch
    from rsseg.runtime import RssegUnsupported
    name = "blobs-3-2-float32"
    planes = [ctx.to_device(p[:100]) for p in K.case(name)["planes"]]
    cen, sc, mn = _args(name)
    with pytest.raises(RssegUnsupported, match="65 feature planes, the kernels take at most 64"):
        ctx.kmeans_predict([planes[0]] * 65, np.zeros((2, 65)), np.ones(65), np.zeros(65))
    with pytest.raises(RssegUnsupported, match="n_clusters=65, the kernels take at most 64"):
        ctx.kmeans_predict(planes, np.zeros((65, 3)), sc, mn)
    with pytest.raises(ValueError, match="planes must all be float32 or all float64"):
        ctx.kmeans_predict([planes[0], planes[1].double(), planes[2]], cen, sc, mn)
    with pytest.raises(ValueError, match="no feature planes"):
        ctx.kmeans_predict([], cen, sc, mn)
    with pytest.raises(ValueError, match="the model has 3 features"):
        ctx.kmeans_predict(planes[:2], cen, sc, mn)
    for what, bad in (("centers", (np.where(np.arange(6).reshape(2, 3) == 4, np.nan, cen), sc, mn)),
                      ("scale", (cen, np.array([1.0, np.inf, 1.0]), mn)), ("min_", (cen, sc, np.array([-np.inf, 0.0, 0.0])))):
        with pytest.raises(ValueError, match=rf"{what}\[\d\] is not finite"):
            ctx.kmeans_predict(planes, *bad)
    with pytest.raises(ValueError, match=r"centers\[1\] is not a float32 value: a model fitted in float64 cannot be applied to float32 planes"):
        ctx.kmeans_predict(planes, cen + np.array([[0, 1e-12, 0], [0, 0, 0]]), sc, mn)
    with pytest.raises(ValueError, match=r"scale\[2\] is not a float32 value"):
        ctx.kmeans_predict(planes, cen, sc * np.array([1, 1, 1 + 2.0 ** -40]), mn)
    # the same values ARE a float64 model
    ctx.kmeans_predict([p.double() for p in planes], cen + np.array([[0, 1e-12, 0], [0, 0, 0]]), sc, mn)
    dp = C.POINTER(C.c_double)
    rc = ctx.lib.rsseg_kmeans_predict(ctx.h, ctx._pp(planes), 3, 7, 100, 2, cen.ctypes.data_as(dp), sc.ctypes.data_as(dp), mn.ctypes.data_as(dp),
                                      C.c_void_p(planes[0].data_ptr()), None, None)
    assert rc == -1 and b"dtype must be RSSEG_F32 or RSSEG_F64" in ctx.lib.rsseg_last_error(ctx.h)
    rc = ctx.lib.rsseg_kmeans_predict(ctx.h, ctx._pp(planes), 3, 0, 100, 0, cen.ctypes.data_as(dp), sc.ctypes.data_as(dp), mn.ctypes.data_as(dp),
                                      C.c_void_p(planes[0].data_ptr()), None, None)
    assert rc == -1 and b"n_clusters=0 must be >= 1" in ctx.lib.rsseg_last_error(ctx.h)
    # an empty stripe: zero counts, inertia 0
    empty = [torch.empty(0, dtype=torch.float32, device=planes[0].device) for _ in range(3)]
    labels, dist, s = ctx.kmeans_predict(empty, cen, sc, mn, want_distance=True, want_summary=True)
    assert labels.numel() == 0 and dist.numel() == 0 and not s["counts"].any() and s["inertia"] == 0.0 and not s["overflow"]


def _stage2(golden_dir):
    g = np.load(os.path.join(golden_dir, "crop96_stage2.npz"))
    d = {str(k): g[f"plane_{i:02d}"] for i, k in enumerate(g["keys"])}
    d["height"], d["width"] = int(g["height"]), int(g["width"])
    d["transform"], d["crs"] = None, None
    return d


def test_fit_and_predict_end_to_end(ctx, golden_dir):
    """On the 55 planes of the stage-2 crop: KMeansModel.fit returns unsupervised_kmeans_classification's labels, and predict on
    the same planes equals to_sklearn()'s predict."""
    from modules.features import extract as E
    from rsseg import runtime as rt
    from rsseg.kmeans_model import KMeansModel
    d = _stage2(golden_dir)
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        want = E.unsupervised_kmeans_classification(d, 8)
        model, labels = KMeansModel.fit_features(d, 8)
        assert labels.dtype == np.int32 and np.array_equal(labels, want)
        assert model.dtype == np.float64 and model.cluster_centers_.shape == (8, 55) and model.n_samples_fit_ == 96 * 96 and model.n_iter_ > 0
        assert model.feature_names == [k for k in d if k not in ("height", "width", "transform", "crs")]
        got = model.predict_features(d)
    finally:
        rt._default_ctx = prev
    planes = [np.asarray(d[k], np.float64) for k in model.feature_names]
    sc, km = model.to_sklearn()
    X = np.nan_to_num(np.stack([p.reshape(-1) for p in planes], 1), nan=0.0)
    assert np.array_equal(got.reshape(-1), km.predict(sc.transform(X)))
    ref = R.apply(np.stack([p.reshape(-1) for p in planes], 1), model.cluster_centers_, model.scale_, model.min_)
    lab, dist = model.predict_with_distance(planes, ctx=ctx)
    assert np.array_equal(lab.reshape(-1), ref["labels"]) and dist.reshape(-1).tobytes() == ref["dist"].tobytes()
    s = model.summary(planes, ctx=ctx)
    assert s["inertia"] == R.summary(ref, 96 * 96, 8)["inertia"] and s["score"] == -s["inertia"]


def test_stage_saves_and_applies_a_model(ctx, golden_dir, tmp_path):
    """--save-kmeans-model leaves the class map byte for byte as a run without it and writes the model; --kmeans-model applies
    it: the four files, the class map = predict + 1."""
    from rsseg import runtime as rt
    from rsseg import stages
    from rsseg.kmeans_model import KMeansModel
    from rsseg.tiff import write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    mpath = str(tmp_path / "model.npz")
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain"), "--classify", "kmeans", "--n-clusters", "5"]) == 0
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "saved"), "--classify", "kmeans", "--n-clusters", "5",
                            "--save-kmeans-model", mpath]) == 0
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "applied"), "--classify", "kmeans", "--kmeans-model", mpath]) == 0
    finally:
        rt._default_ctx = prev
    plain, saved, applied = (tmp_path / d / "segmentation_results" for d in ("plain", "saved", "applied"))
    assert sorted(os.listdir(plain)) == sorted(os.listdir(saved)) == ["classification_kmeans.npy", "kmeans_classification_map.tif"]
    for f in os.listdir(plain):
        assert (plain / f).read_bytes() == (saved / f).read_bytes(), f
    assert sorted(os.listdir(applied)) == ["classification_kmeans.npy", "kmeans_classification_map.tif", "kmeans_distance.npy",
                                           stages.KMEANS_SUMMARY_FILE]
    model = KMeansModel.load(mpath)
    assert model.n_clusters == 5 and model.n_features_in_ == 55 and len(model.feature_names) == 55
    import pickle
    from modules.features.extract import normalize_features_structure
    feats = normalize_features_structure(pickle.load(open(tmp_path / "applied" / "feature_outputs" / "all_features_and_metadata.pkl", "rb")))
    planes = [np.asarray(feats[k]) for k in model.feature_names]
    lab, dist = model.predict_with_distance([np.asarray(p, np.float64) for p in planes], ctx=ctx)
    cm = np.load(applied / "classification_kmeans.npy")
    assert cm.dtype == np.uint8 and cm.shape == (96, 96) and np.array_equal(cm, lab + 1)
    assert np.load(applied / "kmeans_distance.npy").tobytes() == dist.tobytes()
    s = json.load(open(applied / stages.KMEANS_SUMMARY_FILE))
    assert s["model"] == "model.npz" and s["counts"] == np.bincount(lab.reshape(-1), minlength=5).tolist() and s["overflow"] is False
    assert s["inertia"] == model.summary([np.asarray(p, np.float64) for p in planes], ctx=ctx)["inertia"]
    # the stage function by itself, with the plane check: another selection of planes is refused
    with pytest.raises(ValueError, match="the selection gives 1 planes, the model was fitted on 55"):
        stages.run_kmeans_model_stage(str(tmp_path / "applied" / "feature_outputs" / "all_features_and_metadata.pkl"), mpath,
                                      str(tmp_path / "again"), feature_keys=[model.feature_names[0]], ctx=ctx)
