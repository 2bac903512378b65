"""K18 on the CPU: the restatement of the sweep (tests/kmeans_model_ref.py) against scikit-learn on every case of
tests/kmeans_model_cases.py, and the host side of rsseg.kmeans_model (persistence, scikit-learn round trip, plane checks,
command-line options, the C declaration) on a NumPy stand-in for the context."""
import ctypes
import math
import os
import pickle
import re

import numpy as np
import pytest

import kmeans_model_cases as K
import kmeans_model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the fused multiply-add of the restatement ---------------------------------------------------------------------------------
def test_fma_forms_equal_exact_arithmetic():
    rng = np.random.default_rng(0)
    n = 1500
    # float32: random operands, cancelling sums, and the case two roundings get wrong: (1 + 2^-23)(1 - 2^-23) + (2^24 + 2) is
    # 2^24 + 3 - 2^-46; float64 rounds it to the midpoint 2^24 + 3, which ties to 2^24 + 4, while one rounding gives 2^24 + 2
    a, b = ((rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32) for _ in range(2))
    c = ((-a.astype(np.float64) * b).astype(np.float32).astype(np.float64) * (1 + rng.integers(-2, 3, n) * 2.0 ** -23)).astype(np.float32)
    a[0], b[0], c[0] = 1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** 24 + 2
    for cc in (c, rng.standard_normal(n).astype(np.float32)):
        cc[0] = c[0]
        got = R.fma32(a, b, cc)
        want = np.array([R.fma_exact(x, y, z, np.float32) for x, y, z in zip(a, b, cc)], np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert got[0] == np.float32(2.0 ** 24 + 2)
        assert (a.astype(np.float64) * b.astype(np.float64) + cc.astype(np.float64)).astype(np.float32)[0] == np.float32(2.0 ** 24 + 4)
    # float64: the same, where a * b + c in two operations is wrong nearly everywhere (cancellation)
    a, b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n) for _ in range(2))
    c = -(a * b) * (1 + rng.integers(-2, 3, n) * 2.0 ** -52)
    for cc in (c, rng.standard_normal(n), np.zeros(n)):
        got = R.fma64(a, b, cc)
        want = np.array([R.fma_exact(x, y, z) for x, y, z in zip(a, b, cc)])
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert (R.fma64(a, b, c) != a * b + c).sum() > n // 2
    # outside the transformations' range the rational form takes over
    tiny = R.fma64(np.array([2.0 ** -500, 3e-160]), np.array([2.0 ** -500 * (1 + 2.0 ** -30), 7e-160]), np.array([2.0 ** -1040, 1e-310]))
    assert tiny[0] == R.fma_exact(2.0 ** -500, 2.0 ** -500 * (1 + 2.0 ** -30), 2.0 ** -1040) and tiny[1] == R.fma_exact(3e-160, 7e-160, 1e-310)
    if hasattr(math, "fma"):
        assert R.fma_exact(0.1, 0.2, -0.02) == math.fma(0.1, 0.2, -0.02)


# ---- the restatement against scikit-learn --------------------------------------------------------------------------------------
def test_case_list_covers_what_it_says():
    assert [(F, k, dt) for F, k, dt, s in K.CASES.values() if s == "blobs"] == K.WIDTHS
    assert {s for _, _, _, s in K.CASES.values()} == {"blobs", "grid", "nan", "wide", "const", "overflow"}
    assert [n for n in K.NAMES if not K.sklearn_exact(n)] == ["overflow-3-2-float32"]
    for dt in (K.F32, K.F64):
        t, c = R.TILE[dt], R.CHUNK[dt]
        assert K.PIXEL_COUNTS[dt] == [1, 3, t - 1, t + 1, c, c + 3, 2 * c + 5] and K.N_MAX[dt] == 2 * c + 5
    assert R.sq_bound(np.float32) == 512.0 and R.sq_bound(np.float64) == 1024.0


@pytest.mark.parametrize("name", K.NAMES)
def test_restatement_equals_sklearn(name):
    from sklearn.cluster._k_means_common import _euclidean_dense_dense_wrapper
    c, m, ref = K.case(name), K.model(name), K.reference(name)
    dt, k = c["dtype"], c["k"]
    sk = K.sklearn_labels(name)
    ndiff = int((ref["labels"] != sk).sum())
    print(f"{name}: {ndiff} of {len(sk)} labels differ from scikit-learn's predict")
    if K.sklearn_exact(name):
        assert ndiff == 0
    if c["style"] == "grid":     # the ties are there: pixels with two or more centres at exactly the smallest distance
        print(f"{name}: {int(ref['tied'][:4000].sum())} of the first 4000 pixels are tied")
        assert ref["tied"][:4000].mean() >= 0.01 and np.array_equal(np.unique(m.scale_), [1]) and not m.min_.any()
    else:
        assert ref["tied"].mean() < 0.001 or k == 1
    if c["style"] == "nan":
        assert np.isnan(c["X"]).mean() > 0.015
    if c["style"] == "const":
        assert m.scale_[c["F"] // 2] == 1 and m.min_[c["F"] // 2] == dt.type(-0.75)
    # sq: scikit-learn's compiled _euclidean_dense_dense on the first 64 pixels, bit for bit
    xs, cen = ref["xs"], m.cluster_centers_
    for i in range(64):
        want = _euclidean_dense_dense_wrapper(np.ascontiguousarray(xs[i]), np.ascontiguousarray(cen[ref["labels"][i]]), True)
        assert dt.type(want) == ref["sq"][i], i
    assert np.array_equal(ref["dist"], np.sqrt(ref["sq"]))
    # inertia against -KMeans.score: quantisation n * 2^-41, scikit-learn's own accumulation in T over n terms
    # ((n - 1) * eps_T * sum of sq), and the label differences, of which there are none
    if K.sklearn_exact(name):
        sc, km = m.to_sklearn()
        n = len(sk)
        s = R.summary(ref, n, k)
        assert not s["overflow"] and s["counts"].sum() == n and np.array_equal(s["counts"], np.bincount(sk, minlength=k))
        want = -km.score(sc.transform(np.nan_to_num(c["X"], nan=0.0)))
        bound = n * 2.0 ** -41 + (n - 1) * float(np.finfo(dt).eps) * float(ref["sq"].astype(np.float64).sum())
        print(f"{name}: inertia {s['inertia']!r}, -score {want!r}, |difference| {abs(s['inertia'] - want):.3e}, bound {bound:.3e}")
        assert abs(s["inertia"] - want) <= bound
    else:
        far = K.OVERFLOW_AT
        assert R.sq_bound(dt) <= ref["sq"][far] < 2048 and ref["q"][far] == -1 and (ref["q"] < 0).sum() == 1
        s = R.summary(ref, len(sk), k)
        assert s["overflow"] and s["inertia"] == float("inf") and s["counts"].sum() == len(sk)
        assert not R.summary(ref, far, k)["overflow"] and R.summary(ref, far + 1, k)["overflow"]


# ---- rsseg.kmeans_model on a stand-in context ----------------------------------------------------------------------------------
class HostTensor:
    def __init__(self, a):
        self.a = a
        self.dtype = f"torch.{a.dtype.name}"

    def numel(self):
        return self.a.size

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class HostContext:
    """Stands in for rsseg.runtime.Context: K18 is tests/kmeans_model_ref.py; the fit returns a canned model."""

    def __init__(self, fitted=None):
        self.fitted, self.calls = fitted, []

    def to_device(self, a, dtype=None):
        return HostTensor(np.ascontiguousarray(a, dtype))

    def kmeans_fit_predict(self, planes, n_clusters, seed=42, max_iter=300, tol=1e-4):
        self.calls.append(("fit", n_clusters, seed, max_iter, tol))
        m = self.fitted
        meta = dict(centers=m.cluster_centers_.astype(np.float64), scale=m.scale_.astype(np.float64), min=m.min_.astype(np.float64), n_iter=11)
        return HostTensor(np.arange(planes[0].numel(), dtype=np.int32) % n_clusters), meta

    def kmeans_predict(self, planes, centers, scale, min_, want_distance=False, want_summary=False):
        self.calls.append(("predict", want_distance, want_summary))
        X = np.stack([p.a for p in planes], 1)
        assert centers.dtype == scale.dtype == min_.dtype == np.float64
        ref = R.apply(X, centers, scale, min_)
        s = R.summary(ref, len(X), len(centers))
        return (HostTensor(ref["labels"]), HostTensor(ref["dist"]) if want_distance else None,
                dict(counts=s["counts"], inertia=s["inertia"], overflow=s["overflow"], ms=0.0) if want_summary else None)


NAME = "blobs-3-2-float32"


def test_model_methods_on_the_stand_in():
    from rsseg.kmeans_model import KMeansModel
    m, c, ref = K.model(NAME), K.case(NAME), K.reference(NAME)
    hc = HostContext()
    planes = [p[:600].reshape(20, 30) for p in c["planes"]]
    lab = m.predict(planes, ctx=hc)
    assert lab.shape == (20, 30) and lab.dtype == np.int32 and np.array_equal(lab.reshape(-1), ref["labels"][:600])
    lab2, dist = m.predict_with_distance(planes, ctx=hc)
    assert np.array_equal(lab2, lab) and dist.shape == (20, 30) and dist.dtype == np.float32
    assert np.array_equal(dist.reshape(-1), ref["dist"][:600])
    s = m.summary(planes, ctx=hc)
    want = R.summary(ref, 600, 2)
    assert np.array_equal(s["counts"], want["counts"]) and s["inertia"] == want["inertia"] and s["score"] == -want["inertia"] and not s["overflow"]
    assert hc.calls == [("predict", False, False), ("predict", True, False), ("predict", False, True)]
    # device tensors pass through as they are
    t = m.predict([HostTensor(np.ascontiguousarray(p[:600])) for p in c["planes"]], ctx=hc)
    assert isinstance(t, HostTensor) and np.array_equal(t.a, ref["labels"][:600])
    with pytest.raises(ValueError, match="2 planes, the model was fitted on 3"):
        m.predict(planes[:2], ctx=hc)
    with pytest.raises(ValueError, match="float64 planes, the model was fitted in float32"):
        m.predict([p.astype(np.float64) for p in planes], ctx=hc)
    # fit: one kmeans_fit_predict call, its labels unchanged, the model from its meta
    hc = HostContext(fitted=m)
    got, labels = KMeansModel.fit(planes, 2, seed=7, feature_names=["a", "b", "c"], ctx=hc)
    assert hc.calls == [("fit", 2, 7, 300, 1e-4)]
    assert labels.shape == (20, 30) and np.array_equal(labels.reshape(-1), np.arange(600) % 2)
    assert got.cluster_centers_.dtype == np.float32 and np.array_equal(got.cluster_centers_, m.cluster_centers_)
    assert np.array_equal(got.scale_, m.scale_) and np.array_equal(got.min_, m.min_)
    assert (got.n_iter_, got.seed, got.n_samples_fit_, got.feature_names) == (11, 7, 600, ["a", "b", "c"])


def _same(a, b):
    for attr in ("cluster_centers_", "scale_", "min_"):
        x, y = getattr(a, attr), getattr(b, attr)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), attr
    assert (a.feature_names, a.n_iter_, a.seed, a.n_samples_fit_) == (b.feature_names, b.n_iter_, b.seed, b.n_samples_fit_)


@pytest.mark.parametrize("name", [NAME, "const-19-7-float64"])
def test_save_load_and_sklearn_round_trips(name, tmp_path):
    from rsseg.kmeans_model import FORMAT_VERSION, KMeansModel
    m = K.model(name)
    named = KMeansModel(m.cluster_centers_, m.scale_, m.min_, [f"plane {i} é" for i in range(m.n_features_in_)], 9, 42, 1500)
    for i, model in enumerate((m, named)):
        path = model.save(str(tmp_path / f"m{i}.npz"))
        with np.load(path, allow_pickle=False) as z:
            assert int(z["format_version"]) == FORMAT_VERSION and all(z[k].dtype != object for k in z.files)
        _same(KMeansModel.load(path), model)
        sc, km = model.to_sklearn()
        back = KMeansModel.from_sklearn(sc, km, model.feature_names)
        _same(back, model)
        X = np.nan_to_num(K.case(name)["X"][:500], nan=0.0)
        assert np.array_equal(km.predict(sc.transform(X)), K.sklearn_labels(name)[:500])
    # anything pickled is refused: a pickle under the model's name, and an archive with an object member
    bad = tmp_path / "pickled.npz"
    bad.write_bytes(pickle.dumps({"cluster_centers": m.cluster_centers_}))
    with pytest.raises(ValueError, match="pickled data is refused"):
        KMeansModel.load(str(bad))
    with open(tmp_path / "object.npz", "wb") as f:
        np.savez(f, format=np.array("rsseg.KMeansModel"), format_version=np.array(1), cluster_centers=np.array([[1.0, None]], dtype=object))
    with pytest.raises(ValueError, match="pickled data is refused"):
        KMeansModel.load(str(tmp_path / "object.npz"))
    with open(tmp_path / "other.npz", "wb") as f:
        np.savez(f, a=np.zeros(3))
    with pytest.raises(ValueError, match="not a KMeansModel file"):
        KMeansModel.load(str(tmp_path / "other.npz"))
    # a float64 model is not a float32 model
    if m.dtype == np.float64:
        with pytest.raises(ValueError, match="fitted in float64 cannot be applied to float32 planes"):
            KMeansModel(m.cluster_centers_.astype(np.float32), m.scale_, m.min_)


def test_predict_features_checks_the_planes():
    from rsseg.kmeans_model import KMeansModel, plane_names
    m, c, ref = K.model(NAME), K.case(NAME), K.reference(NAME)
    hc = HostContext()
    d = {"ndvi": c["planes"][0][:600].reshape(20, 30), "stack": np.stack([p[:600].reshape(20, 30) for p in c["planes"][1:]], -1),
         "height": 20, "width": 30, "transform": None, "crs": None, "note": np.zeros(5)}
    assert plane_names(d, ["ndvi", "stack"]) == ["ndvi", "stack[0]", "stack[1]"]
    assert plane_names(d) == ["ndvi"]                        # the automatic selection takes the 2-D planes
    got = m.predict_features(d, ["ndvi", "stack"], ctx=hc)
    assert got.shape == (20, 30) and np.array_equal(got.reshape(-1), ref["labels"][:600])
    with pytest.raises(ValueError, match="the selection gives 1 planes, the model was fitted on 3"):
        m.predict_features(d, ctx=hc)
    named = KMeansModel(m.cluster_centers_, m.scale_, m.min_, ["ndvi", "stack[0]", "stack[1]"])
    assert np.array_equal(named.predict_features(d, ["ndvi", "stack"], ctx=hc), got)
    d2 = {"ndwi": d["ndvi"], **{k: v for k, v in d.items() if k != "ndvi"}}
    with pytest.raises(ValueError, match="not the ones the model was fitted on.*'ndwi' != 'ndvi'"):
        named.predict_features(d2, ["ndwi", "stack"], ctx=hc)
    # fit_features names the planes it clustered
    hc = HostContext(fitted=m)
    fm, labels = KMeansModel.fit_features(d, 2, ["ndvi", "stack"], ctx=hc)
    assert fm.feature_names == ["ndvi", "stack[0]", "stack[1]"] and labels.shape == (20, 30)


def test_command_line_options():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans", "--save-kmeans-model", "m.npz", "--evaluate", "roi.npy"])
    assert (a.save_kmeans_model, a.kmeans_model, a.evaluate) == ("m.npz", None, "roi.npy")
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans", "--kmeans-model", "m.npz"])
    assert (a.save_kmeans_model, a.kmeans_model) == (None, "m.npz")
    for argv in (["in.tif", "out", "--kmeans-model", "m.npz"], ["in.tif", "out", "--save-kmeans-model", "m.npz"],
                 ["in.tif", "out", "--classify", "rule_based", "--kmeans-model", "m.npz"],
                 ["in.tif", "out", "--classify", "random_forest", "--save-kmeans-model", "m.npz"],
                 ["in.tif", "out", "--classify", "kmeans", "--kmeans-model", "m.npz", "--save-kmeans-model", "n.npz"]):
        with pytest.raises(SystemExit) as e:
            stages.parse_args(ap, argv)
        assert e.value.code == 2, argv


def test_kmeans_predict_declared_as_in_the_header():
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    decl = re.search(r"\bint rsseg_kmeans_predict\s*\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["rsseg_ctx *ctx", "const void *const *d_planes", "int F", "int dtype", "int64_t n_local", "int k", "const double *centers",
                    "const double *scale", "const double *min_", "int32_t *d_labels", "void *d_dist", "rsseg_kmeans_apply_info *info"]
    dp, C = ctypes.POINTER(ctypes.c_double), ctypes
    res, argtypes = _lib.SIGNATURES["rsseg_kmeans_predict"]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int64, C.c_int, dp, dp, dp, C.c_void_p, C.c_void_p,
                        C.POINTER(_lib.KMeansApplyInfo)]
    struct = re.search(r"typedef struct rsseg_kmeans_apply_info \{(.*?)\} rsseg_kmeans_apply_info;", hdr, re.S).group(1)
    fields = re.findall(r"(int64_t|int32_t|double)\s+(\w+)(\[RSSEG_MAX_CLUSTERS\])?;", struct)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    want = [(n, ctype[t] * _lib.MAX_CLUSTERS if arr else ctype[t]) for t, n, arr in fields]
    assert [f[0] for f in _lib.KMeansApplyInfo._fields_] == [w[0] for w in want] == ["counts", "inertia", "overflow", "ms"]
    for (_, got), (_, exp) in zip(_lib.KMeansApplyInfo._fields_, want):
        assert ctypes.sizeof(got) == ctypes.sizeof(exp)
    assert ctypes.sizeof(_lib.KMeansApplyInfo) == 8 * _lib.MAX_CLUSTERS + 8 + 8 + 8
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), "rsseg_kmeans_predict")
