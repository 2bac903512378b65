"""Nodata-aware classification on the CPU: the NumPy restatement of K19 (tests/compact_ref.py), the scene that shows why the
classifiers must not see nodata pixels, and the host side of rsseg.masked, KMeansModel(mask=...), the masked forest outputs,
the stage keyword and the --mask-nodata option on a NumPy stand-in for the context (its compaction is compact_ref, its fit the
CPU oracle, its sweep tests/kmeans_model_ref.py, its forest the NumPy walk of tests/test_forest_proba_host.py)."""
import os
import re

import numpy as np
import pytest

import compact_ref as CR
import kmeans_model_ref as R
from rsseg.runtime import CompactPlan
from test_forest_proba_host import flat_proba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement itself ----------------------------------------------------------------------------------------------
def test_restatement_round_trips():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000).astype(np.float32)
    m = (rng.random(1000) < 0.4).astype(np.uint8) * rng.integers(1, 256, 1000).astype(np.uint8)   # any non-zero byte is valid
    c = CR.compact(x, m)
    assert c.size == int((m != 0).sum()) and np.array_equal(c, x[m != 0])
    e = CR.expand(c, m, -7)
    assert e.dtype == np.float32 and np.array_equal(e[m != 0], c) and np.all(e[m == 0] == -7)
    assert np.array_equal(CR.compact(x, np.ones(1000, np.uint8)), x) and CR.compact(x, np.zeros(1000, np.uint8)).size == 0
    p = np.array([1.0, np.nan, np.inf, -np.inf, 5.0, 0.0], np.float32)
    q = np.array([5.0, 1.0, 1.0, 1.0, 1.0, np.nan], np.float32)
    assert CR.valid_mask([p, q], CR.VALID_NAN).tolist() == [1, 0, 1, 1, 1, 0]
    assert CR.valid_mask([p, q], CR.VALID_INF).tolist() == [1, 1, 0, 0, 1, 1]
    assert CR.valid_mask([p, q], CR.VALID_VALUE, 5.0).tolist() == [0, 1, 1, 1, 0, 1]
    assert CR.valid_mask([p, q], 7, 5.0, and_mask=np.array([1, 1, 1, 1, 1, 0], np.uint8)).tolist() == [0, 0, 0, 0, 0, 0]
    b = np.array([0, 5, 255], np.uint8)
    assert CR.valid_mask([b], 7, 255.0).tolist() == [1, 1, 0] and CR.valid_mask([b], 7, 256.0).tolist() == [1, 1, 1]
    assert CR.valid_mask([b], 7, 4.5).tolist() == [1, 1, 1] and CR.valid_mask([b], 7, -1.0).tolist() == [1, 1, 1]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_scene_needs_the_mask(oracle, dt):
    """Fitted over all pixels one cluster goes to the nodata pixels alone; fitted over the valid pixels the oracle equals
    scikit-learn label for label."""
    from sklearn.cluster import KMeans
    from sklearn.preprocessing import MinMaxScaler
    planes, mask = CR.blob_scene(dt)
    m = mask.reshape(-1) != 0
    assert (int(m.sum()), int((~m).sum())) == (1792, 1280)
    full, _ = oracle.kmeans_fit_planes(planes, 4)
    nodata_cluster = np.unique(full[~m])
    assert nodata_cluster.size == 1 and not np.any(full[m] == nodata_cluster[0])     # a cluster spent on nodata ...
    assert np.unique(full[m]).size == 3                                             # ... and two blobs merged
    comp = [CR.compact(p, mask) for p in planes]
    lab, info = oracle.kmeans_fit_planes(comp, 4)
    sk = KMeans(4, random_state=42, n_init=1).fit_predict(MinMaxScaler().fit_transform(np.stack(comp, 1)))
    ndiff = int((lab != sk).sum())
    print(f"{np.dtype(dt).name}: {ndiff} of {lab.size} labels differ from scikit-learn's on X[valid]; counts {np.bincount(lab).tolist()}")
    assert ndiff == 0 and np.bincount(lab, minlength=4).tolist() == [441, 465, 480, 406]


# ---- the stand-in context ------------------------------------------------------------------------------------------------
class HostTensor:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)
        self.dtype = f"torch.{self.a.dtype.name}"

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize

    def cpu(self):
        return self

    def numpy(self):
        return self.a

    def t(self):
        return HostTensor(self.a.T)

    def contiguous(self):
        return self

    def __len__(self):
        return len(self.a)

    def __getitem__(self, i):
        return HostTensor(self.a[i])


class HostContext:
    def __init__(self, oracle=None):
        self.oracle, self.calls, self.forest = oracle, [], None

    def to_device(self, a, dtype=None):
        return HostTensor(np.ascontiguousarray(a, dtype))

    # K19 is compact_ref
    def compact_plan(self, mask):
        assert mask.a.dtype == np.uint8 and mask.a.ndim == 1
        self.calls.append(("compact_plan", mask.numel()))
        return CompactPlan(mask, None, mask.numel(), int((mask.a != 0).sum()))

    def compact(self, plan, planes):
        self.calls.append(("compact", len(planes)))
        return [HostTensor(CR.compact(p.a, plan.mask.a)) for p in planes]

    def expand(self, plan, plane, fill):
        assert plane.numel() == plan.n_valid
        self.calls.append(("expand", plane.a.dtype.name, fill))
        return HostTensor(CR.expand(plane.a, plan.mask.a, fill))

    # the classifiers
    def kmeans_fit_predict(self, planes, n_clusters, seed=42, max_iter=300, tol=1e-4):
        self.calls.append(("fit", planes[0].numel(), n_clusters, seed, max_iter, tol))
        if planes[0].numel() < n_clusters:   # the library's own refusal (k9_kmeans.hip)
            raise ValueError(f"kmeans: n_samples={planes[0].numel()} should be >= n_clusters={n_clusters}")
        labels, info = self.oracle.kmeans_fit_planes([p.a for p in planes], n_clusters, max_iter, tol)
        return HostTensor(labels), dict(info)

    def kmeans_predict(self, planes, centers, scale, min_, want_distance=False, want_summary=False):
        self.calls.append(("predict", planes[0].numel(), want_distance, want_summary))
        X = np.stack([p.a for p in planes], 1)
        ref = R.apply(X, centers, scale, min_)
        s = R.summary(ref, len(X), len(centers))
        return (HostTensor(ref["labels"]), HostTensor(ref["dist"]) if want_distance else None,
                dict(counts=s["counts"], inertia=s["inertia"], overflow=s["overflow"], ms=0.0) if want_summary else None)

    def forest_load(self, flat):
        self.forest = flat

    def _proba(self, planes):
        return flat_proba(self.forest, np.stack([p.a for p in planes], 1))

    def forest_predict(self, planes):
        self.calls.append(("forest_predict", planes[0].numel()))
        return HostTensor(np.asarray(self.forest["classes"])[np.argmax(self._proba(planes), 1)].astype(np.int64))

    def forest_predict_proba(self, planes, proba=True, confidence=False, labels=False):
        self.calls.append(("forest_proba", planes[0].numel()))
        p = self._proba(planes)
        return HostTensor(p.T), HostTensor(p.max(1)), None


K19_CALLS = ("compact_plan", "compact", "expand")


def k19_calls(hc):
    return [c for c in hc.calls if c[0] in K19_CALLS]


# ---- rsseg.masked ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_kmeans_fit_predict_masked_wiring(oracle, dt):
    from rsseg.masked import kmeans_fit_predict_masked
    planes, mask = CR.blob_scene(dt)
    comp = [CR.compact(p, mask) for p in planes]
    want, info = oracle.kmeans_fit_planes(comp, 4)
    hc = HostContext(oracle)
    labels, meta = kmeans_fit_predict_masked(planes, mask, 4, ctx=hc)
    assert labels.shape == (48, 64) and labels.dtype == np.int32
    assert np.array_equal(labels[mask != 0], want) and np.all(labels[mask == 0] == -1)
    assert meta["n_valid"] == 1792 and meta["n_iter"] == info["n_iter"] and np.array_equal(meta["init_indices"], info["init_indices"])
    assert meta["init_indices"].max() < 1792                                   # compacted numbering
    assert hc.calls == [("compact_plan", 3072), ("compact", 5), ("fit", 1792, 4, 42, 300, 1e-4), ("expand", "int32", -1)]
    # another fill, a mask of arbitrary non-zero bytes, device planes in -> a flat device tensor out
    hc = HostContext(oracle)
    dev = [HostTensor(p.reshape(-1)) for p in planes]
    lab2, _ = kmeans_fit_predict_masked(dev, HostTensor((mask.reshape(-1) * 200).astype(np.uint8)), 4, fill=9, ctx=hc)
    assert isinstance(lab2, HostTensor) and np.array_equal(lab2.a, np.where(mask.reshape(-1) != 0, labels.reshape(-1), 9))
    # a host mask of another dtype: non-zero = valid
    lab3, _ = kmeans_fit_predict_masked(planes, mask.astype(np.float64) * 0.5, 4, ctx=HostContext(oracle))
    assert np.array_equal(lab3, labels)


def test_error_texts(oracle):
    from rsseg.kmeans_model import KMeansModel
    from rsseg.masked import forest_predict_masked, kmeans_fit_predict_masked
    planes, mask = CR.blob_scene(np.float32)
    hc = HostContext(oracle)
    with pytest.raises(ValueError, match="no valid pixels"):
        kmeans_fit_predict_masked(planes, np.zeros_like(mask), 4, ctx=hc)
    assert [c[0] for c in hc.calls] == ["compact_plan"]                         # nothing was compacted or fitted
    three = np.zeros_like(mask)
    three[10, 10:13] = 1
    with pytest.raises(ValueError, match=r"n_samples=3 should be >= n_clusters=4"):
        kmeans_fit_predict_masked(planes, three, 4, ctx=hc)
    with pytest.raises(ValueError, match="mask: 100 elements, the planes have 3072 pixels"):
        kmeans_fit_predict_masked(planes, np.ones(100, np.uint8), 4, ctx=hc)
    with pytest.raises(ValueError, match="no valid pixels"):
        KMeansModel.fit(planes, 4, ctx=hc, mask=np.zeros_like(mask))
    flat = dict(np.load(os.path.join(ROOT, "tests", "golden", "rf_samples_model_flat.npz")))
    with pytest.raises(ValueError, match="no valid pixels"):
        forest_predict_masked(flat, np.zeros((4, 5, 19)), np.zeros((4, 5)), ctx=hc)
    with pytest.raises(ValueError, match="X has 3 features, but the forest is expecting 19"):
        forest_predict_masked(flat, np.zeros((4, 5, 3)), np.ones((4, 5)), ctx=hc)


# ---- KMeansModel(mask=...) ---------------------------------------------------------------------------------------------------
def test_kmeans_model_with_a_mask(oracle):
    from rsseg.kmeans_model import KMeansModel
    planes, mask = CR.blob_scene(np.float32)
    comp = [CR.compact(p, mask) for p in planes]
    m = mask != 0
    hc = HostContext(oracle)
    model, labels = KMeansModel.fit(planes, 4, ctx=hc, mask=mask)
    plain, plain_labels = KMeansModel.fit(comp, 4, ctx=HostContext(oracle))
    assert model.n_samples_fit_ == 1792 == plain.n_samples_fit_ and model.dtype == np.float32
    for a in ("cluster_centers_", "scale_", "min_"):
        assert getattr(model, a).tobytes() == getattr(plain, a).tobytes(), a
    assert labels.shape == (48, 64) and np.array_equal(labels[m], plain_labels) and np.all(labels[~m] == -1)
    # predict / distance / summary: the unmasked calls on the compacted planes; -1 / NaN elsewhere; counts over the valid pixels
    want_l, want_d = plain.predict_with_distance(comp, ctx=HostContext())
    want_s = plain.summary(comp, ctx=HostContext())
    hc = HostContext()
    lab = model.predict(planes, ctx=hc, mask=mask)
    assert lab.shape == (48, 64) and np.array_equal(lab[m], want_l) and np.all(lab[~m] == -1)
    lab2, dist = model.predict_with_distance(planes, ctx=hc, mask=mask)
    assert np.array_equal(lab2, lab) and dist.dtype == np.float32 and dist.shape == (48, 64)
    assert np.array_equal(dist[m], want_d) and np.all(np.isnan(dist[~m])) and not np.isnan(dist[m]).any()
    s = model.summary(planes, ctx=hc, mask=mask)
    assert np.array_equal(s["counts"], want_s["counts"]) and int(s["counts"].sum()) == 1792 == s["n_valid"]
    assert s["inertia"] == want_s["inertia"] and s["score"] == -want_s["inertia"]
    assert hc.calls == [("compact_plan", 3072), ("compact", 5), ("predict", 1792, False, False), ("expand", "int32", -1),
                        ("compact_plan", 3072), ("compact", 5), ("predict", 1792, True, False), ("expand", "int32", -1)] + \
        [hc.calls[8]] + [("compact_plan", 3072), ("compact", 5), ("predict", 1792, False, True), ("expand", "int32", -1)]
    assert hc.calls[8][:2] == ("expand", "float32") and np.isnan(hc.calls[8][2])
    # the dictionary forms
    d = {f"f{i}": p for i, p in enumerate(planes)}
    d.update(height=48, width=64)
    keys = [f"f{i}" for i in range(5)]
    fm, fl = KMeansModel.fit_features(d, 4, keys, ctx=HostContext(oracle), mask=mask)
    assert np.array_equal(fl, labels) and fm.n_samples_fit_ == 1792 and fm.feature_names == keys
    assert np.array_equal(fm.predict_features(d, keys, ctx=HostContext(), mask=mask), lab)


def test_without_a_mask_nothing_is_compacted(oracle):
    """mask=None: every entry point makes the calls it made before K19 existed."""
    from rsseg import stages
    from rsseg.kmeans_model import KMeansModel
    planes, mask = CR.blob_scene(np.float32)
    zero = [np.nan_to_num(p) for p in planes]
    hc = HostContext(oracle)
    model, _ = KMeansModel.fit(zero, 4, ctx=hc)
    model.predict(zero, ctx=hc)
    model.predict_with_distance(zero, ctx=hc)
    model.summary(zero, ctx=hc)
    d = {f"f{i}": p for i, p in enumerate(zero)}
    d.update(height=48, width=64)
    keys = [f"f{i}" for i in range(5)]
    KMeansModel.fit_features(d, 4, keys, ctx=hc)
    model.predict_features(d, keys, ctx=hc)
    stages.run_kmeans_stage(np.stack(zero, -1), 4, ctx=hc)
    assert hc.calls == [("fit", 3072, 4, 42, 300, 1e-4), ("predict", 3072, False, False), ("predict", 3072, True, False),
                        ("predict", 3072, False, True), ("fit", 3072, 4, 42, 300, 1e-4), ("predict", 3072, False, False),
                        ("fit", 3072, 4, 42, 300, 1e-4)]
    assert k19_calls(hc) == []
    from rsseg import forest as FO
    flat = dict(np.load(os.path.join(ROOT, "tests", "golden", "rf_samples_model_flat.npz")))
    hc = HostContext()
    FO.image_proba_and_confidence(flat, np.zeros((4, 5, 19)), ctx=hc)
    assert hc.calls == [("forest_proba", 20)]


# ---- the forest -----------------------------------------------------------------------------------------------------------
def test_forest_masked_wiring():
    from rsseg import forest as FO
    from rsseg.masked import forest_predict_masked
    flat = dict(np.load(os.path.join(ROOT, "tests", "golden", "rf_samples_model_flat.npz")))
    stack = np.load(os.path.join(ROOT, "tests", "golden", "crop96.npz"))["stack19"][:40, :50].copy()
    stack[3, 4, 2] = np.nan                                                     # a NaN at a valid pixel counts as 0
    mask = CR.collar_and_holes(40, 50, 4, 0.05, 3)
    mask[3, 4] = 1
    m = mask != 0
    X = np.nan_to_num(stack.reshape(-1, 19), nan=0.0).astype(np.float32)
    want = flat_proba(flat, X)
    want_lab = np.asarray(flat["classes"])[np.argmax(want, 1)].reshape(40, 50)
    hc = HostContext()
    lab = forest_predict_masked(flat, stack, mask, ctx=hc)
    nv = int(m.sum())
    assert lab.shape == (40, 50) and lab.dtype == np.int64 and np.array_equal(lab[m], want_lab[m]) and np.all(lab[~m] == 0)
    assert hc.calls == [("compact_plan", 2000), ("compact", 19), ("forest_predict", nv), ("expand", "int64", 0)]
    assert np.all(forest_predict_masked(flat, stack, mask, fill=-5, ctx=hc)[~m] == -5)
    hc = HostContext()
    proba, conf = FO.image_proba_and_confidence(flat, stack, ctx=hc, mask=mask)
    assert proba.shape == (40, 50, 3) and conf.shape == (40, 50) and proba.dtype == conf.dtype == np.float64
    assert np.array_equal(proba[m], want.reshape(40, 50, 3)[m]) and np.array_equal(conf[m], want.max(1).reshape(40, 50)[m])
    assert not proba[~m].any() and not conf[~m].any()
    assert [c[0] for c in hc.calls] == ["compact_plan", "compact", "forest_proba", "expand", "expand", "expand", "expand"]
    assert hc.calls[2] == ("forest_proba", nv)


# ---- stages ---------------------------------------------------------------------------------------------------------------
def test_kmeans_stage_with_a_valid_mask(oracle):
    from rsseg import stages
    planes, mask = CR.blob_scene(np.float32)
    hier = np.stack(planes, -1)
    hc = HostContext(oracle)
    cm = stages.run_kmeans_stage(hier, 4, ctx=hc, valid_mask=mask)
    want, _ = oracle.kmeans_fit_planes([CR.compact(p, mask) for p in planes], 4)
    assert cm.dtype == np.uint8 and cm.shape == (48, 64)
    assert np.array_equal(cm == 0, mask == 0) and np.array_equal(cm[mask != 0], want + 1)
    with pytest.raises(ValueError, match=r"valid_mask: shape \(48, 60\), the raster is \(48, 64\)"):
        stages.run_kmeans_stage(hier, 4, ctx=hc, valid_mask=mask[:, :60])
    import inspect
    for fn in (stages.run_masked_classification_stage, stages.run_kmeans_stage, stages.run_kmeans_model_stage):
        p = inspect.signature(fn).parameters["valid_mask"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_mask_nodata_option():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans"])
    assert a.mask_nodata is None and stages.resolve_mask_nodata(a.mask_nodata, 0.0) is None
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans", "--mask-nodata"])
    assert a.mask_nodata == stages.MASK_NODATA_FROM_TAG
    assert stages.resolve_mask_nodata(a.mask_nodata, 0.0) == 0.0 and stages.resolve_mask_nodata(a.mask_nodata, -9999.0) == -9999.0
    with pytest.raises(SystemExit) as e:                                        # neither a tag nor a value
        stages.resolve_mask_nodata(a.mask_nodata, None)
    assert "no GDAL_NODATA tag" in str(e.value.code)
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "random_forest", "--mask-nodata", "-9999", "--confidence"])
    assert a.mask_nodata == -9999.0 and stages.resolve_mask_nodata(a.mask_nodata, None) == -9999.0
    assert stages.resolve_mask_nodata(a.mask_nodata, 0.0) == -9999.0            # a value given wins over the tag
    a = stages.parse_args(ap, ["in.tif", "out", "--mask-nodata", "0", "--classify", "kmeans"])
    assert a.mask_nodata == 0.0 and stages.resolve_mask_nodata(a.mask_nodata, None) == 0.0
    for argv in (["in.tif", "out", "--mask-nodata"], ["in.tif", "out", "--classify", "kmeans", "--raw", "--mask-nodata", "0"],
                 ["in.tif", "out", "--classify", "random_forest", "--importance", "roi.npy", "--mask-nodata"],
                 ["in.tif", "out", "--classify", "kmeans", "--mask-nodata", "none"]):
        with pytest.raises(SystemExit) as e:
            stages.parse_args(ap, argv)
        assert e.value.code == 2, argv


# ---- the C declarations ---------------------------------------------------------------------------------------------------
def test_k19_declared_as_in_the_header():
    import ctypes as C
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    kinds = {"rsseg_ctx *ctx": C.c_void_p, "int64_t n": C.c_int64, "int P": C.c_int, "int dtype": C.c_int, "int flags": C.c_int,
             "int elem_bytes": C.c_int, "double nodata": C.c_double, "int64_t *n_valid": C.POINTER(C.c_int64),
             "const void *const *d_planes": C.POINTER(C.c_void_p), "const void *const *d_in": C.POINTER(C.c_void_p),
             "void *const *d_out": C.POINTER(C.c_void_p)}
    for name in ("rsseg_valid_mask", "rsseg_compact_plan", "rsseg_compact_planes", "rsseg_expand_plane"):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S).group(1)
        args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            assert t == kinds.get(a, C.c_void_p), (name, a)                     # every other argument is a pointer handed over as void *
            assert a in kinds or "*" in a, (name, a)
    for name in ("rsseg_compact_tile", "rsseg_compact_scan_span"):
        assert re.search(r"\bint %s\(void\);" % name, hdr) and _lib.SIGNATURES[name] == (C.c_int, [])
    assert (_lib.VALID_NAN, _lib.VALID_INF, _lib.VALID_VALUE) == (CR.VALID_NAN, CR.VALID_INF, CR.VALID_VALUE)
    for n, v in (("NAN", 1), ("INF", 2), ("VALUE", 4)):
        assert re.search(r"#define RSSEG_VALID_%s %d\b" % (n, v), hdr)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rsseg_compact_tile() == 4096 and lib.rsseg_compact_scan_span() >= 1
