"""K25 on the GPU: the object table of rsseg_segment_features against its NumPy restatement (tests/objects_ref.py), bit for bit,
across tile seams, the LDS table's overflow, masks and value ranges; then the layers above it: object_table's chunking and
refusals, classify_objects against scikit-learn and tests/gaussian_ref.py, and the --object-features stage."""
import functools
import json
import os

import numpy as np
import pytest

import objects_ref as O
import slic_ref as R

pytestmark = pytest.mark.gpu


def gpu_table(ctx, seg, planes=(), mask=None, n_segments=None, geometry=True):
    seg = np.ascontiguousarray(seg, np.int32)
    H, W = seg.shape
    n = int(seg.max()) if n_segments is None else n_segments
    dev = [ctx.to_device(np.ascontiguousarray(p).reshape(-1)) for p in planes]
    dm = None if mask is None else ctx.to_device((np.asarray(mask) != 0).astype(np.uint8).reshape(-1))
    return ctx.segment_features(ctx.to_device(seg.reshape(-1)), H, W, n, dev, mask=dm, geometry=geometry).cpu().numpy()


def check(ctx, seg, planes=(), mask=None, n_segments=None):
    """with and without the geometry; returns the full table"""
    want = O.object_table_ref(seg, planes, mask, n_segments)
    got = gpu_table(ctx, seg, planes, mask, n_segments)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    bare = gpu_table(ctx, seg, planes, mask, n_segments, geometry=False)
    assert np.array_equal(bare, O.object_table_ref(seg, planes, mask, n_segments, geometry=False))
    empty = O.object_table_ref(np.zeros_like(seg), (), None, 0)[0, 1:O.GEO]
    assert np.array_equal(bare[:, 0], want[:, 0]) and (bare[:, 1:O.GEO] == empty).all() and np.array_equal(bare[:, O.GEO:], want[:, O.GEO:])
    return got


def u8_planes(rs, shape, P):
    return [rs.randint(0, 256, shape).astype(np.uint8) for _ in range(P)]


def f32_planes(rs, shape, P, scale=8.0):
    return [rs.uniform(-scale, scale, shape).astype(np.float32) for _ in range(P)]


@pytest.mark.parametrize("P", [0, 1, 3, 16])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 4)])
def test_degenerate_rasters(ctx, shape, P):
    rs = np.random.RandomState(250 + P)
    seg = rs.randint(0, 4, shape).astype(np.int32)
    check(ctx, seg, u8_planes(rs, shape, P), n_segments=3)
    check(ctx, seg, f32_planes(rs, shape, P), mask=rs.rand(*shape) < 0.7, n_segments=3)


def seam_shapes(ctx):
    tw, th, _ = ctx.segment_features_plan(2)
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw - 1), (65, 513)]


@functools.lru_cache(maxsize=None)
def slic_map(shape):
    rs = np.random.RandomState(251)
    mask = (rs.rand(*shape) < 0.9).astype(np.uint8)
    mask[shape[0] // 2, :] = 0                                 # a masked row through the middle: perimeters along it
    seg, n, _, _ = R.slic_ref(R.scene(252, shape, 2, cell=6, noise=0.1), 8, 0.3, 2, 0, mask)
    return seg, n, mask


@pytest.mark.parametrize("i", range(5))
def test_tile_seams(ctx, i):
    assert ctx.segment_features_plan(0) == ctx.segment_features_plan(16) and ctx.segment_features_plan(0)[2] >= 1
    shape = seam_shapes(ctx)[i]
    seg, n, mask = slic_map(shape)
    rs = np.random.RandomState(253 + i)
    check(ctx, seg, u8_planes(rs, shape, 2), n_segments=n)     # the SLIC map is 0 where its mask is
    keep = rs.rand(*shape) < 0.8                               # and a mask of the call's own over it
    check(ctx, seg, f32_planes(rs, shape, 2), mask=keep, n_segments=n)


def test_segments_that_straddle_every_seam(ctx):
    rs = np.random.RandomState(254)
    t = check(ctx, np.ones((70, 70), np.int32), u8_planes(rs, (70, 70), 1))
    assert t[1, 0] == 4900 and t[1, 10] == 280 and tuple(t[1, 6:10]) == (0, 69, 0, 69)
    cols = np.tile(np.arange(1, 71, dtype=np.int32), (20, 1))  # one column of pixels per segment
    t = check(ctx, cols, f32_planes(rs, cols.shape, 1))
    assert (t[1:, 0] == 20).all() and (t[1:, 10] == 42).all()
    rows = np.ascontiguousarray(cols.T)                        # one row of pixels per segment
    t = check(ctx, rows, u8_planes(rs, rows.shape, 3))
    assert (t[1:, 0] == 20).all() and (t[1:, 10] == 42).all()


def test_lds_overflow(ctx):
    tw, th, slots = ctx.segment_features_plan(3)
    rs = np.random.RandomState(255)
    shape = (2 * th, 2 * tw + 3)                               # every pixel its own segment: far more ids per tile than rows
    seg = (rs.permutation(shape[0] * shape[1]) + 1).astype(np.int32).reshape(shape)
    check(ctx, seg, u8_planes(rs, shape, 3))
    check(ctx, seg, f32_planes(rs, shape, 3), mask=rs.rand(*shape) < 0.7)
    for k in (slots, slots + 1):                               # exactly as many ids as rows, and one more, in one tile
        one = (rs.permutation(th * tw) % k + 1).astype(np.int32).reshape(th, tw)
        assert len(np.unique(one)) == k
        check(ctx, one, f32_planes(rs, (th, tw), 2))
        check(ctx, one, u8_planes(rs, (th, tw), 16))
    gaps = (one * 3).astype(np.int32)                          # labels with gaps: empty rows keep their sentinels
    t = check(ctx, gaps, u8_planes(rs, (th, tw), 1), n_segments=int(gaps.max()) + 5)
    assert t[1, 0] == 0 and tuple(t[1, 6:10]) == (th, -1, tw, -1) and tuple(t[1, 11:]) == (0, 0, O.I64_MAX, O.I64_MIN)
    assert np.array_equal(t[-1], t[1]) and np.array_equal(t[0], t[1])


def test_masks(ctx):
    seg, n, _ = slic_map((45, 83))
    rs = np.random.RandomState(256)
    planes = u8_planes(rs, seg.shape, 2)
    check(ctx, seg, planes, mask=None, n_segments=n)
    check(ctx, seg, planes, mask=rs.rand(*seg.shape) < 0.7, n_segments=n)
    t = check(ctx, seg, planes, mask=np.zeros(seg.shape, np.uint8), n_segments=n)
    assert (t[:, 0] == 0).all()
    # a block with a masked moat and a hole of label 0: the perimeter counts both from the inside
    blk = np.zeros((20, 90), np.int32)
    blk[2:18, 3:88] = 1
    blk[9, 40] = 0
    moat = np.ones(blk.shape, np.uint8)
    moat[5, 10:80] = 0
    t = check(ctx, blk, planes=[np.full(blk.shape, 7, np.uint8)], mask=moat)
    assert t[1, 0] == 16 * 85 - 1 - 70 and t[1, 10] == 2 * (16 + 85) + 4 + 2 * 70 + 2


def test_values(ctx):
    from rsseg import objects as OB
    from rsseg import segment as SG
    seg, n, _ = slic_map((45, 83))
    rs = np.random.RandomState(257)
    ends = (rs.randint(0, 2, seg.shape) * 255).astype(np.uint8)
    check(ctx, seg, [ends, np.zeros(seg.shape, np.uint8), np.full(seg.shape, 255, np.uint8)], n_segments=n)
    assert np.bincount(seg.reshape(-1))[1:].max() * 2047 < 2 ** 23
    wide = rs.uniform(-2047, 2047, seg.shape).astype(np.float32)
    tiny = (rs.uniform(-1, 1, seg.shape) * 2.0 ** -18).astype(np.float32)
    halves = ((rs.randint(-4000, 4000, seg.shape) + 0.5) * 2.0 ** -40).astype(np.float32)
    assert np.array_equal(halves.astype(np.float64) * 2.0 ** 40 % 1.0, np.full(seg.shape, 0.5))
    neg = rs.uniform(-900, -100, seg.shape).astype(np.float32)
    planes = [wide, tiny, halves, neg]
    t = check(ctx, seg, planes, n_segments=n)
    assert (t[1:, O.GEO + 4 * 3 + 3] < 0).all()               # every maximum of the negative plane is negative
    # the sum columns are segment_sums' columns
    mixed = [ends, wide, tiny, halves, neg]
    full = OB.object_table(seg, mixed, ctx=ctx)
    sums = SG.segment_sums(seg, mixed, ctx=ctx)
    assert np.array_equal(full[:, [0, 1, 2]], sums[:, :3]) and np.array_equal(full[:, O.GEO::4], sums[:, 3:])
    assert np.array_equal(full, O.object_table_ref(seg, mixed))


def test_chunking_of_seventeen_mixed_planes(ctx):
    from rsseg import objects as OB
    seg, n, _ = slic_map((45, 83))
    rs = np.random.RandomState(258)
    many = [rs.randint(0, 256, seg.shape).astype(np.uint8) if i % 3 else rs.uniform(-5, 5, seg.shape).astype(np.float32) for i in range(17)]
    m = rs.rand(*seg.shape) < 0.7
    assert np.array_equal(OB.object_table(seg, many, mask=m, ctx=ctx), O.object_table_ref(seg, many, mask=m))
    u8 = u8_planes(rs, seg.shape, 17)
    assert np.array_equal(OB.object_table(seg, u8, ctx=ctx), O.object_table_ref(seg, u8))
    assert np.array_equal(OB.object_table(seg, (), ctx=ctx), O.object_table_ref(seg))


def test_refusals(ctx):
    import ctypes as C
    import torch
    from rsseg import objects as OB
    from rsseg.runtime import RssegUnsupported
    seg, n, _ = slic_map((45, 83))
    with pytest.raises(ValueError, match="outside"):          # a label above n_segments is refused, not used as an index
        OB.object_table(seg, (), n_segments=n - 1, ctx=ctx)
    d_seg = ctx.to_device(np.ascontiguousarray(seg.reshape(-1)))
    p = ctx.to_device(np.zeros(seg.size, np.uint8))
    with pytest.raises(RssegUnsupported):
        ctx.segment_features(d_seg, 45, 83, n, [p] * 17)
    with pytest.raises(RssegUnsupported):                      # 1 x 3e6: H W max^2 = 2.7e19 >= 2^63
        ctx.segment_features(ctx.to_device(np.zeros(3_000_000, np.int32)), 1, 3_000_000, 0, ())
    # an odd-aligned table is refused by name, before anything is launched
    buf = torch.zeros((n + 1) * 11 * 8 + 8, dtype=torch.uint8, device=ctx.device)
    args = lambda table, flags=1, dtype=3, H=45: (ctx.h, C.c_void_p(d_seg.data_ptr()), H, 83, n, None, 0, dtype, None, flags, table)  # noqa: E731
    rc = ctx.lib.rsseg_segment_features(*args(C.c_void_p(buf.data_ptr() + 1)))
    assert rc == -1 and b"d_table" in ctx.lib.rsseg_last_error(ctx.h)
    assert int(buf.sum()) == 0
    for bad in (args(None), args(C.c_void_p(buf.data_ptr()), flags=2), args(C.c_void_p(buf.data_ptr()), dtype=1), args(C.c_void_p(buf.data_ptr()), H=0)):
        assert ctx.lib.rsseg_segment_features(*bad) == -1
    assert int(buf.sum()) == 0
    # the float domain, as segment_means words it
    ok = np.zeros(seg.shape, np.float32)
    big = ok.copy()
    big[30, 40] = 2048.0
    with pytest.raises(ValueError, match=r"planes\[1\]"):
        OB.object_table(seg, [ok, big], ctx=ctx)
    nan = ok.copy()
    nan[30, 40] = np.nan
    with pytest.raises(ValueError, match=r"planes\[0\].*NaN"):
        OB.object_table(seg, [nan], ctx=ctx)
    keep = np.ones(seg.shape, np.uint8)
    keep[30, 40] = 0
    assert np.array_equal(OB.object_table(seg, [nan, big], mask=keep, ctx=ctx), O.object_table_ref(seg, [nan, big], mask=keep))


# ---- classification of objects -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def objects_scene(ctx):
    from rsseg import segment as SG
    shape = (96, 96)
    planes = R.scene(259, shape, 4, cell=7, noise=0.1)
    seg = SG.slic(planes, step=8, max_iter=4, ctx=ctx)
    roi = (1 + (planes[0] >= 120) + (planes[1] >= 120)).astype(np.uint8)    # three classes in blobs
    roi[:, 80:] = 0                                                          # segments without ROI: not trained on
    return seg, planes, roi


def ref_features(seg, planes, roi, stats=("mean", "std"), shape=False):
    from rsseg import objects as OB
    f = OB.features_from_table(O.object_table_ref(seg, planes), [True] * len(planes), stats=stats, shape=shape)
    idx, y = O.training_segments_ref(seg, roi)
    usable = np.isfinite(f.X).all(axis=1) & (f.area > 0)
    return f, idx[usable[idx]], y[usable[idx]], usable


def test_forest_on_objects_equals_scikit_learn(ctx, objects_scene):
    from sklearn.ensemble import RandomForestClassifier
    from rsseg import objects as OB
    seg, planes, roi = objects_scene
    f, idx, y, usable = ref_features(seg, planes, roi)
    assert 0 < len(idx) < seg.max() and set(np.unique(y)) == {1, 2, 3}
    X32 = f.X.astype(np.float32)
    sk = RandomForestClassifier(n_estimators=20, random_state=7).fit(X32[idx], y)
    want = np.where(usable, sk.predict(np.nan_to_num(X32, nan=0.0)), 0).astype(np.uint8)
    res = OB.classify_objects(seg, planes, roi, method="random_forest", estimator=RandomForestClassifier(n_estimators=20, random_state=7), ctx=ctx)
    assert np.array_equal(res.train_idx, idx) and np.array_equal(res.train_y, y)
    assert res.columns == f.columns and np.array_equal(res.X, f.X, equal_nan=True)
    assert res.table.dtype == np.uint8 and res.table[0] == 0 and np.array_equal(res.table, want)
    assert res.class_map.dtype == np.uint8 and np.array_equal(res.class_map, R.paint_ref(seg, want))


@pytest.mark.parametrize("method", ["maximum_likelihood", "mahalanobis", "minimum_distance"])
def test_gaussian_methods_on_objects_equal_the_restatement(ctx, objects_scene, method):
    import gaussian_ref as G
    from rsseg import objects as OB
    seg, planes, roi = objects_scene
    f, idx, y, usable = ref_features(seg, planes, roi)
    res = OB.classify_objects(seg, planes, roi, method=method, ctx=ctx)
    assert np.array_equal(res.train_idx, idx) and np.array_equal(res.train_y, y) and np.array_equal(res.X, f.X, equal_nan=True)
    m = res.model
    got = G.classify(np.nan_to_num(f.X, nan=0.0), m.mean_, m.whiten_, m.offset_, m.class_values_, m.max_dist2_)["labels"]
    want = np.where(usable, got, 0).astype(np.uint8)
    assert np.array_equal(res.table, want) and np.array_equal(res.class_map, R.paint_ref(seg, want))


def test_object_features_and_training_segments(ctx, objects_scene):
    from rsseg import objects as OB
    seg, planes, roi = objects_scene
    rs = np.random.RandomState(260)
    m = rs.rand(*seg.shape) < 0.8
    mixed = [planes[0], rs.uniform(-3, 3, seg.shape).astype(np.float32)]
    f = OB.object_features(seg, mixed, names=["a", "b"], mask=m, ctx=ctx)
    want = OB.features_from_table(O.object_table_ref(seg, mixed, mask=m), [True, False], names=["a", "b"])
    assert f.columns == want.columns and f.columns[:5] == ["a_mean", "a_std", "a_min", "a_max", "b_mean"]
    assert np.array_equal(f.table, want.table) and np.array_equal(f.X, want.X, equal_nan=True) and np.isnan(f.X[0]).all()
    idx, y = OB.training_segments(seg, roi, mask=m, ctx=ctx)
    widx, wy = O.training_segments_ref(seg, roi, mask=m)
    assert np.array_equal(idx, widx) and np.array_equal(y, wy)


def test_stage_flag(ctx, golden_dir, tmp_path, monkeypatch):
    """python -m rsseg.stages ... --classify maximum_likelihood --segment 8 --object-features: the new files appear beside the raw
    map's, which stay byte for byte what they are without the flag; the table is the restatement's on segments.npy."""
    from rsseg import runtime as rt
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    roi = np.zeros((96, 96), np.uint8)
    roi[:, :48], roi[:, 48:] = 4, 8                            # two classes of some 58 superpixels each: the 32 features need 33 per class
    write_tiff(str(tmp_path / "labeled_roi.tif"), roi)
    monkeypatch.chdir(tmp_path)
    common = [str(tmp_path / "in.tif")]
    flags = ["--classify", "maximum_likelihood", "--segment", "8"]
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        assert stages.main(common[:1] + [str(tmp_path / "plain")] + flags) == 0
        assert stages.main(common[:1] + [str(tmp_path / "obj")] + flags + ["--object-features", "--object-based", "--evaluate",
                                                                           str(tmp_path / "labeled_roi.tif")]) == 0
    finally:
        rt._default_ctx = prev
    assert os.path.exists(tmp_path / "obj" / "evaluation_results_object_features") and os.path.exists(tmp_path / "obj" / "evaluation_results_objects")
    plain, obj = tmp_path / "plain" / "segmentation_results", tmp_path / "obj" / "segmentation_results"
    new = ("object_features.npz", "classification_maximum_likelihood_object_features.npy", "maximum_likelihood_classification_map_object_features.tif")
    assert not any((plain / f).exists() for f in new) and all((obj / f).exists() for f in new)
    for f in ("classification_maximum_likelihood.npy", "maximum_likelihood_classification_map.tif", "segments.npy"):
        assert open(plain / f, "rb").read() == open(obj / f, "rb").read(), f
    cm = np.load(obj / new[1])
    assert cm.dtype == np.uint8 and cm.shape == (96, 96) and set(np.unique(cm)) <= {0, 4, 8}
    assert np.array_equal(read_tiff(str(obj / new[2]))[0], cm)
    segments = np.load(obj / "segments.npy")
    z = np.load(obj / "object_features.npz")
    allf = np.load(tmp_path / "obj" / "feature_outputs" / "all_hierarchical_features.npy")
    used = min(allf.shape[-1], 16)
    planes = [np.ascontiguousarray(allf[..., i], dtype=np.float32) for i in range(used)]
    assert np.array_equal(z["table"], O.object_table_ref(segments, planes))
    assert z["X"].shape == (segments.max() + 1, 2 * used) and len(z["columns"]) == 2 * used
    js = json.load(open(obj / "segment_stats.json"))
    assert js["object_features"]["classes"] == [4, 8] and js["object_features"]["columns"] == list(z["columns"])
    assert js["object_features"]["n_train"] == len(O.training_segments_ref(segments, roi)[0])
    assert "object_features" not in json.load(open(plain / "segment_stats.json"))
    assert z["columns"][0] == "hierarchical_feature_1_mean" and z["columns"][1] == "hierarchical_feature_1_std"
    # under a valid mask: the masked pixels are not counted and stay 0
    valid = np.ones((96, 96), np.uint8)
    valid[40:56, 10:90] = 0
    pkl = str(tmp_path / "obj" / "feature_outputs" / "all_features_and_metadata.pkl")
    cm2, res, entry = stages.run_object_features_stage(pkl, segments, str(tmp_path / "masked"), "minimum_distance",
                                                       labeled_roi_file=str(tmp_path / "labeled_roi.tif"), valid_mask=valid, ctx=ctx)
    z2 = np.load(tmp_path / "masked" / "object_features.npz")
    assert np.array_equal(z2["table"], O.object_table_ref(segments, planes, mask=valid))
    widx, wy = O.training_segments_ref(segments, roi, mask=valid)
    assert np.array_equal(res.train_idx, widx) and np.array_equal(res.train_y, wy) and entry["n_train"] == len(widx)
    empty = np.flatnonzero(z2["table"][:, 0] == 0)
    assert (res.table[empty] == 0).all() and np.array_equal(cm2, np.where(valid != 0, R.paint_ref(segments, res.table), 0)) and set(np.unique(res.table)) <= {0, 4, 8}
    assert json.load(open(tmp_path / "masked" / "segment_stats.json")) == {"object_features": entry}
