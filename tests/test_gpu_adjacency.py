"""K27 on the GPU: the region adjacency graph of rsseg_segment_adjacency against its NumPy restatement (tests/adjacency_ref.py),
bit for bit, across tile seams, the LDS table's overflow, masks and the capacity rule; then the layers above it: adjacency(),
neighbour_features / object_features(neighbours=True), merge_regions against merge_regions_ref, and the stage and command."""
import functools
import json
import os

import numpy as np
import pytest

import adjacency_ref as A
import objects_ref as O
import slic_ref as R

pytestmark = pytest.mark.gpu


def gpu_edges(ctx, seg, planes=(), mask=None, n_segments=None, max_edges=None):
    seg = np.ascontiguousarray(seg, np.int32)
    H, W = seg.shape
    n = int(seg.max()) if n_segments is None else n_segments
    dev = [ctx.to_device(np.ascontiguousarray(p).reshape(-1)) for p in planes]
    dm = None if mask is None else ctx.to_device((np.asarray(mask) != 0).astype(np.uint8).reshape(-1))
    return ctx.segment_adjacency(ctx.to_device(seg.reshape(-1)), H, W, n, dev, mask=dm, max_edges=max_edges).cpu().numpy()


def check(ctx, seg, planes=(), mask=None, n_segments=None, max_edges=None):
    want = A.adjacency_ref(seg, planes, mask, n_segments)
    got = gpu_edges(ctx, seg, planes, mask, n_segments, max_edges)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return got


def u8_planes(rs, shape, P):
    return [rs.randint(0, 256, shape).astype(np.uint8) for _ in range(P)]


@pytest.mark.parametrize("P", [0, 1, 3, 16])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 4)])
def test_degenerate_rasters(ctx, shape, P):
    rs = np.random.RandomState(270 + P)
    seg = rs.randint(0, 4, shape).astype(np.int32)
    check(ctx, seg, u8_planes(rs, shape, P), n_segments=3)
    check(ctx, seg, u8_planes(rs, shape, P), mask=rs.rand(*shape) < 0.7, n_segments=3)
    none = check(ctx, np.full(shape, 2, np.int32), u8_planes(rs, shape, P), n_segments=3)   # no edge at all
    assert none.shape == (0, 3 + P)


def seam_shapes(ctx):
    tw, th, _ = ctx.segment_adjacency_plan(2)
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw - 1), (65, 513)]


@functools.lru_cache(maxsize=None)
def slic_map(shape):
    rs = np.random.RandomState(271)
    mask = (rs.rand(*shape) < 0.9).astype(np.uint8)
    mask[shape[0] // 2, :] = 0                                 # a masked row through the middle: no crossing over it
    seg, n, _, _ = R.slic_ref(R.scene(272, shape, 2, cell=6, noise=0.1), 8, 0.3, 2, 0, mask)
    return seg, n, mask


@pytest.mark.parametrize("i", range(5))
def test_tile_seams(ctx, i):
    assert ctx.segment_adjacency_plan(0) == ctx.segment_adjacency_plan(16) and ctx.segment_adjacency_plan(0)[2] >= 1
    shape = seam_shapes(ctx)[i]
    seg, n, mask = slic_map(shape)
    rs = np.random.RandomState(273 + i)
    e = check(ctx, seg, u8_planes(rs, shape, 2), n_segments=n)   # the SLIC map is 0 where its mask is
    assert len(e) > 0
    check(ctx, seg, u8_planes(rs, shape, 5), mask=rs.rand(*shape) < 0.8, n_segments=n)   # and a mask of the call's own over it
    check(ctx, seg, (), n_segments=n)


def test_segments_along_every_seam(ctx):
    tw, th, _ = ctx.segment_adjacency_plan(1)
    rs = np.random.RandomState(274)
    none = check(ctx, np.ones((70, 70), np.int32), u8_planes(rs, (70, 70), 1))
    assert none.shape == (0, 4)
    cols = np.tile(np.arange(1, tw + 8, dtype=np.int32), (th + 5, 1))   # one column of pixels per segment: a crossing on every vertical seam
    e = check(ctx, cols, u8_planes(rs, cols.shape, 1))
    assert len(e) == tw + 6 and (e[:, 2] == th + 5).all() and (e[:, 1] == e[:, 0] + 1).all()
    rows = np.ascontiguousarray(np.tile(np.arange(1, 3 * th + 2, dtype=np.int32), (tw + 9, 1)).T)   # one row per segment: every horizontal seam
    e = check(ctx, rows, u8_planes(rs, rows.shape, 3))
    assert len(e) == 3 * th and (e[:, 2] == tw + 9).all()


def isolated_pixels(th, tw, k):
    """one tile of label 1 with k single pixels of labels 2 ... k + 1, no two of them 4-neighbours: exactly k pairs (1, l)"""
    seg = np.ones((th, tw), np.int32)
    ys, xs = np.nonzero((np.add.outer(np.arange(th), np.arange(tw)) % 2) == 0)
    assert k <= len(ys) - 1
    seg[ys[1:k + 1], xs[1:k + 1]] = np.arange(2, k + 2)
    return seg


def test_lds_overflow(ctx):
    tw, th, slots = ctx.segment_adjacency_plan(3)
    rs = np.random.RandomState(275)
    shape = (2 * th, 2 * tw + 3)                               # every pixel its own segment: far more pairs per tile than rows
    seg = (rs.permutation(shape[0] * shape[1]) + 1).astype(np.int32).reshape(shape)
    e = check(ctx, seg, u8_planes(rs, shape, 3))
    assert len(e) == 2 * shape[0] * shape[1] - shape[0] - shape[1] and (e[:, 2] == 1).all()
    check(ctx, seg, u8_planes(rs, shape, 16), mask=rs.rand(*shape) < 0.7)
    for k in (slots, slots + 1):                               # exactly as many pairs as rows, and one more, in one tile
        one = isolated_pixels(th, tw, k)
        e = check(ctx, one, u8_planes(rs, (th, tw), 2))
        assert len(e) == k
        check(ctx, one, u8_planes(rs, (th, tw), 16))
    gaps = (isolated_pixels(th, tw, slots + 1) * 3).astype(np.int32)   # labels with gaps, n_segments above the largest label
    e = check(ctx, gaps, u8_planes(rs, (th, tw), 1), n_segments=int(gaps.max()) + 5)
    assert (e[:, 0] == 3).all() and (e[:, 1] % 3 == 0).all()
    few = (rs.randint(0, 24, (3 * th + 1, 2 * tw + 5)) + 1).astype(np.int32)   # scattered labels: long runs of crossings per pair
    e = check(ctx, few, u8_planes(rs, few.shape, 4))
    assert len(e) == 24 * 23 // 2


def test_capacity(ctx):
    from rsseg.runtime import RssegUnsupported
    rs = np.random.RandomState(276)
    seg, n, mask = slic_map((65, 513))
    planes = u8_planes(rs, seg.shape, 2)
    true = len(A.adjacency_ref(seg, planes, None, n))
    check(ctx, seg, planes, n_segments=n, max_edges=true)      # exactly the true count fits
    check(ctx, seg, planes, n_segments=n, max_edges=true + 1)
    for cap in (true - 1, true // 2, 1, 0):                    # noticed by the compaction count, or by a probe that went round
        with pytest.raises(RssegUnsupported, match="more than max_edges"):
            gpu_edges(ctx, seg, planes, n_segments=n, max_edges=cap)
    # max_edges=None: 4 n + 64 rows hold every planar map ...
    tw, th, _ = ctx.segment_adjacency_plan(0)
    shape = (th + 3, 2 * tw + 1)
    each = (rs.permutation(shape[0] * shape[1]) + 1).astype(np.int32).reshape(shape)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        check(ctx, each, u8_planes(rs, shape, 1))
        assert ctx.prof_get("segment_adjacency")[1] == 1 and ctx.prof_get("segment_adjacency_compact")[1] == 1
        # ... and scattered labels, whose segments are not connected, can exceed it: the second try takes the hard bound
        n2 = 40
        scat = (rs.randint(0, n2, (3 * th, 3 * tw)) + 1).astype(np.int32)
        assert len(A.adjacency_ref(scat, (), None, n2)) > 4 * n2 + 64
        ctx.prof_reset()
        check(ctx, scat, u8_planes(rs, scat.shape, 2), n_segments=n2)
        assert ctx.prof_get("segment_adjacency")[1] == 2
    finally:
        ctx.prof_enable(False)


def test_refusals(ctx):
    from rsseg.runtime import RssegUnsupported
    seg = np.ones((8, 12), np.int32)
    seg[:, 6:] = 2
    for bad in (3, -1, 2 ** 31 - 1):
        s = seg.copy()
        s[5, 7] = bad
        with pytest.raises(ValueError, match="labels outside"):
            gpu_edges(ctx, s, n_segments=2)
    rs = np.random.RandomState(277)
    with pytest.raises(RssegUnsupported, match="P = 17"):
        gpu_edges(ctx, seg, u8_planes(rs, seg.shape, 17))
    d = ctx.to_device(seg.reshape(-1))
    for H, W in ((0, 12), (8, 0), (-1, 12)):
        with pytest.raises(ValueError, match="must be at least 1"):
            ctx.segment_adjacency(d, H, W, 2, max_edges=16)
    with pytest.raises(ValueError, match="max_edges"):
        ctx.segment_adjacency(d, 8, 12, 2, max_edges=-1)
    with pytest.raises(ValueError, match="uint8"):
        ctx.segment_adjacency(d, 8, 12, 2, [ctx.to_device(np.zeros(96, np.float32))])
    assert np.array_equal(gpu_edges(ctx, seg), [[1, 2, 8]])    # the context works on after the refusals


def test_border_against_k25_on_the_device(ctx):
    from rsseg.regions import RegionGraph
    seg, n, mask = slic_map((65, 513))
    keep = np.random.RandomState(278).rand(*seg.shape) < 0.9
    for m in (None, keep):
        g = RegionGraph.from_table(gpu_edges(ctx, seg, (), m, n), n)
        dm = None if m is None else ctx.to_device(m.astype(np.uint8).reshape(-1))
        per = ctx.segment_features(ctx.to_device(seg.reshape(-1)), seg.shape[0], seg.shape[1], n, (), mask=dm).cpu().numpy()[:, 10]
        assert np.array_equal(g.border() + A.image_border_sides(seg, m, n), per)


def test_adjacency_with_float_planes_and_ranges(ctx):
    from rsseg import regions as RG
    from rsseg import segment as SG
    seg, n, mask = slic_map((45, 83))
    rs = np.random.RandomState(279)
    planes = [rs.uniform(-3, 9, seg.shape).astype(np.float32), rs.randint(0, 256, seg.shape).astype(np.uint8), rs.rand(*seg.shape).astype(np.float32)]
    ranges = [(-2.0, 8.0), None, None]
    q = [p.cpu().numpy().reshape(seg.shape) for p in SG.quantise_planes(ctx, planes, ranges)]
    assert all(p.dtype == np.uint8 for p in q) and np.array_equal(q[1], planes[1])
    g = RG.adjacency(seg, planes, mask=mask, ranges=ranges, ctx=ctx)
    want = A.adjacency_ref(seg, q, mask, n)
    assert g.n_segments == n and np.array_equal(g.table(), want) and g.contrast.shape == (len(want), 3)
    g0 = RG.adjacency(ctx.to_device(seg), ctx=ctx)             # a device map, no plane
    assert np.array_equal(g0.table(), A.adjacency_ref(seg, (), None, n)) and g0.contrast.shape[1] == 0
    with pytest.raises(ValueError, match="at most 16"):
        RG.adjacency(seg, [planes[1]] * 17, ctx=ctx)


def test_neighbour_features_and_object_features(ctx):
    from rsseg import objects as OB
    from rsseg import regions as RG
    seg, n, mask = slic_map((45, 83))
    rs = np.random.RandomState(280)
    planes = u8_planes(rs, seg.shape, 2) + [rs.randint(0, 256, seg.shape).astype(np.float32) / np.float32(4.0)]
    plain = OB.object_features(seg, planes, names=["a", "b", "c"], mask=mask, ctx=ctx)
    off = OB.object_features(seg, planes, names=["a", "b", "c"], mask=mask, ctx=ctx, neighbours=False)
    assert plain.columns == off.columns and plain.X.tobytes() == off.X.tobytes() and plain.table.tobytes() == off.table.tobytes()
    on = OB.object_features(seg, planes, names=["a", "b", "c"], mask=mask, ctx=ctx, neighbours=True)
    D = plain.X.shape[1]
    assert on.columns[:D] == plain.columns and on.X[:, :D].tobytes() == plain.X.tobytes()
    assert on.columns[D:] == ["n_neighbours", "shared_border"] + [f"{s}_boundary_contrast" for s in "abc"] + [f"{s}_neighbour_diff" for s in "abc"]
    from rsseg import segment as SG
    q2 = SG.quantise_planes(ctx, planes[2:], None)[0].cpu().numpy().reshape(seg.shape)   # as slic() quantises a float plane
    assert q2.dtype == np.uint8 and len(np.unique(q2)) > 100
    table = O.object_table_ref(seg, planes, mask, n)
    want = A.neighbour_features_ref(A.adjacency_ref(seg, planes[:2] + [q2], mask, n), table, [True, True, False])
    want[table[:, 0] == 0] = np.nan
    assert np.array_equal(on.X[:, D:], want, equal_nan=True)
    g = RG.adjacency(seg, planes, mask=mask, ctx=ctx)
    assert np.array_equal(RG.neighbour_features(g, table, [True, True, False]), A.neighbour_features_ref(g.table(), table, [True, True, False]))


@functools.lru_cache(maxsize=None)
def merge_scene():
    shape = (96, 130)
    planes = R.scene(281, shape, 3, cell=9, noise=0.05)
    mask = (np.random.RandomState(282).rand(*shape) < 0.95).astype(np.uint8)
    mask[40:44, 60:90] = 0
    return planes, mask


MERGE_CASES = [dict(threshold=30000.0), dict(threshold=40.0, criterion="boundary"), dict(scales=[3000.0, 30000.0, 300000.0]),
               dict(scales=[10.0, 30.0], criterion="boundary", min_area=40), dict(n_regions=12), dict(n_regions=3, criterion="boundary"),
               dict(threshold=3000.0, min_area=150), dict(min_area=120, criterion="boundary", weights=[1.0, 0.25, 3.0]),
               dict(threshold=1e12, max_rounds=2)]


@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
@pytest.mark.parametrize("masked", [False, True])
def test_merge_regions_against_the_restatement(ctx, case, masked):
    from rsseg import regions as RG
    from rsseg import segment as SG
    planes, mask = merge_scene()
    mask = mask if masked else None
    seg = SG.slic(planes, step=8, compactness=8.0, max_iter=4, mask=mask, ctx=ctx)     # a real SLIC map of the context
    n = int(seg.max())
    kw = MERGE_CASES[case]
    got = RG.merge_regions(seg, planes, mask=mask, ctx=ctx, **kw)
    want = A.merge_regions_ref(seg, planes, mask=mask, n_segments=n, **kw)
    assert got.labels.dtype == np.int32 and got.parent.dtype == np.int32 and len(want["history"]) > 0
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(got.parent, want["parent"]) and got.n_regions == want["n_regions"]
    assert [tuple(h) for h in got.history.tolist()] == want["history"]
    if "scales" in kw:
        assert len(got.scale_labels) == len(kw["scales"])
        for a, b, c, d in zip(got.scale_labels, want["scale_labels"], got.scale_parent, want["scale_parent"]):
            assert np.array_equal(a, b) and np.array_equal(c, d)
    else:
        assert got.scale_labels is None and got.scale_parent is None
    if "n_regions" in kw:
        assert got.n_regions == kw["n_regions"]
    assert got.graph == RG.adjacency(got.labels, planes, mask=mask, n_segments=got.n_regions, ctx=ctx)
    assert ((got.labels == 0) == (O.effective_labels(seg, mask) == 0)).all()


REGION_FILES = ("regions.npy", "region_graph.npz", "regions_stats.json")


def snapshot(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_stage_and_command(ctx, golden_dir, tmp_path):
    """python -m rsseg.regions on what a --classify kmeans --segment 8 run left: the region files appear beside the earlier
    files, which stay byte for byte what they are."""
    from rsseg import regions as RG
    from rsseg import runtime as rt
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    out = tmp_path / "run"
    sdir = out / "segmentation_results"
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        assert stages.main([str(tmp_path / "in.tif"), str(out), "--classify", "kmeans", "--n-clusters", "5", "--segment", "8",
                            "--segment-iterations", "4"]) == 0
        before = snapshot(str(out))
        assert RG.main([str(out), "--n-regions", "20", "--min-area", "30", "--class-map", str(sdir / "classification_kmeans.npy"),
                        "--method", "kmeans"]) == 0
        after = snapshot(str(out))
        assert all(after[k] == v for k, v in before.items())
        new = sorted(set(after) - set(before))
        assert new == sorted(os.path.join("segmentation_results", f)
                             for f in REGION_FILES + ("classification_kmeans_regions.npy", "kmeans_classification_map_regions.tif"))
        segments, raw = np.load(sdir / "segments.npy"), np.load(sdir / "classification_kmeans.npy")
        regions = np.load(sdir / "regions.npy")
        assert regions.dtype == np.int32 and regions.shape == segments.shape and regions.min() >= 1
        js = json.load(open(sdir / "regions_stats.json"))
        area = np.bincount(regions.reshape(-1))[1:]
        assert js["segments_in"] == segments.max() and js["regions_out"] == regions.max() == len(area) <= 20 and js["n_regions"] == 20
        assert js["maps"] == [{"regions_out": len(area), "area_min": int(area.min()), "area_median": float(np.median(area)),
                               "area_max": int(area.max())}]
        assert area.min() >= 30 and js["rounds"] >= 1 and js["merges"] == segments.max() - regions.max() and js["criterion"] == "ward"
        assert len(np.unique(np.stack([segments.reshape(-1), regions.reshape(-1)], axis=1), axis=0)) == segments.max()   # nested in the segments
        g = RG.RegionGraph.load(str(sdir / "region_graph.npz"))
        assert g.n_segments == regions.max() and np.array_equal(g.table()[:, :3], A.adjacency_ref(regions, (), None, g.n_segments))
        voted = np.load(sdir / "classification_kmeans_regions.npy")
        assert voted.dtype == np.uint8 and np.array_equal(voted, R.paint_ref(regions, R.segment_majority_ref(regions, raw, ignore=0, fill=0)))
        assert np.array_equal(read_tiff(str(sdir / "kmeans_classification_map_regions.tif"))[0], voted)
        # the stage itself, with scales: one map per scale, nested, into another directory
        import shutil
        other = tmp_path / "scales"
        shutil.copytree(str(out / "feature_outputs"), str(other / "feature_outputs"))
        res, stats, cm = stages.run_region_merge_stage(str(other / "feature_outputs" / "all_features_and_metadata.pkl"), segments,
                                                       str(other / "segmentation_results"), scales=[200.0, 5000.0], criterion="ward", ctx=ctx)
        assert cm is None and stats["scales"] == [200.0, 5000.0] and len(stats["maps"]) == 2
        m0, m1 = (np.load(other / "segmentation_results" / f"regions_{i}.npy") for i in range(2))
        assert m0.dtype == np.int32 and np.array_equal(m1, res.labels) and m0.max() >= m1.max()
        assert len(np.unique(np.stack([m0.reshape(-1), m1.reshape(-1)], axis=1), axis=0)) == m0.max()
        assert not (other / "segmentation_results" / "regions.npy").exists()
    finally:
        rt._default_ctx = prev
