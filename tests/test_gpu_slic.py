"""K23 on the GPU against tests/slic_ref.py: the segmentation (degenerate rasters, grid remainders, tile seams, plane counts,
ties, weights, masks, connectivity enforcement, iteration counts), the per-segment reductions, the float path and the stage.
Everything is an integer or an exact ratio: np.array_equal throughout, the counters included.  The assignment kernel's tile
(64 columns x 16 rows at the time of writing) is read from the library."""
import json
import os

import numpy as np
import pytest

import slic_ref as R

pytestmark = pytest.mark.gpu


def gpu_slic(ctx, planes, S, weight, max_iter, min_area, mask=None):
    H, W = planes[0].shape
    d = [ctx.to_device(np.ascontiguousarray(p).reshape(-1)) for p in planes]
    m = None if mask is None else ctx.to_device(np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1))
    lab, n, it, rg = ctx.slic_u8(d, H, W, S, weight, max_iter, min_area, mask=m)
    return lab.cpu().numpy().reshape(H, W), n, it, rg


def check(ctx, planes, S, weight=0.5, max_iter=4, min_area=0, mask=None):
    got = gpu_slic(ctx, planes, S, weight, max_iter, min_area, mask)
    want = R.slic_ref(planes, S, weight, max_iter, min_area, mask)
    bad = np.argwhere(got[0] != want[0])
    what = (planes[0].shape, len(planes), S, weight, max_iter, min_area)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())
    assert got[0].dtype == np.int32 and got[1:] == want[1:], (what, got[1:], want[1:])
    return want


# ---- degenerate rasters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 4), (7, 9)])
def test_degenerate_rasters(ctx, shape):
    planes = R.scene(1, shape, 2, cell=2, noise=0.3)
    for S in (2, 5, 16):                                     # 16: the image is smaller than one cell
        for min_area in (0, 3):
            check(ctx, planes, S, min_area=min_area)


# ---- grid remainders and tile seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 5, 16, 33])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_grid_remainders(ctx, S, d):
    shape = (2 * S + d, 3 * S - d)
    planes = R.scene(2 + S, shape, 3, cell=max(3, S // 2), noise=0.15)
    want = check(ctx, planes, S, weight=0.2, min_area=S * S // 4)
    assert want[1] >= 1


def seam_shapes(ctx):
    tw, th = ctx.slic_tile()
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (2 * th + 1, 2 * tw - 1), (2 * th - 1, tw + 1), (65, 513)]


@pytest.mark.parametrize("i", range(6))
def test_tile_seams(ctx, i):
    shape = seam_shapes(ctx)[i]
    planes = R.scene(20 + i, shape, 3, cell=6, noise=0.15)
    for S in (5, 16):
        want = check(ctx, planes, S, weight=0.3, max_iter=3, min_area=S * S // 4)
        assert want[3] > 0                                   # pixels were regrown across the seams too


# ---- plane counts, ties, weights ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 7, 16])
def test_plane_counts(ctx, P):
    shape, S = (37, 70), 8
    check(ctx, R.scene(30 + P, shape, P, cell=7, noise=0.1), S, weight=0.4, min_area=16)
    # constant planes: the colour term is 0 for every candidate, only position decides and many distances tie
    const = [np.full(shape, 10 * p + 3, np.uint8) for p in range(P)]
    check(ctx, const, S, weight=1.0, min_area=16)
    # weight 0: position does not count
    check(ctx, R.scene(40 + P, shape, P, cell=5, noise=0.2), S, weight=0.0, min_area=4)


@pytest.mark.parametrize("P", [1, 3, 7, 16])
def test_very_large_weight_returns_the_grid(ctx, P):
    S, shape = 5, (20, 30)                                   # whole cells only: every pixel's own centre is its nearest
    planes = R.scene(50 + P, shape, P, cell=4, noise=0.3)
    want = check(ctx, planes, S, weight=1e12, max_iter=3, min_area=0)
    assert np.array_equal(want[0], R.grid_labels(*shape, S) + 1) and want[2] == 1


@pytest.mark.parametrize("P", [1, 3, 7, 16])
def test_exact_tie_goes_to_the_smaller_id(ctx, P):
    # S = 4, the last two columns masked: centres at x = 1.5 and 4.5 (same y), column 3 is 1.5 from both; constant colour
    mask = np.tile(np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8), (4, 1))
    planes = [np.full((4, 8), 9 * p + 1, np.uint8) for p in range(P)]
    want = check(ctx, planes, 4, weight=1.0, max_iter=5, min_area=0, mask=mask)
    assert want[0][0].tolist() == [1, 1, 1, 1, 2, 2, 0, 0] and want[2] == 1


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def test_masks(ctx):
    shape, S = (41, 75), 8
    planes = R.scene(60, shape, 3, cell=6, noise=0.15)
    check(ctx, planes, S, min_area=16, mask=None)
    strip = np.ones(shape, np.uint8)
    strip[:3], strip[:, -5:] = 0, 0
    check(ctx, planes, S, min_area=16, mask=strip)
    cells = np.ones(shape, np.uint8)                         # whole cells invalid: dead centres among the candidates
    cells[8:24, 16:40] = 0
    cells[32:, :8] = 0
    check(ctx, planes, S, min_area=16, mask=cells)
    check(ctx, planes, S, min_area=16, mask=np.zeros(shape, np.uint8))     # nothing valid: no segment
    assert R.slic_ref(planes, S, 0.5, 4, 16, np.zeros(shape, np.uint8))[1] == 0


def test_small_island_enclosed_by_invalid_pixels_survives(ctx):
    shape, S, min_area = (30, 40), 8, 16
    planes = R.scene(61, shape, 2, cell=6, noise=0.1)
    mask = np.ones(shape, np.uint8)
    mask[9:16, 9:16] = 0
    mask[11:13, 11:14] = 1                                   # six valid pixels, a moat of invalid ones around them
    want = check(ctx, planes, S, min_area=min_area, mask=mask)
    inside = np.zeros(shape, bool)
    inside[11:13, 11:14] = True
    island = np.unique(want[0][inside])                      # its own segment(s): nothing outside shares a label with it
    assert island.min() > 0 and not np.isin(want[0][~inside], island).any()
    assert int(np.isin(want[0], island).sum()) == 6 < min_area


# ---- enforcement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_area", [0, 1, 16, 10 ** 6])
def test_enforcement_on_noisy_blobs(ctx, min_area):
    shape, S = (50, 90), 8                                   # 16 = S * S / 4; 10^6: larger than the image
    planes = [R.blobs(np.random.RandomState(70 + p), shape, [0, 80, 160, 240], cell=5, noise=0.2) for p in range(3)]
    want = check(ctx, planes, S, weight=0.05, max_iter=4, min_area=min_area)
    assert (want[3] > 0) == (min_area == 16)


def test_snake_needs_many_growth_rounds(ctx):
    # a one-pixel path of valid pixels hanging off a valid block: with max_iter = 0 its pieces are smaller than min_area and
    # are regrown from the block, one pixel per round
    H, W, S = 21, 20, 4
    mask = np.zeros((H + 8, W), np.uint8)
    mask[:H] = R.snake(H, W) > 0
    mask[H - 1, 1] = 1
    mask[H:] = 1
    planes = [np.full(mask.shape, 100, np.uint8)]
    lab, _ = R.iterate(planes, S, 1.0, 0, mask)
    _, n_regrown, rounds = R.enforce(lab, 12)
    assert rounds > 40 and n_regrown > 100
    check(ctx, planes, S, weight=1.0, max_iter=0, min_area=12, mask=mask)


# ---- iterations ---------------------------------------------------------------------------------------------------------------------
def test_iteration_counts(ctx):
    shape, S = (40, 64), 8
    smooth = R.scene(80, shape, 2, cell=16, noise=0.0)
    want = check(ctx, smooth, S, weight=0.5, max_iter=40, min_area=0)
    assert 1 <= want[2] < 40                                 # converged early: the same n_iter on the GPU
    noisy = R.scene(81, shape, 3, cell=5, noise=0.3)
    assert R.iterate(noisy, S, 0.01, 6)[1] == 6              # still moving after six iterations
    for max_iter in (0, 1, 2):
        want = check(ctx, noisy, S, weight=0.01, max_iter=max_iter, min_area=0)
        assert want[2] == max_iter


def test_slic_refusals(ctx):
    p = ctx.to_device(np.zeros(12, np.uint8))
    for kw in (dict(step=1), dict(step=4097), dict(weight=-1.0), dict(weight=float("nan")), dict(max_iter=-1), dict(min_area=-1)):
        a = dict(step=4, weight=1.0, max_iter=1, min_area=0)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.slic_u8([p], 3, 4, a["step"], a["weight"], a["max_iter"], a["min_area"])
    from rsseg.runtime import RssegUnsupported
    with pytest.raises(RssegUnsupported):
        ctx.slic_u8([p] * 17, 3, 4, 4, 1.0, 1, 0)
    # a label plane that is not aligned to int32 is refused by name, before anything is launched
    import ctypes as C
    import torch
    buf = torch.zeros(12 * 4 + 4, dtype=torch.uint8, device=ctx.device)
    ns, ni, nr = C.c_int64(0), C.c_int(0), C.c_int64(0)
    rc = ctx.lib.rsseg_slic_u8(ctx.h, ctx._pp([p]), 1, 3, 4, None, 4, C.c_double(1.0), 1, 0, C.c_void_p(buf.data_ptr() + 1), C.byref(ns), C.byref(ni),
                               C.byref(nr))
    assert rc == -1 and b"d_labels" in ctx.lib.rsseg_last_error(ctx.h)
    assert int(buf.sum()) == 0


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segmap():
    shape = (45, 83)
    mask = np.ones(shape, np.uint8)
    mask[:2] = 0
    mask[20:24, 30:50] = 0
    seg, n, _, _ = R.slic_ref(R.scene(90, shape, 3, cell=6, noise=0.15), 8, 0.3, 3, 16, mask)
    return seg, n


def test_segment_sums_and_means(ctx, segmap):
    from rsseg import segment as SG
    seg, n = segmap
    rs = np.random.RandomState(91)
    u8 = [rs.randint(0, 256, seg.shape).astype(np.uint8) for _ in range(3)]
    unit = rs.uniform(-1, 1, seg.shape).astype(np.float32)
    top = rs.uniform(2040, 2047, seg.shape).astype(np.float32)
    bottom = (-top).astype(np.float32)
    assert np.bincount(seg.reshape(-1))[1:].max() * 2047 < 2 ** 23
    # below 2^-17 a float32 times 2^40 is no integer: the device's rounding (half to even) decides, exact halves included
    tiny = (rs.uniform(-1, 1, seg.shape) * 2.0 ** -18).astype(np.float32)
    halves = ((rs.randint(-4000, 4000, seg.shape) + 0.5) * 2.0 ** -40).astype(np.float32)
    assert np.array_equal(halves.astype(np.float64) * 2.0 ** 40 % 1.0, np.full(seg.shape, 0.5))
    planes = [u8[0], unit, u8[1], top, bottom, u8[2], tiny, halves]   # mixed: the wrapper sorts them into uint8 and float32 calls
    want = R.segment_sums_ref(seg, planes)
    assert np.array_equal(SG.segment_sums(seg, planes, ctx=ctx), want)
    assert np.array_equal(SG.segment_sums(seg, (), ctx=ctx), want[:, :3])
    means, (area, cy, cx) = SG.segment_means(seg, planes, ctx=ctx, return_geometry=True)
    assert np.array_equal(means[1:], R.segment_means_ref(seg, planes)[1:]) and np.isnan(means[0]).all()
    assert np.array_equal(area, want[:, 0])
    # a mask takes pixels out; 17 planes go in two calls
    m = rs.rand(*seg.shape) < 0.7
    many = [rs.randint(0, 256, seg.shape).astype(np.uint8) for _ in range(17)]
    assert np.array_equal(SG.segment_sums(seg, many, mask=m, ctx=ctx), R.segment_sums_ref(seg, many, mask=m))


def test_segment_sums_refusals(ctx, segmap):
    from rsseg import segment as SG
    seg, n = segmap
    ok = np.zeros(seg.shape, np.float32)
    big = ok.copy()
    big[30, 40] = 2048.0                                      # 2^11 itself is outside the exact domain
    with pytest.raises(ValueError, match=r"planes\[1\]"):
        SG.segment_means(seg, [ok, big], ctx=ctx)
    nan = ok.copy()
    nan[30, 40] = np.nan
    with pytest.raises(ValueError, match=r"planes\[0\].*NaN"):
        SG.segment_means(seg, [nan], ctx=ctx)
    keep = np.ones(seg.shape, np.uint8)
    keep[30, 40] = 0
    got = SG.segment_means(seg, [nan, big], mask=keep, ctx=ctx)
    assert np.array_equal(got[1:], R.segment_means_ref(seg, [nan, big], mask=keep)[1:])
    with pytest.raises(ValueError, match=r"planes\[0\].*2\^23"):   # one segment of 4900 pixels: area * max|x| >= 2^23
        SG.segment_means(np.ones((70, 70), np.int32), [np.full((70, 70), 2047.0, np.float32)], ctx=ctx)
    with pytest.raises(ValueError, match="outside"):          # a label above n_segments is refused, not used as an index
        SG.segment_sums(seg, (), n_segments=n - 1, ctx=ctx)


def test_segment_majority(ctx, segmap):
    from rsseg import segment as SG
    seg, n = segmap
    rs = np.random.RandomState(92)
    cm = R.blobs(rs, seg.shape, [0, 1, 2, 7, 200, 255], cell=4, noise=0.3)
    cm[seg == 3] = 0                                          # a segment whose only class is nodata: no voter
    s5 = np.flatnonzero(seg.reshape(-1) == 5)                 # an exact tie between 7 and 200 (and one 255 when the area is odd)
    flat = cm.reshape(-1)
    flat[s5] = 255
    flat[s5[:len(s5) // 2]] = 200
    flat[s5[len(s5) // 2:2 * (len(s5) // 2)]] = 7
    for nodata, fill in ((0, None), (None, None), (0, 9), (255, 3)):
        ig = -1 if nodata is None else nodata
        fl = max(ig, 0) if fill is None else fill
        want = R.segment_majority_ref(seg, cm, ignore=ig, fill=fl)
        got = SG.object_majority(seg, cm, nodata=nodata, fill=fill, ctx=ctx)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (nodata, fill)
    t = R.segment_majority_ref(seg, cm, ignore=0, fill=0)
    assert t[3] == 0 and t[5] == 7 and t.max() == 255
    # the object-based map is the table painted back
    assert np.array_equal(SG.object_classify(seg, cm, nodata=0, ctx=ctx), R.paint_ref(seg, t))
    # int32 class maps (KMeans labels) pass through check_class_map
    assert np.array_equal(SG.object_majority(seg, cm.astype(np.int32), nodata=0, ctx=ctx), t)


def test_paint(ctx, segmap):
    from rsseg import segment as SG
    seg, n = segmap
    rs = np.random.RandomState(93)
    for table in (rs.randint(0, 256, n + 1).astype(np.uint8), rs.randn(n + 1).astype(np.float32), rs.randint(-9, 9, n + 1).astype(np.int32)):
        got = SG.paint(seg, table, ctx=ctx)
        assert got.dtype == table.dtype and np.array_equal(got, R.paint_ref(seg, table))
    with pytest.raises(ValueError, match="table"):
        SG.paint(seg, np.zeros(n, np.uint8), ctx=ctx)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_float_planes_are_quantised_first(ctx):
    from rsseg import segment as SG
    import torch
    shape = (40, 70)
    rs = np.random.RandomState(94)
    base = R.scene(95, shape, 3, cell=7, noise=0.1)
    f = [(b.astype(np.float32) / 37.0 - 2.0 + rs.rand(*shape).astype(np.float32) * 0.01) for b in base]
    f[1][5, 5] = np.nan                                       # the range is the finite min / max
    mask = np.ones(shape, np.uint8)
    mask[5, 5] = 0
    q = []
    for p in f:
        fin = p[np.isfinite(p)]
        d = ctx.to_device(p.reshape(-1))
        q.append(ctx.normalize_quantize_u8(d, float(fin.min()), float(fin.max()), 255.0).cpu().numpy().reshape(shape))
    got, st = SG.slic(f, step=8, compactness=6.0, max_iter=3, mask=mask, ctx=ctx, return_stats=True)
    via_u8, st8 = SG.slic(q, step=8, compactness=6.0, max_iter=3, mask=mask, ctx=ctx, return_stats=True)
    assert np.array_equal(got, via_u8) and st == st8 and st["min_area"] == 16
    want = R.slic_ref(q, 8, SG.slic_weight(6.0, 8), 3, 16, mask)
    assert np.array_equal(got, want[0]) and (st["n_segments"], st["n_iter"], st["n_regrown"]) == want[1:]
    # n_segments instead of step; a (P, H, W) array; a device result
    dev = SG.slic(np.stack(q), n_segments=44, max_iter=2, ctx=ctx, device=True)
    S = SG.slic_step(shape, 44)
    assert dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), R.slic_ref(q, S, SG.slic_weight(10.0, S), 2, max(1, S * S // 4))[0])
    # ranges replace the plane's own extrema
    r = SG.slic(f[:1], step=8, ranges=[(-3.0, 6.0)], max_iter=2, ctx=ctx)
    q0 = ctx.normalize_quantize_u8(ctx.to_device(f[0].reshape(-1)), -3.0, 6.0, 255.0).cpu().numpy().reshape(shape)
    assert np.array_equal(r, R.slic_ref([q0], 8, SG.slic_weight(10.0, 8), 2, 16)[0])


SEGMENT_FILES = ("segments.npy", "segment_stats.json")
OBJECT_FILES = ("classification_kmeans_objects.npy", "kmeans_classification_map_objects.tif")


def test_stage_flags(ctx, golden_dir, tmp_path):
    """python -m rsseg.stages ... --classify kmeans --segment 8 --object-based: the segment files appear beside the raw map's,
    which stay byte for byte what they are, and the object map is the majority of that raw map per segment."""
    from rsseg import runtime as rt
    from rsseg import segment as SG
    from rsseg import stages
    from rsseg.tiff import read_tiff, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    common = ["--classify", "kmeans", "--n-clusters", "5"]
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain")] + common) == 0
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "seg")] + common
                           + ["--segment", "8", "--compactness", "12", "--segment-iterations", "4", "--object-based"]) == 0
    finally:
        rt._default_ctx = prev
    plain, seg = tmp_path / "plain" / "segmentation_results", tmp_path / "seg" / "segmentation_results"
    assert not any((plain / f).exists() for f in SEGMENT_FILES + OBJECT_FILES)
    assert all((seg / f).exists() for f in SEGMENT_FILES + OBJECT_FILES)
    for f in ("classification_kmeans.npy", "kmeans_classification_map.tif"):
        assert open(plain / f, "rb").read() == open(seg / f, "rb").read(), f
    segments, raw = np.load(seg / "segments.npy"), np.load(seg / "classification_kmeans.npy")
    assert segments.dtype == np.int32 and segments.shape == raw.shape and segments.min() >= 1
    js = json.load(open(seg / "segment_stats.json"))
    area = np.bincount(segments.reshape(-1))[1:]
    assert js["n_segments"] == segments.max() == len(area) and (js["step"], js["compactness"], js["max_iter"], js["min_area"]) == (8, 12.0, 4, 16)
    assert (js["area_min"], js["area_median"], js["area_max"]) == (area.min(), float(np.median(area)), area.max())
    assert 1 <= js["n_iter"] <= 4 and js["n_regrown"] >= 0 and js["planes_used"] == min(js["planes_in_stack"], 16)
    objects = np.load(seg / OBJECT_FILES[0])
    assert np.array_equal(objects, R.paint_ref(segments, R.segment_majority_ref(segments, raw, ignore=0, fill=0)))
    assert np.array_equal(objects, R.paint_ref(segments, SG.object_majority(segments, raw, ctx=ctx)))
    assert np.array_equal(read_tiff(str(seg / OBJECT_FILES[1]))[0], objects)
