"""K20 on the GPU against tests/postclass_ref.py: the majority filter (every window, tile seams, label groups, ties, special
values, rows form), the multi-class sieve, clean_class_map and the stage.  Everything is an integer: np.array_equal throughout,
the counters included.  The tile is 256 columns x 32 rows, a thread owns 4 columns x 8 rows; windows above 9 stage a wider
halo (8 columns instead of 4)."""
import itertools
import json
import os

import numpy as np
import pytest

import postclass_ref as R

pytestmark = pytest.mark.gpu

WINDOWS = (3, 5, 7, 9, 11, 13, 15)


def gpu_majority(ctx, q, k, ignore=-1, fill=-1, fill_only=False, **kw):
    H, W = q.shape
    out, nc, nu = ctx.majority_u8(ctx.to_device(q.reshape(-1)), H, W, k, ignore=ignore, fill=fill, fill_only=fill_only, **kw)
    return out.cpu().numpy().reshape(-1, W), nc, nu


def check_majority(ctx, q, k, ignore=-1, fill=-1, fill_only=False):
    got, nc, nu = gpu_majority(ctx, q, k, ignore, fill, fill_only)
    want, wc, wu = R.majority_ref(q, k, ignore, fill, fill_only)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (q.shape, k, ignore, fill, fill_only, len(bad), bad[:5].tolist())
    assert (nc, nu) == (wc, wu), (q.shape, k, ignore, fill, fill_only)
    return want, wc, wu


def blobs(rs, shape, labels, cell=5, noise=0.2):
    """cells of `cell` x `cell` pixels of one label, `noise` of the pixels redrawn: smooth regions, edges and speckle"""
    labels = np.asarray(labels)
    H, W = shape
    coarse = labels[rs.randint(0, len(labels), (H // cell + 1, W // cell + 1))]
    q = np.kron(coarse, np.ones((cell, cell), int))[:H, :W]
    flip = rs.rand(H, W) < noise
    q[flip] = labels[rs.randint(0, len(labels), int(flip.sum()))]
    return np.ascontiguousarray(q, dtype=np.uint8)


# ---- majority filter ----
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 5)])
def test_window_larger_than_the_image(ctx, shape):
    q = np.random.RandomState(1).randint(0, 4, shape).astype(np.uint8)
    for k in (3, 15):
        check_majority(ctx, q, k)
        check_majority(ctx, q, k, ignore=0)
        check_majority(ctx, q, k, fill=0)


@pytest.mark.parametrize("shape", [(31, 255), (32, 256), (33, 257), (65, 513), (40, 258), (40, 261)])
def test_tile_seams_and_unaligned_widths(ctx, shape):
    q = blobs(np.random.RandomState(2), shape, range(8))
    for k in (3, 9, 15):
        check_majority(ctx, q, k)


@pytest.mark.parametrize("shape", [(33, 257), (65, 513)])
@pytest.mark.parametrize("k", WINDOWS)
def test_every_window(ctx, k, shape):
    q = blobs(np.random.RandomState(3), shape, range(9), cell=k)      # labels 0..8: two groups
    _, nc, _ = check_majority(ctx, q, k, ignore=0)
    assert nc > 0


LABEL_SETS = {
    "0..7": list(range(8)),
    "0..8": list(range(9)),
    "0..16": list(range(17)),
    "1..64": list(range(1, 65)),
    "sparse": [0, 200, 255],
    "all256": list(range(256)),
}


@pytest.mark.parametrize("k", [5, 11])
@pytest.mark.parametrize("name", sorted(LABEL_SETS))
def test_label_groups(ctx, name, k):
    q = blobs(np.random.RandomState(4), (65, 513), LABEL_SETS[name], cell=4, noise=0.3)
    assert set(np.unique(q).tolist()) == set(LABEL_SETS[name])
    check_majority(ctx, q, k)
    # a group mask naming more groups than occur gives the same map
    got, _, _ = gpu_majority(ctx, q, k, group_mask=0xffffffff)
    assert np.array_equal(got, R.majority_ref(q, k)[0])


def test_constant_map_is_a_fixed_point(ctx):
    for v, k in ((0, 3), (7, 7), (255, 15)):
        q = np.full((33, 257), v, np.uint8)
        want, nc, nu = check_majority(ctx, q, k)
        assert nc == 0 and nu == 0 and np.array_equal(want, q)


def test_ties_centre_rule(ctx):
    yy, xx = np.mgrid[0:40, 0:261]
    board = (1 + (yy + xx) % 2).astype(np.uint8)                  # two-label checkerboard
    stripes = (3 + (xx % 3) * 2).astype(np.uint8) + np.zeros_like(board)   # three-label columns 3, 5, 7
    for q, k in ((board, 5), (board, 3), (stripes, 3), (stripes, 9)):
        centre, smallest = R.tie_kinds(q, k)
        want, _, _ = check_majority(ctx, q, k)
        if q is stripes and k in (3, 9):
            assert centre > q.size // 2, (k, centre)               # k a multiple of 3: every interior count ties
    # an even split needs an even number of cells: only clipped windows on the checkerboard tie
    c3, s3 = R.tie_kinds(board, 3)
    assert c3 > 0 and s3 == 0


def test_ties_smallest_label_rule(ctx):
    """Lone pixels of label 9 on a 1 / 2 checkerboard: a 3 x 3 window centred on a 9 holds four 1s and four 2s, so the centre's
    label is not among the maxima and the smaller label wins; its neighbours lose one vote and tie with the centre among
    the maxima.  Both kinds of tie occur, counted from the reference's box counts alone."""
    yy, xx = np.mgrid[0:65, 0:513]
    q = (1 + (yy + xx) % 2).astype(np.uint8)
    lone = (yy % 6 == 3) & (xx % 6 == 2) & (yy > 0) & (yy < 64) & (xx > 0) & (xx < 512)
    q[lone] = 9
    centre, smallest = R.tie_kinds(q, 3)
    assert smallest >= int(lone.sum()) > 0 and centre > 0
    want, _, _ = check_majority(ctx, q, 3)
    assert (want[lone] == 1).all()
    # the same with labels in different groups of eight: 1 against 200
    q2 = q.copy()
    q2[q == 2] = 200
    want2, _, _ = check_majority(ctx, q2, 3)
    assert (want2[lone] == 1).all()
    for k in (5, 13):
        check_majority(ctx, q2, k)


def test_special_values(ctx):
    rs = np.random.RandomState(6)
    q = blobs(rs, (33, 257), [0, 1, 2, 3, 4, 5, 255], cell=3, noise=0.3)
    for ignore, fill, fill_only in itertools.product([-1, 0, 255, 3], [-1, 0, 255], [False, True]):
        if ignore == fill and ignore >= 0:
            continue
        check_majority(ctx, q, 5, ignore, fill, fill_only)
    check_majority(ctx, q, 13, 3, 0, True)
    check_majority(ctx, q, 13, 255, 0, False)


def test_fill_block_wider_than_the_window_and_all_fill(ctx):
    q = blobs(np.random.RandomState(7), (40, 261), [1, 2, 3])
    q[10:30, 100:140] = 0
    for k in (3, 7, 11):
        for fill_only in (False, True):
            _, nc, nu = check_majority(ctx, q, k, ignore=-1, fill=0, fill_only=fill_only)
            assert nu == (20 - 2 * (k // 2)) * (40 - 2 * (k // 2)) and nc >= 800 - nu
    allfill = np.full((33, 257), 4, np.uint8)
    for k in (3, 15):
        want, nc, nu = check_majority(ctx, allfill, k, fill=4)
        assert nc == 0 and nu == allfill.size and np.array_equal(want, allfill)


@pytest.mark.parametrize("y0,y1", [(0, 30), (30, 70), (70, 97)])
def test_rows_form_equals_the_rows_of_the_whole_map(ctx, y0, y1):
    H, W, k, r = 97, 300, 7, 3
    q = blobs(np.random.RandomState(8), (H, W), range(12))
    q[q == 11] = 0
    whole, _, _ = R.majority_ref(q, k, ignore=-1, fill=0)
    p0, p1 = max(0, y0 - r), min(H, y1 + r)
    stripe = np.ascontiguousarray(q[p0:p1])
    got, nc, nu = gpu_majority(ctx, stripe, k, fill=0, rows=(y0 - p0, y1 - p0), image_rows=(p0, H))
    assert got.shape == (y1 - y0, W) and np.array_equal(got, whole[y0:y1])
    assert nc == int((whole[y0:y1] != q[y0:y1]).sum()) and nu == int(((q[y0:y1] == 0) & (whole[y0:y1] == 0)).sum())
    if p0 > 0:       # a stripe without its halo is refused, not clipped at the stripe's edge
        with pytest.raises(ValueError, match="halo"):
            gpu_majority(ctx, np.ascontiguousarray(q[y0:p1]), k, fill=0, rows=(0, y1 - y0), image_rows=(y0, H))


def test_majority_refuses_bad_arguments(ctx):
    import torch
    q = ctx.to_device(np.zeros(64, np.uint8))
    for kw, word in (({"k": 4}, "k = 4"), ({"k": 17}, "k = 17"), ({"k": 1}, "k = 1"), ({"k": 3, "ignore": 256}, "ignore"),
                     ({"k": 3, "fill": -2}, "fill"), ({"k": 3, "ignore": 5, "fill": 5}, "ignore and fill"), ({"k": 3, "rows": (2, 9)}, "rows"),
                     ({"k": 3, "out": q}, "d_out is d_q")):
        with pytest.raises(ValueError, match=word):
            ctx.majority_u8(q, 8, 8, **kw)
    with pytest.raises(ValueError, match="connectivity"):
        ctx.sieve_u8(q, 8, 8, 3, connectivity=6)
    with pytest.raises(ValueError, match="removed_value"):
        ctx.sieve_u8(q, 8, 8, 3, removed_value=256)


# ---- sieve ----
def gpu_sieve(ctx, q, min_area, connectivity=8, ignore=0, removed_value=0):
    H, W = q.shape
    out, n = ctx.sieve_u8(ctx.to_device(q.reshape(-1)), H, W, min_area, connectivity, ignore, removed_value)
    return out.cpu().numpy().reshape(H, W), n


def check_sieve(ctx, q, min_area, connectivity=8, ignore=0, removed_value=0):
    got, n = gpu_sieve(ctx, q, min_area, connectivity, ignore, removed_value)
    want, wn = R.sieve_ref(q, min_area, connectivity, ignore, removed_value)
    assert np.array_equal(got, want) and n == wn, (q.shape, min_area, connectivity, ignore, removed_value, int((got != want).sum()), n, wn)
    return want, wn


def per_label_today(ctx, q, min_area, ignore=0, removed_value=0):
    """the way it is done without the sieve: remove_small_components once per label on host-made binary masks"""
    H, W = q.shape
    out = q.copy()
    for lab in np.unique(q):
        if lab == ignore:
            continue
        kept = ctx.remove_small_components(ctx.to_device((q == lab).astype(np.uint8).reshape(-1)), H, W, min_area).cpu().numpy().reshape(H, W)
        out[(q == lab) & (kept == 0)] = removed_value
    return out


@pytest.mark.parametrize("n_labels", [2, 8, 65])
def test_sieve_random_maps(ctx, n_labels):
    q = blobs(np.random.RandomState(9), (65, 513), range(n_labels), cell=3, noise=0.25)
    for conn in (8, 4):
        want, n = check_sieve(ctx, q, 6, conn)
        assert 0 < n < q.size
    want, _ = check_sieve(ctx, q, 6, 8)
    assert np.array_equal(per_label_today(ctx, q, 6), want)
    check_sieve(ctx, q, 12, 8, ignore=-1, removed_value=255)


def test_sieve_serpentine_across_tiles(ctx):
    """a one-pixel-wide snake of label 5 through three tile columns and three tile rows on a background of label 2"""
    H, W = 70, 600
    q = np.full((H, W), 2, np.uint8)
    for i, y in enumerate(range(1, H - 1, 2)):
        q[y, 1:W - 1] = 5
        if y + 1 < H - 1:
            q[y + 1, W - 2 if i % 2 == 0 else 1] = 5
    snake = int((q == 5).sum())
    for conn in (4, 8):
        want, n = check_sieve(ctx, q, snake, conn)           # exactly min_area: kept
        assert n == int(((q == 2) & (want == 0)).sum())
        want, n = check_sieve(ctx, q, snake + 1, conn)       # one more: the snake goes
        assert (want[q == 5] == 0).all()
    assert np.array_equal(per_label_today(ctx, q, snake + 1), R.sieve_ref(q, snake + 1)[0])


def test_sieve_connectivity_labels_and_thresholds(ctx):
    q = np.full((33, 257), 1, np.uint8)
    q[4:7, 4:7] = 3
    q[7:10, 7:10] = 3            # touches the first blob only diagonally: one component of 18 at 8, two of 9 at 4
    q[20:23, 100:104] = 4        # 12 pixels of label 4 ...
    q[20:23, 104:108] = 6        # ... edge to edge with 12 pixels of label 6: never merged
    q[28, 30:39] = 7             # exactly 9 pixels
    q[30, 30:40] = 7             # exactly 10 pixels
    w8, n8 = check_sieve(ctx, q, 10, 8)
    assert n8 == 9 and (w8[4:7, 4:7] == 3).all() and (w8[28, 30:39] == 0).all() and (w8[30, 30:40] == 7).all()
    w4, n4 = check_sieve(ctx, q, 10, 4)
    assert n4 == 27 and (w4[4:7, 4:7] == 0).all() and (w4[7:10, 7:10] == 0).all()
    w, n = check_sieve(ctx, q, 13, 8)
    assert (w[20:23, 100:108] == 0).all()                   # 12 + 12 of different labels are two components below 13
    assert np.array_equal(per_label_today(ctx, q, 13), w)
    # ignore pixels split a component: a bar of 3s cut by a column of the ignored value
    s = np.full((9, 40), 1, np.uint8)
    s[4, 5:25] = 3
    s[4, 15] = 0
    w, n = check_sieve(ctx, s, 11, 8, ignore=0, removed_value=0)
    assert n == 19 and (w[4, 5:25] == 0).all()
    w, n = check_sieve(ctx, s, 10, 8, ignore=0, removed_value=0)
    assert n == 9 and (w[4, 5:15] == 3).all()
    # the same bar with nothing ignored: the 0 is a component of one pixel
    check_sieve(ctx, s, 2, 8, ignore=-1, removed_value=9)


def test_sieve_identity_and_everything(ctx):
    q = blobs(np.random.RandomState(10), (40, 261), range(5))
    for min_area in (0, 1):
        want, n = check_sieve(ctx, q, min_area)
        assert n == 0 and np.array_equal(want, q)
    want, n = check_sieve(ctx, q, q.size + 1)
    assert n == int((q != 0).sum()) and not want.any()


# ---- public module and stage ----
def noisy_map(rs, H=70, W=300):
    q = blobs(rs, (H, W), [1, 2, 3, 4, 5], cell=9, noise=0.10)
    q[:3] = 0
    q[-2:] = 0
    q[:, :4] = 0
    q[:, -3:] = 0
    q[30:42, 120:150] = 0          # a nodata hole
    q[50:56, 200:206] = 6          # a block of a label of its own: 36 pixels, more than one 3 x 3 pass grows over
    return q


def test_clean_class_map_equals_the_reference(ctx):
    from rsseg import postclass as PC
    q = noisy_map(np.random.RandomState(12))
    for kw in ({"min_area": 8}, {"min_area": 8, "window": 5, "majority_iterations": 3}, {"min_area": 0, "majority_iterations": 2},
               {"min_area": 40, "max_fill_iterations": 1}, {"min_area": 5, "connectivity": 4}):
        got, st = PC.clean_class_map(q.astype(np.int32), ctx=ctx, return_stats=True, **kw)
        want, wst = R.clean_ref(q, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, want), kw
        assert st == wst, (kw, st, wst)
        assert not got[q == 0].any(), "a nodata pixel gained a label"
        assert not (got == R.hole_value_ref(q, 0)).any(), "the temporary hole value is still in the map"
    got, st = PC.clean_class_map(q, min_area=8, ctx=ctx, return_stats=True)
    assert st["removed"] > 0 and st["filled"] + st["left_as_nodata"] == st["removed"]
    _, st1 = PC.clean_class_map(q, min_area=40, max_fill_iterations=1, ctx=ctx, return_stats=True)
    assert st1["left_as_nodata"] > 0, "the one-pass case must leave holes, or it does not test the leftover path"


def test_majority_filter_and_sieve_functions(ctx):
    import torch
    from rsseg import postclass as PC
    q = noisy_map(np.random.RandomState(13))
    assert np.array_equal(PC.majority_filter(q, 5, ctx=ctx), R.majority_ref(q, 5, ignore=0)[0])
    assert np.array_equal(PC.majority_filter(q, 5, nodata=None, ctx=ctx), R.majority_ref(q, 5)[0])
    assert np.array_equal(PC.majority_filter(q, 3, fill_nodata=True, ctx=ctx), R.majority_ref(q, 3, fill=0)[0])
    # iterations: the reference loop, stopped once a pass changes nothing
    want, changed = q, []
    for _ in range(50):
        want, nc, _ = R.majority_ref(want, 3, ignore=0)
        changed.append(nc)
        if nc == 0:
            break
    assert changed[-1] == 0 and 1 < len(changed) < 50
    got, st = PC.majority_filter(q, 3, iterations=50, ctx=ctx, return_stats=True)
    assert np.array_equal(got, want) and st == {"iterations": len(changed), "n_changed": changed, "n_unfilled": 0}
    got, st = PC.majority_filter(q, 3, iterations=2, ctx=ctx, return_stats=True)
    assert st["n_changed"] == changed[:2]
    # a device tensor in, a device tensor out; the input is not written
    t = torch.from_numpy(q.astype(np.int32)).to(ctx.device)
    out = PC.majority_filter(t, 7, ctx=ctx, device=True)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == q.shape
    assert np.array_equal(out.cpu().numpy(), R.majority_ref(q, 7, ignore=0)[0]) and np.array_equal(t.cpu().numpy(), q)
    got, st = PC.sieve(q, 8, ctx=ctx, return_stats=True)
    want, n = R.sieve_ref(q, 8)
    assert np.array_equal(got, want) and st == {"n_removed": n}
    assert np.array_equal(PC.sieve(q, 8, connectivity=4, ctx=ctx), R.sieve_ref(q, 8, 4)[0])
    assert np.array_equal(ctx.hist_u8(ctx.to_device(q.reshape(-1))[3:]), np.bincount(q.reshape(-1)[3:], minlength=256))


STAGE_FILES = ("classification_kmeans_clean.npy", "kmeans_classification_map_clean.tif", "postclass_stats.json")


def test_run_postclass_stage_writes_the_three_files(ctx, tmp_path):
    from rsseg import stages
    from rsseg.tiff import read_tiff
    q = noisy_map(np.random.RandomState(14))
    clean, stats = stages.run_postclass_stage(q, str(tmp_path), "kmeans", min_area=8, window=3, majority_iterations=2, ctx=ctx)
    want, wst = R.clean_ref(q, min_area=8, window=3, majority_iterations=2)
    assert sorted(os.listdir(tmp_path)) == sorted(STAGE_FILES)
    assert np.array_equal(np.load(tmp_path / STAGE_FILES[0]), want) and np.array_equal(clean, want)
    assert np.array_equal(read_tiff(str(tmp_path / STAGE_FILES[1]))[0], want)
    js = json.load(open(tmp_path / STAGE_FILES[2]))
    assert {k: js[k] for k in wst} == wst
    assert js["class_counts_before"] == {str(v): int((q == v).sum()) for v in np.unique(q)}
    assert js["class_counts_after"] == {str(v): int((want == v).sum()) for v in np.unique(want)}


def test_stage_flags(ctx, golden_dir, tmp_path):
    """python -m rsseg.stages ... --classify kmeans: without the flags none of the three files; with them the cleaned map of
    the very map the run wrote, whose own files do not change."""
    from rsseg import runtime as rt
    from rsseg import stages
    from rsseg.tiff import write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:296]
    write_tiff(str(tmp_path / "in.tif"), dn, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    roi = np.zeros((96, 96), np.int16)          # three labelled blocks: --evaluate assesses the raw map and, beside it, the cleaned one
    roi[10:30, 10:30], roi[40:60, 50:80], roi[70:90, 20:60] = 1, 2, 3
    np.save(tmp_path / "roi.npy", roi)
    common = ["--classify", "kmeans", "--n-clusters", "5", "--evaluate", str(tmp_path / "roi.npy")]
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "plain")] + common) == 0
        assert stages.main([str(tmp_path / "in.tif"), str(tmp_path / "clean")] + common + ["--sieve", "6", "--majority", "3", "--majority-iterations", "2"]) == 0
    finally:
        rt._default_ctx = prev
    assert (tmp_path / "plain" / "evaluation_results" / "evaluation_report.txt").exists() and not (tmp_path / "plain" / "evaluation_results_clean").exists()
    assert (tmp_path / "clean" / "evaluation_results" / "evaluation_report.txt").exists()
    assert (tmp_path / "clean" / "evaluation_results_clean" / "evaluation_report.txt").exists()
    plain, clean = tmp_path / "plain" / "segmentation_results", tmp_path / "clean" / "segmentation_results"
    assert not any((plain / f).exists() for f in STAGE_FILES)
    for f in ("classification_kmeans.npy", "kmeans_classification_map.tif"):
        assert open(plain / f, "rb").read() == open(clean / f, "rb").read(), f
    raw = np.load(clean / "classification_kmeans.npy")
    want, wst = R.clean_ref(raw, min_area=6, window=3, majority_iterations=2)
    assert np.array_equal(np.load(clean / STAGE_FILES[0]), want) and wst["removed"] > 0
    assert all((clean / f).exists() for f in STAGE_FILES)
