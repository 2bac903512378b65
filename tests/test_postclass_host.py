"""CPU checks of the class-map clean-up (K20): the NumPy restatements of tests/postclass_ref.py against independent brute
force, the input validation of rsseg.postclass that needs no GPU, and the new command-line flags."""
import itertools

import numpy as np
import pytest

import postclass_ref as R


def brute_majority(q, k, ignore=-1, fill=-1, fill_only=False):
    """Per pixel: the clipped window, non-voters dropped, np.unique counts, the tie rule."""
    q = q.astype(np.int64)            # -1 ("none") compares unequal to every label
    H, W = q.shape
    r = k // 2
    out = q.copy()
    for y in range(H):
        for x in range(W):
            c = int(q[y, x])
            if c == ignore:
                continue
            if fill_only and c != fill:
                continue
            win = q[max(0, y - r):min(H, y + r + 1), max(0, x - r):min(W, x + r + 1)].ravel()
            win = win[(win != ignore) & (win != fill)]
            if win.size == 0:
                continue
            vals, cnt = np.unique(win, return_counts=True)
            tied = vals[cnt == cnt.max()]
            out[y, x] = c if (c != fill and c in tied) else tied.min()
    n_changed = int((out != q).sum())
    n_unfilled = int(((q == fill) & (out == fill)).sum()) if fill >= 0 else 0
    return out, n_changed, n_unfilled


def flood_sieve(q, min_area, connectivity, ignore, removed_value):
    q = q.astype(np.int64)
    H, W = q.shape
    seen = np.zeros((H, W), bool)
    out = q.copy()
    removed = 0
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for y in range(H):
        for x in range(W):
            if seen[y, x] or q[y, x] == ignore:
                continue
            stack, comp = [(y, x)], []
            seen[y, x] = True
            while stack:
                a, b = stack.pop()
                comp.append((a, b))
                for dy, dx in nb:
                    u, v = a + dy, b + dx
                    if 0 <= u < H and 0 <= v < W and not seen[u, v] and q[u, v] == q[y, x]:
                        seen[u, v] = True
                        stack.append((u, v))
            if len(comp) < min_area:
                removed += len(comp)
                for a, b in comp:
                    out[a, b] = removed_value
    return out, removed


MAPS = {
    "random5": lambda rs: rs.randint(0, 5, (24, 31)).astype(np.uint8),
    "random3_small": lambda rs: rs.randint(0, 3, (7, 5)).astype(np.uint8),
    "blocks": lambda rs: np.kron(rs.randint(0, 4, (6, 8)), np.ones((4, 4), int)).astype(np.uint8)[:23, :30],
    "one_pixel": lambda rs: np.array([[2]], np.uint8),
}


@pytest.mark.parametrize("k", [3, 5, 15])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_majority_ref_equals_brute_force(name, k):
    q = MAPS[name](np.random.RandomState(11))
    for ignore, fill, fill_only in itertools.product([-1, 0, 2], [-1, 0, 1], [False, True]):
        if ignore == fill and ignore >= 0:
            continue
        got = R.majority_ref(q, k, ignore, fill, fill_only)
        want = brute_majority(q, k, ignore, fill, fill_only)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (name, k, ignore, fill, fill_only)


@pytest.mark.parametrize("min_area", [2, 5, 40])
def test_sieve_ref_equals_the_oracle_area_filter_per_class(oracle, min_area):
    """8-connectivity: class by class, the component filter of advanced_post_processing (its middle step alone: no
    smoothing kernel, no hole filling)."""
    q = np.kron(np.random.RandomState(5).randint(0, 4, (8, 9)), np.ones((3, 3), int)).astype(np.uint8)
    flip = np.random.RandomState(6).rand(*q.shape) < 0.15
    q[flip] = np.random.RandomState(7).randint(0, 4, int(flip.sum()))
    got, removed = R.sieve_ref(q, min_area, 8, ignore=0, removed_value=0)
    want = np.zeros_like(q)
    for lab in (1, 2, 3):
        kept = oracle.advanced_post_processing((q == lab).astype(np.uint8), min_area=min_area, smooth_kernel_size=0, fill_holes=False)
        want[kept != 0] = lab
    assert np.array_equal(got, want)
    assert removed == int(((q != 0) & (want == 0)).sum())


@pytest.mark.parametrize("connectivity", [4, 8])
def test_sieve_ref_equals_flood_fill(connectivity):
    q = np.random.RandomState(3).randint(0, 3, (17, 23)).astype(np.uint8)
    for min_area, ignore, rv in [(0, 0, 0), (1, 0, 0), (3, 0, 0), (6, -1, 9), (6, 1, 7), (17 * 23 + 1, 0, 0)]:
        got = R.sieve_ref(q, min_area, connectivity, ignore, rv)
        want = flood_sieve(q, min_area, connectivity, ignore, rv)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], (min_area, ignore, rv)


def test_clean_ref_fills_what_it_removes():
    q = np.full((20, 20), 3, np.uint8)
    q[5, 5] = 1                    # an island of one pixel: removed, then grown over by 3
    q[0, :] = 0                    # nodata row: never votes, never filled
    out, st = R.clean_ref(q, min_area=2, window=3, nodata=0)
    assert st == {"removed": 1, "filled": 1, "left_as_nodata": 0, "fill_iterations": 1, "changed": []}
    assert out[5, 5] == 3 and np.array_equal(out[0], q[0]) and R.hole_value_ref(q, 0) == 255


# ---- rsseg.postclass: what it refuses before it needs a GPU ----
def test_class_map_validation():
    from rsseg import postclass as PC
    ok = PC.check_class_map(np.arange(12, dtype=np.int32).reshape(3, 4))
    assert ok.dtype == np.uint8 and ok.flags.c_contiguous and ok.shape == (3, 4)
    assert PC.check_class_map(np.array([[0, 255]], np.int64)).tolist() == [[0, 255]]
    with pytest.raises(ValueError, match="256"):
        PC.check_class_map(np.array([[1, 256]], np.int32))
    with pytest.raises(ValueError, match="-3"):
        PC.check_class_map(np.array([[-3, 5]], np.int16))
    with pytest.raises(ValueError, match="float"):
        PC.check_class_map(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="bool"):
        PC.check_class_map(np.zeros((2, 2), bool))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        PC.check_class_map(np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="empty"):
        PC.check_class_map(np.zeros((0, 4), np.uint8))


def test_arguments_are_checked_before_a_context_is_needed():
    from rsseg import postclass as PC
    m = np.ones((4, 4), np.uint8)
    with pytest.raises(ValueError, match="nodata=None"):
        PC.sieve(m, 3, nodata=None)
    with pytest.raises(ValueError, match="nodata=None"):
        PC.clean_class_map(m, 3, nodata=None)
    with pytest.raises(ValueError, match="connectivity"):
        PC.sieve(m, 3, connectivity=6)
    with pytest.raises(ValueError, match="min_area"):
        PC.sieve(m, -1)
    for bad in (1, 4, 17, 0):
        with pytest.raises(ValueError, match="window"):
            PC.majority_filter(m, window=bad)
    with pytest.raises(ValueError, match="nodata=300"):
        PC.majority_filter(m, nodata=300)
    with pytest.raises(ValueError, match="iterations"):
        PC.majority_filter(m, iterations=-1)
    with pytest.raises(ValueError, match="float"):
        PC.majority_filter(m.astype(np.float64))


def test_hole_value_and_group_mask():
    from rsseg import postclass as PC
    from rsseg.runtime import RssegUnsupported
    c = np.zeros(256, np.int64)
    c[[0, 3, 255]] = 5
    assert PC.hole_value(c, 0) == 254 and PC.hole_value(c, 254) == 253
    assert PC._group_mask(c, 0) == (1 << 0) | (1 << 31) and PC._group_mask(c, 3, 0) == 1 << 31
    full = np.ones(256, np.int64)
    with pytest.raises(RssegUnsupported):
        PC.hole_value(full, 0)
    full[7] = 0
    assert PC.hole_value(full, 0) == 7
    with pytest.raises(RssegUnsupported):
        PC.hole_value(full, 7)


def test_parser_flags_default_to_off():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "kmeans"])
    assert a.sieve == 0 and a.majority == 0 and a.majority_iterations == 1
    a = stages.parse_args(ap, ["in.tif", "out", "--classify", "random_forest", "--sieve", "50", "--majority", "5", "--majority-iterations", "3"])
    assert (a.sieve, a.majority, a.majority_iterations) == (50, 5, 3)
    for bad in (["--sieve", "5"], ["--classify", "kmeans", "--majority", "4"], ["--classify", "kmeans", "--majority", "17"],
                ["--classify", "kmeans", "--sieve", "-2"]):
        with pytest.raises(SystemExit):
            stages.parse_args(ap, ["in.tif", "out"] + bad)
