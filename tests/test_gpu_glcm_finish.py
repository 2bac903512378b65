"""The per-window finish of the register texture kernels (csrc/k4_glcm.hip: the 32-bit integer finish of k4_glcm_quad,
k4_glcm_pair and k4_glcm_thread, and k4_glcm_quad's table of square roots) on planes that reach the ends of what those
code paths assume:

  * the 32-bit bounds: with np = 42 pairs per angle and levels L, M1 = sum(a + b) <= 2 np (L - 1) and M2 * 2 np,
    Mx * 2 np <= (2 np (L - 1))^2 = 28 005 264 at L = 64.  A plane at the top level everywhere reaches all three at once
    (and den = 0: correlation 1.0); a 0 / top checkerboard at one-pixel pitch has the largest contrast and dissimilarity
    numerators and the largest M2 * 2 np - M1^2; stripes make single angles constant while the others alternate;
  * the table of sqrt(2 i), i = A / 2 = np + D + 2 E2: a constant window is its top (A = 84^2, i = 3528 for 0 / 90 degrees,
    i = 2592 for the diagonals), a window whose pairs are all distinct and off the diagonal its bottom (i = np);
  * odd and even map widths and heights (threads of the 2 x 2 kernel with one or two windows), maps wider than one
    workgroup strip (128 windows).

Everything is compared bit for bit with the oracle (mode 1); at 32 levels also under RSSEG_GLCM_DENSE=pair (above 32 levels
the window runs on k4_glcm_thread, which carries the same finish: the oracle alone is the check there).  A CPU test
checks that the planes put the extrema where this docstring says.
"""
import os

import numpy as np
import pytest

PROPS = ["contrast", "dissimilarity", "homogeneity", "energy", "correlation"]
WIN = 7
NP0, NP1 = WIN * (WIN - 1), (WIN - 1) * (WIN - 1)          # pairs per angle: 0 / 90 degrees, 45 / 135 degrees
OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))                # 0, 45, 90, 135 degrees
SHAPES = ((21, 140), (20, 141), (21, 141), (22, 142))       # maps 15 x 134, 14 x 135, 15 x 135, 16 x 136
SQRT_TABLE_TOP = 2 * NP0 * NP0                              # 3528


def plane(kind, levels, H, W):
    top = levels - 1
    r, c = np.indices((H, W))
    if kind == "top":
        q = np.full((H, W), top)
    elif kind == "zero":
        q = np.zeros((H, W), np.int64)
    elif kind == "mid":
        q = np.full((H, W), levels // 2 + 1)
    elif kind == "checker":
        q = ((r + c) & 1) * top
    elif kind == "columns":
        q = (c & 1) * top
    elif kind == "rows":
        q = (r & 1) * top
    elif kind == "random":
        q = np.random.default_rng([levels, H, W]).integers(0, levels, (H, W))
    elif kind == "mixed":
        # top-level block | checkerboard | random | zero block, side by side: windows straddle every border between them
        q = np.random.default_rng([levels, H, W, 1]).integers(0, levels, (H, W))
        q[:, : W // 4] = top
        q[:, W // 4: W // 2] = (((r + c) & 1) * top)[:, W // 4: W // 2]
        q[H // 2:, 3 * W // 4:] = 0
    else:
        raise ValueError(kind)
    return q.astype(np.uint8)


KINDS = ("top", "zero", "mid", "checker", "columns", "rows", "random", "mixed")


def window_extremes(q, levels):
    """Per angle over all 7 x 7 windows of q: (min A/2, max A/2, max M1, max M2 * 2 np, max Mx * 2 np, max |den|, max contrast
    numerator sum (a - b)^2) from the definitions, in Python integers."""
    H, W = q.shape
    out = []
    q = q.astype(np.int64)
    for dr, dc in OFFSETS:
        lo_i, hi_i, m1, m2n, mxn, den, s2 = 1 << 62, 0, 0, 0, 0, 0, 0
        for y in range(H - WIN + 1):
            for x in range(W - WIN + 1):
                w = q[y:y + WIN, x:x + WIN]
                c0, c1 = (0, WIN - dc) if dc >= 0 else (-dc, WIN)
                a = w[0:WIN - dr, c0:c1].ravel()
                b = w[dr:WIN, c0 + dc:c1 + dc].ravel()
                n = a.size
                key, cnt = np.unique(np.minimum(a, b) * levels + np.maximum(a, b), return_counts=True)
                diag = (key // levels) == (key % levels)
                half = int((cnt[~diag] ** 2).sum() + 2 * (cnt[diag] ** 2).sum())
                M1, M2, Mx = int((a + b).sum()), int((a * a + b * b).sum()), int(2 * (a * b).sum())
                lo_i, hi_i = min(lo_i, half), max(hi_i, half)
                m1, m2n, mxn = max(m1, M1), max(m2n, M2 * 2 * n), max(mxn, Mx * 2 * n)
                den = max(den, abs(M2 * 2 * n - M1 * M1))
                s2 = max(s2, int(((a - b) ** 2).sum()))
        out.append((lo_i, hi_i, m1, m2n, mxn, den, s2))
    return out


@pytest.mark.parametrize("levels", [32, 64])
def test_planes_reach_the_bounds(levels):
    top = levels - 1
    bound = (2 * NP0 * top) ** 2
    assert (2 * NP0 * 63) ** 2 == 28005264 < 1 << 25
    H, W = 13, 40
    ex = window_extremes(plane("top", levels, H, W), levels)
    for (lo_i, hi_i, m1, m2n, mxn, den, s2), n in zip(ex, (NP0, NP1, NP0, NP1)):
        assert lo_i == hi_i == 2 * n * n                      # constant window: one diagonal cell holding every pair
        assert (m1, m2n, mxn, den) == (2 * n * top, (2 * n * top) ** 2, (2 * n * top) ** 2, 0)
    assert ex[0][1] == SQRT_TABLE_TOP and ex[0][3] == bound
    ex = window_extremes(plane("checker", levels, H, W), levels)
    for a in (0, 2):                                          # 0 / 90 degrees: every pair is {0, top}
        assert ex[a][6] == NP0 * top * top and ex[a][4] == 0 and ex[a][0] == NP0 * NP0
        assert ex[a][5] == NP0 * top * top * 2 * NP0 - (NP0 * top) ** 2
    ex = window_extremes(plane("random", levels, *SHAPES[2]), levels)
    for (lo_i, *_), n in zip(ex, (NP0, NP1, NP0, NP1)):
        assert lo_i == n                                      # some window has all pairs distinct and off the diagonal
    for kind in ("columns", "rows"):
        ex = window_extremes(plane(kind, levels, H, W), levels)
        # along the stripes every pair is equal (two diagonal cells of 24 and 18 pairs), across them every pair is {0, top}
        assert max(e[1] for e in ex) == 2 * (24 * 24 + 18 * 18) and max(e[6] for e in ex) == NP0 * top * top


def _maps(ctx, q, levels):
    H, W = q.shape
    got, (oh, ow) = ctx.glcm(ctx.to_device(np.ascontiguousarray(q).reshape(-1)), H, W, levels, WIN, 1)
    assert (oh, ow) == (H - WIN + 1, W - WIN + 1)
    return [g.cpu().numpy().reshape(oh, ow) for g in got]


@pytest.fixture(params=["quad", "pair"])
def dense_kernel(request):
    old = os.environ.get("RSSEG_GLCM_DENSE")
    os.environ["RSSEG_GLCM_DENSE"] = request.param
    yield request.param
    if old is None:
        os.environ.pop("RSSEG_GLCM_DENSE", None)
    else:
        os.environ["RSSEG_GLCM_DENSE"] = old


def _check(ctx, oracle, levels, kind, shape, tag):
    q = plane(kind, levels, *shape)
    want = oracle.glcm_small_maps(q, levels, WIN, 1, mode=1)
    got = _maps(ctx, q, levels)
    for g, k in zip(got, PROPS):
        w = want[k]
        if not np.array_equal(g.view(np.int32), np.asarray(w, np.float32).view(np.int32)):
            bad = np.argwhere(g.view(np.int32) != np.asarray(w, np.float32).view(np.int32))
            y, x = (int(v) for v in bad[0])
            raise AssertionError(f"{tag} levels={levels} plane={kind} map={g.shape} {k}: {len(bad)} windows differ, first at "
                                 f"({y}, {x}): got {g[y, x]!r} want {w[y, x]!r}")
    if kind in ("top", "zero", "mid"):
        assert np.all(got[4] == 1.0) and np.all(got[3] == 1.0) and np.all(got[0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_finish_32_levels_vs_oracle_both_dense_kernels(ctx, oracle, dense_kernel, kind, shape):
    _check(ctx, oracle, 32, kind, shape, dense_kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_finish_64_levels_vs_oracle(ctx, oracle, kind, shape):
    _check(ctx, oracle, 64, kind, shape, "thread")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "mixed", "checker"])
def test_quad_equals_pair_bit_for_bit(ctx, kind):
    """The two dense kernels against each other on a map of several workgroup strips (odd width and height)."""
    q = plane(kind, 32, 53, 403)
    old = os.environ.get("RSSEG_GLCM_DENSE")
    try:
        os.environ["RSSEG_GLCM_DENSE"] = "pair"
        a = _maps(ctx, q, 32)
        os.environ["RSSEG_GLCM_DENSE"] = "quad"
        b = _maps(ctx, q, 32)
    finally:
        if old is None:
            os.environ.pop("RSSEG_GLCM_DENSE", None)
        else:
            os.environ["RSSEG_GLCM_DENSE"] = old
    for x, y, k in zip(a, b, PROPS):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), k
