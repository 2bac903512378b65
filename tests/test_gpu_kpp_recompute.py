"""The recompute form of the k-means++ sampling rounds (km_kpp MODE 2 with the chosen-centre table, km_kpp_chunkq likewise)
and its hand-over to the closest-distance plane, against the CPU oracle (oracle/kmeans_impl.h) bit for bit: seeds, scaler,
tol, n_iter, labels and centres.  A wrong closest value moves a seed.

Rounds c <= depth re-derive min_j d2(centre_j, x) over the c chosen centres; with k - 1 <= depth no plane exists, otherwise
round `depth` stores its values as the whole plane and the later rounds read and rewrite it.  depth is KPP_RECOMPUTE (3) unless
RSSEG_KPP_RECOMPUTE = 0 ... 4 says otherwise (read at each fit), so k - 1 sits below, at and above the depth at k = 2, 3 | 4 |
5, 6, 8, 9, 10, 17, and the override puts the hand-over behind round 1, round 2 and round 4 (every slot of the table in use) of a
fit with k = 8.  F = 33 takes the feature-blocked kernels, which keep the plane rounds, as do the forms the launch table leaves
out (here: float64 with at most 8 planes and at most 4 candidates, the F = 1 cases).  Every plane is an allocation of exactly n elements.

The fits are cut at four Lloyd iterations: the seeding is what is under test, and four sweeps still carry a wrong seed into
the labels and centres."""
import numpy as np
import pytest

from kmeans_fit_cases import blobs, check_fit

pytestmark = pytest.mark.gpu

THREADS, TILES_PER_CHUNK = 256, 16
ENV = "RSSEG_KPP_RECOMPUTE"
FS = [1, 15, 16, 17, 32, 33]
KS = [2, 3, 4, 5, 6, 8, 9, 10, 17]
DTS = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
MAX_ITER = 4


def sizes(dt):
    tile = THREADS * (4 if dt == np.float32 else 2)   # TILE = 256 * PXL
    chunk = TILES_PER_CHUNK * tile
    return [tile - 1, tile + 1, chunk + 1, 2 * chunk + tile + 5]


@DTS
@pytest.mark.parametrize("F", FS)
def test_depth_below_at_and_above_k(ctx, oracle, monkeypatch, dt, F):
    """the default depth: no plane (k - 1 <= 3), hand-over behind round 3 with one (k = 5) to thirteen (k = 17) plane rounds"""
    monkeypatch.delenv(ENV, raising=False)
    for i, n in enumerate(sizes(dt)):
        for k in KS:
            planes = blobs(7000 * F + 10 * k + i, n, F, k, dt, 0.35)
            check_fit(ctx, oracle, planes, k, dict(n=n, F=F, k=k, dt=dt.__name__), max_iter=MAX_ITER)


@DTS
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_hand_over_at_small_depth(ctx, oracle, monkeypatch, depth, dt, F):
    """k = 8 with the hand-over behind round `depth`: the plane is written by a recompute round and read by a plane round"""
    monkeypatch.setenv(ENV, str(depth))
    for i, n in enumerate(sizes(dt)):
        planes = blobs(9000 * F + 100 * depth + i, n, F, 8, dt, 0.35)
        check_fit(ctx, oracle, planes, 8, dict(n=n, F=F, depth=depth, dt=dt.__name__), max_iter=MAX_ITER)


def tie_planes(n, F, dt):
    """integer-valued planes with few distinct rows: every centre has many pixels at distance exactly 0, and pixels halfway
    between two centres have equal distances to both"""
    rng = np.random.default_rng(5)
    X = rng.integers(0, 3, (n, F)) * 2
    return [np.ascontiguousarray(X[:, f]).astype(dt) for f in range(F)]


def nan_planes(n, F, k, dt):
    planes = blobs(31, n, F, k, dt, 0.35)
    rng = np.random.default_rng(32)
    for f in (1, F - 1):
        planes[f][rng.random(n) < 0.05] = np.nan
    return planes


@DTS
@pytest.mark.parametrize("depth", [None, 2])
def test_ties_and_zero_distances(ctx, oracle, monkeypatch, depth, dt):
    monkeypatch.delenv(ENV, raising=False)
    if depth is not None:
        monkeypatch.setenv(ENV, str(depth))
    n = sizes(dt)[-1]
    for F, k in ((3, 8), (4, 10)):
        check_fit(ctx, oracle, tie_planes(n, F, dt), k, dict(case="ties", F=F, k=k, depth=depth, dt=dt.__name__), max_iter=MAX_ITER)


@DTS
@pytest.mark.parametrize("depth", [None, 2])
def test_nans_in_two_planes(ctx, oracle, monkeypatch, depth, dt):
    monkeypatch.delenv(ENV, raising=False)
    if depth is not None:
        monkeypatch.setenv(ENV, str(depth))
    n = sizes(dt)[-1]
    for k in (8, 10):
        check_fit(ctx, oracle, nan_planes(n, 15, k, dt), k, dict(case="nan", k=k, depth=depth, dt=dt.__name__), max_iter=MAX_ITER)


@DTS
def test_depth_0_equals_the_default(ctx, oracle, monkeypatch, dt):
    """RSSEG_KPP_RECOMPUTE=0 (plane rounds throughout) and the default give the same fit in every output"""
    from kmeans_fit_cases import bits, exact_planes
    n = sizes(dt)[-1]
    for F, k in ((15, 8), (17, 4), (33, 8)):
        planes = blobs(50 + F, n, F, k, dt, 0.35)
        out = []
        for depth in (None, 0):
            monkeypatch.delenv(ENV, raising=False)
            if depth is not None:
                monkeypatch.setenv(ENV, str(depth))
            labels, meta = ctx.kmeans_fit_predict(exact_planes(planes), k, max_iter=MAX_ITER)
            out.append((labels.cpu().numpy(), meta))
        (la, ma), (lb, mb) = out
        assert np.array_equal(la, lb), (F, k)
        assert sorted(ma) == sorted(mb)
        for key in ma:
            if key in ("ms_init", "ms_lloyd"):   # wall-clock figures
                continue
            assert np.array_equal(bits(np.asarray(ma[key], dtype=np.float64)), bits(np.asarray(mb[key], dtype=np.float64))), (F, k, key)
        # and both are the oracle's fit
        monkeypatch.setenv(ENV, "0")
        check_fit(ctx, oracle, planes, k, dict(F=F, k=k, depth=0, dt=dt.__name__), max_iter=MAX_ITER)
