"""The software-pipelined tile walk of the k-means sweeps (km_moment, km_kpp, km_lloyd) at its seams, against the CPU oracle
(oracle/kmeans_impl.h) bit for bit: labels, centres, n_iter, the k-means++ seeds and the scaler.

A sweep kernel walks a chunk of 16 tiles and requests tile t + 1 while it consumes tile t; only full tiles are requested
ahead, the ragged tile loads for itself.  The pixel counts below put the end of the planes at every place where that can go
wrong: one tile or two, the tile behind the current one full, ragged or absent, the last tile of a chunk, the first tile of
the next chunk, several chunks with a ragged end.  Every plane is an allocation of exactly n elements, so a request at or
beyond n is not inside a larger buffer of the test's own."""
import numpy as np
import pytest

# the data, the exact-size device planes and the comparison itself are shared with the other k-means fit tests
from kmeans_fit_cases import blobs, check_fit

pytestmark = pytest.mark.gpu

THREADS, TILES_PER_CHUNK = 256, 16


def seam_sizes(dt):
    tile = THREADS * (4 if dt == np.float32 else 2)   # TILE = 256 * PXL
    chunk = TILES_PER_CHUNK * tile
    return [1, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 3, 15 * tile + 7, chunk - 1, chunk, chunk + 1, 2 * chunk + tile + 5]


def check(ctx, oracle, planes, k, tag, max_iter=300):
    return check_fit(ctx, oracle, planes, k, tag, max_iter=max_iter)


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("F", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_seams_of_the_pipelined_walk(ctx, oracle, dt, F, k):
    """every seam size x F (one plane; the bench's 15; a full, an over-full and the widest register-resident width) x k"""
    for i, n in enumerate(seam_sizes(dt)):
        kk = min(k, n)   # a fit with fewer samples than clusters is rejected (as scikit-learn does): n = 1 is fitted with k = 1
        planes = blobs(1000 * F + 10 * k + i, n, F, kk, dt, 0.35)
        check(ctx, oracle, planes, kk, dict(n=n, F=F, k=kk, dt=dt.__name__))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_noop_iterations_behind_convergence(ctx, oracle, dt):
    """Well-separated blobs converge within the first batch of four speculatively enqueued iterations: the sweeps behind the
    converged one find `done` set and return before any request."""
    n = seam_sizes(dt)[-1]
    info = check(ctx, oracle, blobs(77, n, 15, 8, dt, 0.01), 8, dict(n=n, dt=dt.__name__, case="separated"))
    assert info["n_iter"] <= 3, info["n_iter"]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_long_lloyd_run(ctx, oracle, dt):
    """Structureless data keeps Lloyd going (100 - 200 iterations if left alone; capped at 48 here to keep the oracle quick):
    several batches of the device-resident loop, the last one cut short by max_iter."""
    n = seam_sizes(dt)[-1]
    rng = np.random.default_rng(91)
    X = rng.random((n, 15))
    planes = [np.ascontiguousarray(X[:, f]).astype(dt) for f in range(15)]
    info = check(ctx, oracle, planes, 8, dict(n=n, dt=dt.__name__, case="long"), max_iter=48)
    assert info["n_iter"] >= 20, info["n_iter"]
