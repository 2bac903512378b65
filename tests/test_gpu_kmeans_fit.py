"""The k-means fit (rsseg_kmeans_fit_predict) against the CPU oracle bit for bit, in the parts where a wrong result would leave
the labels as they are: seeds, scaler, tol, n_iter, relocated, labels and CENTRES (tests/kmeans_fit_cases.py::assert_fit_equal).

  relocation   which pixel an empty cluster takes (km_farthest at every <T, KMAX, FR>, relocate, fetch_row, host_iteration, the
               hand-over from the device loop to the host loop); several chunks; a donor that runs out of pixels
  centres      every (T, KMAX, Lloyd form) of the launch table
  stop rules   tol and max_iter at every place of the device loop's batches
  seeds        RandomState(seed) other than 42

tests/test_kmeans_fit_cases_host.py checks on the CPU that these cases are what they claim to be.  Every plane is a device
allocation of exactly n elements."""
import numpy as np
import pytest

import kmeans_fit_cases as K

pytestmark = pytest.mark.gpu

RELOC = K.relocation_cases() + K.donor_cases()


@pytest.mark.parametrize("case", RELOC, ids=[c[0] for c in RELOC])
def test_relocated_centres(ctx, oracle, case):
    """The fit ends in the iteration that relocates: labels and n_iter are the same whichever pixels are taken, the centres of
    the relocated clusters are those pixels' rows and the donors' centres lack them."""
    _, gen, seed, n, F, k, d, t = case
    planes, _ = K.case_planes(case)
    info = K.check_fit(ctx, oracle, planes, k, case[0])
    assert info["relocated"] == k - d and info["n_iter"] == 2


def test_constant_planes(ctx, oracle):
    """one distinct row, three clusters: two are empty, the largest distance is 0, relocation is pointless"""
    planes = [np.full(K.small_n(np.float32), v, np.float32) for v in (0.25, -3.0, 7.5)]
    info = K.check_fit(ctx, oracle, planes, 3, "constant")
    labels, meta = ctx.kmeans_fit_predict(K.exact_planes(planes), 3)
    assert meta["relocated"] == 0 == info["relocated"] and not labels.cpu().numpy().any()


@pytest.mark.parametrize("t,k,F", K.table_cases(), ids=[f"{t}-k{k}-F{F}" for t, k, F in K.table_cases()])
def test_centres_across_the_launch_table(ctx, oracle, t, k, F):
    info = K.check_fit(ctx, oracle, K.table_planes(t, k, F), k, (t, k, F))
    assert info["n_iter"] >= 3, info["n_iter"]


@pytest.fixture(scope="module")
def stop_planes():
    return {c: K.stop_planes(c) for c in K.STOP_CASES}


@pytest.mark.parametrize("tol", K.TOLS)
@pytest.mark.parametrize("ci", range(len(K.STOP_CASES)), ids=[K.stop_id(c) for c in K.STOP_CASES])
def test_stop_rules(ctx, oracle, stop_planes, ci, tol):
    """tol x max_iter: the first batch of four, its boundary, a cut batch, and the iteration s in which unchanged labels and
    max_iter coincide; which rule ends the loop decides whether the final E-step runs"""
    c = K.STOP_CASES[ci]
    s = K.STOP_ITERS[ci][1]
    ended = set()
    for m in K.stop_max_iters(s) + [300]:
        info = K.check_fit(ctx, oracle, stop_planes[c], c[1], (K.stop_id(c), tol, m), max_iter=m, tol=tol)
        ended.add(info["n_iter"] == m)
    assert info["n_iter"] == K.STOP_ITERS[ci][K.TOLS.index(tol)]
    assert ended == {True, False}     # cut by max_iter, and ended by another rule before it


def test_max_iter_zero_is_refused(ctx):
    planes = K.exact_planes([np.arange(100, dtype=np.float32)])
    with pytest.raises(ValueError, match="kmeans: max_iter must be >= 1"):
        ctx.kmeans_fit_predict(planes, 2, max_iter=0)


@pytest.mark.parametrize("ci", [0, 3], ids=[K.stop_id(K.STOP_CASES[i]) for i in (0, 3)])
def test_other_seeds(ctx, oracle, stop_planes, ci):
    c = K.STOP_CASES[ci]
    base = oracle.kmeans_fit_planes(stop_planes[c], c[1])[1]["init_indices"]
    differ = 0
    for seed in K.OTHER_SEEDS:
        info = K.check_fit(ctx, oracle, stop_planes[c], c[1], (K.stop_id(c), seed), seed=seed)
        differ += not np.array_equal(info["init_indices"], base)
    assert differ > 0
