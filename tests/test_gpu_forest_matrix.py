"""Every instantiation of the K11 forest kernels once, on the GPU, against the NumPy walk of
tests/test_forest_proba_host.py with exact equality: nine (row width, threads) pairs x {LDS-group, general} x {label,
proba, out-of-bag, permutation counts}.  The cases and what they are there for are in tests/forest_matrix_cases.py;
tests/test_forest_matrix_cases_host.py asserts on the CPU that each case takes the route it claims."""
import numpy as np
import pytest

import forest_matrix_cases as T
from test_forest_proba_host import flat_oob, flat_proba

pytestmark = pytest.mark.gpu


def perm_counts(flat, X, y, src, jobs):
    """What rsseg_forest_permutation_counts counts, from the NumPy walk: the rows whose first-maximum class equals y."""
    out = []
    for f, s in jobs:
        Xs = X.copy()
        if f >= 0:
            Xs[:, f] = X[src[s], f]
        out.append(int((np.argmax(flat_proba(flat, Xs), axis=1) == y).sum()))
    return np.array(out, np.int64)


@pytest.mark.parametrize("name", list(T.BY_NAME))
def test_every_entry_point_equals_the_numpy_walk(ctx, name):
    from rsseg import _lib as L
    case = T.build(name)
    flat, jobs = case.flat, np.array(case.jobs, np.dtype(L.PERM_JOB))
    ctx.forest_load(flat)
    n_all = case.X.shape[0]
    for n in (n_all, 1):          # two workgroups, the second with one pixel; then a single pixel
        X, counts, y = case.X[:n], np.ascontiguousarray(case.counts[:, :n]), case.y[:n]
        src = case.src if n == n_all else np.zeros((2, 1), np.int32)
        want = flat_proba(flat, X)
        labels = flat["classes"][np.argmax(want, axis=1)]
        pl = [ctx.to_device(X[:, f].copy()) for f in range(X.shape[1])]
        assert np.array_equal(ctx.forest_predict(pl).cpu().numpy(), labels), n
        proba, conf, lab = ctx.forest_predict_proba(pl, proba=True, confidence=True, labels=True)
        assert np.array_equal(proba.cpu().numpy().T, want), n
        assert np.array_equal(conf.cpu().numpy(), want.max(1)), n
        assert np.array_equal(lab.cpu().numpy(), labels), n
        want_oob, want_n = flat_oob(flat, X, counts)
        oob, n_oob = ctx.forest_oob(pl, ctx.to_device(counts.reshape(-1).copy()))
        assert np.array_equal(oob.cpu().numpy(), want_oob), n
        assert np.array_equal(n_oob.cpu().numpy(), want_n), n
        got = ctx.forest_permutation_counts(pl, ctx.to_device(y.copy()), ctx.to_device(src.reshape(-1).copy()), jobs)
        assert np.array_equal(got, perm_counts(flat, X, y, src, case.jobs)), n
