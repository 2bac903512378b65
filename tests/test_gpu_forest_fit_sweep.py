"""K16 on the GPU against scikit-learn over the case list of tests/forest_fit_cases.py (what each case reaches is asserted on
the CPU by tests/test_forest_fit_cases_host.py): the sort paths at their root sizes with and without ties, the scan's chunk
seams, the 2048-node launch seam and the DFS stack on chains, value classes, capacity at size, parameters above 4096 samples,
count rows that are no bootstrap, and the refusals of the C entry point.  Whole fitted state, floats bitwise, no tolerance.

Figures for the record (MI355X, one run): chain_5000 (9999 nodes, depth 4999) fits in 0.53 s (scikit-learn 1.04 s), the whole
module takes 15 s; `-s` prints every case with its wall times."""
import ctypes as C
import time

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier

import forest_fit_cases as K
from test_forest_fit_host import state_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_equals_sklearn(ctx, name):
    from rsseg.forest_fit import fit
    _, X, y, kw, _ = K.case(name)
    t0 = time.perf_counter()
    want = RandomForestClassifier(n_jobs=8, **kw).fit(X, y)
    t1 = time.perf_counter()
    got = fit(RandomForestClassifier(n_jobs=8, **kw), X, y, ctx=ctx)
    t2 = time.perf_counter()
    nodes = [t.tree_.node_count for t in want.estimators_]
    print(f"\n[K16 sweep] {name}: n={X.shape[0]} F={X.shape[1]} trees={len(nodes)} nodes<={max(nodes)} depth<={max(t.tree_.max_depth for t in want.estimators_)}: "
          f"K16 {t2 - t1:.3f} s, scikit-learn {t1 - t0:.3f} s")
    state_equal(want, got)


def upload(ctx, X, y, counts):
    planes = [ctx.upload_f32(np.ascontiguousarray(X[:, f])) for f in range(X.shape[1])]
    return planes, ctx.to_device(y, np.int32), ctx.to_device(np.ascontiguousarray(counts).reshape(-1), np.int32)


def caps_of(counts, T):
    m = (np.asarray(counts) > 0).sum(axis=1)
    return 2 * (m if len(m) == T else np.repeat(m, T)) - 1


@pytest.mark.parametrize("name", list(K.DIRECT))
def test_count_rows_equal_sklearn(ctx, name):
    """Context.forest_fit with count rows that sum to n but are no bootstrap, against DecisionTreeClassifier(sample_weight=row)."""
    from rsseg import forest_fit as FF
    _, X, y, counts, seeds, p, _ = K.direct_case(name)
    want = K.direct_reference(name)
    planes, d_y, d_counts = upload(ctx, X, y, counts)
    xs = np.array([FF.splitter_seed(s) for s in seeds], np.uint32)
    trees = ctx.forest_fit(planes, d_y, d_counts, xs, caps_of(counts, len(seeds)), p["max_depth"], p["min_samples_split"],
                           p["min_samples_leaf"], p["max_features"], p["n_classes"])
    assert len(trees) == len(want)
    for t, (w, g) in enumerate(zip(want, trees)):
        K.assert_nodes_equal(FF.tree_nodes(w), g, f"{name}[{t}]")


# ---- refusals of rsseg_forest_fit: each is decided from scalar arguments before any launch, or by k16_fit_init's guards
# (it writes only below the stated m and marks the tree done, so k16_fit_step does nothing) --------------------------------
def small_problem(ctx, T=2, F=3, seed=0):
    from rsseg import forest_fit as FF
    X, y = K.lattice(400, seed=seed)
    X = np.ascontiguousarray(np.resize(X.T, (F, 400)).T)
    counts = np.stack([FF.bootstrap_counts(100 + t, 400) for t in range(T)]).astype(np.int32)
    xs = np.array([FF.splitter_seed(100 + t) for t in range(T)], np.uint32)
    return X, y, counts, xs


def call(ctx, X, y, counts, xs, caps, C_=3, mss=2, msl=1):
    planes, d_y, d_counts = upload(ctx, X, y, counts)
    return ctx.forest_fit(planes, d_y, d_counts, xs, caps, K.INT_MAX, mss, msl, 2, C_)


def raw_call(ctx, X, y, counts, xs, caps, n_arg):
    """rsseg_forest_fit itself, with `n_arg` in place of the planes' length."""
    import torch
    planes, d_y, d_counts = upload(ctx, X, y, counts)
    T = len(xs)
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    total = int(off[-1])
    nc, md = np.zeros(T, np.int64), np.zeros(T, np.int32)
    i32 = [ctx.empty(total, torch.int32) for _ in range(5)]
    f64 = [ctx.empty(total, torch.float64) for _ in range(2)]
    miss, value = ctx.empty(total, torch.uint8), ctx.empty(total * 3, torch.float64)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    ctx._chk(ctx.lib.rsseg_forest_fit(ctx.h, ctx._pp(planes), len(planes), n_arg, vp(d_y), 3, vp(d_counts), 0, T,
                                      xs.ctypes.data_as(C.POINTER(C.c_uint32)), K.INT_MAX, 2, 1, 2, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                      vp(i32[0]), vp(i32[1]), vp(i32[2]), vp(f64[0]), vp(f64[1]), vp(i32[3]), vp(i32[4]), vp(miss), vp(value),
                                      nc.ctypes.data_as(C.POINTER(C.c_int64)), md.ctypes.data_as(C.POINTER(C.c_int32))))


def test_refusals_of_the_entry_point(ctx):
    from rsseg import forest_fit as FF
    from rsseg.runtime import RssegUnsupported
    X, y, counts, xs = small_problem(ctx)
    caps = caps_of(counts, 2)
    X65 = small_problem(ctx, F=65)[0]
    with pytest.raises(RssegUnsupported, match="65 features"):
        call(ctx, X65, y, counts, xs, caps)
    with pytest.raises(RssegUnsupported, match="65 classes"):
        call(ctx, X, y, counts, xs, caps, C_=65)
    with pytest.raises(ValueError, match="min_samples_split=1"):
        call(ctx, X, y, counts, xs, caps, mss=1)
    with pytest.raises(ValueError, match="not 2m-1"):
        call(ctx, X, y, counts, xs, caps + np.array([0, 1]))
    with pytest.raises(ValueError, match="samples > n"):
        call(ctx, X, y, counts, xs, np.array([caps[0], 2 * 401 - 1]))
    with pytest.raises(MemoryError, match="tree 1 .*sample count mismatch"):
        call(ctx, X, y, counts, xs, caps - np.array([0, 2]))      # m understated by one
    with pytest.raises(MemoryError, match="tree 0 .*sample count mismatch"):
        call(ctx, X, y, counts, xs, caps + np.array([2, 0]))      # m overstated by one (still <= n)
    # n = 0 and n = 2^26 are refused from the scalar alone: the buffers are those of the 400-sample problem and are never read
    for n_arg in (0, 1 << 26):
        with pytest.raises(ValueError, match="1 <= n < 2\\^26"):
            raw_call(ctx, X, y, counts, xs, caps, n_arg)
    # the context is as good as before: the same call with honest arguments equals scikit-learn
    from sklearn.tree import DecisionTreeClassifier
    trees = call(ctx, X, y, counts, xs, caps)
    for t in range(2):
        want = DecisionTreeClassifier(max_features=2, random_state=100 + t).fit(X, y, sample_weight=counts[t].astype(np.float64))
        K.assert_nodes_equal(FF.tree_nodes(want), trees[t], f"after refusals[{t}]")


def test_count_rows_that_do_not_sum_to_n_are_refused(ctx):
    """weighted_n_samples is taken as n (include/rsseg.h), so a row with another sum, or a negative count, is RSSEG_ERR_INVALID."""
    X, y, counts, xs = small_problem(ctx, seed=1)
    caps = caps_of(counts, 2)
    k = int(np.flatnonzero(counts[1] > 1)[0])
    for delta in (1, -1, 400):
        bad = counts.copy()
        bad[1, k] += delta                                        # m is unchanged: only the sum is wrong
        assert (bad[1] > 0).sum() == (counts[1] > 0).sum() and bad[1].sum() != 400
        with pytest.raises(ValueError, match="tree 1: the counts are negative or do not sum to n = 400"):
            call(ctx, X, y, bad, xs, caps)
    neg = counts.copy()
    z = int(np.flatnonzero(counts[0] == 0)[0])
    neg[0, z] = -1                                                # the sum is repaired, a count is negative
    neg[0, int(np.flatnonzero(counts[0] > 0)[0])] += 1
    assert neg[0].sum() == 400
    with pytest.raises(ValueError, match="tree 0: the counts are negative or do not sum to n"):
        call(ctx, X, y, neg, xs, caps)
    one = np.full((1, 400), 2, np.int32)                          # a shared row (same_counts) that sums to 2n
    with pytest.raises(ValueError, match="do not sum to n"):
        call(ctx, X, y, one, xs, np.array([799, 799]))
    call(ctx, X, y, counts, xs, caps)                             # and the honest rows still fit
