"""GPU suite: K1 (csrc/k1_select.hip) swept over every path of its radix select against np.sort.

The table of tests/select_cases.py is built so that each case takes a path the earlier K1 tests never reach at their
sizes — the batched loop with four loads in flight (through the RSSEG_K1_GRID workgroup cap), the early stop of the
small-integer pass inside that loop, second `k1_hist` launches for more than eight live prefixes, every shape of the
pass-2 prefix tables, the value classes at the edges of the key — and tests/test_select_cases_host.py checks on the CPU
that it does.  Here every case must return np.sort's values and NaN count, and make exactly the number of `select`
launches tests/select_ref.py predicts for it, so a case that silently took another route fails too.

Comparisons are exact: values with np.array_equal(equal_nan=True) (the sign of a zero is not compared, see
select_ref.py), launch counts as integers."""
import numpy as np
import pytest

import select_cases as T
import select_ref as R

pytestmark = pytest.mark.gpu


def _cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("RSSEG_K1_GRID", raising=False)
    else:
        monkeypatch.setenv("RSSEG_K1_GRID", str(cap))


def _counted(ctx, call):
    """call() and the number of `select` launches it made."""
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        out = call()
        launches = ctx.prof_get("select")[1]
    finally:
        ctx.prof_enable(False)
    return out, launches


def _check(case, i, vals, n_nan):
    want, want_nan = R.expected(case.planes[i], case.ranks[i])
    assert int(n_nan) == want_nan, (case.name, i)
    assert vals.dtype == np.float32
    assert np.array_equal(vals, want, equal_nan=True), (case.name, i, vals, want)


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case(ctx, monkeypatch, name):
    case = T.BY_NAME[name]
    _cap(monkeypatch, case.grid_cap)
    dev = [ctx.to_device(p) for p in case.planes]
    predicted = R.predicted_launches(case.planes, case.ranks)
    (vals, nans), launches = _counted(ctx, lambda: ctx.order_stats_multi(dev, case.ranks))
    for i in range(len(dev)):
        _check(case, i, vals[i], nans[i])
    assert launches == predicted
    if len(dev) == 1:
        (v1, nn1), launches = _counted(ctx, lambda: ctx.order_stats(dev[0], case.ranks[0]))
        _check(case, 0, v1, nn1)
        assert launches == predicted


@pytest.mark.parametrize("name,n,ranks,offset,text", T.REFUSALS, ids=[r[0] for r in T.REFUSALS])
def test_refusals(ctx, monkeypatch, name, n, ranks, offset, text):
    _cap(monkeypatch, None)
    a = np.arange(n + offset, dtype=np.float32)
    if name != "rank-n-ints":
        a += np.float32(0.5)                        # general floats: the rank is refused after pass 0, not after the one-pass route
    d = ctx.to_device(a)[offset:]
    assert d.numel() == n and d.data_ptr() % 16 == 4 * offset
    with pytest.raises(ValueError, match=text):
        ctx.order_stats(d, ranks)
    with pytest.raises(ValueError, match=text):
        ctx.order_stats_multi([d], [ranks])
    # the context works on
    v, nn = ctx.order_stats(ctx.to_device(a[:n]), [0])
    assert v[0] == a[0] and nn == 0


@pytest.mark.parametrize("name", ["g3_11S+5_t2-normal", "g3_11S+5_t2-nan", "g2_8S+777_t3-normal", "g2_8S+777_t3-nan"])
def test_percentiles_end_to_end(ctx, monkeypatch, name):
    """np.percentile / np.nanmedian / np.nanpercentile through the product's own wrappers, inside the batched loop."""
    from rsseg.quantiles import band_percentiles, robust_scaler_stats
    case = T.BY_NAME[name]
    _cap(monkeypatch, case.grid_cap)
    a = case.planes[0]
    d = ctx.to_device(a)
    for got, want in zip(band_percentiles(ctx, d, (2, 98)), (np.percentile(a, 2), np.percentile(a, 98))):
        assert np.asarray(got).dtype == want.dtype
        assert got == want or (np.isnan(got) and np.isnan(want))
    assert np.isnan(np.percentile(a, 2)) == name.endswith("-nan")
    center, scale = robust_scaler_stats(ctx, d)
    want_c = np.nanmedian(a)
    q = np.nanpercentile(a, (25.0, 75.0))
    want_s = q[1] - q[0]
    assert np.asarray(center).dtype == want_c.dtype and np.asarray(scale).dtype == want_s.dtype
    assert center == want_c and scale == want_s


def test_sharded_over_thread_ranks(ctx, monkeypatch):
    """The `wide` plane cut into a rank of five elements, a rank of none and a rank with the rest: every rank returns the
    order statistics and the NaN count of the whole plane, from as many launches as the whole plane needs."""
    from rsseg.runtime import Context
    from test_gpu_dist import _ThreadWorld
    _cap(monkeypatch, None)
    whole, ranks, splits = T.sharded_case()
    whole = whole.copy()
    whole[[7, 1000]] = np.nan                      # a NaN count that only the third rank sees
    want, want_nan = R.expected(whole, ranks)
    predicted = R.predicted_launches([whole], [ranks])
    world = len(splits) - 1
    tw = _ThreadWorld(world)
    out = [None] * world

    class Empty:
        """A zero-length view of a real allocation: torch reports no address for an empty tensor, the entry point
        refuses a null pointer."""
        def __init__(self, base):
            self.base, self.dtype = base, base.dtype

        def data_ptr(self):
            return self.base.data_ptr()

        def numel(self):
            return 0

    def rank_main(r):
        c = Context(0, use_dist=False)
        try:
            c.install_comm_hook(r, world, tw.hook(r))
            a, b = splits[r], splits[r + 1]
            d = c.to_device(whole[a:b].copy()) if b > a else Empty(c.to_device(np.zeros(4, np.float32)))
            c.prof_reset()
            c.prof_enable(True)
            try:
                v, nn = c.order_stats(d, ranks)
                launches = c.prof_get("select")[1]
            finally:
                c.prof_enable(False)
            vm, nm = c.order_stats_multi([d], [ranks])
            out[r] = (v, nn, launches, vm[0], int(nm[0]))
        finally:
            c.close()

    tw.run(rank_main)
    assert tw.calls == 2 * 4                         # per call: the small-integer pass and three radix passes
    for r in range(world):
        v, nn, launches, vm, nm = out[r]
        assert nn == want_nan == 2 and nm == want_nan, r
        assert np.array_equal(v, want, equal_nan=True) and np.array_equal(vm, want, equal_nan=True), r
        assert launches == predicted, r


def test_uint8_two_load_loop(ctx, monkeypatch):
    """k1_hist_u8 on 100.7 MB: 1031 lanes make two iterations of the two-load loop, all others one iteration and one step
    of the tail loop (tests/test_select_cases_host.py::test_u8_plane_splits_the_lanes_as_stated), against np.bincount;
    and the small-integer float32 route on the first 300 007 bytes widened, against np.bincount of that prefix."""
    _cap(monkeypatch, None)
    a = T.u8_plane()
    n = a.size
    assert a.min() == 0 and a.max() == 255
    ranks = T.ranks16(n)
    ranks[1], ranks[-2] = 1, n - 2
    want, _ = R.expected(a, ranks)
    assert want[0] == 0 and want[-1] == 255
    d = ctx.upload_band(a)
    (vals, nn), launches = _counted(ctx, lambda: ctx.order_stats(d, ranks))
    assert nn == 0 and launches == 1
    assert np.array_equal(vals, want)
    m = 300007
    r2 = T.ranks16(m)
    w = ctx.widen_u8(d[:m])
    assert np.array_equal(w.cpu().numpy(), a[:m].astype(np.float32))
    (v2, nn2), launches = _counted(ctx, lambda: ctx.order_stats(w, r2))
    assert nn2 == 0 and launches == 1
    assert np.array_equal(v2, R.expected(a[:m], r2)[0])
