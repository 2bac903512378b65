"""GPU suite for K3 (csrc/k3_pca.hip): every form of the PCA entry points against tests/pca_ref.py, the NumPy / Python-int
restatement of the kernels and their host driver (itself held to scikit-learn and float64 by tests/test_pca_host.py).
Every comparison is bit for bit: model (mean, components, explained variance, ratios), every score plane, the extrema tags,
and for the fused pass the seven indices, the normalised bands and the byte plane."""
import numpy as np
import pytest

import pca_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


# ------------------------------------------------------------------------------------------------ data and helpers
def make_planes(n, nb, kind, seed):
    """nb correlated planes of n pixels.  kind: 'unit' float32 in [0, 1]; 'float' general float32 in [0, 255]; 'bytes' float32
    holding only the integers 0..255; 'u8' the same integers as uint8."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 1.0, n)
    out = []
    for b in range(nb):
        v = np.clip(100 + 12 * b + (28 - 2 * b) * (0.6 * base * (1 if b % 2 else -1) + rng.normal(0.0, 1.0, n)), 0, 255)
        if kind == "unit":
            out.append((v / 255.0).astype(f32))
        elif kind == "float":
            out.append(v.astype(f32))
        else:
            q = v.astype(np.uint8)
            if n <= 16:
                q = (rng.permutation(200)[:n] + b).astype(np.uint8)      # distinct values: the percentiles of a tiny plane must differ
            out.append(q if kind == "u8" else q.astype(f32))
    return out


def stats_of(planes, normalise=True):
    """(lohi, center, scale) as the pipeline derives them, here with NumPy: any values would do, they are the call's arguments."""
    lohi, center, scale = [], [], []
    for p in planes:
        v = np.asarray(p).astype(f32)
        v = v[np.isfinite(v)]
        lo, hi = (f32(np.percentile(v, 2)), f32(np.percentile(v, 98))) if normalise else (f32(0), f32(1))
        lohi.append((lo, hi))
        z = R.norm1(v, lo, hi, R.norm_den(lo, hi)) if normalise else v
        center.append(f32(np.median(z)))
        q = np.percentile(z.astype(np.float64), (25.0, 75.0))
        scale.append(float(q[1] - q[0]) if q[1] - q[0] > 1e-12 else 1.0)
    return np.array(lohi, f32), np.array(center, f32), np.array(scale, np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def gpu_pca(ctx, planes, center, scale, nc, lohi=None, fit=None, device_planes=None):
    d = device_planes if device_planes is not None else [ctx.to_device(p) for p in planes]
    ctx.collect_minmax(True)
    try:
        outs, comp, ratio, mean, ev = ctx.pca_fit_transform(d, center, scale, nc, lohi, fit=fit)
        tags = [t._rsseg_minmax for t in outs]
    finally:
        ctx.collect_minmax(False)
    return dict(scores=np.stack([o.cpu().numpy() for o in outs], axis=1), components=comp, ratio=ratio, mean=mean, explained_variance=ev, tags=tags)


def assert_pca_equal(got, want, label, nan_rows=None):
    for k in ("mean", "components", "explained_variance", "ratio"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (label, k, got[k], want[k])
    g, w = got["scores"], want["scores"]
    if nan_rows is not None:     # the pixels that hold a NaN: a NaN score on both sides (its payload is not part of the contract)
        assert np.isnan(g[nan_rows]).all() and np.isnan(w[nan_rows]).all(), label
        keep = np.ones(g.shape[0], bool)
        keep[nan_rows] = False
        g, w = g[keep], w[keep]
    for c in range(w.shape[1]):
        assert np.array_equal(bits(g[:, c]), bits(w[:, c])), (label, "scores", c, int((bits(g[:, c]) != bits(w[:, c])).sum()))
    assert list(got["tags"]) == list(want["tags"]), (label, got["tags"], want["tags"])


def check(ctx, planes, center, scale, nc, lohi=None, fit=None, label=""):
    want = R.pca(planes, center, scale, nc, lohi, fit)
    got = gpu_pca(ctx, planes, center, scale, nc, lohi, fit)
    assert_pca_equal(got, want, label)
    return want


# ------------------------------------------------------------------------------------------------ (a) every form and band count
@pytest.mark.parametrize("nb", range(1, 9))
def test_model_and_scores_every_form(ctx, nb):
    """k3_gram / k3_project are specialised on the band count and on the plane type: nb = 1..8, 1 and nb components, 1025
    pixels (one vector body of 256, a scalar tail of 1), in the seven forms the entry points take — and the table pass of
    byte-valued float32 planes after a select has left its hint."""
    from rsseg import pipeline as P
    n = 1025
    for nc in sorted({1, nb}):
        unit = make_planes(n, nb, "unit", 10 * nb)
        _, c, s = stats_of(unit, normalise=False)
        check(ctx, unit, c, s, nc, label="pre-normalised float32 + scaler")
        for kind in ("float", "u8"):
            raw = make_planes(n, nb, kind, 10 * nb + 1)
            lohi, c, s = stats_of(raw)
            check(ctx, raw, c, s, nc, lohi, label="raw %s + lohi + scaler" % kind)
        for kind in ("float", "bytes", "u8"):
            raw = make_planes(n, nb, kind, 10 * nb + 2)
            w = check(ctx, raw, None, None, nc, label="%s, no scaler, no lohi" % kind)
            # 0..255 by type (uint8) or by measurement; general floats that stop short of 181 get one bit more
            assert w["Q"] == 32 if kind != "float" else w["Q"] == 48 - np.frexp(w["bound"] ** 2)[1] and w["Q"] in (32, 33)
        # the table pass: the select of band_quantile_bundles sees only integers 0..255 in these float32 planes
        raw = make_planes(n, nb, "bytes", 10 * nb + 3)
        d = [ctx.to_device(p) for p in raw]
        qb = P.band_quantile_bundles(ctx, d, n)
        lohi = np.array([[q["lo"], q["hi"]] for q in qb], f32)
        c = np.array([q["center"] for q in qb], f32)
        s = np.array([q["scale"] for q in qb], np.float64)
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            got = gpu_pca(ctx, raw, c, s, nc, lohi, device_planes=d)
            launches = ctx.prof_get("gram")[1]
        finally:
            ctx.prof_enable(False)
        assert launches == 1                              # the table pass ran, and no general pass after it
        assert_pca_equal(got, R.pca(raw, c, s, nc, lohi), "table pass")


# ------------------------------------------------------------------------------------------------ (b) pixel-count seams
SEAM_N = [2, 3, 4, 5, 7, 1023, 1024, 1027, 2051, 2048 * 1024 + 1024 + 3]


@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("n", SEAM_N)
def test_pixel_count_seams_of_gram_and_projection(ctx, kind, n):
    """Fewer pixels than one vector, exact multiples, ragged tails, more than one workgroup; and 2 098 179 pixels, where the
    grid is capped at 2048 workgroups: 256 threads make a second trip of the grid-stride loops, so threads of one launch
    differ in their term count (the per-thread bias subtraction) and one workgroup holds the 3-pixel tail."""
    raw = make_planes(n, 3, kind, n % 1000 + (kind == "u8"))
    lohi, c, s = stats_of(raw)
    check(ctx, raw, c, s, 2, lohi, label="%s n=%d" % (kind, n))


# ------------------------------------------------------------------------------------------------ (c) fit ranges
@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("off", [0, 1, 2, 3, 5])
def test_fit_ranges(ctx, kind, off):
    """fit = (off, len): the Gram pass takes a scalar head of 0 to 3 pixels up to the first 16-byte boundary (4-byte for uint8
    planes) and a vector body; here heads of every length, bodies of fewer than four pixels, a fit that is only a head
    (off = 1, len = 2), and a long body.  The model is that of the slice, the scores cover all 4099 pixels."""
    n = 4099
    raw = make_planes(n, 3, kind, 77 + off)
    lohi, c, s = stats_of(raw)
    for ln in (2, 3, 4, 6, n - off - 8):
        want = check(ctx, raw, c, s, 2, lohi, fit=(off, ln), label="%s fit=(%d, %d)" % (kind, off, ln))
        assert want["N"] == ln and want["scores"].shape == (n, 2)
        check(ctx, raw, None, None, 3, None, fit=(off, ln), label="%s unscaled fit=(%d, %d)" % (kind, off, ln))


def test_nan_outside_the_fit_range_is_accepted(ctx):
    """No lohi: the value range is measured over the fitted pixels only, the NaN lies outside them.  The fit is accepted, the
    pixel's scores are NaN, the extrema tags read them as 0."""
    n = 4099
    raw = make_planes(n, 3, "float", 5)
    raw = [p - f32(120) for p in raw]           # scores of both signs, so that a 0 is no extremum by itself
    for at, fit in ((4090, (3, 4000)), (1, (5, 4094)), (4098, (0, 4098))):
        pl = [p.copy() for p in raw]
        pl[1][at] = np.nan
        want = R.pca(pl, None, None, 3, None, fit)
        got = gpu_pca(ctx, pl, None, None, 3, None, fit)
        assert_pca_equal(got, want, "NaN at %d" % at, nan_rows=np.array([at]))
        assert all(np.isfinite(t).all() for t in got["tags"])
        _, c, s = stats_of(raw, normalise=False)
        assert_pca_equal(gpu_pca(ctx, pl, c, s, 2, None, fit), R.pca(pl, c, s, 2, None, fit), "NaN at %d, scaler" % at, nan_rows=np.array([at]))


# ------------------------------------------------------------------------------------------------ (d) the fused pass, both mappings
FUSE_ENV = [dict(), dict(RSSEG_FUSE_MAP="1"), dict(RSSEG_FUSE_MAP="1", RSSEG_FUSE_GRID="2")]


def gpu_fused(ctx, planes, lohi, center, scale, nc, quantize, fit=None):
    d = [ctx.to_device(p) for p in planes]
    ctx.collect_minmax(True)
    try:
        idx, norms, pcs, comp, ratio, mean, ev = ctx.indices_pca(d, lohi, center, scale, nc, want_norm=(True,) * 5, fit=fit, quantize=quantize)
        tags = [t._rsseg_minmax for t in idx + pcs]
        q = ctx.last_quantized.cpu().numpy()
    finally:
        ctx.collect_minmax(False)
    return dict(scores=np.stack([o.cpu().numpy() for o in pcs], axis=1), components=comp, ratio=ratio, mean=mean, explained_variance=ev, tags=tags,
                indices=[t.cpu().numpy() for t in idx], norm=[t.cpu().numpy() for t in norms], q=q)


def assert_fused_equal(got, want, label):
    assert_pca_equal(got, want, label)
    for j in range(7):
        assert np.array_equal(bits(got["indices"][j]), bits(want["indices"][j])), (label, "index", j)
    for j in range(5):
        assert np.array_equal(bits(got["norm"][j]), bits(want["norm"][j])), (label, "normalised band", j)
    assert np.array_equal(got["q"], want["q"]), (label, "byte plane")


@pytest.mark.parametrize("n", [3, 4099, 16384 + 3, 4 * (3 * 4096 + 100) + 3])
@pytest.mark.parametrize("kind", ["float", "u8"])
@pytest.mark.parametrize("nb", [5, 7])
def test_fused_pass_in_both_mappings(ctx, oracle, monkeypatch, nb, kind, n):
    """k3_indices_project maps workgroups to pixels in two ways; scenes of 16384^2 take the chunked one (a workgroup owns
    chunks of 4096 vectors), which RSSEG_FUSE_MAP=1 forces at any size.  With RSSEG_FUSE_GRID=2 and 49555 pixels one
    workgroup walks chunks 0 and 2, the other chunk 1 and the partial chunk 3; with 3 pixels there is no chunk at all.
    Every plane, the model and every tag against the restatement, in the default mapping and both forced ones."""
    raw = make_planes(n, nb, kind, n % 1000 + nb)
    lohi, c, s = stats_of(raw)
    nir = R.norm1(np.asarray(raw[3]).astype(f32), lohi[3][0], lohi[3][1], R.norm_den(lohi[3][0], lohi[3][1]))
    quantize = (float(np.percentile(nir, 2)), float(np.percentile(nir, 98)), 31.0)
    for nc in (3, nb):
        want = R.fused(raw, c, s, nc, lohi, quantize, oracle=oracle)
        for env in FUSE_ENV:
            with monkeypatch.context() as mp:
                mp.delenv("RSSEG_FUSE_MAP", raising=False)
                mp.delenv("RSSEG_FUSE_GRID", raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                got = gpu_fused(ctx, raw, lohi, c, s, nc, quantize)
            assert_fused_equal(got, want, "nb=%d %s n=%d nc=%d %s" % (nb, kind, n, nc, env))


# ------------------------------------------------------------------------------------------------ (e) value ranges
def at_magnitude(M, n=20000, seed=3, signed=False):
    pl = make_planes(n, 3, "unit", seed)
    out = [(p.astype(np.float64) / float(p.max()) * M).astype(f32) for p in pl]       # every band's largest value is float32(M)
    if signed:
        out = [(-p if b == 1 else p - f32(0.4 * M)) for b, p in enumerate(out)]
    return out


@pytest.mark.parametrize("M,Q", [(1e-3, 38), (1.0, 38), (255.0, 32), (65535.0, 16), (3e6, 4), (1e9, -12), (2.0 ** 33.25, R.Q_MIN)])
def test_value_ranges_without_scaler(ctx, M, Q):
    """The quantum 2^-Q of the exact sums follows the measured range: Q = 38 down to the coarsest one the fit accepts."""
    for signed in (False, True):
        pl = at_magnitude(M, signed=signed)
        want = check(ctx, pl, None, None, 3, label="M=%g signed=%d" % (M, signed))
        assert want["Q"] == Q


def test_tiny_scale_moves_the_quantum(ctx):
    pl = make_planes(20000, 3, "unit", 4)
    c = np.array([0.5, 0.4, 0.6], f32)
    s = np.array([1e-4, 1e-4, 2e-4], np.float64)
    want = check(ctx, pl, c, s, 3, label="scale 1e-4")
    assert 20 <= want["Q"] <= 24                 # bound about 0.6 / 1e-4


def test_ranges_that_cannot_be_accumulated_are_refused(ctx):
    """Below Q_MIN the first-moment sums are too coarse (tests/test_pca_host.py holds the measured table); a bound whose
    square is not finite has no quantum at all.  RSSEG_ERR_UNSUPPORTED, as the restatement refuses them."""
    from rsseg.runtime import RssegUnsupported
    for M in (2.0 ** 33.75, 1e12, 3e38):       # Q_MIN - 1, -32, far beyond
        pl = at_magnitude(M, n=2051)
        with pytest.raises(R.Unsupported):
            R.pca(pl, None, None, 3)
        with pytest.raises(RssegUnsupported, match="too large for exact accumulation"):
            gpu_pca(ctx, pl, None, None, 3)
    pl = at_magnitude(3e38, n=2051)
    c, s = np.zeros(3, f32), np.full(3, 1e-300)
    with pytest.raises(R.Unsupported):
        R.pca(pl, c, s, 3)
    with pytest.raises(RssegUnsupported, match="too large for exact accumulation"):
        gpu_pca(ctx, pl, c, s, 3)


# ------------------------------------------------------------------------------------------------ (f) special values
def test_nan_inside_the_fit_range_is_refused_in_every_form(ctx):
    from rsseg import pipeline as P
    n = 1025
    unit, raw, byt = make_planes(n, 3, "unit", 1), make_planes(n, 3, "float", 2), make_planes(n, 3, "bytes", 3)
    _, cu, su = stats_of(unit, normalise=False)
    lohi, c, s = stats_of(raw)
    for at in (0, 513, 1024):                    # vector body, another wave, the scalar tail
        for planes, args in ((unit, (cu, su, 2, None)), (raw, (c, s, 2, lohi)), (raw, (None, None, 2, lohi)), (raw, (None, None, 3, None)),
                             (unit, (None, None, 1, None))):
            pl = [p.copy() for p in planes]
            pl[at % 3][at] = np.nan
            with pytest.raises(ValueError, match="contains NaN"):
                R.pca(pl, *args)
            with pytest.raises(ValueError, match="contains NaN"):
                gpu_pca(ctx, pl, *args)
        with pytest.raises(ValueError, match="contains NaN"):
            gpu_pca(ctx, pl, cu, su, 2, None, fit=(max(0, at - 3), 4))
        # the table pass: the hint is left by a select of clean planes, the NaN arrives afterwards
        d = [ctx.to_device(p) for p in byt]
        qb = P.band_quantile_bundles(ctx, d, n)
        d[1][at] = float("nan")
        with pytest.raises(ValueError, match="contains NaN"):
            gpu_pca(ctx, byt, np.array([q["center"] for q in qb], f32), np.array([q["scale"] for q in qb], np.float64), 2,
                    np.array([[q["lo"], q["hi"]] for q in qb], f32), device_planes=d)


def test_infinities(ctx):
    """Without lohi an infinity among the fitted values is refused by name; with lohi robust_normalize clips it like any
    other value and the fit equals the restatement."""
    n = 1025
    raw = make_planes(n, 3, "float", 8)
    lohi, c, s = stats_of(raw)
    for at, v in ((0, np.inf), (700, -np.inf), (1024, np.inf)):
        pl = [p.copy() for p in raw]
        pl[2][at] = v
        for args in ((None, None, 2, None), (c, s, 2, None)):
            with pytest.raises(ValueError, match="infinity"):
                R.pca(pl, *args)
            with pytest.raises(ValueError, match="infinity"):
                gpu_pca(ctx, pl, *args)
        check(ctx, pl, c, s, 3, lohi, label="inf at %d, lohi + scaler" % at)
        check(ctx, pl, None, None, 3, lohi, label="inf at %d, lohi" % at)


def test_fewer_than_two_samples_are_refused(ctx):
    raw = make_planes(9, 2, "float", 1)
    for fit in ((0, 1), (3, 1), (5, 0)):
        with pytest.raises(ValueError, match="at least 2 samples"):
            gpu_pca(ctx, raw, None, None, 1, None, fit)
        with pytest.raises(ValueError, match="at least 2 samples"):
            R.pca(raw, None, None, 1, None, fit)
    one = [p[:1].copy() for p in raw]
    with pytest.raises(ValueError, match="at least 2 samples"):
        gpu_pca(ctx, one, None, None, 1)


def test_scale_that_takes_the_plain_division(ctx):
    """A scale with an all-ones significand fails the host's test for the reciprocal form: every kernel divides."""
    n = 1027
    for kind in ("float", "u8"):
        raw = make_planes(n, 3, kind, 9)
        lohi, c, s = stats_of(raw)
        s[1] = float(np.nextafter(0.5, 0.0))
        assert R.slow_div(s[1]) and not R.slow_div(s[0])
        check(ctx, raw, c, s, 3, lohi, label="slow_div %s" % kind)
    unit = make_planes(n, 3, "unit", 9)
    check(ctx, unit, np.array([0.5, 0.25, 0.75], f32), np.array([0.3, float(np.nextafter(0.25, 0.0)), 0.2]), 2, label="slow_div unit")


def test_negative_zero_reaches_no_output(ctx, oracle):
    """d = v - center = -0.0 is the one input at which the kernels' reciprocal division differs from the IEEE quotient (+0.0
    for -0.0, tests/test_pca_host.py).  Planes holding -0.0 with lo = +0.0 and centre +0.0: every output equals the
    restatement, which divides."""
    n = 1027
    rng = np.random.default_rng(12)
    unit = make_planes(n, 5, "unit", 12)
    for p in unit:
        p[rng.random(n) < 0.3] = f32(-0.0)
        p[rng.random(n) < 0.1] = f32(0.0)
    assert all(np.signbit(p[p == 0]).any() for p in unit)
    c = np.zeros(5, f32)
    s = np.array([0.3, 1 / 3, 0.1, 0.25, 0.7])
    check(ctx, unit, c, s, 5, label="-0.0 pre-normalised")
    lohi = np.array([[0.0, 0.9]] * 5, f32)
    check(ctx, unit, c, s, 5, lohi, label="-0.0 raw + lohi")
    quantize = (0.0, 0.8, 31.0)
    want = R.fused(unit, c, s, 5, lohi, quantize, oracle=oracle)
    assert any(np.signbit(z[z == 0]).any() for z in want["norm"])
    assert_fused_equal(gpu_fused(ctx, unit, lohi, c, s, 5, quantize), want, "-0.0 fused")
