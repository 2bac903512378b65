"""CPU suite: tests/pca_ref.py (the restatement of K3 that tests/test_gpu_pca.py holds the kernels to, bit for bit) against
scikit-learn and a float64 evaluation; its split-sum property; the kernels' reciprocal division against the IEEE quotient;
and rsseg_host_pca_model (the host tail of the PCA entry points, no GPU needed) against the restatement, bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import pca_ref as R
from kmeans_model_ref import fma64, fma_exact

f32 = np.float32
ULP32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ data
def mixed_planes(n, nb, close, seed):
    """nb correlated planes in [0, 1]: latent factors of decreasing strength (close: the second and third of equal
    strength up to 1e-3, so that two eigenvalues nearly coincide), mixed by a random orthogonal matrix."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, nb))
    s = np.array([1.0 / (1.0 + 0.7 * i) for i in range(nb)])
    if close and nb >= 3:
        s[2] = s[1] * (1.0 - 1e-3)
    elif close and nb == 2:
        s[1] = s[0] * (1.0 - 1e-3)
    q, _ = np.linalg.qr(rng.standard_normal((nb, nb)))
    x = 0.5 + 0.12 * (z * s) @ q
    return np.clip(x, 0.0, 1.0).astype(f32)


def truth64(X):
    """float64 evaluation of PCA on the float32 matrix X: mean, variances (descending), components (svd_flip)."""
    X64 = X.astype(np.float64)
    m = X64.mean(0)
    Xc = X64 - m
    Cm = Xc.T @ Xc / (X.shape[0] - 1)
    w, V = np.linalg.eigh(Cm)
    w, Vt = w[::-1].copy(), V[:, ::-1].T.copy()
    Vt *= np.where(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)] < 0, -1.0, 1.0)[:, None]
    return m, np.maximum(w, 0.0), Vt


def sk_pca(X):
    """scikit-learn's float32 PCA with the solver the reference's scenes select (covariance_eigh; named, so that the 50-pixel
    cases run the same steps)."""
    from sklearn.decomposition import PCA
    p = PCA(n_components=X.shape[1], svd_solver="covariance_eigh").fit(X)
    assert p.mean_.dtype == np.float32 and p.components_.dtype == np.float32
    return p.mean_, p.explained_variance_, p.components_


def ref_pca(X, q_min=None):
    """The restatement on a matrix that is already scaled (no lohi, no scaler)."""
    planes = [np.ascontiguousarray(X[:, b]) for b in range(X.shape[1])]
    vmin, vmax = R.value_range(planes)
    Q, _ = R.quantum(vmin, vmax, q_min=q_min)
    return R.model(R.int_sums(X, Q), X.shape[0], Q, X.shape[1], X.shape[1])


GAP = 5e-2


def error_pairs(X, m, components=True):
    """[(name, error of the restatement, error of scikit-learn, floor)] against float64 for the mean, the variances and every
    component with a clear eigenvalue gap: both neighbours farther than GAP = 5e-2 of the largest eigenvalue (closer ones turn
    with the float32 rounding of the covariance, the same in both procedures, and rank nothing).  floor: 4 float32 ulps of
    the data's scale — max |x| for the mean, the largest mean square max_b sum x_b^2 / (N - 1) for the variances (the
    scale of X.T @ X / (N - 1), which both procedures hold in float32), 1 for the unit-length components."""
    mu, w, Vt = truth64(X)
    smu, sw, sV = sk_pca(X)
    m2 = (X.astype(np.float64) ** 2).sum(0).max() / (X.shape[0] - 1)
    out = [("mean", np.abs(m["mean"] - mu).max(), np.abs(smu - mu).max(), 4 * ULP32 * np.abs(X.astype(np.float64)).max()),
           ("variance", np.abs(m["explained_variance"] - w).max(), np.abs(sw - w).max(), 4 * ULP32 * m2)]
    gaps = np.minimum(np.abs(np.diff(w, prepend=np.inf)), np.abs(np.diff(w, append=-np.inf)))

    def comp_err(v, t):
        return min(np.abs(v - t).max(), np.abs(v + t).max())     # a sign decided by two entries of nearly equal size may differ

    for c in range(X.shape[1]) if components else ():
        if X.shape[1] == 1 or gaps[c] > GAP * w[0]:
            out.append(("component %d" % c, comp_err(m["components"][c].astype(np.float64), Vt[c]), comp_err(sV[c].astype(np.float64), Vt[c]), 4 * ULP32))
    return out


def check_pairs(pairs, label):
    bad = []
    for name, e_ref, e_sk, floor in pairs:
        print("%-30s %-12s restatement %.3e  scikit-learn %.3e  floor %.3e" % (label, name, e_ref, e_sk, floor))
        if not (e_ref <= e_sk or (e_ref <= floor and e_sk <= floor)):
            bad.append((name, e_ref, e_sk, floor))
    assert not bad, (label, bad)


def at_magnitude(M, n=9216, seed=7):
    """Three non-negative correlated planes whose largest value is exactly float32(M)."""
    P = mixed_planes(n, 3, False, seed)
    return (P.astype(np.float64) / P.max() * M).astype(f32)


def magnitude_of(Q):
    """A magnitude at which pca_core's quantum is Q (Q <= 38): bound^2 just below 2^(48 - Q)."""
    return 2.0 ** ((48 - Q - 0.5) / 2)


# ------------------------------------------------------------------------------------------------ restatement vs scikit-learn and float64
SCALED_CASES = [(nb, n, close) for nb in (1, 2, 3, 5, 7, 8) for n in (50, 9216, 100003) for close in (False, True) if not (close and nb == 1)]


@pytest.mark.parametrize("nb,n,close", SCALED_CASES)
def test_restatement_vs_sklearn_and_float64(nb, n, close):
    """RobustScaler + PCA on float32 planes in [0, 1], with and without two nearly equal eigenvalues.  The scaler's output
    equals scikit-learn's bit for bit; mean, variances and every clear-gap component are no farther from the float64
    evaluation than scikit-learn's float32 PCA (covariance_eigh) is, or both lie under error_pairs' floor.

    Measured over the 33 cases, largest absolute errors (restatement / scikit-learn): mean 1.3e-8 / 5.3e-8, variance
    1.3e-7 / 3.8e-7, the 97 clear-gap components 1.8e-7 / 1.6e-6.  The restatement's mean is closer in every case.  scikit-learn is
    the closer one in these eight pairs, every one of them with both errors under the floor (restatement / scikit-learn / floor):
      nb=1 n=9216            variance     3.428e-08 / 2.533e-08 / 2.604e-07
      nb=1 n=100003          variance     5.515e-08 / 4.459e-09 / 2.605e-07
      nb=2 n=9216            variance     3.846e-08 / 3.206e-08 / 2.580e-07
      nb=3 n=50     close    component 1  8.269e-08 / 7.748e-08 / 4.768e-07
      nb=3 n=50     close    component 2  1.109e-07 / 1.615e-08 / 4.768e-07
      nb=3 n=100003          component 1  1.344e-07 / 1.338e-07 / 4.768e-07
      nb=3 n=100003          component 2  1.255e-07 / 1.210e-07 / 4.768e-07
      nb=5 n=50     close    component 0  2.312e-08 / 1.851e-08 / 4.768e-07
    So the restatement is not uniformly closer: once the sums are exact, what is left is the float32 rounding of the mean
    term and of the covariance, which both procedures share.  Components whose gap is below GAP are not ranked (at nb = 7,
    n = 9216, close, gaps of 1 to 2 %: 6.2e-7 against 4.7e-7 and 7.3e-7 against 6.7e-7).  Every pair is printed (-s)."""
    from sklearn.preprocessing import RobustScaler
    P = mixed_planes(n, nb, close, 1000 * nb + n % 997 + close)
    rs = RobustScaler().fit(P)
    want = rs.transform(P)
    assert want.dtype == np.float32
    X = R.transform([P[:, b] for b in range(nb)], None, rs.center_.astype(f32), rs.scale_.astype(np.float64))
    assert np.array_equal(X.view(np.int32), want.view(np.int32))
    check_pairs(error_pairs(X, ref_pca(X)), "nb=%d n=%d close=%d" % (nb, n, close))


@pytest.mark.parametrize("M,Q", [(1.0, 38), (255.0, 32), (65535.0, 16), (3e6, 4), (1e9, -12)])
def test_magnitude_sweep_without_scaler(M, Q):
    """Unscaled planes of growing magnitude: the quantum follows the measured range, the bar is the same.
    Measured (restatement / scikit-learn; mean relative to M, variance to M^2, components absolute):
      M = 1      mean 7.8e-9 / 1.3e-6   variance 9.6e-9 / 1.6e-6   components 6.7e-7 .. 3.5e-6 / 5.6e-5 .. 2.5e-4
      M = 255    mean 2.4e-8 / 2.0e-6   variance 1.8e-8 / 2.1e-6   components 1.6e-6 .. 2.7e-6 / 1.0e-4 .. 1.8e-4
      M = 65535  mean 4.5e-8 / 1.3e-6   variance 8.2e-8 / 1.3e-6   components 1.5e-6 .. 8.2e-6 / 2.8e-5 .. 4.2e-4
      M = 3e6    mean 3.6e-8 / 8.8e-7   variance 1.2e-8 / 2.3e-6   components 1.0e-6 .. 5.8e-6 / 4.5e-5 .. 1.1e-4
      M = 1e9    mean 4.2e-8 / 1.6e-6   variance 9.5e-8 / 1.6e-6   components 2.6e-6 .. 6.6e-6 / 4.6e-5 .. 3.2e-4"""
    X = at_magnitude(M)
    m = ref_pca(X)
    assert m["Q"] == Q
    check_pairs(error_pairs(X, m), "M=%g" % M)


def test_large_offset_is_float32_cancellation_in_sklearns_own_steps():
    """Values 1e6 + 100 u: g - (N mu_b) mu_c cancels eight of float32's digits in scikit-learn's steps, which the restatement
    (and the kernels) follow — exact sums do not help after that subtraction.  The same bar for mean and variance; measured
    (restatement / scikit-learn): mean 4.7e-2 / 4.9e+1, variance 1.9e+5 / 2.8e+8, where the true variances are below 150.
    The COMPONENTS ARE NOT CHECKED here: with a covariance that wrong they are noise on both sides (errors 1.29, 0.09, 1.30
    against 1.21, 0.81, 0.82 for entries of unit vectors), and which noise lies closer to float64 says nothing."""
    u = mixed_planes(9216, 3, False, 11)
    X = (1e6 + 100.0 * u.astype(np.float64)).astype(f32)
    check_pairs(error_pairs(X, ref_pca(X), components=False), "1e6 + 100 u")


@pytest.mark.parametrize("Q", list(range(-12, R.Q_MIN - 1, -1)))
def test_every_supported_coarse_quantum_meets_the_bar(Q):
    """The first-moment sums share the quantum sized for the squares, so from some magnitude on the mean is rounded more
    coarsely per pixel than float32 would round it.  One case per Q (three seeds, n = 9216) down to Q_MIN, the smallest
    quantum pca_core accepts, is still no farther from float64 than scikit-learn; the table below Q_MIN is in the docstring
    of test_value_range_below_q_min_is_refused."""
    for seed in (7, 8, 9):
        X = at_magnitude(magnitude_of(Q), seed=seed)
        m = ref_pca(X)
        assert m["Q"] == Q
        check_pairs(error_pairs(X, m), "Q=%d seed=%d" % (Q, seed))


def test_value_range_below_q_min_is_refused():
    """Magnitude 1e12 (Q = -32) and the first quantum below Q_MIN are refused.  Why, measured with the restatement allowed to
    go on (n = 9216, seeds 7, 8, 9; worst ratio restatement error / scikit-learn error over mean, variance, components):
      Q   -12   -14   -16   -18   -19 |  -20   -22   -24   -26   -28   -30   -32   -36   -40
      r  0.15  0.24  0.65  0.59  0.50 |  2.2   1.3   7.9   3.0    23    32    96   247  1563
    At 1e12 (Q = -32), restatement against scikit-learn: mean 1.4e-5 M against 1.0e-6 M, variance 1.0e-5 M^2 against
    1.2e-6 M^2, components 3.0e-4 .. 9.8e-4 against 4.6e-5 .. 9.4e-5.  (With 100003 pixels the rounding averages out further and the bar holds down to Q = -25; with 50 pixels the
    mean falls behind scikit-learn's from Q = -14.)"""
    for M in (1e12, magnitude_of(R.Q_MIN - 1)):
        with pytest.raises(R.Unsupported):
            ref_pca(at_magnitude(M))
    X = at_magnitude(1e12)
    m = ref_pca(X, q_min=-40)
    assert m["Q"] == -32
    pairs = error_pairs(X, m)
    for name, e_ref, e_sk, floor in pairs:
        print("M=1e12 %-12s restatement %.3e  scikit-learn %.3e" % (name, e_ref, e_sk))
    assert all(e_ref > e_sk for _, e_ref, e_sk, _ in pairs)      # the finding itself: were this to change, the range could widen again


# ------------------------------------------------------------------------------------------------ split sums
@pytest.mark.parametrize("Q", [38, 16, -12])
def test_integer_sums_of_any_split_add_to_the_whole(Q):
    rng = np.random.default_rng(Q + 100)
    X = at_magnitude(magnitude_of(Q) if Q < 38 else 1.0, n=10007, seed=3)
    X[::3] *= f32(-1)
    whole = R.int_sums(X, Q)
    for block in (1, 7, 1000, 4096):
        assert R.int_sums(X, Q, block) == whole, block
    for _ in range(4):
        cuts = sorted(set(rng.integers(0, X.shape[0], 5).tolist()) | {0, X.shape[0]})
        parts = [R.int_sums(X[a:b], Q) for a, b in zip(cuts[:-1], cuts[1:])]
        assert [sum(p[i] for p in parts) for i in range(R.NACC)] == whole
    perm = rng.permutation(X.shape[0])
    assert R.int_sums(X[perm], Q) == whole
    a, b = R.model(whole, X.shape[0], Q, 3, 3), R.model(R.int_sums(X[perm], Q, 333), X.shape[0], Q, 3, 3)
    for k in ("mean", "cov", "components", "explained_variance", "ratio", "offs"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------------ the kernels' division
def fast_div(d, s):
    """pca_x / scale_x of k3_pca.hip: q = d * y; r = fma(-q, s, d); float32(fma(r, y, q)) with y = RN(1 / s)."""
    d = np.asarray(d, f32).astype(np.float64)
    s = np.float64(s)
    y = np.float64(1.0) / s
    with np.errstate(all="ignore"):
        q = d * y
        r = fma64(-q, s, d)
        z = fma64(r, y, q)
        for i in np.nonzero(d == 0)[0]:      # the sign of an exact zero: from the scalar form, which adds the zeros as IEEE does
            z[i] = fma_exact(fma_exact(-q[i], s, d[i]), y, q[i])
        return z.astype(f32)


def adversarial_d():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(f32)
    bits = bits[np.isfinite(bits)]
    sub = (np.arange(1, 400, dtype=np.uint32) * np.uint32(20011)).view(f32)                      # float32 subnormals
    ints = (np.arange(256, dtype=f32) / f32(255))
    edge = np.array([0.0, 1.0, -1.0, 3e38, -3e38, 2.0 ** -126, 2.0 ** -149, 1 - 2.0 ** -24, 1 + 2.0 ** -23, 0.1, 1 / 3], f32)
    d = np.concatenate([bits, sub, -sub, ints, ints - f32(0.37), edge, rng.random(5000, dtype=f32), (rng.random(5000) * 255).astype(f32)])
    return d[~((d == 0) & np.signbit(d))]                                                         # -0.0 is the named exception, below


def adversarial_s():
    out = [1 / 3, 0.1, 1e-9, 1e5, 1.0, 3.0, 0.25000000000000006, 1e-30, 1e30]
    for k in (-40, -1, 0, 1, 7, 40):
        for j in (1, 2, 3):
            out += [float(np.nextafter(2.0 ** k, np.inf)) + (j - 1) * 2.0 ** (k - 52), 2.0 ** k * (1 + j * 2.0 ** -30), 2.0 ** k * (1 - j * 2.0 ** -31)]
        out.append(2.0 ** k)
    rng = np.random.default_rng(6)
    out += list(rng.random(40) * 10.0 ** rng.integers(-6, 6, 40))
    return out


def test_reciprocal_division_equals_the_ieee_quotient():
    """The kernels' RN(d / s) through RN(1 / s) and two fmas equals the IEEE quotient for every scale the host lets through
    (slow_div false) over adversarial (d, s) — with ONE exception, d = -0.0: the form returns +0.0 where the quotient is
    -0.0 (q = -0, r = fma(+0, s, -0) = +0, fma(+0, y, -0) = +0).  tests/test_gpu_pca.py checks that the sign reaches no output."""
    d = adversarial_d()
    for s in adversarial_s():
        assert not R.slow_div(s), s
        for sg in (1.0, -1.0):
            with np.errstate(all="ignore"):
                want = (d.astype(np.float64) / np.float64(sg * s)).astype(f32)
            got = fast_div(d, sg * s)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (s, sg)
    for s in (1 / 3, 0.1, 1e5, 2.0):
        got, want = fast_div(np.array([-0.0], f32), s), (np.array([-0.0]) / s).astype(f32)
        assert not np.signbit(got[0]) and np.signbit(want[0]) and got[0] == want[0] == 0      # the exception, by name


def test_scales_the_host_sends_to_the_plain_division():
    """An all-ones significand, a scale whose reciprocal is subnormal (or zero), a subnormal, zero, infinite or NaN scale:
    slow_div — the kernels then divide, which the restatement's quotient is."""
    ones = [float(np.nextafter(2.0 ** k, 0.0)) for k in (-3, 0, 1, 11)]
    for s in ones + [-ones[0], 1e308, 1.7e308, 2.0 ** 1023, 5e-324, 1e-310, 0.0, float("inf"), float("nan")]:
        assert R.slow_div(s), s
    for s in (2.0 ** 1022, 2.0 ** -1022, float(np.nextafter(2.0, 3.0)), 1.0, -0.75):
        assert not R.slow_div(s), s


# ------------------------------------------------------------------------------------------------ rsseg_host_pca_model
def host_model(S, N, Q, nb, nc):
    from rsseg import _lib
    lib = _lib.load()
    lim = R.limbs(S)
    out = dict(mean=np.zeros(nb, f32), cov=np.zeros((nb, nb), f32), components=np.zeros((nc, nb), f32), explained_variance=np.zeros(nc, f32),
               ratio=np.zeros(nc, f32), offs=np.zeros(nc, f32))
    fp = C.POINTER(C.c_float)
    rc = lib.rsseg_host_pca_model(lim.ctypes.data_as(C.POINTER(C.c_int64)), N, Q, nb, nc, *[out[k].ctypes.data_as(fp) for k in
                                  ("mean", "cov", "components", "explained_variance", "ratio", "offs")])
    return rc, out


def assert_model_equal(S, N, Q, nb, nc):
    rc, got = host_model(S, N, Q, nb, nc)
    assert rc == 0
    want = R.model(S, N, Q, nb, nc)
    for k, v in got.items():
        assert np.array_equal(v.view(np.int32), want[k].view(np.int32)), (k, v, want[k])
    return want


def sums_of(rows, Q):
    return R.int_sums(np.asarray(rows, f32), Q)


def hand_sums(nb, Q, first, second):
    """Sums given as values: first[b], second[b][c] (b <= c), in quanta of 2^-Q."""
    S = [0] * R.NACC
    for b in range(nb):
        S[b] = int(round(first[b] * 2.0 ** Q))
        for c in range(b, nb):
            S[R.tri(b, c)] = int(round(second[b][c] * 2.0 ** Q))
    return S


def test_host_model_two_samples():
    m = assert_model_equal(sums_of([[0.25, 0.5, 1.0], [0.75, 0.125, 1.0]], 38), 2, 38, 3, 3)
    assert m["explained_variance"][1] == 0 and m["explained_variance"][2] == 0 and m["explained_variance"][0] > 0
    for N in (1, 0, -5):
        assert host_model(sums_of([[0.25, 0.5]], 38), N, 38, 2, 2)[0] == -1
    assert host_model([0] * R.NACC, 5, 38, 9, 1)[0] == -1 and host_model([0] * R.NACC, 5, 38, 3, 4)[0] == -1 and host_model([0] * R.NACC, 5, 38, 3, 0)[0] == -1


def test_host_model_constant_band_and_identical_bands():
    rng = np.random.default_rng(1)
    x = rng.random((40, 2)).astype(f32)
    zero = np.column_stack([x[:, 0], np.zeros(40, f32), x[:, 1]])
    m = assert_model_equal(sums_of(zero, 38), 40, 38, 3, 3)
    assert not m["cov"][1].any() and not m["cov"][:, 1].any() and m["explained_variance"][2] == 0 and not m["components"][:2, 1].any()
    const = np.column_stack([x[:, 0], np.full(40, 0.375, f32), x[:, 1]])     # its own variance is exactly 0, its covariances are rounding
    m = assert_model_equal(sums_of(const, 38), 40, 38, 3, 3)
    assert m["cov"][1, 1] == 0 and m["explained_variance"][2] <= 1e-8
    twin = np.column_stack([x[:, 0], x[:, 1], x[:, 0], x[:, 1]])
    m = assert_model_equal(sums_of(twin, 38), 40, 38, 4, 4)
    assert np.array_equal(m["cov"][0], m["cov"][2]) and m["explained_variance"][3] <= 1e-7 and np.isfinite(m["ratio"]).all()


def test_host_model_equal_eigenvalues_keep_their_index_order():
    rows = [[1, 0, 0.5], [-1, 0, 0.5], [0, 1, -0.5], [0, -1, -0.5]]       # cov = diag(2/3, 2/3, 1/3): nothing to rotate
    m = assert_model_equal(sums_of(rows, 30), 4, 30, 3, 3)
    assert m["explained_variance"][0] == m["explained_variance"][1] > m["explained_variance"][2]
    assert np.array_equal(m["components"], np.eye(3, dtype=f32))             # band 0 before band 1: the stable order decided
    rows = [[0, 1, 0.5], [0, -1, 0.5], [1, 0, -0.5], [-1, 0, -0.5]]
    m = assert_model_equal(sums_of(rows, 30), 4, 30, 3, 2)
    assert np.array_equal(m["components"], np.eye(3, dtype=f32)[:2])


def test_host_model_negative_eigenvalue_is_clamped():
    """Sums no pixels produce: |sum xy| above sqrt(sum xx * sum yy).  The smaller eigenvalue comes out negative and is
    clamped to 0; the ratios stay finite."""
    S = hand_sums(2, 20, [0.0, 0.0], [[1.0, 1.25], [None, 1.0]])
    m = assert_model_equal(S, 3, 20, 2, 2)
    assert m["cov"][0, 1] > m["cov"][0, 0] and m["explained_variance"][1] == 0 and not np.signbit(m["explained_variance"][1])
    assert np.isfinite(m["ratio"]).all() and m["ratio"][0] == 1.0
    S = hand_sums(3, 10, [3.0, -6.0, 1.5], [[4.0, -9.0, 2.0], [None, 13.0, 1.0], [None, None, 1.0]])
    m = assert_model_equal(S, 3, 10, 3, 3)
    assert m["explained_variance"][2] == 0 and np.isfinite(m["ratio"]).all()


def test_host_model_tie_of_the_two_largest_entries_takes_the_first():
    """cov = [[1, 1/2], [1/2, 1]]: theta = 0, t = 1, c = s exactly: the rows are (c, c) and (-c, c) before the flip; the first
    largest |entry| decides each sign, so the second row becomes (c, -c)."""
    S = hand_sums(2, 20, [0.0, 0.0], [[2.0, 1.0], [None, 2.0]])
    m = assert_model_equal(S, 3, 20, 2, 2)
    c = m["components"]
    assert abs(c[0, 0]) == abs(c[0, 1]) == abs(c[1, 0]) == abs(c[1, 1])
    assert c[0, 0] > 0 and c[1, 0] > 0 and c[0, 1] * c[1, 1] < 0
    S = hand_sums(2, 20, [0.0, 0.0], [[2.0, -1.0], [None, 2.0]])
    c = assert_model_equal(S, 3, 20, 2, 2)["components"]
    assert c[0, 0] > 0 and c[1, 0] > 0


@pytest.mark.parametrize("nb", range(1, 9))
def test_host_model_every_band_and_component_count(nb):
    rng = np.random.default_rng(nb)
    for Q, M in ((38, 1.0), (32, 255.0), (-12, 1e9)):
        X = ((rng.random((301, nb)) - 0.3) @ (np.eye(nb) + 0.3 * rng.random((nb, nb))) * M).astype(f32)
        X *= f32(M) / np.abs(X).max()
        S = R.int_sums(X, Q)
        for nc in range(1, nb + 1):
            assert_model_equal(S, 301, Q, nb, nc)
    # rank deficient by construction and a zero row, from float32-rounded random sums
    X = np.repeat(rng.integers(-3, 4, (60, 1)), nb, axis=1).astype(f32) * np.arange(nb, dtype=f32)
    assert_model_equal(R.int_sums(X, 30), 60, 30, nb, nb)
