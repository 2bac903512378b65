"""K24 without a GPU: what rsseg.signatures computes from a moment table (tests/moments_ref.py supplies the table the kernel
would), against exact rational arithmetic and independent float64 restatements; GaussianClassifier.fit_moments against fit;
the error texts and the stage driver's argument errors."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import gaussian_cases as GC
import gaussian_ref as R
import moments_ref as M

from rsseg import signatures as SIG
from rsseg.gaussian import GaussianClassifier
from rsseg.signatures import ClassMoments


def moments_of(X, y, Q=None, plane_exp=None, n_total=None):
    """The ClassMoments of samples X (n, F) float32 with labels y (>= 1), as class_moments builds it: exponents from the
    largest |x| of each plane, Q from the pixel count."""
    X = np.asarray(X, np.float32)
    pe = np.array([SIG.exponent_for(np.abs(X[:, f]).max()) for f in range(X.shape[1])]) if plane_exp is None else np.asarray(plane_exp)
    Q = SIG.q_for(n_total or X.shape[0]) if Q is None else Q
    table, left = M.moments_table(np.ascontiguousarray(X.T), y, int(np.max(y)) + 1, pe, Q, ignore=0)
    return ClassMoments(table, pe, Q, left)


@functools.lru_cache(maxsize=None)
def scaled_case():
    """n = 3000 pixels of F = 6 planes whose scales run from 1e-3 to 200 (what the per-plane exponents are for), correlated,
    with offsets far from zero on two planes; three classes labelled 1, 2, 5."""
    rng = np.random.default_rng(2401)
    n, F = 3000, 6
    scale = np.array([1e-3, 0.05, 1.0, 7.0, 60.0, 200.0])
    mix = rng.standard_normal((F, F)) / np.sqrt(F) + 0.7 * np.eye(F)
    X = (rng.standard_normal((n, F)) @ mix.T + np.array([0, 3.0, 0, -2.0, 0, 0.5])) * scale / 4.0
    X = np.clip(X, -scale, scale).astype(np.float32)
    y = rng.choice([1, 2, 5], n, p=[0.5, 0.3, 0.2])
    return X, y


def test_exponents_and_q():
    assert [SIG.exponent_for(v) for v in (0.0, 1.0, 0.75, 0.5, 0.500001, 200.0, 256.0, 1e-3)] == [0, 0, 0, 1, 0, -8, -8, 9]
    for v in (1e-30, 3.0, 255.0, 2.0 ** 100, np.float32(1.1e-3)):
        e = SIG.exponent_for(v)
        assert 0.5 < float(v) * 2.0 ** e <= 1.0
    assert [SIG.q_for(n) for n in (1, 2, 3000, 2 ** 17, 2 ** 17 + 1, 16384 ** 2, 2 ** 40)] == [44, 44, 44, 44, 43, 33, 21]
    for n in (1, 3000, 2 ** 17 + 1, 16384 ** 2):
        assert (n << SIG.q_for(n)) < 2 ** 62
    with pytest.raises(ValueError):
        SIG.exponent_for(float("inf"))


def test_covariance_within_the_derived_bound():
    """cov() from the integers against the EXACT rational covariance of the float32 inputs: every entry within
    2 * 2^-Q * 2^-(e_a + e_b).  Derived: every term of S_a, S_b, S_ab is rounded by at most half a unit of 2^-Q, |S_a| <= n 2^Q,
    so S_ab - S_a S_b / (n 2^Q) errs by at most n/2 + n/2 + n/2 units, and 1.5 n / (n - 1) < 2.  (The last rounding to float64,
    2^-53 of an entry that is at most 2^-(e_a + e_b), is nine binary orders below the bound at Q = 44.)"""
    X, y = scaled_case()
    mom = moments_of(X, y)
    assert mom.Q == 44 and mom.n_left_out == 0 and mom.classes.tolist() == [1, 2, 5]
    assert len(set(mom.plane_exp.tolist())) >= 5           # planes of very different scale
    assert np.array_equal(mom.counts[[1, 2, 5]], [(y == c).sum() for c in (1, 2, 5)]) and mom.counts.sum() == 3000
    cov, mean = mom.cov(), mom.mean()
    worst = 0.0
    for j, c in enumerate((1, 2, 5)):
        Xc = X[y == c]
        exact = M.exact_cov(Xc)
        for a in range(6):
            m_exact = sum((Fraction(float(v)) for v in Xc[:, a]), Fraction(0)) / Xc.shape[0]
            assert abs(Fraction(mean[j, a]) - m_exact) <= Fraction(2) ** (-mom.Q - int(mom.plane_exp[a]))
            for b in range(6):
                bound = 2 * Fraction(2) ** (-mom.Q - int(mom.plane_exp[a]) - int(mom.plane_exp[b]))
                err = abs(Fraction(cov[j, a, b]) - exact[a][b])
                worst = max(worst, float(err / bound))
                assert err <= bound, (c, a, b, float(err), float(bound))
        assert np.allclose(cov[j], np.cov(Xc.astype(np.float64), rowvar=False), rtol=1e-9, atol=0)
    print(f"largest error / bound: {worst:.4f}")
    # ddof = 0 and the pooled covariance, against the same exact values
    c0 = mom.cov(ddof=0)
    n1 = int((y == 1).sum())
    assert np.allclose(c0[0] * n1 / (n1 - 1), cov[0], rtol=1e-14, atol=0)
    pooled = sum(((y == c).sum() - 1) * np.cov(X[y == c].astype(np.float64), rowvar=False) for c in (1, 2, 5)) / (3000 - 3)
    assert np.allclose(mom.pooled_cov(), pooled, rtol=1e-9, atol=0)
    assert np.allclose(mom.std(), np.sqrt(np.diagonal(cov, axis1=1, axis2=2)))


def test_uint8_planes_are_plain_integers():
    rng = np.random.default_rng(2402)
    q = rng.integers(0, 256, (3, 500)).astype(np.uint8)
    lab = rng.integers(0, 4, 500)
    table, left = M.moments_table(q, lab, 4, None, 0, ignore=0)
    mom = ClassMoments(table, np.zeros(3, np.int64), 0, left)
    assert left == 0 and mom.classes.tolist() == [1, 2, 3] and np.all(table[0] == 0)
    for j, c in enumerate((1, 2, 3)):
        x = q[:, lab == c].astype(np.int64)
        assert table[c, 0] == x.shape[1] and np.array_equal(table[c, 1:4], x.sum(1))
        assert np.array_equal(table[c, 4:], [(x[a] * x[b]).sum() for a, b in zip(*np.triu_indices(3))])
        assert np.allclose(mom.cov()[j], np.cov(x.astype(np.float64)), rtol=1e-12, atol=0)
        assert np.allclose(mom.mean()[j], x.mean(1), rtol=1e-15, atol=0)


def test_merge_save_load(tmp_path):
    X, y = scaled_case()
    pe = [SIG.exponent_for(np.abs(X[:, f]).max()) for f in range(6)]
    whole = moments_of(X, y, plane_exp=pe)
    top, bottom = moments_of(X[:1100], y[:1100], plane_exp=pe, n_total=3000), moments_of(X[1100:], y[1100:], plane_exp=pe, n_total=3000)
    both = top.merge(bottom)
    assert np.array_equal(both.table, whole.table) and both.Q == whole.Q and np.array_equal(both.plane_exp, whole.plane_exp)
    assert np.array_equal(both.cov(), whole.cov()) and np.array_equal(both.mean(), whole.mean())
    # a stripe without the highest label has fewer rows: the tables still add
    few = moments_of(X[y < 5][:40], y[y < 5][:40], plane_exp=pe, n_total=3000)
    assert few.table.shape[0] == 3 and np.array_equal(few.merge(whole).table, whole.merge(few).table)
    path = whole.save(tmp_path / "sig")
    assert path.endswith("sig.npz")
    back = ClassMoments.load(path)
    assert np.array_equal(back.table, whole.table) and np.array_equal(back.plane_exp, whole.plane_exp)
    assert (back.Q, back.n_left_out) == (whole.Q, whole.n_left_out)
    with pytest.raises(ValueError, match="plane exponents"):
        whole.merge(moments_of(X, y, plane_exp=[e + 1 for e in pe]))
    with pytest.raises(ValueError, match="Q = 44 and Q = 40"):
        whole.merge(moments_of(X, y, Q=40, plane_exp=pe))
    with pytest.raises(ValueError, match="plane exponents"):
        whole.merge(moments_of(X[:, :5], y))


# ---- separability ------------------------------------------------------------------------------------------------------
def _signature(seed, k=5, F=6, cond=1e4):
    """k classes with covariances of condition number <= cond (eigenvalues spread geometrically over [1 / cond, 1] of a scale)"""
    rng = np.random.default_rng(seed)
    cov = []
    for j in range(k):
        Qm, _ = np.linalg.qr(rng.standard_normal((F, F)))
        ev = (0.5 + j) * np.geomspace(1.0, 1.0 / cond ** rng.random(), F)
        cov.append((Qm * ev) @ Qm.T)
    cov = np.array([(c + c.T) / 2 for c in cov])
    assert max(np.linalg.cond(c) for c in cov) <= 1.0001 * cond
    return dict(classes=np.array([2, 3, 5, 8, 13][:k]), mean=0.4 * rng.standard_normal((k, F)), cov=cov)


def _independent(sig, kind):
    """The textbook formulas through np.linalg.slogdet / solve / inv."""
    k = len(sig["classes"])
    out = np.zeros((k, k))
    for i in range(k):
        for j in range(k):
            if i == j:
                continue
            d = sig["mean"][i] - sig["mean"][j]
            S1, S2 = sig["cov"][i], sig["cov"][j]
            if kind in ("jm", "bhattacharyya"):
                S = (S1 + S2) / 2
                B = d @ np.linalg.solve(S, d) / 8 + 0.5 * (np.linalg.slogdet(S)[1] - 0.5 * (np.linalg.slogdet(S1)[1] + np.linalg.slogdet(S2)[1]))
                out[i, j] = B if kind == "bhattacharyya" else 2 * (1 - np.exp(-B))
            else:
                I1, I2 = np.linalg.inv(S1), np.linalg.inv(S2)
                D = 0.5 * np.trace((S1 - S2) @ (I2 - I1)) + 0.5 * np.trace((I1 + I2) @ np.outer(d, d))
                out[i, j] = D if kind == "divergence" else 2000 * (1 - np.exp(-D / 8))
    return out


@pytest.mark.parametrize("cond", [10.0, 1e4])
@pytest.mark.parametrize("kind", SIG.KINDS)
def test_separability_equals_an_independent_restatement(kind, cond):
    """1e-9 relative: both sides are float64 host code on covariances of condition number <= 1e4, expected cond * eps ~ 2e-12;
    the rest is margin for the exp / log chain."""
    sig = _signature(2403 + int(cond), cond=cond)
    got, want = SIG.separability(sig, kind), _independent(sig, kind)
    assert got.shape == (5, 5) and got.dtype == np.float64
    assert np.allclose(got, want, rtol=1e-9, atol=0), float(np.max(np.abs(got - want) / np.maximum(want, 1e-300)))
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0.0) and np.all(got[~np.eye(5, dtype=bool)] > 0)
    if kind == "jm":
        assert np.all((got >= 0) & (got <= 2))
    if kind == "td":
        assert np.all((got >= 0) & (got <= 2000))


def test_separability_of_moments_and_the_report():
    X, y = scaled_case()
    mom = moments_of(X, y)
    sig = dict(classes=mom.classes, mean=mom.mean(), cov=mom.cov())
    for kind in SIG.KINDS:
        assert np.array_equal(SIG.separability(mom, kind), SIG.separability(sig, kind))
    far = dict(classes=[1, 2], mean=np.array([[0.0, 0.0], [1e3, 0.0]]), cov=np.array([np.eye(2), np.eye(2)]))
    assert SIG.separability(far, "jm")[0, 1] == 2.0 and SIG.separability(far, "td")[0, 1] == 2000.0
    same = dict(classes=[1, 2], mean=np.zeros((2, 2)), cov=np.array([np.eye(2), np.eye(2)]))
    assert SIG.separability(same, "jm")[0, 1] == 0.0 and SIG.separability(same, "divergence")[0, 1] == 0.0
    rep = SIG.separability_report(mom)
    assert rep["classes"] == [1, 2, 5] and [p["count"] for p in rep["per_class"]] == [int((y == c).sum()) for c in (1, 2, 5)]
    jm = np.array(rep["jm"]["matrix"])
    iu = np.triu_indices(3, 1)
    p = int(np.argmin(jm[iu]))
    assert rep["jm"]["least_separable"] == dict(classes=[[1, 2, 5][iu[0][p]], [1, 2, 5][iu[1][p]]], value=float(jm[iu][p]))
    assert np.allclose(rep["per_class"][2]["std"], X[y == 5].astype(np.float64).std(0, ddof=1), rtol=1e-9)
    __import__("json").dumps(rep)
    with pytest.raises(ValueError, match="kind"):
        SIG.separability(mom, "euclid")


# ---- the classifiers from moments ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_case():
    Xtr, ytr, Xte, _ = GC.blobs(4, 3, 1.5, 2404, n_train=600, n_test=1500)
    return Xtr, ytr, Xte, moments_of(Xtr, ytr)


@pytest.mark.parametrize("method", ["ml", "mahalanobis", "mindist"])
def test_fit_moments_equals_fit(method):
    """Means within half a unit of 2^-Q 2^-e_f (plus float64 rounding of the host mean); whitening matrices within the
    covariance bound propagated through the Cholesky factor and its inverse, to first order (Sun 1991, Stewart 1993)
      |dW|_F <= |W|_2^2 |L|_2 kappa_2(S) |dS|_F / (sqrt(2) |S|_2),
    doubled for the higher-order terms, with dS the derived bound per entry plus the rounding of np.cov itself
    (n eps sqrt(S_aa S_bb) per entry).  Labels: identical at every test pixel, all of which have a margin above 1e-6 under
    the fit() model."""
    Xtr, ytr, Xte, mom = fit_case()
    a = GaussianClassifier(method).fit(Xtr, ytr)
    b = GaussianClassifier(method).fit_moments(mom)
    assert np.array_equal(a.classes_, b.classes_) and np.array_equal(a.class_values_, b.class_values_)
    assert np.array_equal(a.class_counts_, b.class_counts_) and np.array_equal(a.priors_, b.priors_) and a.max_dist2_ == b.max_dist2_
    F, n, eps = 4, Xtr.shape[0], np.finfo(np.float64).eps
    unit = 2.0 ** (-mom.Q - mom.plane_exp.astype(np.float64))
    assert np.all(np.abs(a.mean_ - b.mean_) <= unit + n * eps * np.abs(Xtr).max(0))
    i, f = np.tril_indices(F)
    for j, c in enumerate(a.classes_):
        Wa, Wb = np.zeros((F, F)), np.zeros((F, F))
        Wa[i, f], Wb[i, f] = a.whiten_[j], b.whiten_[j]
        if method == "mindist":
            assert np.array_equal(Wa, np.eye(F)) and np.array_equal(Wb, Wa)
            continue
        L = np.linalg.inv(Wa)
        S = L @ L.T
        dS = 2.0 * np.outer(unit, unit) * 2.0 ** mom.Q + n * eps * np.sqrt(np.outer(np.diag(S), np.diag(S)))
        nrm = lambda m: np.linalg.norm(m, 2)   # noqa: E731
        tol = 2.0 * nrm(Wa) ** 2 * nrm(L) * np.linalg.cond(S) * np.linalg.norm(dS, "fro") / (np.sqrt(2.0) * nrm(S))
        assert np.linalg.norm(Wa - Wb, "fro") <= tol, (c, np.linalg.norm(Wa - Wb, "fro"), tol)
        assert tol < 1e-4 * nrm(Wa)   # the bound says something: four orders below the matrix it bounds
    pa, pb = a.params(), b.params()
    ra = R.classify(Xte, pa["mean"], pa["whiten"], pa["offset"], pa["class_values"], pa["max_dist2"])
    margin = ra["second"] - ra["best"]
    assert np.all(margin > 1e-6), float(margin.min())           # the condition, on the reference first
    rb = R.classify(Xte, pb["mean"], pb["whiten"], pb["offset"], pb["class_values"], pb["max_dist2"])
    assert np.array_equal(ra["labels"], rb["labels"])


def test_fit_moments_error_texts():
    Xtr, ytr, _, mom = fit_case()
    few = moments_of(np.concatenate([Xtr[ytr == 3], Xtr[ytr == 7][:4]]), np.concatenate([ytr[ytr == 3], ytr[ytr == 7][:4]]))
    with pytest.raises(ValueError, match="class 7 has 4 samples, a covariance of 4 features needs at least 5"):
        GaussianClassifier("ml").fit_moments(few)
    GaussianClassifier("mindist").fit_moments(few)
    flat = Xtr.copy()
    flat[:, 2] = 0.25
    singular = moments_of(flat, ytr)
    with pytest.raises(ValueError, match="covariance of class 3 is not positive definite"):
        GaussianClassifier("ml").fit_moments(singular)
    with pytest.raises(ValueError, match="pooled classes is not positive definite"):
        GaussianClassifier("mahalanobis").fit_moments(singular)
    with pytest.raises(ValueError, match="covariance of class 3 is singular"):
        SIG.separability(singular, "jm")
    left = ClassMoments(mom.table, mom.plane_exp, mom.Q, n_left_out=2)
    with pytest.raises(ValueError, match="X holds NaN or infinite values"):
        GaussianClassifier("ml").fit_moments(left)
    with pytest.raises(ValueError, match="integers in 1..255"):
        GaussianClassifier("ml").fit_moments(ClassMoments(np.concatenate([mom.table[3:4], mom.table[1:]]), mom.plane_exp, mom.Q))
    with pytest.raises(ValueError, match="labels no pixel"):
        GaussianClassifier("ml").fit_moments(ClassMoments(np.zeros_like(mom.table), mom.plane_exp, mom.Q))
    with pytest.raises(ValueError, match="columns"):
        ClassMoments(mom.table[:, :-1], mom.plane_exp, mom.Q)
    # the restatement itself: a value beyond the stated range leaves the pixel out, a bad label is refused
    X2 = Xtr[:50].copy()
    X2[7, 1] = np.inf
    X2[9, 0] = np.nan
    pe = [SIG.exponent_for(np.abs(Xtr[:, f]).max()) for f in range(4)]
    m2 = moments_of(X2, ytr[:50], plane_exp=pe)
    assert m2.n_left_out == 1 and m2.counts.sum() == 49
    with pytest.raises(ValueError, match="label"):
        M.moments_table(np.zeros((1, 4), np.float32), [0, 1, 2, 3], 3, [0], 10)


def test_stage_argument_errors(capsys):
    from rsseg import stages as S
    ap = S.build_parser()
    for argv in (["a.tif", "o", "--signatures"], ["a.tif", "o", "--signatures", "roi.tif"], ["a.tif", "o", "--fit-on-device"],
                 ["a.tif", "o", "--classify", "kmeans", "--fit-on-device"], ["a.tif", "o", "--classify", "random_forest", "--fit-on-device"]):
        with pytest.raises(SystemExit):
            S.parse_args(ap, argv)
    capsys.readouterr()
    a = S.parse_args(ap, ["a.tif", "o", "--classify", "kmeans", "--signatures"])
    assert a.signatures == S.SIGNATURES_OF_MAP and not a.fit_on_device
    a = S.parse_args(ap, ["a.tif", "o", "--classify", "maximum_likelihood", "--signatures", "roi.tif", "--fit-on-device", "--mask-nodata", "0"])
    assert a.signatures == "roi.tif" and a.fit_on_device
    a = S.parse_args(ap, ["a.tif", "o", "--classify", "kmeans"])
    assert a.signatures is None and not a.fit_on_device
