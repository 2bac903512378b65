"""K29 without a GPU: the restatement of the sweep and of the EM loop (tests/gmm_ref.py) against np.log, exact rational
arithmetic and scikit-learn; rsseg.gmm on the restated sweep: the fit, the files, the scikit-learn round trip, the parameter
counts, the refusals."""
import functools
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

import gmm_ref as R

from rsseg import gmm as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "rsseg.h")) as f:
        text = f.read()
    assert "rsseg_gmm_sweep(" in text and "rsseg_gmm_plan(" in text
    from rsseg import _lib
    assert "rsseg_gmm_sweep" in _lib.SIGNATURES and "rsseg_gmm_plan" in _lib.SIGNATURES


# measured on the grid below (200001 points of [1, 64] and the seven powers of two): 1.0 ulp; 2 ulp is the contract's limit
LOG_ULP_MEASURED = 1.0


def test_gmm_log_against_np_log():
    s = np.concatenate([np.linspace(1.0, 64.0, 200001), 2.0 ** np.arange(7)])
    got, want = R.gmm_log(s), np.log(s)
    ulp = np.abs(got - want) / np.spacing(np.where(want == 0, 1.0, np.abs(want)))
    print("gmm_log: max ulp", ulp.max())
    assert ulp.max() <= LOG_ULP_MEASURED <= 2.0
    assert np.array_equal(got[-7:], want[-7:])   # the powers of two: e LN2_HI + e LN2_LO is the rounded e ln 2
    assert got[0] == 0.0


def test_terms_are_one_rounding_of_the_exact_product():
    rng = np.random.default_rng(3)
    q = rng.integers(1, 2 ** 20 + 1, 400).astype(np.float64)
    ua = rng.uniform(-1, 1, 400).astype(np.float32).astype(np.float64)
    ub = rng.uniform(-1, 1, 400).astype(np.float32).astype(np.float64)
    got = R.fx_term(q * (ua * 2.0 ** 30), ub)
    for i in range(400):
        exact = Fraction(q[i]) * Fraction(ua[i]) * Fraction(ub[i]) * 2 ** 30
        assert int(got[i]) == round(exact)   # Python rounds a Fraction half to even


@functools.lru_cache(maxsize=None)
def overlapping(F=5, n=2000, seed=5):
    """three overlapping components in [-1, 1]^F, n float32 samples -> ((F, n) planes, the generating means)"""
    rng = np.random.default_rng(seed)
    mus = np.array([[-0.15] * F, [0.1] * F, [0.2, -0.1, 0.15, 0.0, -0.2][:F] + [0.0] * max(0, F - 5)])
    parts = []
    for j, m in enumerate(mus):
        A = rng.normal(size=(F, F)) * 0.08 + np.eye(F) * 0.12
        parts.append(m + rng.normal(size=(n // 3 + (j == 0) * (n - 3 * (n // 3)), F)) @ A.T)
    X = np.clip(np.concatenate(parts), -1, 1).astype(np.float32)
    X.setflags(write=False)
    P = np.ascontiguousarray(X.T)
    P.setflags(write=False)
    return P, mus


def start(F=5, k=3):
    _, mus = overlapping(F)
    return np.array([0.3, 0.3, 0.4]), mus + 0.05, np.stack([np.eye(F) * 0.05] * k)


@functools.lru_cache(maxsize=None)
def ref_fit(ct, max_iter=30, masked=False):
    P, _ = overlapping()
    w0, mu0, cov0 = start()
    mask = (np.arange(P.shape[1]) % 7 != 0).astype(np.uint8) if masked else None
    return R.em_ref(P, mask, np.zeros(5, int), w0, mu0, cov0, ct, tol=0.0, reg_covar=1e-6, max_iter=max_iter)


# scikit-learn 1.7.2, 30 iterations, the reference against GaussianMixture (weights, means, covariances):
#   full  1.13e-8  1.21e-8  5.94e-9        diag  7.22e-8  7.70e-8  2.00e-8
# the tolerances are ten times these; none may pass 1e-6
SK_TOL = {"full": (1.2e-7, 1.3e-7, 6.0e-8), "diag": (7.3e-7, 7.7e-7, 2.0e-7)}


@pytest.mark.parametrize("ct", ["full", "diag"])
def test_reference_em_against_scikit_learn(ct):
    from sklearn import mixture
    P, _ = overlapping()
    w0, mu0, cov0 = start()
    prec = np.stack([np.linalg.inv(c) for c in cov0]) if ct == "full" else 1.0 / np.stack([np.diag(c) for c in cov0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = mixture.GaussianMixture(3, covariance_type=ct, tol=0.0, reg_covar=1e-6, max_iter=30, weights_init=w0, means_init=mu0,
                                     precisions_init=prec).fit(P.T.astype(np.float64))
    o = ref_fit(ct)
    assert o["n_iter"] == gm.n_iter_ == 30
    resp = gm.predict_proba(P.T.astype(np.float64))
    assert (resp.max(axis=1) < 0.99).mean() > 0.2   # the components overlap: the responsibilities are not 0 or 1
    cov = o["covs"] if ct == "full" else np.stack([np.diag(c) for c in o["covs"]])
    d = (np.abs(o["weights"] - gm.weights_).max(), np.abs(o["means"] - gm.means_).max(), np.abs(cov - gm.covariances_).max())
    print(ct, "reference - scikit-learn: weights %.3g means %.3g covariances %.3g" % d)
    assert max(SK_TOL[ct]) <= 1e-6
    assert d[0] <= SK_TOL[ct][0] and d[1] <= SK_TOL[ct][1] and d[2] <= SK_TOL[ct][2]


def _model(ct, max_iter=30, **kw):
    w0, mu0, cov0 = start()
    cov = {"full": cov0, "diag": np.stack([np.diag(c) for c in cov0]), "tied": cov0[0], "spherical": np.full(3, 0.05)}[ct]
    return G.GaussianMixtureModel(3, ct, tol=0.0, reg_covar=1e-6, max_iter=max_iter, init=(w0, mu0, cov), **kw)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ct", ["full", "diag"])
def test_fit_on_the_restated_sweep_equals_the_restated_loop(ct, masked):
    P, _ = overlapping()
    o = ref_fit(ct, 8, masked)
    mask = (np.arange(P.shape[1]) % 7 != 0).astype(np.uint8) if masked else None
    m = _model(ct, 8)
    res = m.fit(P, mask=mask, ranges=[(-1, 1)] * 5, sweep=R.ref_sweep, keep_tables=True)
    assert m.n_iter_ == o["n_iter"] == 8 and m.tables_ == o["tables"]
    assert np.array_equal(m.weights_, o["weights"]) and np.array_equal(m.means_, o["means"]) and np.array_equal(m._cov, o["covs"])
    assert np.array_equal(res.labels.reshape(-1), o["labels"]) and res.n_left_out == o["n_left_out"] == 0
    assert len(res.history) == 8 and all(h["dropped"] == [] and h["n_far"] == 0 for h in res.history)
    assert abs(sum(res.history[-1]["weights"]) - 1.0) < 1e-12
    if masked:
        assert np.all(res.labels.reshape(-1)[::7] == 0) and np.all(res.labels.reshape(-1)[1::7] > 0)


def test_stopping_rule_and_the_other_covariance_types():
    P, _ = overlapping()
    for ct in ("tied", "spherical"):
        m = _model(ct, 100)
        m.tol = 1e-3
        res = m.fit(P, ranges=[(-1, 1)] * 5, sweep=R.ref_sweep)
        lb = [h["lower_bound"] for h in res.history]
        assert m.converged_ and 2 <= m.n_iter_ < 100 and abs(lb[-1] - lb[-2]) < 1e-3 and all(abs(b - a) >= 1e-3 for a, b in zip(lb[:-2], lb[1:-1]))
        assert all(b >= a - 1e-9 for a, b in zip(lb, lb[1:]))   # EM does not lower the likelihood (beyond the quantum of q)
        c = m.covariances_
        assert c.shape == ((5, 5) if ct == "tied" else (3,))
        gc = m.to_gaussian_classifier()
        assert gc.mean_.shape == (3, 5) and list(gc.class_values_) == [1, 2, 3] and np.array_equal(gc.priors_, m.weights_)


def test_stripes_add_up_to_the_whole():
    P, _ = overlapping()
    w0, mu0, cov0 = start()
    for ct in ("full", "diag"):
        km = R.kernel_model_ref(w0, mu0, cov0, np.zeros(5, int), 20, ct)
        args = (np.zeros(5, int), 20, km["mean"], km["whiten"], km["offset"], km["diag"])
        whole = R.sweep_ref(P[:, :900], None, *args)
        a, b = R.sweep_ref(P[:, :389], None, *args), R.sweep_ref(P[:, 389:900], None, *args)
        assert np.array_equal(R.table_array(whole["table"]), R.table_array(a["table"]) + R.table_array(b["table"]))
        for key in ("n_counted", "n_left_out", "n_far", "ll_sum"):
            assert whole[key] == a[key] + b[key]
        assert (np.asarray(whole["q"]).sum(axis=0) - 2 ** 20).max() <= 2   # the weights of a pixel sum to 2^20 but for their roundings


def test_save_load_and_scikit_learn_round_trip(tmp_path):
    P, _ = overlapping()
    for ct in G.COVARIANCE_TYPES:
        m = _model(ct, 3)
        m.fit(P, ranges=[(-1, 1)] * 5, sweep=R.ref_sweep)
        path = m.save(str(tmp_path / f"gmm_{ct}"))
        assert path.endswith(".npz")
        with np.load(path, allow_pickle=False) as z:
            assert str(z["format"]) == "rsseg.GaussianMixtureModel" and int(z["version"]) == G.FORMAT_VERSION
        back = G.GaussianMixtureModel.load(path)
        assert back.covariance_type == ct and back.n_iter_ == 3 and back.dtype_ == "float32" and np.array_equal(back.plane_exp_, m.plane_exp_)
        for x, y in ((back.weights_, m.weights_), (back.means_, m.means_), (back.covariances_, m.covariances_)):
            assert np.array_equal(x, y)
        assert np.array_equal(back.predict(P, sweep=R.ref_sweep), m.predict(P, sweep=R.ref_sweep))
        gm = m.to_sklearn()
        X = P.T.astype(np.float64)
        assert gm.covariances_.shape == m.covariances_.shape
        # scikit-learn's own densities from the exported parameters: the labels and the mean log-likelihood
        lab = m.predict(P, sweep=R.ref_sweep).reshape(-1)
        resp = gm.predict_proba(X)
        srt = np.sort(resp, axis=1)
        clear = srt[:, -1] - srt[:, -2] > 1e-6
        assert np.array_equal(gm.predict(X)[clear] + 1, lab[clear])
        assert abs(gm.score(X) - m.score(P, sweep=R.ref_sweep)) < 1e-6
        assert np.allclose(gm.score_samples(X), m.score_samples(P, sweep=R.ref_sweep), rtol=0, atol=1e-5)   # a float32 map
        again = G.GaussianMixtureModel.from_sklearn(gm)
        for x, y in ((again.weights_, m.weights_), (again.means_, m.means_), (again.covariances_, m.covariances_)):
            assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="not a Gaussian mixture model file"):
        np.savez(str(tmp_path / "other.npz"), a=np.zeros(1))
        G.GaussianMixtureModel.load(str(tmp_path / "other.npz"))


def test_bic_aic_parameter_counts_are_scikit_learns():
    P, _ = overlapping()
    X = P.T.astype(np.float64)
    for ct in G.COVARIANCE_TYPES:
        m = _model(ct, 2)
        m.fit(P, ranges=[(-1, 1)] * 5, sweep=R.ref_sweep)
        gm = m.to_sklearn()
        assert m.n_parameters() == gm._n_parameters() == G.n_parameters(3, 5, ct)
        assert abs(m.bic(P, sweep=R.ref_sweep) - gm.bic(X)) < 1e-6 * X.shape[0] * 2 + 1e-6
        assert abs(m.aic(P, sweep=R.ref_sweep) - gm.aic(X)) < 1e-6 * X.shape[0] * 2 + 1e-6


def test_select_components_prefers_the_generating_count():
    P, _ = overlapping()
    lab = np.arange(P.shape[1]) * 3 // P.shape[1]   # the generating component; a label >= k labels nothing
    table, best = G.select_components(P, (1, 2, 3), ranges=[(-1, 1)] * 5, sweep=R.ref_sweep, covariance_type="full", max_iter=15, init=lab)
    assert [row["k"] for row in table] == [1, 2, 3] and best.n_components == 3
    assert table[2]["bic"] < table[1]["bic"] < table[0]["bic"] and table[2]["aic"] < table[0]["aic"]
    with pytest.raises(ValueError, match="criterion"):
        G.select_components(P, (1,), criterion="icl", sweep=R.ref_sweep)


def test_a_component_without_weight_is_dropped():
    P, _ = overlapping()
    w0, mu0, cov0 = start()
    mu = np.vstack([mu0, [[0.95] * 5]])
    m = G.GaussianMixtureModel(4, "diag", tol=0.0, max_iter=2,
                               init=(np.array([0.3, 0.3, 0.3, 0.1]), mu, np.vstack([np.full((3, 5), 0.05), np.full((1, 5), 1e-5)])))
    res = m.fit(P, ranges=[(-1, 1)] * 5, sweep=R.ref_sweep)
    assert res.history[0]["dropped"] == [3] and m.n_components == 3 and len(res.weights) == 3 and res.labels.max() == 3


def test_refusals():
    P, _ = overlapping()
    with pytest.raises(ValueError, match="n_components=33"):
        G.GaussianMixtureModel(33)
    with pytest.raises(ValueError, match="covariance_type"):
        G.GaussianMixtureModel(2, "banded")
    with pytest.raises(ValueError, match="gmm: 65 planes, at most 64"):
        G.GaussianMixtureModel(1, init=np.zeros(4)).fit(np.zeros((65, 4), np.float32), sweep=R.ref_sweep)
    with pytest.raises(ValueError, match="Q=31"):
        G.check_q(31, 16)
    with pytest.raises(ValueError, match="Q=20"):
        G.check_q(20, 2 ** 23)
    G.check_q(G.q_for(2 ** 28), 2 ** 28)
    with pytest.raises(ValueError, match="uint8 pixels in one call, at most 2\\^26"):   # fit and predict check before anything goes to the device
        G.GaussianMixtureModel(1, init=np.zeros(4)).fit(np.zeros((1, 2 ** 26 + 1), np.uint8), sweep=R.ref_sweep)
    assert G.q_for(2 ** 28) == 14 and G.q_for(100) == 30 and G.q_for(2 ** 28 + 1) == 13
    with pytest.raises(AssertionError):
        R.sweep_ref(P[:, :10], None, np.zeros(5, int), 31, np.zeros((1, 5)), R.pack_lower(np.eye(5)[None]), np.zeros(1))
    bad = np.eye(5) * 0.05
    bad[0, 1] = bad[1, 0] = 0.06
    with pytest.raises(ValueError, match="not positive definite"):
        G.GaussianMixtureModel.from_params([1.0], np.zeros((1, 5)), bad[None])
    with pytest.raises(ValueError, match="all be float32 or all uint8"):
        G.GaussianMixtureModel(1, init=np.zeros(4)).fit([np.zeros(4, np.float32), np.zeros(4, np.uint8)], sweep=R.ref_sweep)
    with pytest.raises(ValueError, match="sum to 1"):
        G.GaussianMixtureModel.from_params([0.5, 0.6], np.zeros((2, 5)), np.stack([np.eye(5)] * 2))
    m = G.GaussianMixtureModel.from_params([1.0], np.zeros((1, 5)), np.eye(5)[None])
    with pytest.raises(ValueError, match="4 planes"):
        m.predict(P[:4], sweep=R.ref_sweep)
    with pytest.raises(ValueError, match="uint8 planes"):
        m.predict(np.zeros((5, 8), np.uint8), sweep=R.ref_sweep)
    with pytest.raises(ValueError, match="not fitted"):
        G.GaussianMixtureModel(2).predict(P, sweep=R.ref_sweep)


# ---- the stage driver's options ---------------------------------------------------------------------------------------------
def test_command_line_options_reach_the_stage(monkeypatch, capsys):
    from rsseg import stages as S
    seen = []
    monkeypatch.setattr(S, "_run_scripts_2_3", lambda *args: seen.append(args) or {"paths": {"pkl": "somewhere"}, "class_map": np.zeros((1, 1), np.uint8)})
    assert S.main(["scene.tif", "out", "--classify", "gmm", "--n-clusters", "5", "--gmm-covariance", "tied", "--gmm-iterations", "7", "--gmm-tol", "0.01",
                   "--gmm-reg-covar", "1e-4", "--gmm-posterior", "--gmm-model", "m.npz", "--sieve", "3"]) == 0
    (image, out, o, ctx), = seen
    assert (image, out, ctx) == ("scene.tif", "out", None) and isinstance(o, S.GmmRunOptions) and isinstance(o, S.RunOptions)
    assert o.gmm == dict(covariance="tied", iterations=7, tol=0.01, reg_covar=1e-4, posterior=True, model_path="m.npz")
    assert (o.classify, o.n_clusters, o.sieve, o.isodata) == ("gmm", 5, 3, None)
    seen.clear()
    assert S.main(["scene.tif", "out", "--classify", "gmm"]) == 0
    assert seen[0][2].gmm == dict(covariance="full", iterations=100, tol=1e-3, reg_covar=1e-6, posterior=False, model_path=None) == S.GMM_DEFAULTS
    seen.clear()
    assert S.main(["scene.tif", "out", "--classify", "kmeans"]) == 0
    assert type(seen[0][2]) is S.RunOptions   # every other run keeps the options it had
    capsys.readouterr()
    for argv, text in ((["--classify", "kmeans", "--gmm-posterior"], "--gmm-posterior need --classify gmm"),
                       (["--gmm-covariance", "diag"], "--gmm-covariance need --classify gmm"),
                       (["--classify", "gmm", "--n-clusters", "33"], "--n-clusters in 1..32"),
                       (["--classify", "gmm", "--gmm-iterations", "0"], "--gmm-iterations takes a positive count"),
                       (["--classify", "gmm", "--gmm-tol", "-1"], "--gmm-tol takes a finite non-negative number"),
                       (["--classify", "gmm", "--gmm-covariance", "banded"], "invalid choice")):
        with pytest.raises(SystemExit):
            S.main(["scene.tif", "out"] + argv)
        assert text in capsys.readouterr().err, argv
    assert seen == [seen[0]]
    import inspect
    sig = inspect.signature(S.run_gmm_stage).parameters
    assert {k: sig[k].default for k in S.GMM_DEFAULTS} == S.GMM_DEFAULTS
