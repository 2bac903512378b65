"""The preconditions of tests/test_gpu_kmeans_fit.py, checked on the CPU against the oracle alone, so that the GPU tests cannot
pass vacuously: every relocation case relocates, the oracle's relocation equals a NumPy restatement of scikit-learn's own
expression (independent of oracle/kmeans_impl.h), the donor-exhausted cases exhaust a donor, the stop cases end by every rule
and a cut changes the result, other seeds give other draws."""
import numpy as np
import pytest

import kmeans_fit_cases as K

RELOC = K.relocation_cases()
DONOR = K.donor_cases()


def test_the_case_tables_cover_the_launch_table():
    """the grid the tables were searched for, whole; all 32 km_farthest<T, KMAX, FR> and every (T, KMAX, Lloyd form)"""
    grid = {(F, k, d, t) for t in ("f32", "f64") for F in K.RELOC_F for (k, d) in K.RELOC_KD}
    assert set(K.RELOC_SEEDS_SMALL) == grid and len(grid) == 90
    assert set(K.RELOC_SEEDS_LARGE) == set(K.RELOC_LARGE) and len(K.DONOR_SEEDS) == 32
    per = {}
    for _, _, _, _, F, k, d, t in RELOC + DONOR:
        assert d < k
        key = (t, K.km_kmax(k), K.km_width(F))
        per[key] = per.get(key, 0) + 1
    assert len(per) == 32 and min(per.values()) >= 2, per
    assert len({(t, K.km_kmax(k), K.km_width(F)) for (F, k, d, t) in K.DONOR_SEEDS}) == 32
    forms = {(t, K.km_kmax(k), K.lloyd_form(t, k, F)) for t, k, F in K.table_cases()}
    want = {(t, km, K.lloyd_form(t, km, fr)) for t in ("f32", "f64") for km in (8, 16, 32, 64) for fr in (8, 16, 32, 64)}
    assert forms == want and len(want) == 30 and ("f64", 64, 64) in want and ("f32", 8, 64) in want
    assert all(len(K.table_planes(t, k, F)[0]) == K.small_n(K.DT[t]) for t, k, F in K.table_cases()[:1] + K.table_cases()[-1:])


def test_generators():
    for gen in (K.protos, K.protos_flat):
        for dt, n in ((np.float32, 2051), (np.float64, 1027)):
            planes, who = gen(5, n, 9, 21, dt)
            X = np.stack(planes, 1)
            assert X.shape == (n, 9) and X.dtype == dt
            rows, inv, cnt = np.unique(X, axis=0, return_inverse=True, return_counts=True)
            assert rows.shape[0] == 21 and cnt.min() >= 3
            assert len(set(zip(inv.reshape(-1).tolist(), who.tolist()))) == 21           # `who` names the distinct rows
            span = np.ptp(X, axis=0).astype(np.float64)
            assert span.max() / span.min() > 100                     # the planes' ranges differ by orders of magnitude
            assert np.any(np.diff(who) < 0)                          # shuffled
            if gen is K.protos:
                c = np.bincount(who)
                assert np.all(np.diff(c) <= 0) and c[0] > 5 * c[-1]  # Zipf-like
            else:
                c = np.bincount(who)
                assert np.array_equal(c[2:], np.full(19, 3)) and c[0] - c[1] in (1, 2)


def _relocation_facts(oracle, case):
    _, gen, seed, n, F, k, d, t = case
    planes, who = K.case_planes(case)
    assert planes[0].size == n and planes[0].dtype == K.DT[t] and len(planes) == F
    lab, info = oracle.kmeans_fit_planes(planes, k)
    # the degenerate event: the fit ends in the iteration that relocates, so no label depends on the relocation
    assert info["relocated"] > 0 and info["n_iter"] == 2, (info["relocated"], info["n_iter"])
    if k >= 16:
        assert info["relocated"] > 1
    r = K.restate_relocation(oracle, planes, k)
    assert r["n_iter1"] == 1 and np.array_equal(r["lab"], lab)
    assert r["empty"].size == info["relocated"] == k - d and r["dist"].max() > 0
    # the relocated clusters hold exactly the rows that scikit-learn's expression picks
    got = info["centers"][r["empty"]]
    assert np.array_equal(K.bits(got), K.bits(r["rows"])), np.flatnonzero((K.bits(got) != K.bits(r["rows"])).any(axis=1))
    return planes, who, lab, info, r


@pytest.mark.parametrize("case", RELOC, ids=[c[0] for c in RELOC])
def test_relocation_cases_relocate_as_sklearns_expression_says(oracle, case):
    _relocation_facts(oracle, case)


@pytest.mark.parametrize("case", DONOR, ids=[c[0] for c in DONOR])
def test_donor_exhausted_cases(oracle, case):
    """the farthest row has 3 copies and there are k - d > 3 relocations, no multiple of 3: they go on to a second row (at
    least), a donor cluster's count reaches 0 and that cluster takes the centre of the largest one, another donor keeps some"""
    _, gen, seed, n, F, k, d, t = case
    planes, who, lab, info, r = _relocation_facts(oracle, case)
    assert k - d > 3
    taken_protos = who[r["far"]]
    assert len(set(taken_protos.tolist())) >= 2
    row2 = r["rows"][np.flatnonzero(taken_protos != taken_protos[0])[0]]
    assert (K.bits(info["centers"]) == K.bits(row2)[None, :]).all(axis=1).any()   # a relocated row of a second prototype is a centre
    given = np.bincount(lab[r["far"]], minlength=k)
    cnt = np.bincount(lab, minlength=k) - given
    assert np.any((given > 0) & (cnt > 0))      # and a donor that keeps pixels: its centre is the sum less the rows it gave
    cnt[r["empty"]] = 1
    exhausted = np.flatnonzero(cnt == 0)
    assert exhausted.size >= 1 and np.all(exhausted < d)
    big = int(np.argmax(cnt))                                                 # _average_centers: first largest weight
    for j in exhausted:
        assert np.array_equal(K.bits(info["centers"][j]), K.bits(info["centers"][big])), j


def test_constant_planes_relocate_nothing(oracle):
    planes = [np.full(K.small_n(np.float32), v, np.float32) for v in (0.25, -3.0, 7.5)]
    lab, info = oracle.kmeans_fit_planes(planes, 3)
    assert info["relocated"] == 0 and not lab.any()


@pytest.fixture(scope="module")
def stop_fits(oracle):
    """per stop case: planes, the three iteration counts, the uncut tol-0 fit"""
    out = []
    for c in K.STOP_CASES:
        planes = K.stop_planes(c)
        iters = tuple(int(oracle.kmeans_fit_planes(planes, c[1], tol=tol)[1]["n_iter"]) for tol in K.TOLS)
        out.append((c, planes, iters, oracle.kmeans_fit_planes(planes, c[1], tol=0.0)))
    return out


def test_stop_cases_end_by_every_rule(stop_fits):
    assert tuple(s[2] for s in stop_fits) == K.STOP_ITERS
    assert any(a < b for a, b, _ in K.STOP_ITERS)           # a case that the default tol ends before the labels settle
    assert any(c in (1, 2) for _, _, c in K.STOP_ITERS)     # tol = 10 ends at once
    assert {c[:4] for c in K.STOP_CASES} == {(5, 8, "f32", 2051), (9, 40, "f32", 2051), (5, 8, "f64", 1027), (9, 40, "f64", 1027),
                                             (5, 8, "f32", 33797)}


def test_a_cut_fit_differs_from_the_uncut_one(oracle, stop_fits):
    """Every max_iter below the tol-0 count s gives another result than the uncut fit.  The uncut fit ends in iteration s
    because E-step s repeats the labels of E-step s - 1, and a fit cut at m returns the labels of E-step m + 1.  So up to
    m = s - 3 the LABELS differ; m = s - 2 returns the final labels (E-step s - 1) with the centres of one M-step earlier; m = s - 1
    returns the final labels and centres and differs in n_iter alone."""
    for c, planes, (_, s, _), (full, finfo) in stop_fits:
        assert finfo["n_iter"] == s
        for m in K.stop_max_iters(s):
            lab, info = oracle.kmeans_fit_planes(planes, c[1], tol=0.0, max_iter=m)
            assert info["n_iter"] == min(m, s), (c, m)
            same_labels = np.array_equal(lab, full)
            same_centres = np.array_equal(K.bits(info["centers"]), K.bits(finfo["centers"]))
            if m <= s - 3:
                assert not same_labels, (c, m)
            elif m == s - 2:
                assert same_labels and not same_centres, (c, m)
            else:
                assert same_labels and same_centres, (c, m)


def test_other_seeds_give_other_draws(oracle):
    """the oracle's seed parameter: RandomState(seed) itself, 42 by default; other seeds seed the fit elsewhere"""
    for n, k, dt in ((2051, 8, np.float32), (1027, 40, np.float64)):
        a = oracle.kmeans_random_draws(n, k, dt)
        b = oracle.kmeans_random_draws(n, k, dt, seed=42)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        for seed in K.OTHER_SEEDS:
            rs = np.random.RandomState(seed)
            w = np.ones(n, dtype=dt)
            cid = int(rs.choice(n, p=w / w.sum()))
            u = np.concatenate([rs.uniform(size=2 + int(np.log(k))) for _ in range(k - 1)])
            got = oracle.kmeans_random_draws(n, k, dt, seed=seed)
            assert got[0] == cid and np.array_equal(got[1], u) and not np.array_equal(u, a[1])
    for c in (K.STOP_CASES[0], K.STOP_CASES[3]):
        planes = K.stop_planes(c)
        base = oracle.kmeans_fit_planes(planes, c[1])[1]["init_indices"]
        for seed in K.OTHER_SEEDS:
            assert not np.array_equal(oracle.kmeans_fit_planes(planes, c[1], seed=seed)[1]["init_indices"], base), (c, seed)
