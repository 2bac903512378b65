"""The case list of the K16 sweep (tests/test_forest_fit_cases_host.py on the CPU, tests/test_gpu_forest_fit_sweep.py on the
GPU): synthetic, seeded inputs built to reach the seams of csrc/k16_forest_fit.hip.

  sort path    root sizes around the 256-position scan chunk and the 4096-key LDS sort (one run, two runs, a run without a
               partner, 5 and 17 runs), each with continuous values and with heavy ties (max_features=None)
  scan seams   F = 1: the best split on the last lane of a chunk and the first of the next (256 / 257, 4096 / 4097), a
               same-value group over the seam, the first and the last candidate of a node
  launch seam  the alternating chain, its mirror image and a chain that peels on the right (the DFS stack grows with the
               depth) at 2047 / 2049 / 9999 nodes, with max_depth, and a bootstrap forest whose trees finish in different launches
  values       signed zeros, denormals, +-FLT_MAX, one-ulp neighbours, an all-negative matrix, at both sort paths
  capacity     64 classes, 64 features, one class, label kinds, 1 and 600 trees
  parameters   a seeded grid above 4096 samples ($RSSEG_FUZZ_N widens it)
  count rows   (DIRECT, through Context.forest_fit) integer rows that sum to n but are no bootstrap

`case(name)` returns (name, X, y, estimator kwargs, claims) and `direct_case(name)` returns (name, X, y_enc, counts, seeds,
params, claims).  `claims` says what the case exists to reach; the host test asserts every claim from scikit-learn's fitted
trees or from X itself, so a case that stops reaching its seam fails instead of passing for nothing."""
import functools
import os

import numpy as np

FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
DENORM = np.float32(1e-45)          # the smallest denormal
INT_MAX = int(np.iinfo(np.int32).max)

SORT_SIZES = (255, 256, 257, 512, 513, 4095, 4096, 4097, 8192, 8193, 12289, 20481, 65537)

# the node-size classes of ff_sort / ff_scan, by the samples of a node that is searched (a non-leaf node)
SIZE_CLASSES = {
    "<=256": lambda n: n <= 256,                      # one scan chunk
    "257-4096": lambda n: 257 <= n <= 4096,           # one LDS sort, several chunks
    "==4096": lambda n: n == 4096,                    # the largest LDS sort
    "4097-8192": lambda n: 4097 <= n <= 8192,         # two runs, one merge round
    "3 runs": lambda n: 8193 <= n <= 12288,           # a run without a partner
    ">=5 runs": lambda n: n > 16384,
    ">=17 runs": lambda n: n > 65536,
}

CASES = {}
DIRECT = {}


def _add(name, fn, *args, **kw):
    assert name not in CASES, name
    CASES[name] = functools.partial(fn, *args, **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    X, y, kw, claims = CASES[name]()
    return name, np.ascontiguousarray(X, np.float32), y, kw, claims


@functools.lru_cache(maxsize=None)
def direct_case(name):
    X, y, counts, seeds, params, claims = DIRECT[name]()
    assert all(int(r.sum()) == X.shape[0] for r in counts), name       # the contract of rsseg_forest_fit
    return name, np.ascontiguousarray(X, np.float32), y.astype(np.int32), counts.astype(np.int32), [int(s) for s in seeds], params, claims


# ---- generators -------------------------------------------------------------------------------------------------------
def continuous(n, F=6, C=3, seed=0, noise=0.1):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, F).astype(np.float32)
    y = ((X[:, 0] * 2 + X[:, min(3, F - 1)] > 1.4).astype(int) + (X[:, min(2, F - 1)] > 0.6).astype(int)) % C
    flip = rs.rand(n) < noise
    y[flip] = rs.randint(0, C, int(flip.sum()))
    return X, y


def lattice(n, C=3, seed=0, levels=8):
    """At most `levels` values per column, a constant column, two identical columns, duplicate rows with conflicting labels."""
    rs = np.random.RandomState(seed)
    X = (rs.randint(0, levels, (n, 6)) / 255.0).astype(np.float32)
    X[:, 2] = 0.5
    X[:, 4] = X[:, 3]
    y = ((X[:, 0] * 255 + 2 * X[:, 3] * 255 + X[:, 5] * 255) // 3).astype(int) % C
    flip = rs.rand(n) < 0.3
    y[flip] = rs.randint(0, C, int(flip.sum()))
    q = n // 4
    X[:q] = X[q:2 * q]
    y[:q] = (y[q:2 * q] + rs.randint(0, 2, q)) % C
    return X, y


# ---- sort path ----------------------------------------------------------------------------------------------------------
def sort_continuous(n):
    X, y = continuous(n, seed=n)
    return X, y, dict(n_estimators=2, bootstrap=False, random_state=n % 97), dict(root_n=n)


def sort_ties(n):
    X, y = lattice(n, seed=n + 1)
    return X, y, dict(n_estimators=2, bootstrap=False, max_features=None, random_state=n % 89), dict(
        root_n=n, max_levels=8, constant_column=2, identical_columns=(3, 4), conflicting_duplicates=True)


for _n in SORT_SIZES:
    _add(f"sort_continuous_{_n}", sort_continuous, _n)
    _add(f"sort_ties_{_n}", sort_ties, _n)


# ---- scan seams (F = 1; `rank` is a sample's position in the sorted column) -----------------------------------------
def _ranked(n, seed):
    rs = np.random.RandomState(seed)
    return rs, rs.permutation(n)


def seam_boundary(n, p):
    """Class 0 fills sorted positions [0, p), classes 1 and 2 share the rest: the root splits at position p."""
    rs, rank = _ranked(n, 1000 + p)
    X = (rank.astype(np.float32) * np.float32(0.25) - np.float32(100.0)).reshape(n, 1)
    y = np.where(rank < p, 0, 1 + rs.randint(0, 2, n))
    return X, y, dict(n_estimators=1, bootstrap=False, random_state=3), dict(root_n=n, root_left=p)


def seam_group(n, a, b):
    """Sorted positions a..b hold one value, with conflicting labels inside the group."""
    rs, rank = _ranked(n, 2000 + a)
    v = np.arange(n, dtype=np.float32)
    v[a:b + 1] = v[a]
    X = v[rank].reshape(n, 1)
    y = (rank // 40) % 2
    inside = (rank >= a) & (rank <= b)
    y[inside] = rank[inside] % 2
    flip = rs.rand(n) < 0.05
    y[flip] = 1 - y[flip]
    return X, y, dict(n_estimators=1, bootstrap=False, random_state=4), dict(root_n=n, equal_span=(a, b))


def seam_edge(n, last):
    """One sample of class 1 at the bottom or the top of the column: the first (pos = 1) or the last (pos = n - 1) candidate."""
    rs, rank = _ranked(n, 3000 + n + int(last))
    X = (rank.astype(np.float32) - np.float32(n // 2)).reshape(n, 1)
    y = (rank == (n - 1 if last else 0)).astype(int)
    return X, y, dict(n_estimators=1, bootstrap=False, random_state=5), dict(root_n=n, root_left=n - 1 if last else 1)


_add("seam_boundary_256", seam_boundary, 600, 256)
_add("seam_boundary_257", seam_boundary, 600, 257)
_add("seam_boundary_4096", seam_boundary, 9000, 4096)
_add("seam_boundary_4097", seam_boundary, 9000, 4097)
_add("seam_group_250_260", seam_group, 600, 250, 260)
_add("seam_group_4090_4100", seam_group, 9000, 4090, 4100)
_add("seam_first_513", seam_edge, 513, False)
_add("seam_last_513", seam_edge, 513, True)
_add("seam_first_4097", seam_edge, 4097, False)
_add("seam_last_4097", seam_edge, 4097, True)


# ---- launch seam and stack ----------------------------------------------------------------------------------------------
def chain(n, sign, max_depth=None, tie_low=False):
    """Alternating labels on a sorted column: every split peels one sample, so the tree is a chain of depth n - 1.  Peeling
    the lowest and the highest sample score the same and the first maximum wins, so the plain chain and its mirror image
    both peel on the left (the stack stays at two entries).  With tie_low the two lowest samples share one value and
    conflicting labels: position 1 is no candidate, the chain peels on the right, every level leaves one more entry on
    the stack, and the tree ends in an impure leaf of two (2n - 3 nodes, depth n - 2)."""
    v = np.arange(n, dtype=np.float32)
    if tie_low:
        v[0] = v[1]
    X = (sign * v).reshape(n, 1)
    y = np.arange(n) % 2
    claims = dict(root_n=n, chain=True, peeled="right" if tie_low and sign > 0 else "left")
    if max_depth is None:
        claims.update(nodes=2 * n - 3, depth=n - 2) if tie_low else claims.update(nodes=2 * n - 1, depth=n - 1)
    else:
        claims.update(nodes=2 * max_depth + 1, depth=max_depth)
    return X, y, dict(n_estimators=1, bootstrap=False, random_state=0, max_depth=max_depth), claims


for _n in (1024, 1025, 5000):                  # 2047, 2049 and 9999 nodes
    _add(f"chain_{_n}", chain, _n, 1)
    _add(f"chain_mirror_{_n}", chain, _n, -1)
    _add(f"chain_right_{_n + 1}", chain, _n + 1, 1, tie_low=True)
_add("chain_5000_depth50", chain, 5000, 1, 50)
_add("chain_mirror_5000_depth50", chain, 5000, -1, 50)
_add("chain_right_5001_depth50", chain, 5001, 1, 50, tie_low=True)


def mixed_launches():
    """Random labels on one continuous column: a tree has about as many nodes as samples, and the bootstrap spreads the
    trees of one forest over both sides of the 2048-node launch budget."""
    rs = np.random.RandomState(21)
    n = 3200
    X = rs.rand(n, 1).astype(np.float32)
    y = rs.randint(0, 2, n)
    return X, y, dict(n_estimators=12, bootstrap=True, random_state=8), dict(mixed_launch=2048)


_add("mixed_launches", mixed_launches)


# ---- value classes ------------------------------------------------------------------------------------------------------
def _nx(v, to):
    return np.nextafter(np.float32(v), np.float32(to))


POOLS = {
    "zeros_denormals": np.array([-FLT_MIN, -1e-38, -DENORM, -0.0, 0.0, DENORM, 1e-38, FLT_MIN], np.float32),
    "flt_max": np.array([-FLT_MAX, _nx(-FLT_MAX, 0), -1e38, -1.0, 1.0, 1e38, _nx(FLT_MAX, 0), FLT_MAX], np.float32),
    "ulp": np.array([v for b in (-1e30, -65536.0, -1.0, -0.5, -1e-30, 1e-30, 1e-3, 0.5, 1.0, 255.0, 65536.0, 1e30)
                     for v in sorted((np.float32(b), _nx(b, np.inf)))], np.float32),
}


def values(kind, n, kw):
    rs = np.random.RandomState(len(kind) * 1000 + n)
    pool = POOLS[kind]
    idx = rs.randint(0, len(pool), (n, 4))
    X = pool[idx]
    claims = dict(pool=kind)
    if kind == "zeros_denormals":
        X[:, 2] = np.where(rs.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0))   # constant for scikit-learn
        claims["zero_sign_column"] = 2
    y = idx[:, 0] % 3                                   # neighbours in the pool carry different labels
    flip = rs.rand(n) < 0.15
    y[flip] = rs.randint(0, 3, int(flip.sum()))
    return X, y, dict(n_estimators=3, max_features=None, random_state=n % 50, **kw), claims


def all_negative(n, kw):
    rs = np.random.RandomState(n + 5)
    X = -(rs.rand(n, 4) * 10.0 ** rs.randint(-3, 4, (n, 4))).astype(np.float32) - FLT_MIN
    y = (np.log10(-X[:, 0].astype(np.float64)) + 3).astype(int) % 3
    flip = rs.rand(n) < 0.1
    y[flip] = rs.randint(0, 3, int(flip.sum()))
    return X, y, dict(n_estimators=3, random_state=n % 50, **kw), dict(all_negative=True)


_add("zeros_denormals_600", values, "zeros_denormals", 600, {})
_add("zeros_denormals_9000", values, "zeros_denormals", 9000, {})
_add("flt_max_600", values, "flt_max", 600, {})
_add("flt_max_9000", values, "flt_max", 9000, {})
_add("ulp_600", values, "ulp", 600, dict(min_samples_leaf=4))
_add("ulp_9000", values, "ulp", 9000, {})
_add("all_negative_600", all_negative, 600, dict(max_depth=4))
_add("all_negative_9000", all_negative, 9000, {})


# ---- capacity at size ---------------------------------------------------------------------------------------------------
def classes_64():
    rs = np.random.RandomState(64)
    n = 20000
    X = rs.rand(n, 5).astype(np.float32)
    y = np.minimum((X[:, 0] * 64).astype(int), 63)
    flip = rs.rand(n) < 0.1
    y[flip] = rs.randint(0, 64, int(flip.sum()))
    y[:64] = np.arange(64)
    return X, y, dict(n_estimators=2, random_state=6), dict(n_classes=64, min_n=20000)


def features_64():
    rs = np.random.RandomState(65)
    n = 10000
    X = rs.rand(n, 64).astype(np.float32)
    y = (X[:, 7] + X[:, 40] > 1.0).astype(int) + (X[:, 63] > 0.5).astype(int)
    flip = rs.rand(n) < 0.02
    y[flip] = rs.randint(0, 3, int(flip.sum()))
    return X, y, dict(n_estimators=1, max_features=None, random_state=7), dict(n_features=64, min_n=10000)


def one_class():
    X, _ = lattice(300, seed=9)
    return X, np.zeros(300, int), dict(n_estimators=3, random_state=1), dict(n_classes=1, nodes=1)


def labels_strings():
    X, y = lattice(500, C=4, seed=10)
    return X, np.array(["water", "Bare soil", "forest", "urban"])[y], dict(n_estimators=4, random_state=2), dict(n_classes=4)


def labels_negative_sparse():
    X, y = lattice(500, C=4, seed=11)
    return X, np.array([-7, -2, 5, 1000])[y], dict(n_estimators=4, random_state=2), dict(n_classes=4)


def single_tree():
    X, y = lattice(300, seed=12)
    return X, y, dict(n_estimators=1, random_state=3), dict(n_estimators=1)


def many_trees():
    X, y = lattice(64, seed=13)
    return X, y, dict(n_estimators=600, random_state=4), dict(n_estimators=600)


_add("classes_64_n20000", classes_64)
_add("features_64_n10000", features_64)
_add("one_class", one_class)
_add("labels_strings", labels_strings)
_add("labels_negative_sparse", labels_negative_sparse)
_add("single_tree", single_tree)
_add("trees_600", many_trees)


# ---- parameters above 4096 samples -------------------------------------------------------------------------------------
def grid(i):
    rs = np.random.RandomState(7700 + i)
    n, F, C = int(rs.randint(5000, 30001)), int(rs.randint(2, 12)), int(rs.randint(2, 6))
    if rs.randint(2):
        X, y = continuous(n, F=F, C=C, seed=i)
    else:
        X = (rs.randint(0, 16, (n, F)) / 255.0).astype(np.float32)
        y = (X.sum(1) * 255 / 5 + rs.randint(0, 2, n)).astype(int) % C
    kw = dict(n_estimators=2, random_state=i, **{k: v[i] for k, v in _grid_table().items()})
    return X, y, kw, dict(min_n=5000)


GRID_VALUES = dict(max_depth=[1, 3, None], min_samples_leaf=[1, 50, 0.01], min_samples_split=[2, 200], max_features=[1, "sqrt", None],
                   bootstrap=[False, True])


@functools.lru_cache(maxsize=None)
def _grid_table():
    """Each parameter's values dealt out evenly over the grid (a seeded shuffle per parameter), so that a dozen cases hold
    every value of every parameter several times instead of whatever independent draws happen to give."""
    rs = np.random.RandomState(7700)
    table = {}
    for key, vals in GRID_VALUES.items():
        order = np.concatenate([rs.permutation(len(vals)) for _ in range(-(-GRID_N // len(vals)))])[:GRID_N]
        table[key] = [vals[j] for j in order]
    return table


GRID_N = int(os.environ.get("RSSEG_FUZZ_N", "12"))
for _i in range(GRID_N):
    _add(f"grid_{_i:02d}", grid, _i)


# ---- count rows that are no bootstrap (Context.forest_fit directly) ---------------------------------------------------
def _direct_data(n=2000, seed=0):
    X, y = lattice(n, seed=100 + seed, levels=32)
    X[:, 2] = X[:, 1] * np.float32(0.5) - np.float32(0.01)
    return X, y


_PARAMS = dict(max_depth=INT_MAX, min_samples_split=2, min_samples_leaf=1, max_features=2, n_classes=3)


def _skewed(rs, n):
    pick = rs.choice(n, n // 50, replace=False)
    p = np.zeros(n)
    p[pick] = rs.dirichlet(np.full(len(pick), 0.5))
    return rs.multinomial(n, p)


def _one(n, k):
    c = np.zeros(n, np.int64)
    c[k] = n
    return c


def _two(n, y):
    c = np.zeros(n, np.int64)
    a = 2 * (n // 4) + 1                      # outside the duplicated rows
    b = a + 1 + int(np.flatnonzero(y[a + 1:] != y[a])[0])
    c[a], c[b] = n // 2, n - n // 2
    return c


def direct_one_sample():
    X, y = _direct_data()
    return X, y, np.stack([_one(2000, 1234)]), [11], _PARAMS, dict(m=[1])


def direct_two_samples():
    X, y = _direct_data()
    return X, y, np.stack([_two(2000, y)]), [12], _PARAMS, dict(m=[2], nodes=[3])


def direct_skewed():
    X, y = _direct_data()
    rs = np.random.RandomState(13)
    return X, y, np.stack([_skewed(rs, 2000), _skewed(rs, 2000)]), [13, 14], _PARAMS, dict(m_about=2000 // 50)


def direct_mixed_m():
    from rsseg.forest_fit import bootstrap_counts
    X, y = _direct_data(6000, seed=1)
    n = 6000
    rs = np.random.RandomState(15)
    rows = [_one(n, 17), _two(n, y), _skewed(rs, n), bootstrap_counts(99, n).astype(np.int64), np.ones(n, np.int64)]
    return X, y, np.stack(rows), [21, 22, 23, 24, 25], _PARAMS, dict(m=[1, 2, None, None, n])


def direct_shared_ones():
    X, y = _direct_data()
    return X, y, np.ones((1, 2000), np.int64), [31, 32, 33], _PARAMS, dict(shared=True)


DIRECT.update(one_sample=direct_one_sample, two_samples=direct_two_samples, skewed=direct_skewed, mixed_m=direct_mixed_m,
              shared_ones=direct_shared_ones)


def direct_reference(name):
    """scikit-learn's tree for every tree of a DIRECT case: DecisionTreeClassifier fitted with the count row as sample_weight."""
    from sklearn.tree import DecisionTreeClassifier
    _, X, y, counts, seeds, p, _ = direct_case(name)
    trees = []
    for t, seed in enumerate(seeds):
        row = counts[t if len(counts) > 1 else 0]
        trees.append(DecisionTreeClassifier(max_features=p["max_features"], random_state=seed,
                                            max_depth=None if p["max_depth"] == INT_MAX else p["max_depth"],
                                            min_samples_split=p["min_samples_split"], min_samples_leaf=p["min_samples_leaf"])
                     .fit(X, y, sample_weight=row.astype(np.float64)))
    return trees


def assert_nodes_equal(want, got, path="tree"):
    """Node arrays in K16's layout (forest_fit.tree_nodes), floats compared bitwise."""
    assert set(want) == set(got), (path, set(want) ^ set(got))
    for k in want:
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape, (path, k, a.shape, b.shape)
        if a.dtype.kind == "f":
            assert b.dtype == a.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (path, k)
        else:
            assert np.array_equal(a, b), (path, k)
