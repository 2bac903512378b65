"""The case table of the K11 instantiation matrix (tests/test_gpu_forest_matrix.py runs it on the GPU,
tests/test_forest_matrix_cases_host.py checks on the CPU that every case takes the route it claims).  No GPU; every input
comes from a seeded NumPy generator.  The one import beyond NumPy is `lds_cap` of tests/test_gpu_forest_proba.py, the
restatement of the library's rf_lds_cap(F, TH) as a function of (F, classes) — it derives the threads from both — which that
module (and through it scikit-learn) brings along.

K11 has 72 kernel instantiations: nine (vote-row width NC, threads TH) pairs x {LDS-group, general} x {label, proba,
out-of-bag, permutation counts}.  A case is one forest and one set of rows that reach one (NC, TH, kind); the GPU module
calls the four entry points on it.  Forests are synthetic flattened dicts with the keys of rsseg.forest.flatten_forest:
random binary trees written in breadth-first order (the order rsseg_forest_load renumbers to, so a node's index here is its
index in the kernels), leaf rows that are random fractions or one-hot, internal nodes with missing_left set or cleared.

    lds     six trees of at most 63 nodes: one full group of four trees and one group of two (dummy-leaf chains); tree 2
            has a path of depth >= 10, which sets two_rounds
    shallow the same with every tree at depth <= 5: the exit test of the walk runs every round
    gen     six trees, a refill and a short last group; tree 0 has rf_lds_cap + 3 nodes, which sends the whole forest to
            the general kernel, and tree 4 (in the refilled block) has more than ntop nodes too

Rows: n = TH + 1, two workgroups, the second with one pixel.  Rows 0 and 7 carry a NaN in the feature the root of tree 0
tests and no other row carries one: the first workgroup takes the NaN-aware walk, the second the plain one."""
import collections
import functools

import numpy as np

RF_C = 4                                   # trees walked at a time
Spec = collections.namedtuple("Spec", "name th F C nc kind")
Case = collections.namedtuple("Case", "spec flat X counts y src jobs nan_feature")

ENTRY_POINTS = ("label", "proba", "oob", "perm")
#         threads, F, classes, padded row width
PAIRS = [(1024, 5, 3, 4), (1024, 5, 5, 8), (1024, 5, 9, 16), (1024, 5, 17, 32),
         (512, 33, 3, 4), (512, 33, 5, 8), (512, 33, 9, 16), (512, 33, 17, 32),
         (512, 5, 33, 64)]
SPECS = [Spec(f"{kind}-nc{nc}-th{th}", th, F, C, nc, kind) for th, F, C, nc in PAIRS for kind in ("lds", "gen")]
SPECS.append(Spec("shallow-nc4-th1024", 1024, 5, 3, 4, "shallow"))
BY_NAME = {s.name: s for s in SPECS}
assert len(BY_NAME) == len(SPECS)


# ---- what the host side of K11 decides, restated ----------------------------------------------------------------------
def rf_threads(F, C):
    return 1024 if F <= 32 and C <= 32 else 512


def row_width(C):
    return next(w for w in (4, 8, 16, 32, 64) if C <= w)


def gen_ntop(F, th):
    """Nodes per tree the general kernel keeps in LDS: 3 * TH, lowered in steps of 256 while the LDS bound binds."""
    ntop = 3 * th
    while ntop > 256 and F * th * 4 + RF_C * ntop * 8 > 158 * 1024:
        ntop -= 256
    return ntop


# ---- generators ---------------------------------------------------------------------------------------------------------
def random_tree(rng, n_nodes, F, C, max_depth=None, spine=0):
    """A random binary tree of n_nodes (odd; fewer when max_depth leaves nothing to split) in breadth-first order: a random
    leaf is split until the count is reached, after a first path of `spine` splits.  Returns the per-node arrays."""
    kids = [None]                # per node: (left, right) or None, in creation order
    depth = [0]
    open_leaves = [0]

    def split(k):
        node = open_leaves[k]
        open_leaves[k] = open_leaves[-1]
        open_leaves.pop()
        kids[node] = (len(kids), len(kids) + 1)
        for _ in range(2):
            kids.append(None)
            depth.append(depth[node] + 1)
            if max_depth is None or depth[-1] < max_depth:
                open_leaves.append(len(kids) - 1)

    for _ in range(spine):       # the newest leaf is always the last one of the list
        split(len(open_leaves) - 1)
    while len(kids) < n_nodes and open_leaves:
        split(int(rng.integers(len(open_leaves))))
    order, new = [0], {0: 0}
    for node in order:           # breadth-first numbering: the children of a node become neighbours
        if kids[node] is not None:
            for k in kids[node]:
                new[k] = len(order)
                order.append(k)
    n = len(order)
    left = np.full(n, -1, np.int32)
    right = np.full(n, -1, np.int32)
    for h, node in enumerate(order):
        if kids[node] is not None:
            left[h], right[h] = new[kids[node][0]], new[kids[node][1]]
    inner = left != -1
    feature = np.where(inner, rng.integers(0, F, n), -2).astype(np.int32)
    threshold = np.where(inner, rng.integers(0, 15, n) + 0.5, -2.0)
    missing = (inner & (rng.random(n) < 0.5)).astype(np.uint8)
    value = np.zeros((n, C))
    leaves = np.flatnonzero(~inner)
    frac = rng.random((leaves.size, C)) + 0.01
    frac /= frac.sum(axis=1, keepdims=True)
    hot = rng.random(leaves.size) < 0.4          # a share of one-hot rows: both kinds of vote row occur
    frac[hot] = np.eye(C)[rng.integers(0, C, int(hot.sum()))]
    value[leaves] = frac
    return dict(left=left, right=right, feature=feature, threshold=threshold, missing_left=missing, value=value)


def tree_sizes(spec, rng):
    """(n_nodes, max_depth, spine) of the six trees."""
    small = [(int(rng.integers(8, 32)) * 2 + 1, None, 0) for _ in range(6)]      # 17 .. 63 nodes
    if spec.kind == "shallow":
        return [(n, 5, 0) for n, _, _ in small]
    if spec.kind == "lds":
        small[2] = (63, None, 10)
        return small
    from test_gpu_forest_proba import lds_cap      # rf_lds_cap(F, rf_threads(F, classes))
    small[0] = (lds_cap(spec.F, spec.C) + 3, None, 0)
    small[4] = (2 * gen_ntop(spec.F, spec.th) + 1, None, 0)
    return small


@functools.lru_cache(maxsize=None)
def build(name):
    spec = BY_NAME[name]
    rng = np.random.default_rng(1000 + SPECS.index(spec))
    trees = [random_tree(rng, n, spec.F, spec.C, md, sp) for n, md, sp in tree_sizes(spec, rng)]
    flat = {k: np.concatenate([t[k] for t in trees]) for k in trees[0]}
    flat["value"] = np.ascontiguousarray(flat["value"])
    flat["tree_off"] = np.concatenate([[0], np.cumsum([len(t["left"]) for t in trees])]).astype(np.int64)
    flat["classes"] = (10 + 3 * np.arange(spec.C)).astype(np.int64)
    flat["n_features"] = spec.F
    n = spec.th + 1
    X = rng.integers(0, 16, (n, spec.F)).astype(np.float32)
    nan_feature = int(flat["feature"][0])          # the root of tree 0 tests it: every row meets it
    X[[0, 7], nan_feature] = np.nan
    counts = rng.integers(0, 3, (len(trees), n)).astype(np.int32)
    counts[:, 1] = 1                               # in the bag of every tree: n_oob = 0, denominator 1
    counts[:, 2] = 0                               # in none
    y = rng.integers(-1, spec.C, n).astype(np.int32)
    other = (nan_feature + 1 + int(rng.integers(0, spec.F - 1))) % spec.F
    carry = rng.permutation(n).astype(np.int32)
    at = int(np.flatnonzero(carry == 0)[0])        # row 0's NaN goes to the one row of the second workgroup
    carry[at], carry[n - 1] = carry[n - 1], 0
    src = np.stack([rng.permutation(n).astype(np.int32), carry])
    jobs = [(-1, 0), (other, 0), (nan_feature, 1)]
    for a in list(flat.values()) + [X, counts, y, src]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return Case(spec, flat, X, counts, y, src, jobs, nan_feature)
