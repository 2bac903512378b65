"""The K16 case list (tests/forest_fit_cases.py) on the CPU: every case reaches what it claims (asserted from scikit-learn's
fitted trees or from X itself, never from the code under test), the kernel's formulation (tests/forest_fit_ref.py) equals
scikit-learn on every case of at most 10 000 samples, and the list has teeth: each deliberate mistake of
forest_fit_ref.VARIANTS is told apart from scikit-learn by a case of at most 1000 samples."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "rs-image-segmentation_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from sklearn.ensemble import RandomForestClassifier  # noqa: E402

import forest_fit_cases as K  # noqa: E402
import forest_fit_ref as R  # noqa: E402
from rsseg import forest_fit as FF  # noqa: E402
from test_forest_fit_host import ref_fit, state_equal  # noqa: E402

REF_MAX_N = 10_000      # the NumPy reference is O(n C) per node: larger cases are compared on the GPU only
VARIANT_MAX_N = 1000


@functools.lru_cache(maxsize=None)
def sk_fit(name):
    _, X, y, kw, _ = K.case(name)
    return RandomForestClassifier(n_jobs=8, **kw).fit(X, y)


def searched_sizes(forest):
    """n_node_samples of every non-leaf node of every tree."""
    return np.concatenate([t.tree_.n_node_samples[t.tree_.children_left >= 0] for t in forest.estimators_])


def nodes_equal(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]).view(np.uint8) if np.asarray(a[k]).dtype.kind == "f" else a[k],
                                                   np.asarray(b[k]).view(np.uint8) if np.asarray(b[k]).dtype.kind == "f" else b[k])
                                    for k in a)


# ---- the claims -----------------------------------------------------------------------------------------------------
def has_value_class(X, kind):
    neg0 = (X == 0) & np.signbit(X)
    pos0 = (X == 0) & ~np.signbit(X)
    a = np.abs(X)
    if kind == "zeros_denormals":
        return neg0.any() and pos0.any() and ((a > 0) & (a < K.FLT_MIN)).any() and (X == K.DENORM).any() and (X == -K.DENORM).any() \
            and (a == K.FLT_MIN).any()
    if kind == "flt_max":
        below = np.nextafter(K.FLT_MAX, np.float32(0))
        return all((X == v).any() for v in (K.FLT_MAX, -K.FLT_MAX, below, -below, np.float32(1e38), np.float32(-1e38)))
    if kind == "ulp":
        u = np.unique(X)
        pairs = u[:-1][np.nextafter(u[:-1], np.float32(np.inf)) == u[1:]]
        return (pairs < -1).any() and ((pairs < 0) & (pairs > -1e-20)).any() and (pairs > 60000).any() and (np.abs(pairs) >= 1e30).any()
    raise AssertionError(kind)


CLAIM_KEYS = {"root_n", "root_left", "equal_span", "nodes", "depth", "chain", "peeled", "mixed_launch", "pool", "zero_sign_column",
              "all_negative", "n_classes", "n_features", "n_estimators", "min_n", "max_levels", "constant_column", "identical_columns",
              "conflicting_duplicates"}


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_reaches_what_it_claims(name):
    _, X, y, kw, claims = K.case(name)
    assert claims and set(claims) <= CLAIM_KEYS, set(claims) - CLAIM_KEYS
    f = sk_fit(name)
    trees = [t.tree_ for t in f.estimators_]
    n = X.shape[0]
    for key, want in claims.items():
        if key == "root_n":
            assert kw.get("bootstrap") is False and n == want
            assert all(t.n_node_samples[0] == want for t in trees)
        elif key == "root_left":
            assert all(t.n_node_samples[t.children_left[0]] == want for t in trees)
        elif key == "equal_span":
            col = np.sort(X[:, 0])
            a, b = want
            assert col[a] == col[b] and col[a - 1] < col[a] and col[b] < col[b + 1]
            seams = [s for s in (256, 4096) if a < s <= b]
            assert seams and all(col[s - 1] == col[s] for s in seams)          # equal on both sides of the seam
            inside = np.argsort(X[:, 0], kind="stable")[a:b + 1]
            assert len(set(y[inside])) > 1
        elif key == "nodes":
            assert all(t.node_count == want for t in trees)
        elif key == "depth":
            assert all(t.max_depth == want for t in trees)
        elif key == "chain":
            for t in trees:      # every split has a leaf child
                inner = np.flatnonzero(t.children_left >= 0)
                assert np.all((t.children_left[t.children_left[inner]] < 0) | (t.children_left[t.children_right[inner]] < 0))
        elif key == "peeled":
            for t in trees:      # which child is the one-sample leaf, at most of the splits
                inner = np.flatnonzero(t.children_left >= 0)
                left_leaf = t.children_left[t.children_left[inner]] < 0
                right_leaf = t.children_left[t.children_right[inner]] < 0
                share = np.mean(left_leaf & ~right_leaf) if want == "left" else np.mean(right_leaf & ~left_leaf)
                assert share > 0.9, share
        elif key == "mixed_launch":
            counts = [t.node_count for t in trees]
            assert kw["bootstrap"] is True and min(counts) <= want < max(counts), counts
        elif key == "pool":
            assert has_value_class(X, want)
        elif key == "zero_sign_column":
            col = X[:, want]
            assert np.all(col == 0) and np.signbit(col).any() and not np.signbit(col).all()
            assert all(want not in t.feature for t in trees)               # constant for scikit-learn
        elif key == "all_negative":
            assert np.all(X < 0)
        elif key == "n_classes":
            assert f.n_classes_ == want
        elif key == "n_features":
            assert X.shape[1] == want and kw.get("max_features", "sqrt") is None
        elif key == "n_estimators":
            assert len(trees) == want
        elif key == "min_n":
            assert n >= want
        elif key == "max_levels":
            assert max(len(np.unique(X[:, j])) for j in range(X.shape[1])) <= want and kw["max_features"] is None
        elif key == "constant_column":
            assert len(np.unique(X[:, want])) == 1
        elif key == "identical_columns":
            assert np.array_equal(X[:, want[0]], X[:, want[1]]) and len(np.unique(X[:, want[0]])) > 1
        elif key == "conflicting_duplicates":
            _, inv = np.unique(X, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            assert any(len(set(y[inv == g])) > 1 for g in range(min(inv.max() + 1, 50)))


def test_chains_peel_on_both_sides_at_every_node_count():
    """Measured on scikit-learn: the mirror image of the alternating chain peels on the same side as the chain itself (the
    two ends tie and the first maximum wins), so the chain that grows the stack is the one with the tied lowest pair."""
    for n, nodes in ((1024, 2047), (1025, 2049), (5000, 9999)):
        sides = set()
        for name in (f"chain_{n}", f"chain_mirror_{n}", f"chain_right_{n + 1}"):
            claims = K.case(name)[4]
            assert claims["nodes"] == nodes and claims["depth"] == (nodes - 1) // 2
            sides.add(claims["peeled"])
        assert sides == {"left", "right"}
    assert K.case("chain_right_5001_depth50")[4]["peeled"] == "right"


def test_sort_sizes_and_grid_are_as_the_list_says():
    for n in K.SORT_SIZES:
        for kind in ("continuous", "ties"):
            assert K.case(f"sort_{kind}_{n}")[4]["root_n"] == n
    assert set(K.SORT_SIZES) >= {255, 256, 257, 512, 513, 4095, 4096, 4097, 8192, 8193, 12289, 20481, 65537}
    grid = [K.case(k)[3] for k in K.CASES if k.startswith("grid_")]
    assert len(grid) >= 12
    assert K.GRID_VALUES == dict(max_depth=[1, 3, None], min_samples_leaf=[1, 50, 0.01], min_samples_split=[2, 200],
                                 max_features=[1, "sqrt", None], bootstrap=[False, True])
    for key, values in K.GRID_VALUES.items():
        for v in values:
            assert sum(kw[key] == v and type(kw[key]) is type(v) for kw in grid) >= len(grid) // len(values), (key, v)
    assert all(5000 <= K.case(k)[1].shape[0] <= 30000 for k in K.CASES if k.startswith("grid_"))


@pytest.mark.parametrize("kind", ["continuous", "ties"])
def test_node_size_classes_are_hit(kind):
    """Both halves of the sort family, each on its own, search nodes of every size class of ff_sort / ff_scan."""
    sizes = np.concatenate([searched_sizes(sk_fit(f"sort_{kind}_{n}")) for n in K.SORT_SIZES])
    for name, pred in K.SIZE_CLASSES.items():
        assert any(pred(int(s)) for s in np.unique(sizes)), (kind, name)


@pytest.mark.parametrize("name", ["classes_64_n20000", "features_64_n10000"] + [k for k in K.CASES if k.startswith("grid_")])
def test_capacity_and_grid_cases_search_nodes_above_one_lds_sort(name):
    assert searched_sizes(sk_fit(name)).max() > 4096


# ---- the formulation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in K.CASES if K.case(k)[1].shape[0] <= REF_MAX_N])
def test_reference_formulation_equals_sklearn(name):
    _, X, y, kw, _ = K.case(name)
    state_equal(RandomForestClassifier(**kw).fit(X, y), ref_fit(RandomForestClassifier(**kw), X, y))


@pytest.mark.parametrize("name", list(K.DIRECT))
def test_count_row_cases(name):
    """The count rows sum to n, reach the m they claim, and forest_fit_ref equals DecisionTreeClassifier(sample_weight=row)."""
    _, X, y, counts, seeds, p, claims = K.direct_case(name)
    n = X.shape[0]
    want = K.direct_reference(name)
    assert len(want) == len(seeds)
    m = [int((counts[t if len(counts) > 1 else 0] > 0).sum()) for t in range(len(seeds))]
    assert all(int(r.sum()) == n and r.min() >= 0 for r in counts)
    if "m" in claims:
        assert all(w is None or w == g for w, g in zip(claims["m"], m))
        assert len(m) == 1 or max(m) > 20 * min(m)         # very different m in one call
        assert [t.tree_.n_node_samples[0] for t in want] == m
    if "nodes" in claims:
        assert [t.tree_.node_count for t in want] == claims["nodes"]
    if "m_about" in claims:
        assert all(0.5 * claims["m_about"] <= v <= claims["m_about"] for v in m), m
    if "shared" in claims:
        assert counts.shape == (1, n) and np.all(counts == 1) and len(seeds) > 1
    for t, seed in enumerate(seeds):
        got = R.build_tree(X, y, counts[t if len(counts) > 1 else 0], p["n_classes"], FF.splitter_seed(seed), p["max_depth"],
                           p["min_samples_split"], p["min_samples_leaf"], p["max_features"])
        assert nodes_equal(FF.tree_nodes(want[t]), got), (name, t)


# ---- the teeth ------------------------------------------------------------------------------------------------------
def variant_differs(name, variant, max_trees=4):
    """True when forest_fit_ref with the deliberate mistake grows a tree that differs from scikit-learn's on this case."""
    _, X, y, kw, _ = K.case(name)
    f = sk_fit(name)
    Xf, y_enc, classes, rp = FF.prepare(RandomForestClassifier(**kw), X, y)
    for t in f.estimators_[:max_trees]:
        s = int(t.random_state)
        counts = FF.bootstrap_counts(s, len(y_enc)) if kw.get("bootstrap", True) else np.ones(len(y_enc), np.int32)
        args = (Xf, y_enc, counts, len(classes), FF.splitter_seed(s), rp["max_depth"], rp["min_samples_split"], rp["min_samples_leaf"],
                rp["max_features"])
        assert nodes_equal(FF.tree_nodes(t), R.build_tree(*args)), name        # the unpatched builder is right here
        if not nodes_equal(FF.tree_nodes(t), R.build_tree(*args, variant=variant)):
            return True
    return False


SMALL = [k for k in K.CASES if K.case(k)[1].shape[0] <= VARIANT_MAX_N]


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_every_deliberate_mistake_is_caught_by_a_small_case(variant):
    caught = [name for name in SMALL if variant_differs(name, variant)]
    print(f"\n[K16 cases] variant {variant!r} ({R.VARIANTS[variant]}): caught by {', '.join(caught) or 'NOTHING'}")
    assert caught, f"no case of at most {VARIANT_MAX_N} samples tells variant {variant!r} from scikit-learn"
