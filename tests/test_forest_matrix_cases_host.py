"""CPU checks of the K11 instantiation matrix (tests/forest_matrix_cases.py): every case reaches the (row width, threads)
pair and the kernel kind it claims, by the rules of rsseg_forest_load and the launch plan restated here, and the table as
a whole covers the 72 instantiations.  What tests/test_gpu_forest_matrix.py relies on is asserted here, so that a case
cannot quietly take another route.  No GPU."""
import os
import re

import numpy as np
import pytest

import forest_matrix_cases as T
from test_forest_proba_host import flat_leaves
from test_gpu_forest_proba import lds_cap

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rs-image-segmentation_amd", "csrc")


def depths(flat, t):
    """Depth of every node of tree t (breadth-first order: a child comes after its parent)."""
    b, e = int(flat["tree_off"][t]), int(flat["tree_off"][t + 1])
    d = np.zeros(e - b, np.int64)
    for h in range(e - b):
        if flat["left"][b + h] != -1:
            d[flat["left"][b + h]] = d[flat["right"][b + h]] = d[h] + 1
    return d


def takes_lds_groups(flat, cap):
    """The plan rule of rsseg_forest_load: groups start at an even node, and a single tree that does not fit the node area
    behind its group's start sends the whole forest to the general kernel."""
    off = flat["tree_off"]
    return all(int(off[t + 1] - off[t]) + (int(off[t]) & 1) <= cap for t in range(len(off) - 1))


def test_constants_are_the_kernels():
    hdr = open(os.path.join(CSRC, "k11_forest.h")).read()
    assert int(re.search(r"#define RF_C (\d+)", hdr).group(1)) == T.RF_C
    assert "(F <= 32 && n_classes <= 32) ? 1024 : 512" in hdr
    assert "160L * 1024 - 256 - (long)(F | 1) * TH * 4 - 16" in hdr
    assert lds_cap(5, 3) == 12288 and lds_cap(33, 3) == 6144 and lds_cap(5, 33) == 6144
    assert T.gen_ntop(5, 1024) == 3072 and T.gen_ntop(33, 512) == 1536 and T.gen_ntop(64, 512) == 768


def test_the_table_covers_all_72_instantiations():
    combos = {(s.nc, s.th, "lds" if s.kind != "gen" else "gen", e) for s in T.SPECS for e in T.ENTRY_POINTS}
    pairs = {(nc, th) for th, _, _, nc in T.PAIRS}
    assert pairs == {(4, 1024), (8, 1024), (16, 1024), (32, 1024), (4, 512), (8, 512), (16, 512), (32, 512), (64, 512)}
    assert combos == {(nc, th, k, e) for nc, th in pairs for k in ("lds", "gen") for e in ("label", "proba", "oob", "perm")}
    assert len(combos) == 72
    assert sum(s.kind == "shallow" for s in T.SPECS) == 1


@pytest.mark.parametrize("name", list(T.BY_NAME))
def test_case_takes_the_route_it_claims(name):
    case = T.build(name)
    spec, flat, X = case.spec, case.flat, case.X
    off = flat["tree_off"]
    sizes = np.diff(off)
    assert flat["value"].shape[1] == spec.C and X.shape == (spec.th + 1, spec.F) and flat["n_features"] == spec.F
    assert (T.row_width(spec.C), T.rf_threads(spec.F, spec.C)) == (spec.nc, spec.th)
    assert len(sizes) == 6                                   # a group (or block) of four trees, then a short one of two
    cap = lds_cap(spec.F, spec.C)
    deepest = max(int(depths(flat, t).max()) for t in range(6))
    leaves = flat_leaves(flat, X)
    if spec.kind == "gen":
        ntop = T.gen_ntop(spec.F, spec.th)
        assert not takes_lds_groups(flat, cap)
        assert sizes[0] == cap + 3 and sizes[0] % 2 == 1 and sizes[4] > ntop
        for t in (0, 4):                                     # a row whose path leaves the nodes held in LDS, in both blocks
            assert ((leaves[t] - off[t]) >= ntop).any() and ((leaves[t] - off[t]) < ntop).any(), t
    else:
        assert takes_lds_groups(flat, cap) and sizes.max() <= 63
        assert int(off[4]) + (int(off[0]) & 1) <= cap and int(off[5] - off[4]) <= cap      # groups of four and of two
        assert (deepest >= 10) == (spec.kind == "lds") and (spec.kind == "lds" or deepest <= 5)
        if spec.kind == "lds":
            assert int(depths(flat, 2).max()) >= 10
    # both kinds of vote row are reached, by rows of both workgroups together
    rows = flat["value"][leaves.reshape(-1)]
    one_hot = ((rows == 1).sum(1) == 1) & ((rows == 0).sum(1) == spec.C - 1)
    assert one_hot.any() and (~one_hot).any()
    inner = flat["left"] != -1
    assert (flat["missing_left"][inner] == 1).sum() >= 3 and (flat["missing_left"][inner] == 0).sum() >= 3
    # NaN in rows 0 and 7 only, in a feature every row meets at the root of tree 0; the second workgroup has none
    assert np.flatnonzero(np.isnan(X).any(1)).tolist() == [0, 7] and np.isnan(X[[0, 7], case.nan_feature]).all()
    assert flat["feature"][0] == case.nan_feature and inner[0]
    # out-of-bag counts in {0, 1, 2}; a row in the bag of every tree and a row in none
    assert set(np.unique(case.counts)) == {0, 1, 2}
    assert (case.counts > 0).all(0).any() and (case.counts == 0).all(0).any()
    # the three jobs: no substitution, a seeded permutation of one feature, and one of the NaN feature that puts row 0's NaN
    # into the second workgroup
    (f0, _), (f1, s1), (f2, s2) = case.jobs
    n = spec.th + 1
    assert f0 == -1 and f1 not in (-1, case.nan_feature) and f2 == case.nan_feature and (s1, s2) == (0, 1)
    assert all(sorted(r.tolist()) == list(range(n)) for r in case.src)
    assert case.src[1, spec.th] == 0 and np.isnan(X[case.src[1, spec.th], f2])
    assert (case.y == -1).any() and (case.y >= 0).any() and case.y.max() < spec.C and case.y.min() >= -1
