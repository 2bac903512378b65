"""K27 without a GPU: the header and the bindings agree; the restatement of the region adjacency graph (tests/adjacency_ref.py)
is consistent with K25's perimeter and commutes with relabelling; RegionGraph.merge equals the dictionary restatement; the
restated region merging keeps its promises (adjacent merges, nested scales, an exact region count, no small region left); and
the command line refuses what it must."""
import functools
import os
import re

import numpy as np
import pytest

import adjacency_ref as A
import objects_ref as O
import slic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_bindings():
    import ctypes as C
    from rsseg import _lib
    hdr = open(os.path.join(ROOT, "include", "rsseg.h")).read()
    for name, nargs in (("rsseg_segment_adjacency", 11), ("rsseg_segment_adjacency_plan", 4)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in rsseg.h"
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs
    assert _lib.SIGNATURES["rsseg_segment_adjacency"][0] is C.c_int and _lib.SIGNATURES["rsseg_segment_adjacency_plan"][0] is None
    lib = _lib.load()
    tw, th, slots = C.c_int(0), C.c_int(0), C.c_int(0)
    lib.rsseg_segment_adjacency_plan(16, C.byref(tw), C.byref(th), C.byref(slots))   # host-only: needs no GPU
    assert tw.value >= 4 and th.value >= 1 and slots.value >= 1
    assert "segment_adjacency" in open(os.path.join(ROOT, "rs-image-segmentation_amd", "csrc", "k27_adjacency.hip")).read()


@functools.lru_cache(maxsize=None)
def small_scene(masked=False):
    shape = (40, 56)
    planes = R.scene(270, shape, 3, cell=6, noise=0.1)
    mask = None
    if masked:
        mask = (np.random.RandomState(271).rand(*shape) < 0.9).astype(np.uint8)
        mask[shape[0] // 2, :] = 0
    seg, n, _, _ = R.slic_ref(planes, 8, 0.3, 2, 0, mask)
    return seg, n, planes, mask


def test_border_lengths_add_up_to_the_perimeter():
    seg, n, planes, _ = small_scene()
    assert seg.min() >= 1                                        # a map without label 0
    edges = A.adjacency_ref(seg, planes, None, n)
    assert edges.shape[1] == 6 and (edges[:, 0] < edges[:, 1]).all() and (edges[:, 2] > 0).all()
    per = O.object_table_ref(seg, (), None, n)[:, 10]
    assert np.array_equal(A.border_ref(edges, n) + A.image_border_sides(seg, None, n), per)
    masked, nm, _, mask = small_scene(True)                      # with label 0 and a mask: the sides facing 0 join the image border's
    em = A.adjacency_ref(masked, (), mask, nm)
    assert np.array_equal(A.border_ref(em, nm) + A.image_border_sides(masked, mask, nm), O.object_table_ref(masked, (), mask, nm)[:, 10])


@pytest.mark.parametrize("masked", [False, True])
def test_graph_commutes_with_relabelling(masked):
    seg, n, planes, mask = small_scene(masked)
    rs = np.random.RandomState(272)
    parent = np.concatenate([[0], rs.randint(1, n // 3 + 1, n)]).astype(np.int64)
    edges = A.adjacency_ref(seg, planes, mask, n)
    painted = parent[seg].astype(np.int32)
    want = A.adjacency_ref(painted, planes, mask, int(parent.max()))
    assert np.array_equal(A.merge_graph_ref(edges, parent), want)


def test_region_graph_merge_and_sums():
    from rsseg.regions import RegionGraph
    seg, n, planes, mask = small_scene(True)
    edges = A.adjacency_ref(seg, planes, mask, n)
    g = RegionGraph.from_table(edges, n)
    assert np.array_equal(g.table(), edges) and np.array_equal(g.border(), A.border_ref(edges, n))
    assert np.array_equal(g.degree(), np.bincount(edges[:, :2].reshape(-1), minlength=n + 1))
    rs = np.random.RandomState(273)
    for k in (1, 2, n // 4, n):
        parent = np.concatenate([[0], rs.randint(1, k + 1, n)]).astype(np.int32)
        m = g.merge(parent)
        assert m.n_segments == int(parent.max()) and np.array_equal(m.table(), A.merge_graph_ref(edges, parent))
    parent[3] = 0                                                # a segment mapped to no region loses its edges
    assert np.array_equal(g.merge(parent).table(), A.merge_graph_ref(edges, parent))
    with pytest.raises(ValueError):
        g.merge(parent[:-1])
    with pytest.raises(ValueError):
        g.merge(np.ones(n + 1, np.int32))                        # parent[0] != 0


def test_region_graph_save_load(tmp_path):
    from rsseg.regions import RegionGraph
    seg, n, planes, mask = small_scene()
    g = RegionGraph.from_table(A.adjacency_ref(seg, planes, None, n), n)
    path = str(tmp_path / "graph.npz")
    g.save(path)
    assert os.path.exists(path) and RegionGraph.load(path) == g
    empty = RegionGraph.from_table(np.zeros((0, 5), np.int64), 4)
    assert empty.contrast.shape == (0, 2) and empty.border().shape == (5,) and empty.merge(np.arange(5)).pairs.shape == (0, 2)


def test_neighbour_features_against_the_restatement():
    from rsseg.regions import RegionGraph, neighbour_features
    seg, n, planes, mask = small_scene(True)
    edges = A.adjacency_ref(seg, planes, mask, n)
    table = O.object_table_ref(seg, planes, mask, n)
    got = neighbour_features(RegionGraph.from_table(edges, n), table, [True] * 3)
    want = A.neighbour_features_ref(edges, table, [True] * 3)
    assert got.shape == (n + 1, 8) and np.array_equal(got, want)
    assert (got[0] == 0).all() and got[1:, 0].max() >= 3


def adjacent(edges_now, a, b):
    return (min(a, b), max(a, b)) in edges_now


def replay(seg, planes, mask, n, history):
    """walk a history and assert that every merge joins two regions adjacent at that time; returns the final root of every segment"""
    edges = {(int(r[0]), int(r[1])) for r in A.adjacency_ref(seg, planes, mask, n)}
    root = np.arange(n + 1)
    for rnd, a, b, cost, area in history:
        assert a < b and adjacent(edges, a, b), (rnd, a, b)
        root[root == b] = a
        edges = {(min(root[u], root[v]), max(root[u], root[v])) for u, v in edges if root[u] != root[v]}
        assert area == int(np.isin(O.effective_labels(seg, mask), np.flatnonzero(root == a)).sum())
    return root


@pytest.mark.parametrize("criterion", ["ward", "boundary"])
def test_restated_merging_keeps_its_promises(criterion):
    seg, n, planes, mask = small_scene(True)
    t = {"ward": 4000.0, "boundary": 60.0}[criterion]
    res = A.merge_regions_ref(seg, planes, threshold=t, criterion=criterion, mask=mask, n_segments=n)
    assert 1 < res["n_regions"] < n and len(res["history"]) == n - res["n_regions"]
    root = replay(seg, planes, mask, n, res["history"])
    assert all(c <= t for _, _, _, c, _ in res["history"])
    rounds = [h[0] for h in res["history"]]
    assert rounds == sorted(rounds) and rounds[0] == 1
    # the regions are numbered in the order of their smallest segment, and the map is the painted parent, 0 where masked
    roots = np.unique(root[1:])
    assert np.array_equal(res["parent"][1:], np.searchsorted(roots, root[1:]) + 1)
    assert np.array_equal(res["labels"], res["parent"][O.effective_labels(seg, mask)])
    assert ((res["labels"] == 0) == (O.effective_labels(seg, mask) == 0)).all()


def test_restated_scales_are_nested():
    seg, n, planes, mask = small_scene(True)
    res = A.merge_regions_ref(seg, planes, scales=[500.0, 4000.0, 30000.0], mask=mask, n_segments=n)
    maps = res["scale_labels"]
    counts = [int(m.max()) for m in maps]
    assert counts[0] > counts[1] > counts[2] >= 1 and np.array_equal(maps[-1], res["labels"])
    for fine, coarse in zip(maps, maps[1:]):
        pairs = np.unique(np.stack([fine.reshape(-1), coarse.reshape(-1)], axis=1), axis=0)
        assert len(pairs) == len(np.unique(fine))                # every fine region lies in exactly one coarse region
    one = A.merge_regions_ref(seg, planes, threshold=500.0, mask=mask, n_segments=n)
    assert np.array_equal(one["labels"], maps[0])


@pytest.mark.parametrize("k", [1, 7, 30])
def test_restated_region_count_is_hit_exactly(k):
    seg, n, planes, mask = small_scene()
    res = A.merge_regions_ref(seg, planes, n_regions=k, n_segments=n)
    assert res["n_regions"] == k and len(np.unique(res["labels"])) == k and len(res["history"]) == n - k
    replay(seg, planes, None, n, res["history"])


def test_restated_min_area_leaves_no_small_region_with_a_neighbour():
    seg, n, planes, mask = small_scene(True)
    before = np.bincount(O.effective_labels(seg, mask).reshape(-1))[1:]
    assert (before < 80).any()
    res = A.merge_regions_ref(seg, planes, threshold=500.0, min_area=80, mask=mask, n_segments=n)
    area = np.bincount(res["labels"].reshape(-1), minlength=res["n_regions"] + 1)
    small = {r for r in range(1, res["n_regions"] + 1) if area[r] < 80}
    ends = {int(v) for row in A.adjacency_ref(res["labels"], (), None, res["n_regions"]) for v in row[:2]}
    assert not (small & ends)
    replay(seg, planes, mask, n, res["history"])


MERGE_CASES = [dict(threshold=4000.0), dict(threshold=60.0, criterion="boundary"), dict(scales=[500.0, 4000.0, 30000.0], min_area=30),
               dict(n_regions=7), dict(n_regions=5, criterion="boundary", weights=[1.0, 0.5, 2.0]), dict(threshold=500.0, min_area=80),
               dict(min_area=100, criterion="boundary"), dict(threshold=1e9, max_rounds=2)]


@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
@pytest.mark.parametrize("masked", [False, True])
def test_merge_tables_equals_the_restatement(case, masked):
    """the vectorised host half of merge_regions on the restated tables: parent and history bit for bit"""
    from rsseg import regions as RG
    seg, n, planes, mask = small_scene(masked)
    kw = dict(MERGE_CASES[case])
    want = A.merge_regions_ref(seg, planes, mask=mask, n_segments=n, **kw)
    table = O.object_table_ref(seg, planes, mask, n)
    graph = RG.RegionGraph.from_table(A.adjacency_ref(seg, planes, mask, n), n)
    scales, w, min_area, max_rounds = RG._check_merge_args(kw.get("threshold"), kw.get("scales"), kw.get("criterion", "ward"), kw.get("weights"),
                                                           kw.get("min_area", 0), kw.get("n_regions"), kw.get("max_rounds", 64), 3)
    parents, history = RG.merge_tables(table[:, 0], table[:, O.GEO::4], graph, kw.get("threshold"), scales, kw.get("criterion", "ward"), w, min_area,
                                       kw.get("n_regions"), max_rounds)
    assert np.array_equal(parents[-1], want["parent"]) and parents[-1].dtype == np.int32
    if "scales" in kw:
        assert len(parents) == 3 and all(np.array_equal(p, q) for p, q in zip(parents, want["scale_parent"]))
    assert [tuple(h) for h in history.tolist()] == want["history"] and len(history) > 0
    assert np.array_equal(graph.merge(parents[-1]).table(), A.adjacency_ref(want["labels"], planes, mask, want["n_regions"]))


def test_merge_regions_refuses_bad_arguments_before_any_device_work():
    from rsseg import regions as RG
    for kw in (dict(criterion="median", threshold=1.0), dict(scales=[1.0], threshold=1.0), dict(scales=[2.0, 1.0]), dict(),
               dict(threshold=1.0, weights=[1.0]), dict(n_regions=0), dict(threshold=1.0, min_area=-1)):
        with pytest.raises(ValueError):
            RG._check_merge_args(kw.get("threshold"), kw.get("scales"), kw.get("criterion", "ward"), kw.get("weights"), kw.get("min_area", 0),
                                 kw.get("n_regions"), 64, 2)
    with pytest.raises(ValueError, match="at most 16"):
        RG.adjacency(np.ones((4, 4), np.int32), [np.zeros((4, 4), np.uint8)] * 17)


def test_command_line_argument_checks(tmp_path, capsys):
    from rsseg import regions as RG
    out = str(tmp_path / "run")
    for argv in ([out], [out, "--threshold", "1", "--n-regions", "3"], [out, "--threshold", "1", "--scales", "1,2"],
                 [out, "--threshold", "1", "--criterion", "median"], [out, "--threshold", "1", "--class-map", "x.npy"]):
        with pytest.raises(SystemExit) as e:
            RG.main(argv)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                         # nothing of an earlier run is there
        RG.main([out, "--threshold", "1"])
    assert e.value.code == 2 and "segments.npy" in capsys.readouterr().err
    assert not os.path.exists(out)                               # and nothing was made
    a = RG.build_parser().parse_args([out, "--scales", "1,2.5", "--min-area", "9"])
    assert a.scales == [1.0, 2.5] and a.min_area == 9 and a.threshold is None and a.n_regions is None and a.criterion == "ward"
