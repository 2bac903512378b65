"""
The region adjacency graph of a segment map and bottom-up region merging (K27, csrc/k27_adjacency.hip).  This goes beyond the
reference, which has no segmentation step: adjacency() takes, in one pass over the raster on the GPU, every pair of segments
that touch, the length of their border and the summed step of every 8-bit plane across it; neighbour_features() turns that
into per-segment columns for rsseg.objects.object_features; merge_regions() merges superpixels (rsseg.segment.slic) until
they are as heterogeneous as the caller allows, at one scale or at several nested ones.

The graph is rsseg_segment_adjacency's table (include/rsseg.h); it and the merging are restated in tests/adjacency_ref.py, to
which both are equal bit for bit.  Under a merge the counts, the plane sums, the border lengths and the contrasts all add, so
the raster is read twice (K25 for the sums, K27 for the graph) and not again until the merged map is painted.

    python -m rsseg.regions OUTDIR [--threshold T | --scales T1,T2,... | --n-regions N] [--criterion ward|boundary]
                                   [--min-area A] [--class-map PATH --method NAME]
merges the superpixels a `python -m rsseg.stages ... --classify ... --segment STEP` run left under OUTDIR (run_region_merge_stage).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import segment as SG
from .runtime import Context

CRITERIA = ("ward", "boundary")
NEIGHBOUR_COLUMNS = ("n_neighbours", "shared_border")


class RegionGraph:
    """pairs int64 [E, 2] (a < b, ascending by (a, b)), length int64 [E], contrast int64 [E, P], n_segments."""
    __slots__ = ("pairs", "length", "contrast", "n_segments")

    def __init__(self, pairs, length, contrast, n_segments: int):
        self.pairs = np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)
        self.length = np.ascontiguousarray(length, np.int64).reshape(-1)
        contrast = np.ascontiguousarray(contrast, np.int64)
        self.contrast = contrast.reshape(self.pairs.shape[0], contrast.shape[-1] if contrast.ndim == 2 else 0 if contrast.size == 0 else -1)
        self.n_segments = int(n_segments)
        if self.length.shape[0] != self.pairs.shape[0]:
            raise ValueError(f"RegionGraph: {self.pairs.shape[0]} pairs and {self.length.shape[0]} lengths")

    @classmethod
    def from_table(cls, table, n_segments: int) -> "RegionGraph":
        """from the int64 [E, 3 + P] rows of rsseg_segment_adjacency, sorted by (a, b)"""
        t = np.asarray(table, np.int64)
        return cls(t[:, 0:2], t[:, 2], t[:, 3:], n_segments)

    def table(self) -> np.ndarray:
        return np.concatenate([self.pairs, self.length[:, None], self.contrast], axis=1)

    def __eq__(self, other) -> bool:
        return (isinstance(other, RegionGraph) and self.n_segments == other.n_segments and np.array_equal(self.pairs, other.pairs)
                and np.array_equal(self.length, other.length) and np.array_equal(self.contrast, other.contrast))

    __hash__ = None

    def merge(self, parent) -> "RegionGraph":
        """The graph of the regions that `parent` (integers [n_segments + 1], parent[0] == 0) maps the segments to: lengths and
        contrasts of coinciding pairs add, pairs inside a region (and pairs with region 0) vanish."""
        parent = np.asarray(parent)
        if parent.ndim != 1 or parent.shape[0] != self.n_segments + 1 or not np.issubdtype(parent.dtype, np.integer):
            raise ValueError(f"RegionGraph.merge: parent must be {self.n_segments + 1} integers, got {parent.dtype} {parent.shape}")
        if parent[0] != 0 or parent.min() < 0:
            raise ValueError("RegionGraph.merge: parent[0] must be 0 and no entry negative")
        parent = parent.astype(np.int64)
        a, b = parent[self.pairs[:, 0]], parent[self.pairs[:, 1]]
        pairs, vals = _aggregate(a, b, np.concatenate([self.length[:, None], self.contrast], axis=1))
        return RegionGraph(pairs, vals[:, 0], vals[:, 1:], int(parent.max()))

    def degree(self) -> np.ndarray:
        """int64 [n_segments + 1]: the number of neighbours"""
        return np.bincount(self.pairs.reshape(-1), minlength=self.n_segments + 1).astype(np.int64)

    def border(self) -> np.ndarray:
        """int64 [n_segments + 1]: the summed length of the borders with the neighbours"""
        out = np.zeros(self.n_segments + 1, np.int64)
        np.add.at(out, self.pairs[:, 0], self.length)
        np.add.at(out, self.pairs[:, 1], self.length)
        return out

    def save(self, path: str) -> None:
        with open(path, "wb") as f:   # the name as given: np.savez would append .npz to a path
            np.savez(f, pairs=self.pairs, length=self.length, contrast=self.contrast, n_segments=np.int64(self.n_segments))

    @classmethod
    def load(cls, path: str) -> "RegionGraph":
        with np.load(path) as z:
            return cls(z["pairs"], z["length"], z["contrast"], int(z["n_segments"]))


def _aggregate(a, b, vals):
    """rows (a, b, vals) -> one row per unordered pair a != b, both > 0, ascending, with the vals added (lexsort + reduceat)"""
    keep = (a != b) & (a > 0) & (b > 0)
    lo, hi, vals = np.minimum(a, b)[keep], np.maximum(a, b)[keep], vals[keep]
    if lo.size == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, vals.shape[1]), vals.dtype)
    order = np.lexsort((hi, lo))
    lo, hi, vals = lo[order], hi[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])]))
    return np.stack([lo[first], hi[first]], axis=1), np.add.reduceat(vals, first, axis=0)


def _device_inputs(segments, planes, mask, n_segments, ranges, ctx, what):
    """(ctx, flat int32 segment plane, H, W, n_segments, flat uint8 planes, flat uint8 mask or None)"""
    seg = SG.check_segments(segments, what)
    pls = SG._plane_list(planes, "planes", what) if (SG._is_tensor(planes) or isinstance(planes, np.ndarray) or len(planes)) else []
    if len(pls) > SG.MAX_PLANES:
        raise ValueError(f"{what}: planes holds {len(pls)} planes, at most {SG.MAX_PLANES} cross a border at once")
    shape = SG._check_shapes(pls, "planes", what, shape=seg.shape)
    if ranges is not None and len(ranges) != len(pls):
        raise ValueError(f"{what}: ranges has {len(ranges)} entries for {len(pls)} planes")
    mask = SG._check_mask(mask, shape, what)
    ctx = SG._context(ctx, what)
    d_seg, h, w, ns = SG._upload_segments(ctx, seg, n_segments)
    return ctx, d_seg, h, w, ns, SG.quantise_planes(ctx, pls, ranges), SG._dev_mask(ctx, mask)


def adjacency(segments, planes=(), mask=None, n_segments: Optional[int] = None, ranges=None, ctx: Optional[Context] = None) -> RegionGraph:
    """The region adjacency graph of a segment map under 4-connectivity: every pair of segments a < b with a pixel of one beside
    or above a pixel of the other (both counted: label >= 1, mask byte non-zero), the number of such crossings and, per plane,
    the sum of |v(pixel) - v(neighbour)| over them.  planes: 0 ... 16; uint8 planes as they are, float planes as slic() quantises
    them (segment.quantise_planes: `ranges`[p] = (lo, hi), or the plane's finite min / max)."""
    ctx, d_seg, h, w, ns, q, dmask = _device_inputs(segments, planes, mask, n_segments, ranges, ctx, "adjacency")
    return RegionGraph.from_table(ctx.segment_adjacency(d_seg, h, w, ns, q, mask=dmask).cpu().numpy(), ns)


def neighbour_features(graph: RegionGraph, table: np.ndarray, plane_is_u8: Sequence[bool]) -> np.ndarray:
    """float64 [(n + 1), 2 + 2 P] from a graph and the object table (rsseg.objects.object_table) of the same segments and planes:
    the number of neighbours, the shared border, per plane the mean boundary contrast (sum contrast / sum length over the
    segment's edges, in the units of the graph's 8-bit planes) and the border-weighted mean absolute difference between the
    segment's plane mean and its neighbours' (added in ascending neighbour id).  A segment without a neighbour is all zero."""
    from .objects import GEO_COLUMNS, Q_SCALE_BITS
    table = np.asarray(table)
    n, P = graph.n_segments, len(plane_is_u8)
    if table.shape != (n + 1, GEO_COLUMNS + 4 * P) or graph.contrast.shape[1] != P:
        raise ValueError(f"neighbour_features: {P} planes and {n} segments need a table of {(n + 1, GEO_COLUMNS + 4 * P)} and {P} contrasts, "
                         f"got {table.shape} and {graph.contrast.shape[1]}")
    out = np.zeros((n + 1, 2 + 2 * P), np.float64)
    border = graph.border()
    has = border > 0
    out[:, 0], out[:, 1] = graph.degree(), border
    node = np.concatenate([graph.pairs[:, 0], graph.pairs[:, 1]])
    other = np.concatenate([graph.pairs[:, 1], graph.pairs[:, 0]])
    eid = np.concatenate([np.arange(len(graph.length))] * 2)
    order = np.lexsort((other, node))
    node, other, eid = node[order], other[order], eid[order]
    fb = border.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cnt = table[:, 0].astype(np.float64)
        for p in range(P):
            csum = np.zeros(n + 1, np.int64)
            np.add.at(csum, node, graph.contrast[eid, p])
            out[has, 2 + p] = csum[has].astype(np.float64) / fb[has]
            scale = 1.0 if plane_is_u8[p] else float(2 ** Q_SCALE_BITS)
            mean = table[:, GEO_COLUMNS + 4 * p].astype(np.float64) / scale / cnt
            acc = np.zeros(n + 1, np.float64)
            np.add.at(acc, node, graph.length[eid].astype(np.float64) * np.abs(mean[node] - mean[other]))   # one by one, in order
            out[has, 2 + P + p] = acc[has] / fb[has]
    return out


def neighbour_columns(names: Sequence[str]) -> List[str]:
    return list(NEIGHBOUR_COLUMNS) + [f"{s}_boundary_contrast" for s in names] + [f"{s}_neighbour_diff" for s in names]


# ---- region merging ----------------------------------------------------------------------------------------------------------
class RegionMerge(NamedTuple):
    labels: np.ndarray               # int32 (H, W): 0 = masked, else 1 ... n_regions
    n_regions: int
    parent: np.ndarray               # int32 [n_segments + 1]: the region of every segment, 0 for none and for empty segments
    history: np.ndarray              # one record per merge: round, a, b, cost, area (after)
    graph: RegionGraph               # of the regions
    scale_labels: Optional[list] = None    # with scales: one map and one parent per scale (the last are labels / parent)
    scale_parent: Optional[list] = None


HISTORY_DTYPE = np.dtype([("round", np.int64), ("a", np.int64), ("b", np.int64), ("cost", np.float64), ("area", np.int64)])


class _Merger:
    """The state of a merging run: per region the count and the plane sums, the edges sorted by (a, b) with their lengths and
    contrasts, and the region every segment belongs to so far.  Ids are the segments' own: a merged region keeps the smaller."""

    def __init__(self, count, sums, graph: RegionGraph, criterion: str, weights):
        self.count = count.astype(np.int64).copy()          # [n + 1]
        self.sums = sums.astype(np.int64).copy()            # [n + 1, P]
        self.pairs = graph.pairs.copy()
        self.vals = np.concatenate([graph.length[:, None], graph.contrast], axis=1)
        self.root = np.arange(self.count.shape[0], dtype=np.int64)
        self.criterion, self.w = criterion, weights
        self.history: list = []
        self.round = 0

    def n_regions(self) -> int:
        alive = self.count > 0
        alive[0] = False
        return int(alive.sum())

    def costs(self, a, b, vals) -> np.ndarray:
        """float64 per edge; the planes are added one after the other in ascending p (the restatement's order)"""
        P = self.sums.shape[1]
        if self.criterion == "ward":
            na, nb = self.count[a].astype(np.float64), self.count[b].astype(np.float64)
            f = (na * nb) / (na + nb)
            d = np.zeros(a.shape[0], np.float64)
            for p in range(P):
                diff = self.sums[a, p].astype(np.float64) / na - self.sums[b, p].astype(np.float64) / nb
                d = d + self.w[p] * (diff * diff)
            return f * d
        num = np.zeros(a.shape[0], np.float64)
        for p in range(P):
            num = num + self.w[p] * vals[:, 1 + p].astype(np.float64)
        return num / vals[:, 0].astype(np.float64)

    def mutual(self, sel: np.ndarray):
        """(edge indices, costs) of the edges among `sel` (indices into the sorted edge list) that both their ends pick as their
        best under the total order (cost, a, b), in that order.  The edge list is sorted by (a, b), so an index stands for it."""
        a, b = self.pairs[sel, 0], self.pairs[sel, 1]
        cost = self.costs(a, b, self.vals[sel])
        order = np.argsort(cost, kind="stable")               # `sel` ascends, so ties keep the order of (a, b)
        rank = np.empty(sel.shape[0], np.int64)
        rank[order] = np.arange(sel.shape[0])                 # an edge's place in the total order
        best = np.full(self.count.shape[0], sel.shape[0], np.int64)
        np.minimum.at(best, a, rank)
        np.minimum.at(best, b, rank)
        m = np.flatnonzero((best[a] == rank) & (best[b] == rank))
        m = m[np.argsort(rank[m])]
        return sel[m], cost[m]

    def apply(self, edges: np.ndarray, cost: np.ndarray) -> None:
        """merge along these edges (a matching: no region is in two of them)"""
        self.round += 1
        a, b = self.pairs[edges, 0], self.pairs[edges, 1]
        self.count[a] += self.count[b]
        self.sums[a] += self.sums[b]
        self.count[b] = 0
        self.sums[b] = 0
        to = np.arange(self.count.shape[0], dtype=np.int64)
        to[b] = a
        self.root = to[self.root]
        self.history.append(np.rec.fromarrays([np.full(a.shape[0], self.round, np.int64), a, b, cost, self.count[a]], dtype=HISTORY_DTYPE))
        self.pairs, self.vals = _aggregate(to[self.pairs[:, 0]], to[self.pairs[:, 1]], self.vals)

    def threshold_phase(self, threshold: float, n_regions: Optional[int], max_rounds: int) -> None:
        for _ in range(max_rounds):
            room = self.n_regions() - n_regions if n_regions is not None else self.pairs.shape[0]
            if room <= 0 or self.pairs.shape[0] == 0:
                break
            edges, cost = self.mutual(np.arange(self.pairs.shape[0]))
            ok = cost <= threshold
            edges, cost = edges[ok][:room], cost[ok][:room]
            if edges.size == 0:
                break
            self.apply(edges, cost)

    def min_area_phase(self, min_area: int) -> None:
        while True:
            small = self.count < min_area
            sel = np.flatnonzero(small[self.pairs[:, 0]] | small[self.pairs[:, 1]])
            if sel.size == 0:
                break
            self.apply(*self.mutual(sel))

    def parent(self) -> np.ndarray:
        """int32 [n + 1]: regions numbered 1 ... in ascending order of their smallest member, which is the id they kept"""
        alive = self.count > 0
        alive[0] = False
        rank = np.zeros(self.count.shape[0], np.int64)
        rank[alive] = np.arange(1, int(alive.sum()) + 1)
        return rank[self.root].astype(np.int32)


def merge_tables(count, sums, graph: RegionGraph, threshold, scales, criterion: str, weights, min_area: int, n_regions, max_rounds: int):
    """merge_regions' host half (no device needed): the per-segment counts [n + 1] and plane sums [n + 1, P] and the graph ->
    (one parent table per scale, or one; the history).  The arguments are merge_regions', already checked."""
    mg = _Merger(np.asarray(count), np.asarray(sums).reshape(len(count), -1), graph, criterion, np.asarray(weights, np.float64))
    parents = []
    if scales is not None:
        for t in scales:
            mg.threshold_phase(float(t), None, max_rounds)
            if min_area > 0:
                mg.min_area_phase(min_area)
            parents.append(mg.parent())
    else:
        if threshold is not None or n_regions is not None:
            mg.threshold_phase(math.inf if threshold is None else float(threshold), n_regions, max_rounds)
        if min_area > 0:
            mg.min_area_phase(min_area)
        parents.append(mg.parent())
    return parents, (np.concatenate(mg.history) if mg.history else np.zeros(0, HISTORY_DTYPE))


def _check_merge_args(threshold, scales, criterion, weights, min_area, n_regions, max_rounds, P):
    if criterion not in CRITERIA:
        raise ValueError(f"merge_regions: criterion {criterion!r}, must be one of {CRITERIA}")
    if scales is not None and (threshold is not None or n_regions is not None):
        raise ValueError("merge_regions: scales goes with neither threshold nor n_regions")
    if scales is None and threshold is None and n_regions is None and not min_area:
        raise ValueError("merge_regions: give threshold, scales, n_regions or min_area")
    if threshold is not None and not (isinstance(threshold, (int, float, np.floating, np.integer)) and not math.isnan(float(threshold))):
        raise ValueError(f"merge_regions: threshold={threshold!r} is not a number")
    if scales is not None:
        scales = [float(t) for t in scales]
        if not scales or any(math.isnan(t) for t in scales) or any(t1 < t0 for t0, t1 in zip(scales, scales[1:])):
            raise ValueError(f"merge_regions: scales={scales!r} must be ascending thresholds")
    w = np.ones(P, np.float64) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w.shape[0] != P or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"merge_regions: weights must be {P} finite non-negative numbers")
    min_area = SG._check_count(min_area, "min_area", "merge_regions")
    max_rounds = SG._check_count(max_rounds, "max_rounds", "merge_regions")
    if n_regions is not None and SG._check_count(n_regions, "n_regions", "merge_regions") < 1:
        raise ValueError("merge_regions: n_regions must be at least 1")
    return scales, w, min_area, max_rounds


def merge_regions(segments, planes, threshold: Optional[float] = None, scales: Optional[Sequence[float]] = None, criterion: str = "ward",
                  weights=None, min_area: int = 0, n_regions: Optional[int] = None, max_rounds: int = 64, mask=None, ranges=None,
                  ctx: Optional[Context] = None) -> RegionMerge:
    """Bottom-up merging of the segments of a map (deterministic; restated in tests/adjacency_ref.py, merge_regions_ref).
    A region's state is its pixel count and, per 8-bit plane, the sum of its pixels (one object_table call, K25); the graph is
    one adjacency() call (K27).  The cost of an edge (a, b), float64:
      'ward'      n_a n_b / (n_a + n_b) * sum_p w_p (mu_a,p - mu_b,p)^2, mu = sum / n, the planes added in ascending p;
      'boundary'  sum_p w_p contrast_p / length: the mean weighted step across the shared border.
    A round: every region picks its best edge under the total order (cost, smaller id, larger id); an edge picked from both
    ends whose cost is <= threshold merges, the region keeping the smaller id; the graph is aggregated again.  Rounds repeat
    until one merges nothing, at most max_rounds times.  The globally cheapest edge is always picked from both ends, so every
    round merges something while an admissible edge is left.
    n_regions: stop at exactly that many regions (the last round applies its merges in the total order until the count is
    reached); with no threshold every edge is admissible.
    min_area: afterwards regions of fewer pixels merge along their cheapest edge whatever the threshold (the same round rule
    over the edges with a small end), until none is left or none has a neighbour.
    scales: ascending thresholds; merging continues from one to the next (min_area after each), so the maps are nested.
    Returns RegionMerge(labels, n_regions, parent, history, graph[, scale_labels, scale_parent]): regions numbered 1 ... in
    ascending order of their smallest segment; labels int32 (H, W), 0 where the pixel is masked or belongs to no segment."""
    import torch
    from . import objects as OB
    ctx, d_seg, h, w, ns, q, dmask = _device_inputs(segments, planes, mask, None, ranges, ctx, "merge_regions")
    P = len(q)
    scales, wts, min_area, max_rounds = _check_merge_args(threshold, scales, criterion, weights, min_area, n_regions, max_rounds, P)
    seg2 = d_seg.reshape(h, w)
    mask2 = None if dmask is None else dmask.reshape(h, w)
    table = OB.object_table(seg2, [p.reshape(h, w) for p in q], mask=mask2, n_segments=ns, ctx=ctx)
    graph = RegionGraph.from_table(ctx.segment_adjacency(d_seg, h, w, ns, q, mask=dmask).cpu().numpy(), ns)
    parents, history = merge_tables(table[:, 0], table[:, OB.GEO_COLUMNS::4], graph, threshold, scales, criterion, wts, min_area, n_regions, max_rounds)

    def paint(parent):
        out = ctx.segment_paint(d_seg, ns, ctx.to_device(parent))
        if dmask is not None:
            out = torch.where(dmask != 0, out, torch.zeros_like(out))
        return out.cpu().numpy().reshape(h, w)

    maps = [paint(p) for p in parents]
    return RegionMerge(maps[-1], int(parents[-1].max()), parents[-1], history, graph.merge(parents[-1]),
                       maps if scales is not None else None, parents if scales is not None else None)


# ---- command line ------------------------------------------------------------------------------------------------------------
def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rsseg.regions",
                                 description="Merge the superpixels of an earlier `python -m rsseg.stages ... --classify ... --segment STEP` run "
                                             "into regions (segmentation_results/regions.npy, region_graph.npz, regions_stats.json).")
    ap.add_argument("outdir", metavar="OUTDIR", help="the output directory of that run")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--threshold", type=float, help="merge while the cheapest edge costs at most this")
    g.add_argument("--scales", type=lambda s: [float(t) for t in s.split(",")], help="ascending thresholds T1,T2,...: one nested map per scale")
    g.add_argument("--n-regions", type=int, help="merge until exactly this many regions are left")
    ap.add_argument("--criterion", choices=CRITERIA, default="ward")
    ap.add_argument("--min-area", type=int, default=0, help="afterwards merge regions of fewer pixels into their cheapest neighbour")
    ap.add_argument("--class-map", help="a per-pixel class map (.npy) to vote per region")
    ap.add_argument("--method", help="with --class-map: the name in classification_<method>_regions.npy")
    return ap


def main(argv=None) -> int:
    import os
    ap = build_parser()
    a = ap.parse_args(argv)
    if (a.class_map is None) != (a.method is None):
        ap.error("--class-map and --method go together")
    sdir = os.path.join(a.outdir, "segmentation_results")
    spath = os.path.join(sdir, "segments.npy")
    fpath = os.path.join(a.outdir, "feature_outputs", "all_features_and_metadata.pkl")
    for path, what in ((spath, "run the stages command with --segment first"), (fpath, "the feature file of the earlier run")):
        if not os.path.exists(path):
            ap.error(f"{path} not found: {what}")
    if a.class_map is not None and not os.path.exists(a.class_map):
        ap.error(f"{a.class_map} not found")
    from .stages import run_region_merge_stage
    vpath = os.path.join(a.outdir, "feature_outputs", "valid_mask.npy")
    valid = np.load(vpath) if os.path.exists(vpath) else None
    _, stats, _ = run_region_merge_stage(fpath, np.load(spath), sdir, threshold=a.threshold, scales=a.scales, criterion=a.criterion,
                                         min_area=a.min_area, n_regions=a.n_regions, class_map=None if a.class_map is None else np.load(a.class_map),
                                         method=a.method, valid_mask=valid)
    print(f"regions: {stats['segments_in']} segments -> {stats['regions_out']} regions in {stats['rounds']} rounds ({a.criterion})")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
