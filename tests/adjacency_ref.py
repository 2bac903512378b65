"""K27 restated (include/rsseg.h: rsseg_segment_adjacency; rsseg/regions.py: RegionGraph.merge, neighbour_features,
merge_regions): what the kernel's table and the region merging are equal to, bit for bit.  The graph comes from shifted arrays
and np.unique; the merging is written with plain dictionaries and loops over regions, shares no code with rsseg/regions.py and
states the float64 operation order of the costs with np.float64 scalars."""
import numpy as np

from objects_ref import effective_labels

INF = float("inf")


def adjacency_ref(seg, planes=(), mask=None, n_segments=None):
    """int64 [E, 3 + P] sorted by (a, b): a < b, the number of crossings, per uint8 plane the summed |step| across them"""
    eff = effective_labels(seg, mask)
    planes = [np.asarray(p).astype(np.int64) for p in planes]
    a_all, b_all, d_all = [], [], []
    for dy, dx in ((0, 1), (1, 0)):   # a pixel and its right neighbour, a pixel and its lower neighbour
        H, W = eff.shape
        p0, p1 = eff[:H - dy, :W - dx], eff[dy:, dx:]
        m = (p0 > 0) & (p1 > 0) & (p0 != p1)
        a_all.append(np.minimum(p0, p1)[m])
        b_all.append(np.maximum(p0, p1)[m])
        d_all.append(np.stack([np.abs(q[:H - dy, :W - dx] - q[dy:, dx:])[m] for q in planes], axis=1) if planes
                     else np.zeros((int(m.sum()), 0), np.int64))
    a, b, d = np.concatenate(a_all), np.concatenate(b_all), np.concatenate(d_all)
    packed, inv = np.unique((a << 32) | b, return_inverse=True)
    out = np.zeros((len(packed), 3 + len(planes)), np.int64)
    out[:, 0], out[:, 1] = packed >> 32, packed & 0xffffffff
    np.add.at(out[:, 2], inv, 1)
    for p in range(len(planes)):
        np.add.at(out[:, 3 + p], inv, d[:, p])
    return out


def image_border_sides(seg, mask=None, n_segments=None):
    """int64 [n + 1]: per segment the pixel sides that lie on the image border or face a pixel of effective label 0"""
    eff = effective_labels(seg, mask)
    n = int(np.asarray(seg).max()) if n_segments is None else int(n_segments)
    H, W = eff.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = eff
    out = np.zeros(n + 1, np.int64)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        m = (eff > 0) & (pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] == 0)
        np.add.at(out, eff[m], 1)
    return out


def merge_graph_ref(edges, parent):
    """the table of the regions `parent` maps the segments to: a dictionary over the pairs"""
    P = edges.shape[1] - 3
    acc = {}
    for row in edges:
        a, b = int(parent[row[0]]), int(parent[row[1]])
        if a == b or a == 0 or b == 0:
            continue
        k = (min(a, b), max(a, b))
        if k not in acc:
            acc[k] = [0] * (1 + P)
        for c in range(1 + P):
            acc[k][c] += int(row[2 + c])
    out = np.zeros((len(acc), 3 + P), np.int64)
    for i, k in enumerate(sorted(acc)):
        out[i, 0], out[i, 1] = k
        out[i, 2:] = acc[k]
    return out


def border_ref(edges, n):
    out = np.zeros(n + 1, np.int64)
    for row in edges:
        out[row[0]] += row[2]
        out[row[1]] += row[2]
    return out


def neighbour_features_ref(edges, table, plane_is_u8):
    """float64 [(n + 1), 2 + 2 P]: the number of neighbours, the shared border, per plane the mean boundary contrast
    (sum contrast / sum length) and the border-weighted mean absolute difference of the plane means; a row without a neighbour
    is all zero"""
    n = table.shape[0] - 1
    P = len(plane_is_u8)
    assert edges.shape[1] == 3 + P
    out = np.zeros((n + 1, 2 + 2 * P), np.float64)
    means = np.full((n + 1, P), np.nan, np.float64)
    for s in range(n + 1):
        for p in range(P):
            if table[s, 0] > 0:
                scale = np.float64(1.0) if plane_is_u8[p] else np.float64(2.0 ** 40)
                means[s, p] = np.float64(table[s, 11 + 4 * p]) / scale / np.float64(table[s, 0])
    nb = {s: [] for s in range(n + 1)}
    for row in edges:
        nb[int(row[0])].append((int(row[1]), row))
        nb[int(row[1])].append((int(row[0]), row))
    for s in range(n + 1):
        if not nb[s]:
            continue
        out[s, 0] = len(nb[s])
        border = sum(int(r[2]) for _, r in nb[s])
        out[s, 1] = border
        for p in range(P):
            out[s, 2 + p] = np.float64(sum(int(r[3 + p]) for _, r in nb[s])) / np.float64(border)
            acc = np.float64(0.0)
            for o, r in sorted(nb[s], key=lambda t: t[0]):   # ascending neighbour id, added one by one
                acc = acc + np.float64(r[2]) * np.abs(means[s, p] - means[o, p])
            out[s, 2 + P + p] = acc / np.float64(border)
    return out


# ---- region merging ----------------------------------------------------------------------------------------------------------
def _cost(criterion, w, cnt, sums, a, b, edge):
    """float64, in this order of operations"""
    P = len(w)
    if criterion == "ward":
        na, nb = np.float64(cnt[a]), np.float64(cnt[b])
        f = (na * nb) / (na + nb)
        d = np.float64(0.0)
        for p in range(P):
            diff = np.float64(sums[a][p]) / na - np.float64(sums[b][p]) / nb
            d = d + np.float64(w[p]) * (diff * diff)
        return float(f * d)
    num = np.float64(0.0)
    for p in range(P):
        num = num + np.float64(w[p]) * np.float64(edge[1 + p])
    return float(num / np.float64(edge[0]))


class _State:
    def __init__(self, seg, planes, mask, n, criterion, weights):
        eff = effective_labels(seg, mask)
        self.n = n
        self.P = len(planes)
        self.criterion = criterion
        self.w = [1.0] * self.P if weights is None else [float(x) for x in weights]
        self.cnt = {}
        self.sums = {}
        for s in range(1, n + 1):
            m = eff == s
            c = int(m.sum())
            if c:
                self.cnt[s] = c
                self.sums[s] = [int(np.asarray(p)[m].astype(np.int64).sum()) for p in planes]
        self.edges = {}   # (a, b) with a < b -> [length, contrast ...]
        for row in adjacency_ref(seg, planes, mask, n):
            self.edges[(int(row[0]), int(row[1]))] = [int(v) for v in row[2:]]
        self.root = {s: s for s in self.cnt}
        self.history = []
        self.round = 0

    def costs(self, keys):
        return {k: _cost(self.criterion, self.w, self.cnt, self.sums, k[0], k[1], self.edges[k]) for k in keys}

    def mutual(self, keys):
        """the edges among `keys` that both their ends pick as their best under (cost, a, b), in that order"""
        cost = self.costs(keys)
        best = {}
        for k in keys:
            t = (cost[k], k[0], k[1])
            for r in k:
                if r not in best or t < best[r]:
                    best[r] = t
        return sorted(t for t in set(best.values()) if best[t[1]] == t and best[t[2]] == t)

    def apply(self, picks):
        self.round += 1
        for c, a, b in picks:
            self.cnt[a] += self.cnt.pop(b)
            sb = self.sums.pop(b)
            self.sums[a] = [x + y for x, y in zip(self.sums[a], sb)]
            self.history.append((self.round, a, b, c, self.cnt[a]))
            for s in self.root:
                if self.root[s] == b:
                    self.root[s] = a
            new = {}
            for (u, v), val in self.edges.items():
                u, v = (a if u == b else u), (a if v == b else v)
                if u == v:
                    continue
                k = (min(u, v), max(u, v))
                new[k] = [x + y for x, y in zip(new[k], val)] if k in new else list(val)
            self.edges = new

    def threshold_phase(self, threshold, n_regions, max_rounds):
        for _ in range(max_rounds):
            room = len(self.cnt) - n_regions if n_regions is not None else len(self.cnt)
            if room <= 0:
                break
            picks = [t for t in self.mutual(list(self.edges)) if t[0] <= threshold][:room]
            if not picks:
                break
            self.apply(picks)

    def min_area_phase(self, min_area):
        while True:
            keys = [k for k in self.edges if self.cnt[k[0]] < min_area or self.cnt[k[1]] < min_area]
            picks = self.mutual(keys)
            if not picks:
                break
            self.apply(picks)

    def snapshot(self, seg, mask):
        roots = sorted(set(self.root.values()))
        rank = {r: i + 1 for i, r in enumerate(roots)}
        parent = np.zeros(self.n + 1, np.int32)
        for s, r in self.root.items():
            parent[s] = rank[r]
        labels = parent[effective_labels(seg, mask)].astype(np.int32)
        return labels, parent, len(roots)


def merge_regions_ref(seg, planes, threshold=None, scales=None, criterion="ward", weights=None, min_area=0, n_regions=None, max_rounds=64,
                      mask=None, n_segments=None):
    """dict(labels, parent, n_regions, history[, scale_labels, scale_parent]) for uint8 planes"""
    seg = np.asarray(seg)
    n = int(seg.max()) if n_segments is None else int(n_segments)
    st = _State(seg, planes, mask, n, criterion, weights)
    out = {}
    if scales is not None:
        out["scale_labels"], out["scale_parent"] = [], []
        for t in scales:
            st.threshold_phase(float(t), None, max_rounds)
            if min_area > 0:
                st.min_area_phase(min_area)
            labels, parent, _ = st.snapshot(seg, mask)
            out["scale_labels"].append(labels)
            out["scale_parent"].append(parent)
    else:
        if threshold is not None or n_regions is not None:
            st.threshold_phase(INF if threshold is None else float(threshold), n_regions, max_rounds)
        if min_area > 0:
            st.min_area_phase(min_area)
    out["labels"], out["parent"], out["n_regions"] = st.snapshot(seg, mask)
    out["history"] = list(st.history)
    out["edges"] = dict(st.edges)
    return out
