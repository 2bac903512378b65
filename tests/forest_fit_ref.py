"""NumPy restatement of K16's tree builder (csrc/k16_forest_fit.hip): scikit-learn 1.7.2's depth-first Gini best-split
builder as the kernel formulates it.  Per drawn feature the node's samples are sorted by (float32 value, sample index), the
class counts left of every position come from a cumulative sum of integer weights, and the first maximum of the Gini proxy
wins.  Used by tests/test_forest_fit_host.py to check the formulation against scikit-learn itself on small cases.

`build_tree(..., variant=NAME)` switches in one deliberate mistake (VARIANTS): tests/test_forest_fit_cases_host.py uses them
to show that the case list of tests/forest_fit_cases.py tells each of them apart from scikit-learn.  The default path
(variant=None) is the builder as it was; every variant is an added line that overrides what the line before it formed."""
import numpy as np

# FEATURE_THRESHOLD as the released scikit-learn 1.7.2 build applies it: 0, although tree/_partitioner.pxd:13 declares 1e-7
# (test_feature_threshold_is_zero_in_the_installed_sklearn pins it)
FT = np.float32(0.0)
EPS = np.finfo(np.float64).eps

VARIANTS = {
    "ft": '"same value" means within 1e-7 (FEATURE_THRESHOLD as the source declares it)',
    "ftz": "denormals flushed to zero",
    "zeros": "-0.0 sorted before +0.0 and the step between them taken as a split candidate",
    "depth": "depth > max_depth instead of >=",
    "mslw": "min_samples_leaf applied to weights instead of sample counts",
    "lastmax": "the last maximum of the proxy wins instead of the first",
    "featge": "a later feature wins proxy ties (>=)",
    "mid32": "the threshold midpoint formed in float32",
    "missw": "missing_go_to_left from weights instead of counts",
}
_TINY = np.finfo(np.float32).tiny


def _rand(state):
    s = state[0] or 1
    s ^= (s << 13) & 0xFFFFFFFF
    s ^= s >> 17
    s ^= (s << 5) & 0xFFFFFFFF
    state[0] = s
    return s % (2147483647 + 1)


def build_tree(X, y, counts, C, seed, max_depth, mss, msl, max_features, variant=None):
    """X: (n, F) float32; y: int class indices; counts: int weights (the bootstrap counts, which sum to n: w_total below is
    weighted_n_samples, and K16 takes it as n and refuses a row with another sum); seed: the xorshift start; variant: None, or
    one of VARIANTS.  Returns the node arrays in K16's layout (as forest_fit.tree_nodes gives them)."""
    assert variant is None or variant in VARIANTS, variant
    X = np.asarray(X, np.float32)
    n_all, F = X.shape
    samples = np.flatnonzero(counts > 0)
    w_total = float(counts.sum())
    features = list(range(F))
    constants = list(range(F))
    state = [int(seed)]
    rec = {k: [] for k in ("left", "right", "feature", "threshold", "impurity", "n_node_samples",
                           "weighted_n_node_samples", "missing_go_to_left", "value")}
    stack = [(0, len(samples), 0, -1, 0, None, 0)]
    max_seen = 0
    while stack:
        start, end, depth, parent, is_left, impurity, n_const = stack.pop()
        ns = samples[start:end]
        n = end - start
        tot = np.bincount(y[ns], weights=counts[ns], minlength=C).astype(np.int64)
        W = int(tot.sum())
        if impurity is None:
            impurity = 1.0 - float((tot * tot).sum()) / (float(W) * float(W))
        leaf = depth >= max_depth or n < mss or n < 2 * msl or impurity <= EPS
        if variant == "depth":
            leaf = depth > max_depth or n < mss or n < 2 * msl or impurity <= EPS
        best = None   # (score, pos, gl, gr, wl, feature, order, lo, hi)
        if not leaf:
            f_i, nvis, nfound, ndrawn = F, 0, 0, 0
            nknown = ntotal = n_const
            while f_i > ntotal and (nvis < max_features or nvis <= nfound + ndrawn):
                nvis += 1
                fj = ndrawn + _rand(state) % (f_i - nfound - ndrawn)
                if fj < nknown:
                    features[ndrawn], features[fj] = features[fj], features[ndrawn]
                    ndrawn += 1
                    continue
                fj += nfound
                f = features[fj]
                order = ns[np.lexsort((ns, X[ns, f]))]
                v = X[order, f]
                if variant == "zeros":
                    order = ns[np.lexsort((ns, ~np.signbit(X[ns, f]), X[ns, f]))]
                    v = X[order, f]
                if variant == "ftz":
                    v = np.where(np.abs(v) < _TINY, np.float32(0), v)
                if variant == "ft" and float(v[-1]) <= float(v[0]) + 1e-7:
                    v = np.full_like(v, v[0])
                if float(v[-1]) <= float(v[0]) + float(FT):
                    features[fj], features[ntotal] = features[ntotal], features[fj]
                    nfound += 1
                    ntotal += 1
                    continue
                f_i -= 1
                features[f_i], features[fj] = features[fj], features[f_i]
                onehot = np.zeros((n, C), np.int64)
                onehot[np.arange(n), y[order]] = counts[order]
                L = np.cumsum(onehot, axis=0)[:-1]           # left counts for positions p = 1 .. n-1
                R = tot[None, :] - L
                pos = np.arange(1, n)
                cand = (v[1:].astype(np.float64) > v[:-1].astype(np.float64) + float(FT)) & (pos >= msl) & (n - pos >= msl)
                if variant == "ft":
                    cand &= v[1:].astype(np.float64) > v[:-1].astype(np.float64) + 1e-7
                if variant == "zeros":
                    cand |= (v[1:] == 0) & (v[:-1] == 0) & np.signbit(v[:-1]) & ~np.signbit(v[1:]) & (pos >= msl) & (n - pos >= msl)
                if variant == "mslw":
                    cand = (v[1:] > v[:-1]) & (L.sum(1) >= msl) & (R.sum(1) >= msl)
                if not cand.any():
                    continue
                wl = L.sum(1).astype(np.float64)
                wr = R.sum(1).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    gl = 1.0 - (L * L).sum(1).astype(np.float64) / (wl * wl)
                    gr = 1.0 - (R * R).sum(1).astype(np.float64) / (wr * wr)
                    score = -wr * gr - wl * gl
                score = np.where(cand, score, -np.inf)
                k = int(np.argmax(score))                    # first maximum
                if variant == "lastmax":
                    k = len(score) - 1 - int(np.argmax(score[::-1]))
                if variant == "featge" and best is not None and score[k] == best[0]:
                    best = None
                if best is None or score[k] > best[0]:
                    best = (score[k], k + 1, gl[k], gr[k], int(wl[k]), f, order, v[k], v[k + 1])
            for i in range(nknown):
                features[i] = constants[i]
            for i in range(nfound):
                constants[nknown + i] = features[nknown + i]
            n_const = ntotal
        split = False
        if best is not None:
            _, p, gl, gr, wl, f, order, lo, hi = best
            wn, wlf, wrf = float(W), float(wl), float(W - wl)
            improvement = (wn / w_total) * (impurity - (wrf / wn * gr) - (wlf / wn * gl))
            split = not (improvement + EPS < 0.0)
            thr = float(lo) / 2.0 + float(hi) / 2.0
            if variant == "mid32":
                thr = float(np.float32(lo) / np.float32(2) + np.float32(hi) / np.float32(2))
            if thr == float(hi) or np.isinf(thr):
                thr = float(lo)
        node = len(rec["left"])
        if parent >= 0:
            rec["left" if is_left else "right"][parent] = node
        rec["left"].append(-1)
        rec["right"].append(-1)
        rec["impurity"].append(impurity)
        rec["n_node_samples"].append(n)
        rec["weighted_n_node_samples"].append(W)
        rec["value"].append(tot / float(W))
        if split:
            rec["feature"].append(f)
            rec["threshold"].append(thr)
            rec["missing_go_to_left"].append(1 if p > n - p else 0)
            if variant == "missw":
                rec["missing_go_to_left"][-1] = 1 if wl > W - wl else 0
            samples[start:end] = order
            stack.append((start + p, end, depth + 1, node, 0, gr, n_const))
            stack.append((start, start + p, depth + 1, node, 1, gl, n_const))
        else:
            rec["feature"].append(-2)
            rec["threshold"].append(-2.0)
            rec["missing_go_to_left"].append(0)
        max_seen = max(max_seen, depth)
    out = {k: np.asarray(v) for k, v in rec.items()}
    for k in ("left", "right", "feature", "n_node_samples", "weighted_n_node_samples"):
        out[k] = out[k].astype(np.int32)
    out["missing_go_to_left"] = out["missing_go_to_left"].astype(np.uint8)
    out["value"] = np.asarray(rec["value"], np.float64).reshape(-1, C)
    out["max_depth"] = max_seen
    return out
