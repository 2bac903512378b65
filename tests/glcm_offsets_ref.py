"""The texture function's contract for any (distance, angle) entries, restated in NumPy for the tests of
rsseg_glcm_offsets_u8 (csrc/k4_glcm_offsets.hip):

  literal_maps  graycomatrix(window, distances, angles, levels, symmetric=True, normed=True) followed by
                graycoprops(...).mean() for each property, in float64 (scikit-image 0.18 feature/texture.py), per window;
  spec_maps     the kernel's formulation: exact integer statistics per distinct offset, each entry's five properties
                in float64 with correctly rounded operations, the entries summed left to right in entry order, divided
                by their count, rounded to float32.  The kernel equals this bit for bit.
Both take the (dr, dc) entries of rsseg.pipeline.glcm_offset_plan."""
import numpy as np

PROPS = ["contrast", "dissimilarity", "homogeneity", "energy", "correlation"]
HQ40 = np.array([round(2.0 ** 40 / (1.0 + d * d)) for d in range(256)], np.int64)   # llrint of the same double


def literal_props(win_img, entries, levels):
    """graycomatrix + graycoprops of one window: (5, n_entries) float64."""
    w = np.asarray(win_img, np.int64)
    R, Cn = w.shape
    out = np.zeros((5, len(entries)))
    i_idx, j_idx = np.meshgrid(np.arange(levels), np.arange(levels), indexing="ij")
    for e, (dr, dc) in enumerate(entries):
        G = np.zeros((levels, levels), np.float64)
        r0, r1 = max(0, -dr), min(R, R - dr)
        c0, c1 = max(0, -dc), min(Cn, Cn - dc)
        if r1 > r0 and c1 > c0:
            a = w[r0:r1, c0:c1].ravel()
            b = w[r0 + dr:r1 + dr, c0 + dc:c1 + dc].ravel()
            np.add.at(G, (a, b), 1.0)
        P = G + G.T
        s = P.sum()
        P = P / (s if s != 0 else 1.0)
        d = (i_idx - j_idx).astype(np.float64)
        out[0, e] = np.sum(P * d * d)
        out[1, e] = np.sum(P * np.abs(d))
        out[2, e] = np.sum(P / (1.0 + d * d))
        out[3, e] = np.sqrt(np.sum(P * P))
        mi, mj = np.sum(i_idx * P), np.sum(j_idx * P)
        si = np.sqrt(np.sum(P * (i_idx - mi) ** 2))
        sj = np.sqrt(np.sum(P * (j_idx - mj) ** 2))
        cov = np.sum(P * (i_idx - mi) * (j_idx - mj))
        out[4, e] = 1.0 if (si < 1e-15 or sj < 1e-15) else cov / (si * sj)
    return out


def literal_maps(q, levels, win, step, entries):
    q = np.asarray(q)
    oh, ow = (q.shape[0] - win) // step + 1, (q.shape[1] - win) // step + 1
    maps = np.zeros((5, oh, ow), np.float64)
    for y in range(oh):
        for x in range(ow):
            maps[:, y, x] = literal_props(q[y * step:y * step + win, x * step:x * step + win], entries, levels).mean(axis=1)
    return dict(zip(PROPS, maps.astype(np.float32)))


def offset_stats(wins, dr, dc):
    """Exact integer statistics of offset (dr, dc) over a stack of windows (N, win, win):
    np, S1, S2, Hq (2^-40 fixed point), M1, M2, Mx, A = sum_ij (G_ij + G_ji)^2."""
    N, win, _ = wins.shape
    z = np.zeros(N, np.int64)
    if abs(dr) >= win or abs(dc) >= win:
        return 0, z, z, z, z, z, z, z
    r0, r1 = max(0, -dr), min(win, win - dr)
    c0, c1 = max(0, -dc), min(win, win - dc)
    x = wins[:, r0:r1, c0:c1].reshape(N, -1).astype(np.int64)
    y = wins[:, r0 + dr:r1 + dr, c0 + dc:c1 + dc].reshape(N, -1).astype(np.int64)
    npairs = x.shape[1]
    d = np.abs(x - y)
    S1, S2 = d.sum(1), (d * d).sum(1)
    Hq = HQ40[d].sum(1)
    M1, M2, Mx = (x + y).sum(1), (x * x + y * y).sum(1), (2 * x * y).sum(1)
    lo, hi = np.minimum(x, y), np.maximum(x, y)
    key = np.sort(lo * 256 + hi, axis=1)
    diag = (key // 256) == (key % 256)
    # rank of each key within its run of equal keys: sum over a run of (2 rank + 1) is c^2
    start = np.ones_like(key, bool)
    start[:, 1:] = key[:, 1:] != key[:, :-1]
    pos = np.broadcast_to(np.arange(npairs), key.shape)
    rank = pos - np.maximum.accumulate(np.where(start, pos, 0), axis=1)
    A = ((2 * rank + 1) * np.where(diag, 4, 2)).sum(1)
    return npairs, S1, S2, Hq, M1, M2, Mx, A


def entry_values(st):
    """The five float64 properties of one offset's statistics (per window)."""
    npairs, S1, S2, Hq, M1, M2, Mx, A = st
    N = len(S1)
    if npairs == 0:
        return [np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), np.ones(N)]
    dn = float(npairs)
    den = M2 * (2 * npairs) - M1 * M1
    num = Mx * (2 * npairs) - M1 * M1
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = np.where(den == 0, 1.0, num.astype(np.float64) / den.astype(np.float64))
    return [S2.astype(np.float64) / dn, S1.astype(np.float64) / dn, (Hq.astype(np.float64) / dn) * 2.0 ** -40,
            np.sqrt(A.astype(np.float64)) / float(2 * npairs), corr]


def spec_windows(wins, entries):
    """spec properties of a stack of windows (N, win, win) of a uint8 plane: (5, N) float32."""
    wins = np.asarray(wins, np.uint8)
    cache = {}
    s = [np.zeros(len(wins)) for _ in range(5)]
    for dr, dc in entries:
        key = (dr, dc) if dr > 0 or (dr == 0 and dc >= 0) else (-dr, -dc)
        if key not in cache:
            cache[key] = entry_values(offset_stats(wins, *key))
        v = cache[key]
        s = [s[t] + v[t] for t in range(5)]
    n = float(len(entries))
    return np.stack([(st / n).astype(np.float32) for st in s])


def spec_maps(q, levels, win, step, entries):
    q = np.ascontiguousarray(q, np.uint8)
    oh, ow = (q.shape[0] - win) // step + 1, (q.shape[1] - win) // step + 1
    v = np.lib.stride_tricks.sliding_window_view(q, (win, win))[::step, ::step][:oh, :ow]
    props = spec_windows(v.reshape(oh * ow, win, win), entries)
    return dict(zip(PROPS, props.reshape(5, oh, ow)))
