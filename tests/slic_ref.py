"""K23 restated in NumPy (include/rsseg.h: rsseg_slic_u8, rsseg_segment_sums, rsseg_segment_majority_u8, rsseg_segment_paint),
operation for operation: what the kernels are equal to, bit for bit.  Also the scenes the host and GPU tests share."""
import numpy as np
from scipy import ndimage

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def grid_labels(H, W, S, mask=None):
    """cell id cy * nx + cx per pixel, -1 where masked"""
    yy, xx = np.mgrid[0:H, 0:W]
    nx = -(-W // S)
    lab = (yy // S) * nx + xx // S
    if mask is not None:
        lab = np.where(np.asarray(mask) != 0, lab, -1)
    return lab.astype(np.int64)


def centres(lab, q, K):
    """integer sums over the valid pixels of every label -> (count int64, c_y, c_x, [c_p]) with one float64 division each"""
    H, W = lab.shape
    yy, xx = np.mgrid[0:H, 0:W]
    v = lab >= 0
    l = lab[v]
    cnt = np.zeros(K, np.int64)
    sy = np.zeros(K, np.int64)
    sx = np.zeros(K, np.int64)
    np.add.at(cnt, l, 1)
    np.add.at(sy, l, yy[v].astype(np.int64))
    np.add.at(sx, l, xx[v].astype(np.int64))
    sq = []
    for p in q:
        s = np.zeros(K, np.int64)
        np.add.at(s, l, p[v].astype(np.int64))
        sq.append(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = cnt.astype(np.float64)
        return cnt, sy.astype(np.float64) / c, sx.astype(np.float64) / c, [s.astype(np.float64) / c for s in sq]


def assign(lab, q, S, weight, cen):
    """one assignment: candidates in ascending id, the first taken as it is, then strictly smaller D only"""
    H, W = lab.shape
    ny, nx = -(-H // S), -(-W // S)
    cnt, c_y, c_x, c_p = cen
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = yy // S, xx // S
    valid = lab >= 0
    yf, xf = yy.astype(np.float64), xx.astype(np.float64)
    qf = [p.astype(np.float64) for p in q]
    w = np.float64(weight)
    best = np.full((H, W), -1, np.int64)
    bestD = np.zeros((H, W), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gy, gx = cy + dy, cx + dx
                ok = valid & (gy >= 0) & (gy < ny) & (gx >= 0) & (gx < nx)
                k = np.where(ok, gy * nx + gx, 0)
                ok &= cnt[k] > 0
                dc = np.zeros((H, W), np.float64)
                for p in range(len(q)):
                    d = qf[p] - c_p[p][k]
                    dc = dc + d * d
                ddy = yf - c_y[k]
                ddx = xf - c_x[k]
                ds = ddy * ddy + ddx * ddx
                D = dc + w * ds
                take = ok & ((best < 0) | (D < bestD))
                best = np.where(take, k, best)
                bestD = np.where(take, D, bestD)
    assert (best[valid] >= 0).all()      # the invariant: a pixel's own label is always a live candidate
    return np.where(valid, best, -1)


def iterate(planes, S, weight, max_iter, mask=None):
    """(centre id per pixel with -1 = masked, n_iter)"""
    H, W = planes[0].shape
    K = (-(-H // S)) * (-(-W // S))
    lab = grid_labels(H, W, S, mask)
    n_iter = 0
    for t in range(1, max_iter + 1):
        new = assign(lab, planes, S, weight, centres(lab, planes, K))
        changed = int((new != lab).sum())
        lab = new
        n_iter = t
        if changed == 0:
            break
    return lab, n_iter


def components(lab):
    """4-connected components of equal label >= 0: (H, W) ids 1 ... n, 0 where lab < 0.  scipy.ndimage.label with the
    4-neighbour structure on the doubled grid: pixels at even positions, a bridge between two neighbours of equal label."""
    H, W = lab.shape
    g = np.zeros((2 * H - 1, 2 * W - 1), bool)
    v = lab >= 0
    g[::2, ::2] = v
    g[::2, 1::2] = v[:, :-1] & v[:, 1:] & (lab[:, :-1] == lab[:, 1:])
    g[1::2, ::2] = v[:-1, :] & v[1:, :] & (lab[:-1, :] == lab[1:, :])
    ids, _ = ndimage.label(g, structure=FOUR)
    return ids[::2, ::2].astype(np.int64)


def shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx], 0 outside"""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
    yd, xd = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
    out[ys, xs] = a[yd, xd]
    return out


def enforce(lab, min_area):
    """(segment key per pixel with 0 = masked, n_regrown, rounds): components below min_area regrown in Jacobi rounds"""
    comp = components(lab)
    valid = comp > 0
    area = np.bincount(comp.reshape(-1))
    seg = np.where(valid & (area[comp] >= min_area), comp, 0)     # > 0: assigned
    n_regrown, rounds = 0, 0
    while True:
        open_ = valid & (seg == 0)
        new = np.zeros_like(seg)
        for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):          # up, left, right, down
            nb = shift(seg, dy, dx)
            new = np.where(open_ & (new == 0) & (nb > 0), nb, new)
        got = int((new > 0).sum())
        if got == 0:
            break
        seg = np.where(new > 0, new, seg)
        n_regrown += got
        rounds += 1
    return np.where(valid, np.where(seg > 0, seg, comp), 0), n_regrown, rounds


def renumber(key):
    """1 ... n in the order of every key's first pixel (raster order); 0 stays 0"""
    flat = key.reshape(-1)
    idx = np.flatnonzero(flat > 0)
    out = np.zeros(flat.shape, np.int32)
    if idx.size == 0:
        return out.reshape(key.shape), 0
    u, first, inv = np.unique(flat[idx], return_index=True, return_inverse=True)
    rank = np.empty(len(u), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(1, len(u) + 1)
    out[idx] = rank[inv]
    return out.reshape(key.shape), len(u)


def slic_ref(planes, S, weight, max_iter, min_area, mask=None):
    """(labels int32 (H, W), n_segments, n_iter, n_regrown)"""
    planes = [np.asarray(p, np.uint8) for p in planes]
    lab, n_iter = iterate(planes, S, weight, max_iter, mask)
    key, n_regrown, _ = enforce(lab, min_area)
    out, n = renumber(key)
    return out, n, n_iter, n_regrown


def fixed40(x):
    """llrint(x * 2^40), round to nearest even: the product is exact in float64 for a float32 x"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * np.float64(2.0 ** 40)).astype(np.int64)


def segment_sums_ref(seg, planes=(), mask=None, n_segments=None):
    """int64 [(n + 1), 3 + P]: count, sum y, sum x, plane sums (uint8 as integers, float32 as fixed40); row 0 zero"""
    seg = np.asarray(seg)
    H, W = seg.shape
    n = int(seg.max()) if n_segments is None else int(n_segments)
    yy, xx = np.mgrid[0:H, 0:W]
    v = seg > 0
    if mask is not None:
        v &= np.asarray(mask) != 0
    l = seg[v].astype(np.int64)
    out = np.zeros((n + 1, 3 + len(planes)), np.int64)
    np.add.at(out[:, 0], l, 1)
    np.add.at(out[:, 1], l, yy[v].astype(np.int64))
    np.add.at(out[:, 2], l, xx[v].astype(np.int64))
    for i, p in enumerate(planes):
        p = np.asarray(p)
        vals = p[v].astype(np.int64) if p.dtype == np.uint8 else fixed40(p[v])
        np.add.at(out[:, 3 + i], l, vals)
    return out


def segment_means_ref(seg, planes, mask=None, n_segments=None):
    sums = segment_sums_ref(seg, planes, mask, n_segments)
    scale = np.array([1.0 if np.asarray(p).dtype == np.uint8 else 2.0 ** 40 for p in planes], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return sums[:, 3:].astype(np.float64) / scale[None, :] / sums[:, 0].astype(np.float64)[:, None]


def segment_majority_ref(seg, class_map, ignore=-1, fill=0, n_segments=None):
    """uint8 [n + 1]: most votes, ties to the smallest label, `fill` without a voter and for entry 0"""
    seg = np.asarray(seg)
    cm = np.asarray(class_map, np.uint8)
    n = int(seg.max()) if n_segments is None else int(n_segments)
    votes = np.zeros((n + 1, 256), np.int64)
    v = (seg > 0) & (cm != ignore)
    np.add.at(votes, (seg[v].astype(np.int64), cm[v].astype(np.int64)), 1)
    table = np.where(votes.max(axis=1) > 0, votes.argmax(axis=1), fill).astype(np.uint8)   # argmax: the first maximum
    table[0] = fill
    return table


def paint_ref(seg, table):
    return np.asarray(table)[np.asarray(seg)]


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def blobs(rs, shape, values, cell=5, noise=0.2):
    """cells of cell x cell pixels of one value, `noise` of the pixels redrawn: smooth regions, edges and speckle"""
    values = np.asarray(values)
    H, W = shape
    coarse = values[rs.randint(0, len(values), (H // cell + 1, W // cell + 1))]
    q = np.kron(coarse, np.ones((cell, cell), int))[:H, :W]
    flip = rs.rand(H, W) < noise
    q[flip] = values[rs.randint(0, len(values), int(flip.sum()))]
    return np.ascontiguousarray(q, dtype=np.uint8)


def scene(seed, shape, P, cell=7, noise=0.1):
    """P uint8 planes: blobs of a few grey levels, different per plane"""
    rs = np.random.RandomState(seed)
    return [blobs(rs, shape, [10, 60, 120, 200, 250], cell=cell + (p % 3), noise=noise) for p in range(P)]


def snake(H, W):
    """a one-pixel path of value 255 winding over a 0 background, rows 1, 3, 5 ... joined alternately right and left"""
    q = np.zeros((H, W), np.uint8)
    for r, y in enumerate(range(1, H - 1, 2)):
        q[y, 1:W - 1] = 255
        if y + 2 < H - 1:
            q[y + 1, W - 2 if r % 2 == 0 else 1] = 255
    return q
