"""Seeded inputs and case tables for the k-means fit tests (tests/test_kmeans_fit_cases_host.py on the CPU,
tests/test_gpu_kmeans_fit.py and tests/test_gpu_dist.py on the GPU), and the one comparison of a GPU fit with the CPU oracle
(oracle/kmeans_impl.h) that those tests and tests/test_gpu_kmeans_pipelined.py share.

Three parts of the fit are pinned here:

  relocation   An empty cluster takes the pixel farthest from its centre (_relocate_empty_clusters_dense).  k-means++ seeds
               on distinct rows never run empty, so the reachable event is the degenerate one: d < k distinct rows.  The
               first d seeds are the distinct rows, the other k - d are copies of pixel 0's row and stay empty.  Iteration 1
               relocates nothing (every pixel sits on its seed: max distance 0) and gives the empty clusters the centre of
               the largest cluster; unless that is pixel 0's own cluster, the centre shift is far above tol.  Iteration 2 finds
               the averaged centres a rounding error away from their rows, relocates k - d pixels by those rounding-level
               distances, changes no label and ends the fit: n_iter == 2, and only the CENTRES tell which pixels were taken.
  stop rules   unchanged labels, shift <= tol, max_iter; cut at every place of the device loop's batches (4, then max(2, it / 3)).
  seeds        RandomState(seed) for seeds other than the reference's 42.

Every seed below was found on the CPU with the oracle alone (the first seed from 0 whose fit relocates) and is pinned;
tests/test_kmeans_fit_cases_host.py holds the preconditions."""
import numpy as np

THREADS, TILES_PER_CHUNK = 256, 16
F32, F64 = np.float32, np.float64
DT = {"f32": F32, "f64": F64}


def tile(dt):
    return THREADS * (4 if np.dtype(dt) == np.float32 else 2)   # TILE = 256 * PXL


def small_n(dt):
    """two tiles + 3 pixels: 2051 (float32), 1027 (float64)"""
    return 2 * tile(dt) + 3


def large_n(dt):
    """two chunks + one tile + 5 pixels: 33797 (float32), 16901 (float64)"""
    return 2 * TILES_PER_CHUNK * tile(dt) + tile(dt) + 5


# ------------------------------------------------------------------------------------------------ generators
def blobs(seed, n, F, k, dt, sigma):
    rng = np.random.default_rng(seed)
    cen = rng.random((max(k, 2), F)) * 4
    X = cen[rng.integers(0, cen.shape[0], n)] + rng.normal(0, sigma, (n, F))
    return [np.ascontiguousarray(X[:, f]).astype(dt) for f in range(F)]


def _prototype_rows(rng, d, F):
    # arbitrary (non-grid) values; the planes' ranges differ by orders of magnitude (1e-3 ... 1e3) and sit off zero
    mag = 10.0 ** rng.uniform(-3, 3, F)
    return (rng.standard_normal((d, F)) + rng.uniform(-2, 2, F)[None, :]) * mag[None, :]


def protos(seed, n, F, d, dt):
    """d distinct rows, every pixel a copy of one of them: Zipf-like multiplicities (row r about 1 / (r + 1) of the pixels),
    every row at least 3 times, shuffled.  -> (planes, prototype index of every pixel)"""
    rng = np.random.default_rng(seed)
    rows = _prototype_rows(rng, d, F)
    w = 1.0 / np.arange(1, d + 1)
    extra = np.floor((n - 3 * d) * w / w.sum()).astype(np.int64)
    extra[0] += n - 3 * d - extra.sum()
    who = np.repeat(np.arange(d), 3 + extra)
    rng.shuffle(who)
    X = rows[who]
    return [np.ascontiguousarray(X[:, f]).astype(dt) for f in range(F)], who


def protos_flat(seed, n, F, d, dt):
    """as protos(), but every row exactly 3 times except rows 0 and 1, which share the rest (row 0 one or two more than row 1):
    with k - d > 3 the farthest row can run out of copies; then the relocations go on to the next row, and the emptied donor
    takes the centre of the largest cluster.  (Two heavy rows, so that pixel 0 is often not in the largest cluster.)"""
    rng = np.random.default_rng(seed)
    rows = _prototype_rows(rng, d, F)
    rest = n - 3 * (d - 2)
    who = np.repeat(np.arange(d), [rest - (rest - 1) // 2, (rest - 1) // 2] + [3] * (d - 2))
    rng.shuffle(who)
    X = rows[who]
    return [np.ascontiguousarray(X[:, f]).astype(dt) for f in range(F)], who


# ------------------------------------------------------------------------------------------------ relocation cases
RELOC_F = (1, 7, 8, 9, 16, 17, 32, 33, 64)          # km_farthest widths 8 | 8 | 8 | 16 | 16 | 32 | 32 | blocked | blocked
RELOC_KD = ((8, 5), (16, 11), (32, 20), (33, 21), (64, 40))   # KMAX 8 | 16 | 32 | 64 | 64
RELOC_LARGE = ((9, 16, 11, "f32"), (9, 16, 11, "f64"), (33, 32, 20, "f32"), (33, 32, 20, "f64"), (64, 64, 40, "f32"), (1, 64, 40, "f64"))

# (F, k, d, type) -> seed of protos(); small_n pixels
RELOC_SEEDS_SMALL = {
    (1, 8, 5, 'f32'): 0, (1, 16, 11, 'f32'): 1, (1, 32, 20, 'f32'): 0, (1, 33, 21, 'f32'): 0, (1, 64, 40, 'f32'): 0,
    (7, 8, 5, 'f32'): 0, (7, 16, 11, 'f32'): 1, (7, 32, 20, 'f32'): 0, (7, 33, 21, 'f32'): 1, (7, 64, 40, 'f32'): 0,
    (8, 8, 5, 'f32'): 0, (8, 16, 11, 'f32'): 0, (8, 32, 20, 'f32'): 1, (8, 33, 21, 'f32'): 0, (8, 64, 40, 'f32'): 0,
    (9, 8, 5, 'f32'): 1, (9, 16, 11, 'f32'): 0, (9, 32, 20, 'f32'): 0, (9, 33, 21, 'f32'): 0, (9, 64, 40, 'f32'): 1,
    (16, 8, 5, 'f32'): 2, (16, 16, 11, 'f32'): 0, (16, 32, 20, 'f32'): 1, (16, 33, 21, 'f32'): 0, (16, 64, 40, 'f32'): 1,
    (17, 8, 5, 'f32'): 0, (17, 16, 11, 'f32'): 0, (17, 32, 20, 'f32'): 1, (17, 33, 21, 'f32'): 2, (17, 64, 40, 'f32'): 0,
    (32, 8, 5, 'f32'): 0, (32, 16, 11, 'f32'): 1, (32, 32, 20, 'f32'): 1, (32, 33, 21, 'f32'): 0, (32, 64, 40, 'f32'): 0,
    (33, 8, 5, 'f32'): 0, (33, 16, 11, 'f32'): 0, (33, 32, 20, 'f32'): 0, (33, 33, 21, 'f32'): 6, (33, 64, 40, 'f32'): 0,
    (64, 8, 5, 'f32'): 1, (64, 16, 11, 'f32'): 0, (64, 32, 20, 'f32'): 1, (64, 33, 21, 'f32'): 2, (64, 64, 40, 'f32'): 0,
    (1, 8, 5, 'f64'): 0, (1, 16, 11, 'f64'): 0, (1, 32, 20, 'f64'): 2, (1, 33, 21, 'f64'): 1, (1, 64, 40, 'f64'): 0,
    (7, 8, 5, 'f64'): 0, (7, 16, 11, 'f64'): 0, (7, 32, 20, 'f64'): 1, (7, 33, 21, 'f64'): 0, (7, 64, 40, 'f64'): 0,
    (8, 8, 5, 'f64'): 0, (8, 16, 11, 'f64'): 0, (8, 32, 20, 'f64'): 1, (8, 33, 21, 'f64'): 0, (8, 64, 40, 'f64'): 0,
    (9, 8, 5, 'f64'): 1, (9, 16, 11, 'f64'): 0, (9, 32, 20, 'f64'): 1, (9, 33, 21, 'f64'): 0, (9, 64, 40, 'f64'): 0,
    (16, 8, 5, 'f64'): 1, (16, 16, 11, 'f64'): 0, (16, 32, 20, 'f64'): 2, (16, 33, 21, 'f64'): 0, (16, 64, 40, 'f64'): 0,
    (17, 8, 5, 'f64'): 1, (17, 16, 11, 'f64'): 0, (17, 32, 20, 'f64'): 1, (17, 33, 21, 'f64'): 0, (17, 64, 40, 'f64'): 0,
    (32, 8, 5, 'f64'): 0, (32, 16, 11, 'f64'): 3, (32, 32, 20, 'f64'): 0, (32, 33, 21, 'f64'): 0, (32, 64, 40, 'f64'): 0,
    (33, 8, 5, 'f64'): 0, (33, 16, 11, 'f64'): 0, (33, 32, 20, 'f64'): 0, (33, 33, 21, 'f64'): 0, (33, 64, 40, 'f64'): 0,
    (64, 8, 5, 'f64'): 0, (64, 16, 11, 'f64'): 0, (64, 32, 20, 'f64'): 0, (64, 33, 21, 'f64'): 0, (64, 64, 40, 'f64'): 0,
}
# (F, k, d, type) -> seed of protos(); large_n pixels
RELOC_SEEDS_LARGE = {
    (9, 16, 11, 'f32'): 0, (9, 16, 11, 'f64'): 1, (33, 32, 20, 'f32'): 0,
    (33, 32, 20, 'f64'): 0, (64, 64, 40, 'f32'): 0, (1, 64, 40, 'f64'): 1,
}
# (F, k, d, type) -> seed of protos_flat(); small_n pixels: one per type, cluster bound and km_farthest width
DONOR_SEEDS = {
    (5, 8, 4, 'f32'): 9, (5, 16, 11, 'f32'): 3, (5, 32, 21, 'f32'): 0, (5, 33, 22, 'f32'): 0,
    (9, 8, 4, 'f32'): 0, (9, 16, 11, 'f32'): 0, (9, 32, 21, 'f32'): 0, (9, 33, 22, 'f32'): 2,
    (17, 8, 4, 'f32'): 0, (17, 16, 11, 'f32'): 0, (17, 32, 21, 'f32'): 5, (17, 33, 22, 'f32'): 0,
    (33, 8, 4, 'f32'): 0, (33, 16, 11, 'f32'): 0, (33, 32, 21, 'f32'): 6, (33, 33, 22, 'f32'): 1,
    (5, 8, 4, 'f64'): 2, (5, 16, 11, 'f64'): 0, (5, 32, 21, 'f64'): 2, (5, 33, 22, 'f64'): 3,
    (9, 8, 4, 'f64'): 2, (9, 16, 11, 'f64'): 0, (9, 32, 21, 'f64'): 0, (9, 33, 22, 'f64'): 0,
    (17, 8, 4, 'f64'): 1, (17, 16, 11, 'f64'): 0, (17, 32, 21, 'f64'): 0, (17, 33, 22, 'f64'): 1,
    (33, 8, 4, 'f64'): 6, (33, 16, 11, 'f64'): 2, (33, 32, 21, 'f64'): 0, (33, 33, 22, 'f64'): 5,
}


def relocation_cases():
    """[(id, generator, seed, n, F, k, d, type name)]: the grid at two tiles + 3, the handful at two chunks + one tile + 5"""
    out = []
    for (F, k, d, t), seed in RELOC_SEEDS_SMALL.items():
        out.append((f"{t}-F{F}-k{k}-d{d}", protos, seed, small_n(DT[t]), F, k, d, t))
    for (F, k, d, t), seed in RELOC_SEEDS_LARGE.items():
        out.append((f"{t}-F{F}-k{k}-d{d}-chunks", protos, seed, large_n(DT[t]), F, k, d, t))
    return out


def donor_cases():
    return [(f"{t}-F{F}-k{k}-d{d}-donor", protos_flat, seed, small_n(DT[t]), F, k, d, t) for (F, k, d, t), seed in DONOR_SEEDS.items()]


def case_planes(case):
    _, gen, seed, n, F, k, d, t = case
    return gen(seed, n, F, d, DT[t])


def km_width(F):
    return 8 if F <= 8 else 16 if F <= 16 else 32 if F <= 32 else 64


def km_kmax(k):
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


def lloyd_form(t, k, F):
    """the Lloyd kernel of (type, k, F): a register-resident width, or 64 = the feature-blocked form (k9_kmeans.h)"""
    return 64 if (t == "f64" and km_kmax(k) == 64 and F > 8) else km_width(F)


# ------------------------------------------------------------------------------------------------ the NumPy restatement
def q40(x):
    """a value of the planes' type, rounded to a multiple of 2^-40 as the exact sums hold it, back in that type"""
    return (np.rint(x.astype(np.float64) * 2.0 ** 40) * 2.0 ** -40).astype(x.dtype)


def restate_relocation(oracle, planes, k):
    """scikit-learn's own expression for the relocation of iteration 2 (_relocate_empty_clusters_dense:
    distances = ((X - centers_old[labels])**2).sum(axis=1); the n_empty farthest pixels, ties to the lowest index), from the
    oracle's max_iter = 1 fit: its centres are those after iteration 1, its labels iteration 2's E-step.
    -> dict(empty, far, rows, lab, dist): the empty clusters in index order, the pixel each one takes, that pixel's row rounded
    to 2^-40 (the relocated cluster's centre: a sum of one row, times 1 / 1)."""
    dt = planes[0].dtype
    lab, info = oracle.kmeans_fit_planes(planes, k, max_iter=1)
    X = np.stack(planes, axis=1)
    Xs = (X * info["scale"].astype(dt)[None, :] + info["min"].astype(dt)[None, :]) - info["mean"].astype(dt)[None, :]
    assert Xs.dtype == dt
    C1 = info["centers"].astype(dt)
    dist = ((Xs - C1[lab]) ** 2).sum(axis=1)
    assert dist.dtype == dt
    empty = np.flatnonzero(np.bincount(lab, minlength=k) == 0)
    order = np.lexsort((np.arange(dist.size), -dist.astype(np.float64)))   # farthest first, ties to the lowest index
    far = order[:empty.size]
    return dict(empty=empty, far=far, rows=q40(Xs[far]), lab=lab, dist=dist, n_iter1=info["n_iter"])


# ------------------------------------------------------------------------------------------------ stop cases
SIGMA_STOP = 0.6
# (F, k, type, n, seed of blobs() = F + k): sigma large enough that cutting the fit changes labels
STOP_CASES = ((5, 8, "f32", 2051, 13), (9, 40, "f32", 2051, 49), (5, 8, "f64", 1027, 13), (9, 40, "f64", 1027, 49), (5, 8, "f32", 33797, 13))
# the oracle's n_iter at tol = 1e-4, 0 and 10 (asserted by tests/test_kmeans_fit_cases_host.py)
STOP_ITERS = ((9, 12, 1), (9, 9, 2), (14, 14, 1), (13, 13, 2), (8, 13, 1))
TOLS = (1e-4, 0.0, 10.0)
OTHER_SEEDS = (0, 1, 7, 12345, 2 ** 31)


def stop_id(c):
    F, k, t, n, seed = c
    return f"{t}-F{F}-k{k}-n{n}"


def stop_planes(c):
    F, k, t, n, seed = c
    return blobs(seed, n, F, k, DT[t], SIGMA_STOP)


def stop_max_iters(s):
    """s: the case's iteration count at tol 0.  1 ... 4: inside the first batch of four speculatively enqueued iterations and
    its boundary; 5, 6: the second batch (two), cut and whole; 7, 9: later batches; s - 1, s, s + 1: around the iteration in
    which unchanged labels and max_iter coincide"""
    return sorted({1, 2, 3, 4, 5, 6, 7, 9, s - 1, s, s + 1} - {0})


# ------------------------------------------------------------------------------------------------ launch-table cases
def table_cases():
    """[(type, k, F)]: every (type, KMAX, Lloyd form): 2 x 4 x 4 register-resident widths and blocked forms; in float64 with
    KMAX = 64 the widths 16 and 32 are the feature-blocked form too.  k and F sit off the table's edges."""
    return [(t, k, F) for t in ("f32", "f64") for k in (5, 12, 27, 41) for F in (6, 13, 29, 47)]


def table_planes(t, k, F):
    dt = DT[t]
    return blobs(100 * k + F, small_n(dt), F, k + 3, dt, 0.3)


# ------------------------------------------------------------------------------------------------ GPU fit == oracle
def exact_planes(planes):
    """one device allocation of exactly n elements per plane"""
    import torch
    out = []
    for p in planes:
        t = torch.empty(p.size, dtype=torch.float32 if p.dtype == np.float32 else torch.float64, device="cuda")
        t.copy_(torch.from_numpy(p))
        out.append(t)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_fit_equal(meta, got, info, want, dt, tag):
    """one fit's results against the oracle's, bit for bit: seeds, scaler, tol, n_iter, relocated, labels, centres"""
    assert [int(x) for x in meta["init_indices"]] == [int(x) for x in info["init_indices"]], tag
    for key in ("scale", "min", "mean"):
        assert np.array_equal(bits(meta[key]), bits(info[key])), (tag, key)
    assert np.array_equal(bits(meta["tol"]), bits(info["tol"])), (tag, meta["tol"], info["tol"])
    assert int(meta["n_iter"]) == int(info["n_iter"]), (tag, meta["n_iter"], info["n_iter"])
    assert int(meta["relocated"]) == int(info["relocated"]), (tag, meta["relocated"], info["relocated"])
    assert got.shape == want.shape and np.array_equal(got, want), (tag, int((got != want).sum()))
    # the oracle reports the centres of the centred space; the library adds the mean back in the planes' type, as
    # scikit-learn does (best_centers += X_mean): one rounded addition per value, repeated here on the oracle's numbers
    want_centers = (info["centers"].astype(dt) + info["mean"].astype(dt)[None, :]).astype(np.float64)
    bad = np.flatnonzero((bits(meta["centers"]) != bits(want_centers)).any(axis=1))
    assert bad.size == 0, (tag, "centres of clusters", bad.tolist())


def check_fit(ctx, oracle, planes, k, tag, dev=exact_planes, **kw):
    """kw: max_iter, tol, seed, passed to both sides by name; -> the oracle's info"""
    want, info = oracle.kmeans_fit_planes(planes, k, **kw)
    labels, meta = ctx.kmeans_fit_predict(dev(planes), k, **kw)
    assert_fit_equal(meta, labels.cpu().numpy(), info, want, planes[0].dtype, tag)
    return info
