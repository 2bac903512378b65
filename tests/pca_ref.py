"""NumPy / Python-int restatement of K3 (csrc/k3_pca.hip and its host driver pca_core), operation for operation.  No torch.

Per band b and pixel, in float32 unless said otherwise, every operation one IEEE operation:
  v   = the plane's value (a uint8 plane: the byte as a float32)
  v   = norm1(v; lo_b, hi_b, den_b) when `lohi` is given, den_b = (hi_b - lo_b) + 1e-10f          (common.h)
  x_b = float32((float64)(v - center_b) / scale_b) when a scaler is given — the IEEE QUOTIENT: the kernels reach it with
        a reciprocal and two fmas (or the division itself for a scale that fails slow_div()'s test), which is their claim
Range of the fitted values: [0, 1] with `lohi`, 0..255 for uint8 planes without it, otherwise measured (NaN ignored);
bound = max(1, max_b max(|vmin_b - c_b|, |vmax_b - c_b|) / |s_b| * 1.000001), e2 = frexp(bound^2), Q = min(38, 48 - e2).
Sums over the fitted pixels as exact integers: rint(x_b * 2^Q) and rint(x_b * 2^Q * x_c) (both products exact in float64,
np.rint rounds half to even like the kernel's fma(.., 1.5 * 2^52)), int64 per block of at most 4096 pixels, Python ints
across blocks.  model() is then the host tail: float(S) * 2^-Q, scikit-learn's float32 mean and covariance steps, cyclic
Jacobi line for line, stable descending order, clamp at 0, float32 running total, sign by the first largest |entry|, offs
as a float32 fma chain, ratios.  Scores: the fma32 chain over the bands minus offs."""
import math

import numpy as np

from kmeans_model_ref import fma32

MAXB = 8
NACC = MAXB + MAXB * (MAXB + 1) // 2
Q_MAX = 38
Q_MIN = -19   # pca_core refuses a value range whose quantum would be coarser (RSSEG_ERR_UNSUPPORTED)
BLOCK = 4096
f32 = np.float32


class Unsupported(Exception):
    pass


def tri(b, c):
    """pca_tri: the slot of sum x_b * x_c (b <= c) after the MAXB first-moment slots."""
    return MAXB + b * MAXB - b * (b - 1) // 2 + (c - b)


def norm_den(lo, hi):
    return f32(f32(f32(hi) - f32(lo)) + f32(1e-10))


def norm1(x, lo, hi, den):
    """common.h: c = x < lo ? lo : x; c = c > hi ? hi : c; (c - lo) / den — a NaN and a -0.0 equal to lo pass through."""
    x = np.asarray(x, f32)
    lo, hi, den = f32(lo), f32(hi), f32(den)
    c = np.where(x < lo, lo, x)
    c = np.where(c > hi, hi, c)
    with np.errstate(all="ignore"):
        return ((c - lo) / den).astype(f32)


def scale_x(v, center, scale):
    """RobustScaler.transform of one column: float32 subtraction, float64 IEEE quotient, rounded to float32."""
    d = (np.asarray(v, f32) - f32(center)).astype(f32)
    with np.errstate(all="ignore"):
        return (d.astype(np.float64) / np.float64(scale)).astype(f32)


def slow_div(scale):
    """The host's condition for the plain division in the kernels: the scale or its reciprocal is not a normal number, or
    the scale's significand is all ones (the reciprocal form is then not provably the IEEE quotient)."""
    s = np.float64(scale)
    with np.errstate(all="ignore"):
        r = np.float64(1.0) / s

    def normal(v):
        return bool(np.isfinite(v)) and abs(float(v)) >= 2.0 ** -1022

    return (not normal(s)) or (not normal(r)) or (int(s.view(np.uint64)) & 0xFFFFFFFFFFFFF) == 0xFFFFFFFFFFFFF


def transform(planes, lohi=None, center=None, scale=None):
    """pca_x of every pixel: (n, nb) float32.  planes: float32 or uint8 arrays of equal length."""
    cols = []
    for b, p in enumerate(planes):
        v = np.asarray(p).reshape(-1).astype(f32)
        if lohi is not None:
            lo, hi = f32(lohi[b][0]), f32(lohi[b][1])
            v = norm1(v, lo, hi, norm_den(lo, hi))
        if center is not None:
            v = scale_x(v, center[b], scale[b])
        cols.append(v)
    return np.stack(cols, axis=1)


def value_range(planes_fit, lohi=None):
    """(vmin, vmax) per band as pca_core derives them; ValueError("infinity") as it refuses."""
    nb = len(planes_fit)
    if lohi is not None:
        return np.zeros(nb), np.ones(nb)
    if np.asarray(planes_fit[0]).dtype == np.uint8:
        return np.zeros(nb), np.full(nb, 255.0)
    vmin, vmax = np.zeros(nb), np.zeros(nb)
    for b, p in enumerate(planes_fit):
        p = np.asarray(p, f32)
        ok = ~np.isnan(p)
        if ok.any():
            vmin[b], vmax[b] = float(p[ok].min()), float(p[ok].max())
        if np.isinf(vmin[b]) or np.isinf(vmax[b]):
            raise ValueError("pca: Input X contains infinity")
    return vmin, vmax


def quantum(vmin, vmax, center=None, scale=None, q_min=None):
    """(Q, bound).  Unsupported below q_min (default Q_MIN, the library's)."""
    q_min = Q_MIN if q_min is None else q_min
    bound = 1.0
    for b in range(len(vmin)):
        c = float(f32(center[b])) if center is not None else 0.0
        s = float(scale[b]) if scale is not None else 1.0
        with np.errstate(all="ignore"):
            bound = max(bound, float(np.float64(max(abs(vmin[b] - c), abs(vmax[b] - c))) / np.float64(abs(s)) * 1.000001))
    if not math.isfinite(bound * bound):
        raise Unsupported("pca: scaled band range too large for exact accumulation (bound %.3g)" % bound)
    _, e2 = math.frexp(bound * bound)
    Q = min(Q_MAX, 48 - e2)
    if Q < q_min:
        raise Unsupported("pca: scaled band range too large for exact accumulation (bound %.3g)" % bound)
    return Q, bound


def int_sums(X, Q, block=BLOCK):
    """The NACC exact sums of the pixels of X (n, nb) in quanta of 2^-Q, as Python ints (slots of bands >= nb stay 0)."""
    assert 1 <= block <= BLOCK
    n, nb = X.shape
    S = [0] * NACC
    fx = math.ldexp(1.0, Q)
    for i0 in range(0, n, block):
        x = X[i0:i0 + block].astype(np.float64)
        xs = x * fx
        for b in range(nb):
            S[b] += int(np.rint(xs[:, b]).astype(np.int64).sum())
            for c in range(b, nb):
                S[tri(b, c)] += int(np.rint(xs[:, b] * x[:, c]).astype(np.int64).sum())
    return S


def limbs(S):
    """The sums as rsseg_host_pca_model takes them: {hi, lo} with value (hi << 32) + lo, lo in [0, 2^32)."""
    out = np.zeros(2 * NACC, np.int64)
    for i, s in enumerate(S):
        out[2 * i], out[2 * i + 1] = s >> 32, s & 0xFFFFFFFF
    return out


def jacobi_eigh(A):
    """jacobi_eigh of k3_pca.hip, line for line, on Python floats (IEEE float64, no contraction).  A: n x n list of lists,
    changed in place.  Returns (w, V) with V's columns the eigenvectors."""
    n = len(A)
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _sweep in range(64):
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += A[p][q] * A[p][q]
        if off < 1e-300:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (math.fabs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def model(S, N, Q, nb, nc):
    """The host tail of pca_core on the exact sums S (Python ints, int_sums' layout)."""
    if not (1 <= nb <= MAXB and 1 <= nc <= nb) or N < 2:
        raise ValueError("pca: bad arguments or fewer than 2 samples")
    inv = math.ldexp(1.0, -Q)

    def val(i):
        return float(S[i]) * inv     # int -> float rounds to nearest even, like the conversion of the 128-bit integer

    with np.errstate(all="ignore"):
        Nf, N1f = f32(N), f32(N - 1)
        mu = np.array([f32(val(b)) / Nf for b in range(nb)], f32)
        cov = np.zeros((nb, nb), f32)
        for b in range(nb):
            for c in range(b, nb):
                g = f32(val(tri(b, c)))
                nm = f32(Nf * mu[b])
                nmm = f32(nm * mu[c])
                cov[b, c] = cov[c, b] = f32(f32(g - nmm) / N1f)
        w, V = jacobi_eigh([[float(cov[i, j]) for j in range(nb)] for i in range(nb)])
        order = sorted(range(nb), key=lambda i: -w[i])     # stable: equal eigenvalues keep their index order
        ev = np.zeros(nb, f32)
        for i in range(nb):
            e = f32(w[order[i]])
            ev[i] = f32(0) if e < f32(0) else e
        total = f32(0)
        for i in range(nb):
            total = f32(total + ev[i])
        comp = np.zeros((nc, nb), f32)
        offs = np.zeros(nc, f32)
        for c in range(nc):
            row = np.array([f32(V[b][order[c]]) for b in range(nb)], f32)
            am = 0
            for b in range(nb):
                if abs(row[b]) > abs(row[am]):
                    am = b
            sg = f32(-1) if row[am] < f32(0) else f32(1)
            comp[c] = row * sg
            o = f32(0)
            for b in range(nb):
                o = fma32(mu[b:b + 1], comp[c, b:b + 1], np.array([o], f32))[0]
            offs[c] = o
        ratio = (ev[:nc] / total).astype(f32)
    return dict(mean=mu, cov=cov, components=comp, explained_variance=ev[:nc].copy(), ratio=ratio, offs=offs, ev_all=ev, Q=Q, N=N)


def scores(X, m):
    """k3_project: per component the fma chain over the bands from 0, minus offs.  (n, nc) float32."""
    comp, offs = m["components"], m["offs"]
    out = np.zeros((X.shape[0], comp.shape[0]), f32)
    with np.errstate(all="ignore"):
        for c in range(comp.shape[0]):
            s = np.zeros(X.shape[0], f32)
            for b in range(X.shape[1]):
                s = fma32(X[:, b], comp[c, b], s)
            out[:, c] = s - offs[c]
    return out


def tag(plane):
    """The extrema tag of a produced plane: (min, max) with a NaN read as 0."""
    z = np.where(np.isnan(plane), f32(0), plane)
    return (float(z.min()), float(z.max()))


def pca(planes, center, scale, nc, lohi=None, fit=None):
    """An rsseg_pca_fit_transform_* call: the model of the pixels [fit[0], fit[0] + fit[1]) and the scores of all of them.
    Raises ValueError with the library's wording for NaN / infinity / too few samples, Unsupported for the value range."""
    n = np.asarray(planes[0]).size
    f0, fn = (0, n) if fit is None else fit
    fitp = [np.asarray(p).reshape(-1)[f0:f0 + fn] for p in planes]
    vmin, vmax = value_range(fitp, lohi)
    Q, bound = quantum(vmin, vmax, center, scale)
    X = transform(planes, lohi, center, scale)
    Xf = X[f0:f0 + fn]
    if np.isnan(Xf).any():
        raise ValueError("pca: Input X contains NaN.")
    if fn < 2:
        raise ValueError("pca: needs at least 2 samples")
    m = model(int_sums(Xf, Q), fn, Q, X.shape[1], nc)
    m["bound"] = bound
    m["scores"] = scores(X, m)
    m["tags"] = [tag(m["scores"][:, c]) for c in range(nc)]
    return m


def fused(planes, center, scale, nc, lohi, quantize, fit=None, oracle=None):
    """An rsseg_indices_pca_* call with every optional output: pca()'s dict plus the seven indices (oracle.ref_np's
    restatement of them on the normalised bands 0..4), the five normalised bands, the byte plane
    trunc(norm1(normalised NIR; lo2, hi2) * mult) and the tags of indices then components."""
    O = oracle
    m = pca(planes, center, scale, nc, lohi, fit)
    nrm = [norm1(np.asarray(planes[b]).reshape(-1).astype(f32), lohi[b][0], lohi[b][1], norm_den(lohi[b][0], lohi[b][1])) for b in range(5)]
    b_, g_, r_, n_, s_ = nrm
    idx = [O.calculate_ndvi(n_, r_), O.calculate_evi(n_, r_, b_), O.calculate_msavi(n_, r_), O.calculate_ndwi(g_, n_),
           O.calculate_mndwi(g_, s_), O.calculate_ndbi(s_, n_), O.calculate_bsi(b_, r_, n_, s_)]
    lo2, hi2, mult = quantize
    q = (norm1(n_, lo2, hi2, norm_den(lo2, hi2)) * f32(mult)).astype(f32)
    m["indices"] = [np.asarray(i, f32) for i in idx]
    m["norm"] = nrm
    m["q"] = q.astype(np.int32).astype(np.uint8)
    m["tags"] = [tag(i) for i in m["indices"]] + m["tags"]
    return m
