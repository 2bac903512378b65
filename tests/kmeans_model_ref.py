"""NumPy restatement of K18 (rsseg_kmeans_predict), the sweep of a fitted KMeans model, for float32 and float64.

Per pixel, in the planes' type T, every operation one IEEE operation:
  xs_f  = (NaN -> 0)(x_f) * scale_f + min_f
  dot_j = fma chain over f = 0 .. F-1 of xs_f * c_jf         csq_j = fma chain of c_jf * c_jf
  d_j   = fma(-2, dot_j, csq_j);  label = the lowest j with the smallest d_j
  sq    = _euclidean_dense_dense(xs, c_label, squared=True) (sklearn/cluster/_k_means_common.pyx:16-43): per group of four
          features result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3, the remaining features one at a time
  dist  = sqrt(sq)
and over the pixels: counts per label, inertia = the exact integer sum of rint(sq * 2^40), as a double times 2^-40.

A fused multiply-add is one rounding of the exact a*b + c.  NumPy has none, so it is built from error-free transformations:
the product's error (exact in float64 for float32 operands; Dekker's product for float64 ones), the sum's error (Knuth's
two-sum), and ROUND-TO-ODD of the low parts before the last addition (Boldo & Melquiond, "Emulation of a FMA and correctly
rounded sums: proved algorithms using rounding to odd", IEEE TC 2008, algorithm 5), which makes the final rounding the
correct one.  Where Python has math.fma (3.13) or not, fma_exact() is the same value from exact rational arithmetic: the
tests pin the vectorised forms against it, and elements outside the transformations' range (products near the underflow or
overflow threshold) are computed by it."""
import math
from fractions import Fraction

import numpy as np

Q40 = 2.0 ** 40
CHUNK = {np.dtype(np.float32): 16384, np.dtype(np.float64): 8192}   # km_chunk<T>(): 256 threads x PXL x 16 tiles
TILE = {np.dtype(np.float32): 1024, np.dtype(np.float64): 512}


def qmax(dt) -> int:
    """Quanta of 2^-40 a pixel may add to its chunk's signed 64-bit partial: below 2^63 / chunk."""
    return (1 << 63) // CHUNK[np.dtype(dt)]


def sq_bound(dt) -> float:
    """The squared distance from which a pixel is left out of the inertia (overflow): 512 for float32, 1024 for float64."""
    return qmax(dt) / Q40


def fma_exact(a, b, c, dt=np.float64):
    """fma of three scalars in dtype dt, from exact arithmetic (math.fma where Python has it and dt is float64)."""
    if np.dtype(dt) == np.float64 and hasattr(math, "fma"):
        return np.float64(math.fma(float(a), float(b), float(c)))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if np.dtype(dt) == np.float64:
        return np.float64(float(exact)) if exact != 0 else np.float64(float(a) * float(b) + float(c))   # Fraction -> float rounds to nearest even
    # float32: round the rational to 24 bits, ties to even
    if exact == 0:
        return np.float32(np.float32(a) * np.float32(b) + np.float32(c))   # the sign of an exact zero follows the operands
    s = -1 if exact < 0 else 1
    m = abs(exact)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    e = max(e, -126)                       # subnormals share the exponent of the smallest normal
    ulp = Fraction(2) ** (e - 23)
    n, r = divmod(m, ulp)
    n = int(n)
    if r > ulp / 2 or (r == ulp / 2 and n & 1):
        n += 1
    return np.float32(s * float(Fraction(n) * ulp))


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _to_odd(s, e):
    """RN(x) = s with x = s + e exactly -> x rounded to odd: s when exact or already odd, else its neighbour towards x."""
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where((e > 0) == (s > 0), 1, -1)   # moving away from zero raises the bit pattern, towards zero lowers it
    # s == 0 with e != 0 cannot occur: then RN(x) = x = e
    return np.where(fix, (bits + toward).view(np.float64), s)


def fma32(a, b, c):
    """float32 fma, elementwise: the product is exact in float64; where it matters the sum is rounded to odd in float64
    (53 >= 2 * 24 + 2 bits) before it is rounded once to float32."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = np.ascontiguousarray(p + c)
    # The two roundings (to float64, then to float32) differ from one only when the float64 sum lies exactly half way between
    # two float32 values (its low 29 mantissa bits are 1 0...0) and is itself inexact: only there is the sum's error looked at.
    # (float32 subnormals have fewer bits: whatever is that small takes the rational form.)
    z = s.astype(np.float32)
    half = (s.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    if half.any():
        i = np.nonzero(half)
        s_i, e_i = _two_sum(p[i], c[i])
        z[i] = _to_odd(np.ascontiguousarray(s_i), e_i).astype(np.float32)
    tiny = (s != 0) & (np.abs(s) < 2.0 ** -120)
    for i in zip(*np.nonzero(tiny)):
        z[i] = fma_exact(a[i], b[i], c[i], np.float32)
    return z


_SPLIT = 134217729.0   # 2^27 + 1


def _two_prod(a, b):
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """float64 fma, elementwise: (uh, ul) = a * b exactly, (th, tl) = c + uh exactly, RN(th + RO(tl + ul))."""
    a, b, c = (np.ascontiguousarray(v) for v in np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64),
                                                                  np.asarray(c, np.float64)))
    if hasattr(math, "fma"):
        return np.vectorize(math.fma, otypes=[np.float64])(a, b, c)
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        vs, ve = _two_sum(tl, ul)
        z = th + _to_odd(np.ascontiguousarray(vs), ve)
        # outside the range in which the transformations are exact: the rational form, element by element
        big = 2.0 ** 990
        bad = ((uh != 0) & (np.abs(uh) < 2.0 ** -960)) | (np.abs(a) > big) | (np.abs(b) > big) | (np.abs(c) > big) | ~np.isfinite(z)
    if bad.any():
        z = z.copy()
        for i in zip(*np.nonzero(bad)):
            z[i] = fma_exact(a[i], b[i], c[i])
    return z


def tfma(dt):
    return fma32 if np.dtype(dt) == np.float32 else fma64


def model_arrays(centers, scale, min_, dt):
    dt = np.dtype(dt)
    c = np.ascontiguousarray(centers, dtype=dt)
    fma = tfma(dt)
    csq = np.zeros(c.shape[0], dt)
    for f in range(c.shape[1]):
        csq = fma(c[:, f], c[:, f], csq)
    return c, np.asarray(scale, dt).reshape(-1), np.asarray(min_, dt).reshape(-1), csq


def scale_planes(X, scale, min_):
    """MinMaxScaler.transform after NaN -> 0, in X's dtype: (n, F)."""
    X = np.where(np.isnan(X), X.dtype.type(0), X)
    return X * scale[None, :] + min_[None, :]


def sq_dist(xs, crow):
    """_euclidean_dense_dense(a, b, F, squared=True) row by row: xs (n, F), crow (n, F), both of dtype T."""
    n, F = xs.shape
    res = np.zeros(n, xs.dtype)
    d = xs - crow
    g = F // 4
    for i in range(g):
        d0, d1, d2, d3 = (d[:, 4 * i + r] for r in range(4))
        res = res + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
    for f in range(4 * g, F):
        res = res + d[:, f] * d[:, f]
    return res


def apply(X, centers, scale, min_):
    """X (n, F) float32 or float64 raw values -> dict of per-pixel labels (int32), sq, dist (X's dtype), q (int64 quanta, -1
    for a pixel left out of the inertia), xs (the scaled values), tied (more than one centre at the smallest d_j).  Every entry is per pixel, so a prefix of X has the prefix of every entry."""
    dt = X.dtype
    c, sc, mn, csq = model_arrays(centers, scale, min_, dt)
    fma = tfma(dt)
    with np.errstate(all="ignore"):
        xs = scale_planes(X, sc, mn)
        dot = np.zeros((X.shape[0], c.shape[0]), dt)
        for f in range(c.shape[1]):
            dot = fma(xs[:, f][:, None], c[:, f][None, :], dot)
        d = fma(dt.type(-2), dot, csq[None, :])
        labels = np.argmin(d, axis=1).astype(np.int32)     # first occurrence: the lowest index among equals
        tied = (d == d.min(axis=1)[:, None]).sum(axis=1) > 1
        sq = sq_dist(xs, c[labels])
        dist = np.sqrt(sq)
        ok = sq < dt.type(2048)
        q = np.where(ok, np.rint(np.where(ok, sq, 0).astype(np.float64) * Q40), -1.0).astype(np.int64)
        q[q >= qmax(dt)] = -1
    return dict(labels=labels, sq=sq, dist=dist, q=q, xs=xs, tied=tied)


def summary(ref, n, k):
    """counts, inertia, overflow of the first n pixels of apply()'s result."""
    q = ref["q"][:n]
    overflow = bool((q < 0).any())
    total = sum(int(v) for v in q.tolist() if v >= 0)
    return dict(counts=np.bincount(ref["labels"][:n], minlength=k).astype(np.int64),
                inertia=float("inf") if overflow else float(total) * 2.0 ** -40, overflow=overflow, quanta=total)
