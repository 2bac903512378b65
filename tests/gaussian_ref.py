"""NumPy restatement of K22 (rsseg_gauss_classify): Gaussian maximum-likelihood / Mahalanobis / minimum-distance
classification, in float64, every operation one IEEE operation.

A model is k classes over F features: mean[k][F]; whiten[k][F (F + 1) / 2], the rows of a lower-triangular W_j packed
row-major; offset[k]; class_values[k] (uint8, distinct, 1..255; 0 is "unclassified"); max_dist2 (+inf: no threshold).
Per pixel, for j ascending:
  x_f = the plane value widened to float64 (exact), a NaN read as 0
  d_f = x_f - mean[j][f]
  z_i = fma chain z = fma(W_j[i][f], d_f, z) over f = 0..i, from +0
  m_j = fma chain m = fma(z_i, z_i, m) over i = 0..F-1, from +0
  g_j = m_j + offset[j]
  best = second = +inf, win = -1;  g_j < best: second = best, best = g_j, win = j;  else g_j < second: second = g_j
and then label = class_values[win], or 0 when win == -1 or m_win > max_dist2; dist2 = float32(m_win), margin =
float32(second - best), both NaN when win == -1 (and written whether or not the threshold zeroed the label); k == 1 leaves
second = +inf, so the margin is +inf.

The fma is kmeans_model_ref.fma64 (error-free transformations, one rounding).  Its transformations take finite operands:
where an operand is not finite (a plane holding +-inf) or the plain a * b + c already overflows, the plain IEEE value stands,
which is the fma's own value there except when a * b alone overflows and c brings the sum back into range (|c| near 1e308:
nothing here goes there)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from kmeans_model_ref import fma64



def tri(F: int) -> int:
    return F * (F + 1) // 2


def pack_lower(W) -> np.ndarray:
    """(k, F, F) lower-triangular matrices -> (k, F (F + 1) / 2) rows packed row-major."""
    W = np.asarray(W, np.float64)
    F = W.shape[-1]
    i, f = np.tril_indices(F)
    return np.ascontiguousarray(W[..., i, f])


def fma(a, b, c):
    """fma64 where a * b + c is finite (then every operand is), else the plain IEEE value (module docstring)."""
    a, b, c = (np.ascontiguousarray(v) for v in np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64),
                                                                  np.asarray(c, np.float64)))
    if a.size == 0:
        return a * b + c
    with np.errstate(all="ignore"):
        plain = a * b + c
        fin = np.isfinite(plain)
    if fin.all():
        return fma64(a, b, c)
    if fin.any():
        plain[fin] = fma64(a[fin], b[fin], c[fin])
    return plain


def _rows(d, plain_d, whiten_j, rows):
    """z_i of the given rows of one class: the fma chain over f = 0..i."""
    n = d[0].shape[0]
    out = []
    with np.errstate(all="ignore"):
        for i in rows:
            o = tri(i)
            z = np.zeros(n, np.float64)
            for f in range(i + 1):
                # fma(0, d, z) is z itself for a finite d (z is never -0: it starts at +0 and an exact cancellation gives
                # +0), so the zeros of a sparse W (the identity of 'mindist') are passed over
                if whiten_j[o + f] == 0.0 and plain_d[f]:
                    continue
                z = fma(whiten_j[o + f], d[f], z)
            out.append(z)
    return out


_pool = None
_WORKERS = max(1, min(8, os.cpu_count() or 1))
_RUN = 1 << 16   # pixels per task: shorter runs were slower (measured at 8192: the lock is held for a larger share of the time)


def quadratic_forms(X, mean, whiten) -> np.ndarray:
    """m[k][n]: the whitened quadratic form of every class at every pixel.  X (n, F) float32 or float64."""
    global _pool
    mean = np.asarray(mean, np.float64)
    k, F = mean.shape
    whiten = np.asarray(whiten, np.float64).reshape(k, tri(F))
    x = np.asarray(X).astype(np.float64)   # widening a float32 is exact
    x = np.ascontiguousarray(np.where(np.isnan(x), 0.0, x).reshape(-1, F).T)
    n = x.shape[1]
    out = np.zeros((k, n), np.float64)
    # the rows z_i of a class do not depend on one another: on a large case they are dealt to threads over whole-length
    # arrays (NumPy's loops release the interpreter lock; the longer the arrays the smaller the share of the time it is held)
    groups = [list(range(r, F, 2 * _WORKERS)) for r in range(min(F, 2 * _WORKERS))]
    threaded = _WORKERS > 1 and len(groups) > 1 and n * F >= 1 << 16
    if threaded and _pool is None:
        _pool = ThreadPoolExecutor(_WORKERS)
    with np.errstate(all="ignore"):
        for j in range(k if n else 0):
            d = [x[f] - mean[j, f] for f in range(F)]
            plain_d = [bool(np.isfinite(v).all()) for v in d]
            z = [np.empty(n, np.float64) for _ in range(F)]

            def work(t):
                g, s = t
                for i, zi in zip(g, _rows([v[s:s + _RUN] for v in d], plain_d, whiten[j], g)):
                    z[i][s:s + _RUN] = zi

            tasks = [(g, s) for s in range(0, n, _RUN) for g in groups]
            if threaded:
                list(_pool.map(work, tasks))
            else:
                for t in tasks:
                    work(t)
            m = np.zeros(n, np.float64)
            for i in range(F):
                m = fma(z[i], z[i], m)
            out[j] = m
    return out


def decide(m, offset, class_values, max_dist2=np.inf):
    """The arg-min over m[k][n] -> dict(labels uint8, dist2 float32, margin float32, win, g, best, second)."""
    m = np.asarray(m, np.float64)
    k, n = m.shape
    offset = np.asarray(offset, np.float64)
    cv = np.asarray(class_values, np.uint8)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    win = np.full(n, -1, np.int64)
    g = np.empty((k, n), np.float64)
    with np.errstate(all="ignore"):
        for j in range(k):
            g[j] = m[j] + offset[j]
            lt = g[j] < best
            lt2 = ~lt & (g[j] < second)
            second = np.where(lt, best, np.where(lt2, g[j], second))
            best = np.where(lt, g[j], best)
            win = np.where(lt, j, win)
        none = win < 0
        m_win = m[np.maximum(win, 0), np.arange(n)]
        labels = np.where(none | (m_win > max_dist2), 0, cv[np.maximum(win, 0)]).astype(np.uint8)
        dist2 = np.where(none, np.float32(np.nan), m_win.astype(np.float32)).astype(np.float32)
        margin = np.where(none, np.float32(np.nan), (second - best).astype(np.float32)).astype(np.float32)
    return dict(labels=labels, dist2=dist2, margin=margin, win=win, g=g, best=best, second=second, m=m)


def classify(X, mean, whiten, offset, class_values, max_dist2=np.inf):
    return decide(quadratic_forms(X, mean, whiten), offset, class_values, max_dist2)
