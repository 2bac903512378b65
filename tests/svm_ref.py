"""NumPy restatement of K28 (rsseg_svm_classify): one-vs-one support vector machine classification, in float64, every
operation one IEEE operation.

A model is a dict: offset[F], scale[F]; sv[S][F], the support vectors in scaled units grouped by class, classes ascending;
n_support[k]; coef[k - 1][S]; bias[P], P = k (k - 1) / 2; class_values[k] (uint8, distinct, 1..255); kernel 'rbf' | 'poly' |
'linear'; gamma, coef0, degree; w[P][F] for 'linear'.  Per pixel:
  x_f = the plane value widened to float64 (exact), a NaN read as 0; a pixel with any +-inf x_f gets label 0 and margin NaN
  z_f = (x_f - offset_f) * scale_f
  rbf:   q = +0; f ascending: d = z_f - sv_if, q = fma(d, d, q);  K_i = svm_exp(-(gamma * q))
  poly:  t = +0; f ascending: t = fma(sv_if, z_f, t);  u = fma(gamma, t, coef0);  K_i = u, then degree - 1 times K_i = K_i * u
  pairs p = (a, b), a < b, in the order (0,1), (0,2), ..., (k-2,k-1): s = +0; over class a's support vectors ascending
  s = fma(coef[b-1][i], K_i, s), then over class b's s = fma(coef[a][i], K_i, s);  d_p = s + bias_p.  No term is skipped.
  linear: d_p = (t = +0; f ascending: t = fma(w_pf, z_f, t)) + bias_p
  d_p > 0 votes a, anything else (a NaN too) votes b; label = the lowest class index with the most votes
  margin = float32(min |d_p| over the winner's pairs), m = +inf and |d_p| < m: m = |d_p|, so a NaN is never taken
svm_exp(t), t <= 0: t < -708 -> +0; n = rint(t LOG2E); r = fma(-n, LN2_HI, t); r = fma(-n, LN2_LO, r); p = c_13, j = 12 ... 0:
p = fma(p, r, c_j), c_j the double nearest 1 / j!; p * 2^n with 2^n built from its exponent field.

The fma is gaussian_ref.fma: kmeans_model_ref.fma64 (error-free transformations, one rounding) where a * b + c is finite,
the plain IEEE value where it is not (a poly kernel that overflowed: the fma's own value there)."""
import math

import numpy as np

from gaussian_ref import fma

LOG2E = np.array(0x3FF71547652B82FE, np.uint64).view(np.float64)[()]
LN2_HI = np.array(0x3FE62E42FEE00000, np.uint64).view(np.float64)[()]
LN2_LO = np.array(0x3DEA39EF35793C76, np.uint64).view(np.float64)[()]
EXP_C = [1.0 / math.factorial(j) for j in range(14)]   # an exact integer divided once: the double nearest 1 / j!


def svm_exp(t) -> np.ndarray:
    t = np.asarray(t, np.float64)
    shape = t.shape
    t = np.ascontiguousarray(t).reshape(-1)
    with np.errstate(all="ignore"):
        under = t < -708.0
        tc = np.where(under, -708.0, t)
        n = np.rint(tc * LOG2E)
        r = fma(-n, LN2_HI, tc)
        r = fma(-n, LN2_LO, r)
        p = np.full(t.shape, EXP_C[13])
        for j in range(12, -1, -1):
            p = fma(p, r, EXP_C[j])
        two_n = ((n.astype(np.int64) + 1023) << 52).view(np.float64)
        return np.where(under, 0.0, p * two_n).reshape(shape)


def pairs(k: int):
    return [(a, b) for a in range(k - 1) for b in range(a + 1, k)]


def _starts(n_support):
    return np.concatenate([[0], np.cumsum(np.asarray(n_support, np.int64))])


def scaled(X, model):
    """(z (n, F) float64 with the refused pixels' rows zeroed, refused (n,) bool)."""
    x = np.asarray(X).astype(np.float64)   # widening a float32 is exact
    x = np.where(np.isnan(x), 0.0, x)
    bad = np.isinf(x).any(axis=1)
    x[bad] = 0.0
    with np.errstate(all="ignore"):
        z = (x - np.asarray(model["offset"], np.float64)) * np.asarray(model["scale"], np.float64)
    return z, bad


def kernel_values(z, model) -> np.ndarray:
    """K[S][n] of the rbf and poly kernels."""
    sv = np.asarray(model["sv"], np.float64)
    S, F = sv.shape
    n = z.shape[0]
    s = np.zeros((S, n), np.float64)
    with np.errstate(all="ignore"):
        for f in range(F):
            if model["kernel"] == "rbf":
                d = z[None, :, f] - sv[:, f, None]
                s = fma(d, d, s)
            else:
                s = fma(sv[:, f, None], z[None, :, f], s)
        if model["kernel"] == "rbf":
            return svm_exp(-(float(model["gamma"]) * s))
        u = fma(float(model["gamma"]), s, float(model["coef0"]))
        K = u
        for _ in range(int(model["degree"]) - 1):
            K = K * u
        return K


def fold_linear(sv, n_support, coef) -> np.ndarray:
    """w[P][F]: per pair the fma chain, in the decision's order, of coef * sv_if."""
    sv, coef = np.asarray(sv, np.float64), np.asarray(coef, np.float64)
    st = _starts(n_support)
    k = len(n_support)
    w = np.zeros((k * (k - 1) // 2, sv.shape[1]), np.float64)
    for p, (a, b) in enumerate(pairs(k)):
        t = np.zeros(sv.shape[1], np.float64)
        for i in range(st[a], st[a + 1]):
            t = fma(coef[b - 1, i], sv[i], t)
        for i in range(st[b], st[b + 1]):
            t = fma(coef[a, i], sv[i], t)
        w[p] = t
    return w


def decisions(z, model, K=None) -> np.ndarray:
    """d[P][n].  K: kernel_values(z, model), computed when not given (unused by 'linear')."""
    k = len(model["n_support"])
    n = z.shape[0]
    bias = np.asarray(model["bias"], np.float64)
    out = np.zeros((k * (k - 1) // 2, n), np.float64)
    with np.errstate(all="ignore"):
        if model["kernel"] == "linear":
            w = np.asarray(model["w"], np.float64)
            t = np.zeros((w.shape[0], n), np.float64)
            for f in range(w.shape[1]):
                t = fma(w[:, f, None], z[None, :, f], t)
            return t + bias[:, None]
        if K is None:
            K = kernel_values(z, model)
        coef = np.asarray(model["coef"], np.float64)
        st = _starts(model["n_support"])
        for p, (a, b) in enumerate(pairs(k)):
            s = np.zeros(n, np.float64)
            for i in range(st[a], st[a + 1]):
                s = fma(coef[b - 1, i], K[i], s)
            for i in range(st[b], st[b + 1]):
                s = fma(coef[a, i], K[i], s)
            out[p] = s + bias[p]
    return out


def decide(d, class_values, bad=None):
    """The vote over d[P][n] -> dict(labels uint8, margin float32, win)."""
    d = np.asarray(d, np.float64)
    cv = np.asarray(class_values, np.uint8)
    k = cv.size
    n = d.shape[1]
    votes = np.zeros((k, n), np.int64)
    for p, (a, b) in enumerate(pairs(k)):
        pos = d[p] > 0
        votes[a] += pos
        votes[b] += ~pos
    win = np.argmax(votes, axis=0)   # the first of the largest
    m = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for p, (a, b) in enumerate(pairs(k)):
            ad = np.abs(d[p])
            take = ((win == a) | (win == b)) & (ad < m)
            m = np.where(take, ad, m)
        labels = cv[win]
        margin = m.astype(np.float32)
    if bad is not None:
        labels = np.where(bad, 0, labels).astype(np.uint8)
        margin = np.where(bad, np.float32(np.nan), margin).astype(np.float32)
    return dict(labels=labels, margin=margin, win=win)


def classify(X, model):
    """dict(labels, margin, win, d, K (None for 'linear'), bad) of the rows of X (n, F) float32 or float64."""
    z, bad = scaled(X, model)
    K = None if model["kernel"] == "linear" else kernel_values(z, model)
    d = decisions(z, model, K)
    return dict(decide(d, model["class_values"], bad), d=d, K=K, bad=bad)
