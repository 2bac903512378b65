"""NumPy / Python-int restatement of K29 (rsseg_gmm_sweep, include/rsseg.h), operation for operation, and of the EM loop of
rsseg/gmm.py with its rational M-step.

A pixel is counted when its mask byte is non-zero (mask None: all).
float32 planes: v_f = the value, NaN read as +0; u_f = v_f * 2^plane_exp[f] in float64 (exact); a counted pixel with any
|u_f| > 1 (+-inf included) is left out; QM = Q.  uint8 planes: u_f = v_f (plane_exp None), QM = 0, no pixel is left out for
its values.
The model is in u units, K22's layout (gaussian_ref): mean[k][F], whiten[k][F (F + 1) / 2], offset[k]; diag: W_j diagonal.
Per counted pixel that is not left out, in float64:
  g_j = gaussian_ref.quadratic_forms(u)[j] + offset[j], j ascending (diag: the off-diagonal of W zeroed; the zeros that
        gaussian_ref._rows skips are bit-neutral)
  best = +inf;  g_j < best: best = g_j, win = j;  best not finite: the pixel is left out
  e_j = svm_ref.svm_exp(-0.5 * (g_j - best));  s = +0, j ascending: s = s + e_j;  r_j = e_j / s;  q_j = rint(r_j * 2^20)
  ll = fma(-0.5, best, gmm_log(s))
  row j, where q_j != 0:  column 0 += q_j;  column 1 + f += rint(q_j u_f 2^QM);
     full: column 1 + F + tri(a, b) += rint(q_j u_a u_b 2^QM), a <= b row-major;  diag: column 1 + F + f += rint(q_j u_f u_f 2^QM)
  each term one rounding to nearest-even of the exact product: fma(q_j u_a 2^QM, u_b, 1.5 * 2^52) with the constant taken off as
  integers (common.h's fx_bits), the fma being kmeans_model_ref.fma64 (one rounding)
  n_counted += 1;  |ll| < 2^20: ll_sum += rint(ll * 2^Q), else n_far += 1
labels = win + 1, posterior = float32(r_win), loglik = float32(ll), proba[j] = float32(r_j); 0, NaN, NaN, NaN elsewhere.
The sums are Python ints."""
import math
from fractions import Fraction

import numpy as np

from gaussian_ref import fma, quadratic_forms, tri
from svm_ref import LN2_HI, LN2_LO, svm_exp

QBITS = 20
FX_MAGIC = 6755399441055744.0   # 1.5 * 2^52


def _f64(bits: int) -> float:
    return float(np.array(bits, np.uint64).view(np.float64)[()])


SQRT2 = _f64(0x3FF6A09E667F3BCD)
LG = [_f64(b) for b in (0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF, 0x3FC7466496CB03DE,
                        0x3FC39A09D078C69F, 0x3FC2F112DF3E5244)]


def n_columns(F: int, diag: bool) -> int:
    return 1 + 2 * F if diag else 1 + F + tri(F)


def gmm_log(s) -> np.ndarray:
    """ln(s), s in [1, 64]: the contract's sequence of float64 operations."""
    s = np.ascontiguousarray(np.asarray(s, np.float64))
    shape = s.shape
    s = s.reshape(-1)
    bits = s.view(np.int64)
    e = (bits >> 52) - 1023
    m = ((bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000).view(np.float64)
    big = m > SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    f = m - 1.0
    t = f / (2.0 + f)
    z = t * t
    R = np.full(s.shape, LG[6])
    for i in range(5, -1, -1):
        R = fma(R, z, LG[i])
    R = R * z
    hfsq = (0.5 * f) * f
    dk = e.astype(np.float64)
    return (dk * LN2_HI - ((hfsq - (t * (hfsq + R) + dk * LN2_LO)) - f)).reshape(shape)


def fx_term(x, y) -> np.ndarray:
    """rint(x * y) as int64, one rounding of the exact product (|x y| < 2^51): fma(x, y, 1.5 * 2^52) less the constant, as integers."""
    magic = np.array(FX_MAGIC).view(np.int64)[()]
    return fma(x, y, FX_MAGIC).view(np.int64) - magic


def diag_only(whiten, F: int) -> np.ndarray:
    """The packed rows with everything but the diagonal zeroed."""
    w = np.array(whiten, np.float64).reshape(-1, tri(F))
    keep = np.zeros(tri(F), bool)
    keep[[tri(i) + i for i in range(F)]] = True
    return np.where(keep, w, 0.0)


def scaled(planes, mask, plane_exp):
    """(u (F, n) float64, counted (n,), out_of_range (n,), QM is Q) of the planes; uint8: u = v."""
    planes = np.asarray(planes)
    F, n = planes.shape
    counted = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if planes.dtype == np.uint8:
        assert plane_exp is None
        return planes.astype(np.float64), counted, np.zeros(n, bool)
    assert planes.dtype == np.float32
    x = planes.astype(np.float64)
    x[np.isnan(x)] = 0.0
    with np.errstate(over="ignore"):
        u = np.ldexp(x, np.asarray(plane_exp, np.int64).reshape(F, 1))
    return u, counted, np.any(~(np.abs(u) <= 1.0), axis=0)


def sweep_ref(planes, mask, plane_exp, Q, mean, whiten, offset, diag=False, want_table=True):
    """planes (F, n) float32 or uint8 -> dict(table: k rows of Python ints (None without want_table), n_counted, n_left_out,
    n_far, ll_sum, labels uint8 (n,), posterior, loglik float32 (n,), proba float32 (k, n), q int64 (k, n), r, ll float64)."""
    planes = np.asarray(planes)
    F, n = planes.shape
    mean = np.asarray(mean, np.float64)
    k = mean.shape[0]
    offset = np.asarray(offset, np.float64).reshape(k)
    whiten = np.asarray(whiten, np.float64).reshape(k, tri(F))
    u8 = planes.dtype == np.uint8
    assert 1 <= k <= 32 and 1 <= F <= 64 and 0 <= Q <= 30 and n <= 2 ** (42 - Q) and (not u8 or n <= 2 ** 26)
    u, counted, out_of_range = scaled(planes, mask, plane_exp)
    keep = np.flatnonzero(counted & ~out_of_range)
    uk = u[:, keep]
    with np.errstate(all="ignore"):
        m = quadratic_forms(np.ascontiguousarray(uk.T), mean, diag_only(whiten, F) if diag else whiten)
        g = m + offset[:, None]
        best = np.full(keep.size, np.inf)
        win = np.full(keep.size, -1, np.int64)
        for j in range(k):
            lt = g[j] < best
            best = np.where(lt, g[j], best)
            win = np.where(lt, j, win)
        fin = np.isfinite(best)
    n_left = int((counted & out_of_range).sum()) + int((~fin).sum())
    keep, uk, g, best, win = keep[fin], uk[:, fin], g[:, fin], best[fin], win[fin]
    nk = keep.size
    e = np.stack([svm_exp(-0.5 * (g[j] - best)) for j in range(k)]) if nk else np.zeros((k, 0))
    s = np.zeros(nk)
    for j in range(k):
        s = s + e[j]
    r = e / s if nk else e
    q = np.rint(r * float(1 << QBITS)).astype(np.int64)
    ll = fma(-0.5, best, gmm_log(s)) if nk else np.zeros(0)
    near = np.abs(ll) < 2.0 ** 20
    ll_sum = sum(int(v) for v in fx_term(ll[near], float(2 ** Q))) if near.any() else 0
    table = None
    if want_table:
        two_qm = 1.0 if u8 else float(2 ** Q)
        y = np.vstack([uk, np.ones((1, nk))])   # row F: the ones of the first moments
        if diag:
            ca = list(range(F)) + list(range(F))
            cb = [F] * F + list(range(F))
        else:
            a, b = np.triu_indices(F)
            ca = list(range(F)) + a.tolist()
            cb = [F] * F + b.tolist()
        table = []
        for j in range(k):
            sel = q[j] != 0
            row = [0] * n_columns(F, diag)
            if sel.any():
                qj = q[j, sel].astype(np.float64)
                ys = y[:, sel]
                row[0] = int(q[j, sel].sum())
                for c, (ai, bi) in enumerate(zip(ca, cb)):
                    row[1 + c] = int(fx_term(qj * (ys[ai] * two_qm), ys[bi]).sum())   # < 2^62: the int64 sum is the exact one
            table.append(row)
    labels = np.zeros(n, np.uint8)
    posterior = np.full(n, np.nan, np.float32)
    loglik = np.full(n, np.nan, np.float32)
    proba = np.full((k, n), np.nan, np.float32)
    labels[keep] = win + 1
    if nk:
        posterior[keep] = r[win, np.arange(nk)].astype(np.float32)
        loglik[keep] = ll.astype(np.float32)
        proba[:, keep] = r.astype(np.float32)
    return dict(table=table, n_counted=nk, n_left_out=n_left, n_far=int((~near).sum()), ll_sum=ll_sum, labels=labels, posterior=posterior,
                loglik=loglik, proba=proba, q=q, r=r, ll=ll, keep=keep)


def table_array(table) -> np.ndarray:
    return np.array(table, dtype=np.int64).reshape(len(table), -1)


def ref_sweep(planes, model, mask=None, want_table=True, want_labels=False, want_posterior=False, want_loglik=False, want_proba=False):
    """Context.gmm_sweep's signature on host arrays: what GaussianMixtureModel.fit(..., sweep=ref_sweep) runs without a GPU."""
    P = np.stack([np.asarray(p).reshape(-1) for p in planes])
    o = sweep_ref(P, mask, model.get("plane_exp"), int(model["Q"]), model["mean"], model["whiten"], model["offset"], bool(model.get("diag", False)),
                  want_table)
    return dict(table=table_array(o["table"]) if want_table else None, labels=o["labels"] if want_labels else None,
                posterior=o["posterior"] if want_posterior else None, loglik=o["loglik"] if want_loglik else None,
                proba=o["proba"] if want_proba else None, n_counted=o["n_counted"], n_left_out=o["n_left_out"], n_far=o["n_far"], ll_sum=o["ll_sum"])


# ---- the M-step and the EM loop, restated ---------------------------------------------------------------------------------
def cholesky_whiten(cov):
    """(W = L^-1 lower triangular, ln |cov|): the Cholesky-Banachiewicz rows, then forward substitution column by column, every
    sum taken in index order in plain float64."""
    F = len(cov)
    L = [[0.0] * F for _ in range(F)]
    for i in range(F):
        for j in range(i + 1):
            s = float(cov[i][j])
            for p in range(j):
                s = s - L[i][p] * L[j][p]
            if i == j:
                if not s > 0.0:
                    raise ValueError("not positive definite")
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    W = [[0.0] * F for _ in range(F)]
    for c in range(F):
        for i in range(c, F):
            s = 1.0 if i == c else 0.0
            for p in range(c, i):
                s = s - L[i][p] * W[p][c]
            W[i][c] = s / L[i][i]
    logdet = 0.0
    for i in range(F):
        logdet = logdet + math.log(L[i][i])
    return np.array(W), 2.0 * logdet


def m_step_ref(rows, F, QM, plane_exp, diag_table, covariance_type, reg_covar):
    """The rows of a sweep table (Python ints) -> (kept row indices, weights, means (k', F), covariances (k', F, F)) in feature
    units x_f = u_f 2^-plane_exp[f].  With N = column 0, S_f and S_ab the moment columns:
      weight = N / sum N;  mean_f = S_f / (N 2^QM) 2^-e_f;  c_ab = (S_ab / (N 2^QM) - S_a S_b / (N 2^QM)^2) 2^-(e_a + e_b)
      full: c + reg I;  tied: sum_j N_j c_j / sum_j N_j + reg I;  diag: diag(c) + reg;  spherical: mean(diag(c)) + reg
    as scikit-learn derives them, in exact rationals, every entry rounded to float64 once.  A row with N = 0 is dropped."""
    e = [int(v) for v in plane_exp]
    kept = [j for j, row in enumerate(rows) if row[0] > 0]
    tot = sum(rows[j][0] for j in kept)
    tri_pos, p = {}, 0
    for x in range(F):
        for y in range(x, F):
            tri_pos[(x, y)] = p
            p += 1
    only_diag = diag_table or covariance_type in ("diag", "spherical")
    weights, means, covs = [], [], []
    for j in kept:
        N = rows[j][0]
        S = rows[j][1:1 + F]
        P = rows[j][1 + F:]
        den = N * 2 ** QM
        weights.append(float(Fraction(N, tot)))
        means.append([float(Fraction(S[f], den) * Fraction(2) ** -e[f]) for f in range(F)])
        c = [[Fraction(0)] * F for _ in range(F)]
        for x in range(F):
            for y in ([x] if only_diag else range(x, F)):
                sab = P[x] if diag_table else P[tri_pos[(x, y)]]
                c[x][y] = c[y][x] = (Fraction(sab, den) - Fraction(S[x] * S[y], den * den)) * Fraction(2) ** -(e[x] + e[y])
        covs.append(c)
    if covariance_type == "tied":
        t = [[sum(rows[j][0] * c[x][y] for j, c in zip(kept, covs)) / tot for y in range(F)] for x in range(F)]
        covs = [t for _ in kept]
    if covariance_type == "spherical":
        covs = [[[sum(c[f][f] for f in range(F)) / F if x == y else Fraction(0) for y in range(F)] for x in range(F)] for c in covs]
    reg = Fraction(float(reg_covar))
    out = np.zeros((len(kept), F, F))
    for i, c in enumerate(covs):
        for x in range(F):
            for y in range(F):
                out[i, x, y] = float(c[x][y] + reg) if x == y else float(c[x][y])
    return kept, np.array(weights), np.array(means).reshape(len(kept), F), out


def pack_lower(W) -> np.ndarray:
    W = np.asarray(W, np.float64)
    i, f = np.tril_indices(W.shape[-1])
    return np.ascontiguousarray(W[..., i, f])


def kernel_model_ref(weights, means, covs, plane_exp, Q, covariance_type) -> dict:
    """The model in u units: mean 2^e, cov 2^(e_a + e_b) (exact), W and ln |S| by cholesky_whiten, offset = ln |S| - 2 ln w."""
    k, F = means.shape
    e = np.zeros(F, np.int64) if plane_exp is None else np.asarray(plane_exp, np.int64)
    diag = covariance_type in ("diag", "spherical")
    W, offset = np.zeros((k, F, F)), np.zeros(k)
    for j in range(k):
        cu = np.ldexp(covs[j], e[:, None] + e[None, :])
        if diag:
            cu = np.diag(np.diag(cu))
        W[j], logdet = cholesky_whiten(cu)
        offset[j] = logdet - 2.0 * math.log(weights[j])
    return dict(mean=np.ldexp(means, e[None, :]), whiten=pack_lower(W), offset=offset, plane_exp=None if plane_exp is None else e, Q=int(Q), diag=diag)


def q_for(n: int) -> int:
    return min(30, 42 - (max(int(n), 1) - 1).bit_length())


def em_ref(planes, mask, plane_exp, weights, means, covs, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100):
    """The EM loop from explicit parameters (weights (k,), means (k, F), covs (k, F, F), feature units) over planes (F, n):
    per iteration one sweep_ref, the lower bound ll_sum / 2^Q / n_counted, m_step_ref; stop when the bound moved by less than tol
    (scikit-learn's rule) or after max_iter.  -> dict(weights, means, covs, n_iter, converged, tables, bounds, labels)."""
    planes = np.asarray(planes)
    F, n = planes.shape
    u8 = planes.dtype == np.uint8
    Q = q_for(n)
    e = np.zeros(F, np.int64) if u8 else np.asarray(plane_exp, np.int64)
    diag = covariance_type in ("diag", "spherical")
    weights, means, covs = np.asarray(weights, np.float64), np.asarray(means, np.float64), np.asarray(covs, np.float64)
    tables, bounds = [], []
    prev, converged = -math.inf, False
    for it in range(1, max_iter + 1):
        km = kernel_model_ref(weights, means, covs, None if u8 else e, Q, covariance_type)
        o = sweep_ref(planes, mask, km["plane_exp"], Q, km["mean"], km["whiten"], km["offset"], diag)
        tables.append(o["table"])
        lb = float(Fraction(o["ll_sum"], o["n_counted"] * 2 ** Q))
        bounds.append(lb)
        _, weights, means, covs = m_step_ref(o["table"], F, 0 if u8 else Q, e, diag, covariance_type, reg_covar)
        if abs(lb - prev) < tol:
            converged = True
            break
        prev = lb
    km = kernel_model_ref(weights, means, covs, None if u8 else e, Q, covariance_type)
    o = sweep_ref(planes, mask, km["plane_exp"], Q, km["mean"], km["whiten"], km["offset"], diag, want_table=False)
    return dict(weights=weights, means=means, covs=covs, n_iter=it, converged=converged, tables=tables, bounds=bounds, labels=o["labels"],
                n_left_out=o["n_left_out"])
