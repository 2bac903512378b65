"""
Gaussian mixture clustering (K29, csrc/k29_gmm.hip; no counterpart in the reference): the unsupervised Gaussian classifier,
fitted by expectation-maximisation.  Every iteration is ONE pass over the raster on the GPU (Context.gmm_sweep: every
component's density at every pixel, the responsibilities, and every component's weighted count, sum and sum of products as
exact integers); the M-step happens here, in rational arithmetic on the k x columns table, rounded to float64 once.  There is
no per-pixel host work and, past the initial label map, no random number.

  GaussianMixtureModel(n_components=, covariance_type=, ...).fit(features)  ->  GMMResult(labels, model, weights, history, n_left_out)
  predict / predict_proba / score_samples / score / bic / aic               one sweep without a table each
  save / load                                                               an .npz of plain arrays, no pickle
  to_sklearn / from_sklearn, to_gaussian_classifier                         the same mixture as a GaussianMixture / a K22 'ml' model
  select_components(features, ks)                                           fits each k, returns the BIC / AIC table and the best model

The kernel works in u units, u_f = x_f 2^plane_exp[f] in [-1, 1] (K24's fixed point); weights_, means_ and covariances_ are kept
in feature units and are what scikit-learn would call them.  A power of two moves between the two exactly.

The M-step, per component j with N_j = sum q (a component with N_j = 0 is dropped and recorded in the history):
  weight_j = N_j / sum_j N_j;  mean_jf = S_f / (N_j 2^QM) 2^-e_f;  cov_jab = (S_ab / (N_j 2^QM) - mean mean) 2^-(e_a + e_b)
  'full': cov_j + reg_covar I;  'tied': sum_j N_j cov_j / sum_j N_j + reg_covar I;  'diag': the diagonal + reg_covar;
  'spherical': the mean of the diagonal + reg_covar         (scikit-learn's derivations), all exact, rounded once.
Stopping: scikit-learn's rule, |change of ll_sum / 2^Q / n_counted| < tol after an M-step, or max_iter.
"""
from __future__ import annotations

import json
import math
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

from . import isodata as ISO
from . import signatures as SIG
from .gaussian import pack_lower

COVARIANCE_TYPES = ("full", "tied", "diag", "spherical")
MAX_COMPONENTS = 32
MAX_FEATURES = 64
QBITS = 20
Q_CAP = 30
FORMAT_VERSION = 1
_FORMAT_NAME = "rsseg.GaussianMixtureModel"
LN_2PI = math.log(2.0 * math.pi)


def q_for(n_total: int) -> int:
    """Q = min(30, 42 - ceil(log2(n))): no term passes 2^50 and no sum 2^62."""
    n_total = max(int(n_total), 1)
    return min(Q_CAP, 42 - (n_total - 1).bit_length())


def check_q(Q: int, n: int, u8: bool = False):
    """The limits rsseg_gmm_sweep sets, checked before a raster goes to the device: Q, and 2^26 pixels of uint8 planes."""
    if not 0 <= int(Q) <= min(Q_CAP, 42 - (max(int(n), 1) - 1).bit_length()):
        raise ValueError(f"gmm: Q={Q} is outside 0 ... min(30, 42 - ceil(log2 n)) for n={n} pixels")
    if u8 and int(n) > 1 << 26:
        raise ValueError(f"gmm: {n} uint8 pixels in one call, at most 2^26 (the sums of q u u would pass 2^62)")


def n_columns(F: int, diag: bool) -> int:
    return 1 + 2 * F if diag else 1 + F + F * (F + 1) // 2


def n_parameters(k: int, F: int, covariance_type: str) -> int:
    """The free parameters scikit-learn counts: covariances, means, weights."""
    cov = {"full": k * F * (F + 1) // 2, "diag": k * F, "tied": F * (F + 1) // 2, "spherical": k}[covariance_type]
    return int(cov + k * F + k - 1)


def cholesky_whiten(cov, what: str = "a component", diag: bool = False):
    """(W = L^-1 lower triangular, ln |cov|) of a covariance by one fixed-order routine: the Cholesky-Banachiewicz rows, then
    forward substitution column by column, every sum in index order in plain float64.  diag: the same operations on the
    diagonal alone.  ValueError naming `what` when the matrix is not positive definite."""
    cov = np.asarray(cov, np.float64)
    F = cov.shape[0]
    bad = ValueError(f"gmm: the covariance of {what} is not positive definite (constant or linearly dependent features, or a "
                     f"collapsed component: raise reg_covar)")
    if not np.all(np.isfinite(cov)):
        raise bad
    L = [[0.0] * F for _ in range(F)]
    W = [[0.0] * F for _ in range(F)]
    c = cov.tolist()
    if diag:
        for i in range(F):
            if not c[i][i] > 0.0:
                raise bad
            L[i][i] = math.sqrt(c[i][i])
            W[i][i] = 1.0 / L[i][i]
    else:
        for i in range(F):
            for j in range(i + 1):
                s = c[i][j]
                for p in range(j):
                    s = s - L[i][p] * L[j][p]
                if i == j:
                    if not s > 0.0:
                        raise bad
                    L[i][i] = math.sqrt(s)
                else:
                    L[i][j] = s / L[j][j]
        for col in range(F):
            for i in range(col, F):
                s = 1.0 if i == col else 0.0
                for p in range(col, i):
                    s = s - L[i][p] * W[p][col]
                W[i][col] = s / L[i][i]
    logdet = 0.0
    for i in range(F):
        logdet = logdet + math.log(L[i][i])
    W = np.array(W, np.float64).reshape(F, F)
    if not (np.all(np.isfinite(W)) and math.isfinite(logdet)):
        raise bad
    return W, 2.0 * logdet


def m_step(rows, F: int, QM: int, plane_exp, diag_table: bool, covariance_type: str, reg_covar: float):
    """The rows of a table (Python ints; K29's columns, or K24's with weight 1) -> (kept row indices, weights (k',), means
    (k', F), covariances (k', F, F)) in feature units; see the module text."""
    e = [int(v) for v in plane_exp]
    kept = [j for j, row in enumerate(rows) if row[0] > 0]
    if not kept:
        raise ValueError("gmm: no pixel carries any weight (every pixel masked, left out or out of the model's range)")
    tot = sum(rows[j][0] for j in kept)
    a, b = np.triu_indices(F)
    pos = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(a, b))}
    reg = Fraction(float(reg_covar))
    pairs = [(x, x) for x in range(F)] if (diag_table or covariance_type in ("diag", "spherical")) else [(x, y) for x in range(F) for y in range(x, F)]
    weights, means, covs = [], [], []
    for j in kept:
        row = rows[j]
        den = row[0] << QM
        mu = [Fraction(row[1 + f], den) for f in range(F)]
        weights.append(float(Fraction(row[0], tot)))
        means.append([float(mu[f] / Fraction(2) ** e[f]) for f in range(F)])
        c = {}
        for x, y in pairs:
            sab = row[1 + F + (x if diag_table else pos[(x, y)])]
            c[(x, y)] = (Fraction(sab, den) - mu[x] * mu[y]) / Fraction(2) ** (e[x] + e[y])
        covs.append(c)
    if covariance_type == "tied":
        t = {p: sum(Fraction(rows[j][0]) * c[p] for j, c in zip(kept, covs)) / tot for p in pairs}
        covs = [t] * len(kept)
    elif covariance_type == "spherical":
        covs = [{(x, x): sum(c.values()) / F for x in range(F)} for c in covs]
    out = np.zeros((len(kept), F, F))
    for i, c in enumerate(covs):
        for (x, y), v in c.items():
            out[i, x, y] = out[i, y, x] = float(v + reg if x == y else v)
    return kept, np.array(weights, np.float64), np.array(means, np.float64).reshape(len(kept), F), out


def kernel_model(weights, means, covs, plane_exp, Q: int, covariance_type: str) -> dict:
    """What Context.gmm_sweep takes: mean, whiten, offset in u units, plane_exp (None for uint8 planes), Q, diag."""
    weights = np.asarray(weights, np.float64).reshape(-1)
    k, F = means.shape
    e = np.zeros(F, np.int64) if plane_exp is None else np.asarray(plane_exp, np.int64)
    diag = covariance_type in ("diag", "spherical")
    mean_u = np.ldexp(np.asarray(means, np.float64), e[None, :])
    cov_u = np.ldexp(np.asarray(covs, np.float64), (e[:, None] + e[None, :])[None])
    W = np.zeros((k, F, F))
    offset = np.zeros(k)
    for j in range(k):
        if j == 0 or covariance_type != "tied":   # tied: one matrix, one call of the routine
            Wj, logdet = cholesky_whiten(cov_u[j], f"component {j}", diag)
        W[j] = Wj
        if not weights[j] > 0.0:
            raise ValueError(f"gmm: the weight of component {j} is not positive")
        offset[j] = logdet - 2.0 * math.log(weights[j])
    return dict(mean=mean_u, whiten=pack_lower(W), offset=offset, plane_exp=None if plane_exp is None else e, Q=int(Q), diag=diag)


def _rows(table):
    t = table.cpu().numpy() if hasattr(table, "data_ptr") else np.asarray(table)
    return [[int(v) for v in row] for row in t]


def _hard_table_host(planes, labels, k: int, plane_exp, Q: int, mask):
    """K24's table (tests/moments_ref.py) of a host label map, for the host sweep: rows 0 ... k - 1, Python ints."""
    P = np.stack([np.asarray(p).reshape(-1) for p in planes])
    F, n = P.shape
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    counted = (lab >= 0) & (lab < k)
    if mask is not None:
        counted &= np.asarray(mask).reshape(-1) != 0
    if P.dtype == np.uint8:
        u = P.astype(np.float64)
    else:
        x = P.astype(np.float64)
        x[np.isnan(x)] = 0.0
        with np.errstate(over="ignore"):
            u = np.ldexp(x, np.asarray(plane_exp, np.int64).reshape(F, 1))
        counted &= np.all(np.abs(u) <= 1.0, axis=0)
    a, b = np.triu_indices(F)
    two_q = float(2 ** Q)
    rows = []
    for j in range(k):
        uj = u[:, counted & (lab == j)]
        rows.append([int(uj.shape[1])] + [int(v) for v in np.rint(uj * two_q).astype(np.int64).sum(axis=1)] +
                    [int(v) for v in np.rint((uj[a] * two_q) * uj[b]).astype(np.int64).sum(axis=1)])
    return rows


class GMMResult(NamedTuple):
    labels: object        # uint8, component + 1, 0 = not counted or left out: a host array of the planes' shape, or a flat device plane
    model: "GaussianMixtureModel"
    weights: np.ndarray   # float64 (k,)
    history: list         # per iteration: dict(lower_bound, n_far, weights, dropped)
    n_left_out: int       # counted pixels beyond the ranges, or with no finite density


class GaussianMixtureModel:
    """GaussianMixtureModel(n_components=, covariance_type='full' | 'tied' | 'diag' | 'spherical', tol=1e-3, reg_covar=1e-6,
    max_iter=100, init='kmeans' | 'isodata' | a label array (0 ... k - 1; anything else labels nothing) | (weights, means,
    covariances), random_state=).  Fitted: weights_ (k,), means_ (k, F), covariances_ (scikit-learn's shape for the type), in
    feature units; plane_exp_, dtype_, converged_, n_iter_, lower_bound_ (the mean log-likelihood, constants included),
    history_.  init='isodata' runs rsseg.isodata with k_target = k_max = n_components: where it settles on fewer clusters, the
    components left without one are dropped (history_[0]['dropped']) and n_components shrinks."""

    def __init__(self, n_components: int = 1, covariance_type: str = "full", tol: float = 1e-3, reg_covar: float = 1e-6, max_iter: int = 100,
                 init="kmeans", random_state: Optional[int] = None):
        n_components = int(n_components)
        if not 1 <= n_components <= MAX_COMPONENTS:
            raise ValueError(f"GaussianMixtureModel: n_components={n_components}, must be 1 ... {MAX_COMPONENTS}")
        if covariance_type not in COVARIANCE_TYPES:
            raise ValueError(f"GaussianMixtureModel: covariance_type {covariance_type!r}, must be one of {COVARIANCE_TYPES}")
        if not (math.isfinite(float(tol)) and float(tol) >= 0.0):
            raise ValueError(f"GaussianMixtureModel: tol={tol!r}, must be finite and >= 0")
        if not (math.isfinite(float(reg_covar)) and float(reg_covar) >= 0.0):
            raise ValueError(f"GaussianMixtureModel: reg_covar={reg_covar!r}, must be finite and >= 0")
        if int(max_iter) < 1:
            raise ValueError(f"GaussianMixtureModel: max_iter={max_iter}, must be >= 1")
        if isinstance(init, str) and init not in ("kmeans", "isodata"):
            raise ValueError(f"GaussianMixtureModel: init {init!r}, must be 'kmeans', 'isodata', a label array or (weights, means, covariances)")
        self.n_components, self.covariance_type = n_components, covariance_type
        self.tol, self.reg_covar, self.max_iter = float(tol), float(reg_covar), int(max_iter)
        self.init, self.random_state = init, random_state

    # ---- the parameters ---------------------------------------------------------------------------------------------------
    def _check_fitted(self):
        if not hasattr(self, "means_"):
            raise ValueError("GaussianMixtureModel: not fitted (fit, from_params, from_sklearn or load first)")

    @property
    def n_features_in_(self) -> int:
        return int(self.means_.shape[1])

    @property
    def covariances_(self) -> np.ndarray:
        c = self._cov
        if self.covariance_type == "full":
            return c.copy()
        if self.covariance_type == "tied":
            return c[0].copy()
        d = np.diagonal(c, axis1=1, axis2=2)
        return d.copy() if self.covariance_type == "diag" else d[:, 0].copy()

    @staticmethod
    def _full_cov(cov, k: int, F: int, covariance_type: str) -> np.ndarray:
        cov = np.asarray(cov, np.float64)
        want = {"full": (k, F, F), "tied": (F, F), "diag": (k, F), "spherical": (k,)}[covariance_type]
        if cov.shape != want:
            raise ValueError(f"GaussianMixtureModel: covariances {cov.shape}, '{covariance_type}' over {k} components and {F} features is {want}")
        if covariance_type == "full":
            return cov.copy()
        if covariance_type == "tied":
            return np.repeat(cov[None], k, axis=0)
        out = np.zeros((k, F, F))
        idx = np.arange(F)
        out[:, idx, idx] = cov if covariance_type == "diag" else cov[:, None]
        return out

    def _set(self, weights, means, cov_full, plane_exp, dtype: str):
        self.weights_ = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self.means_ = np.ascontiguousarray(means, dtype=np.float64)
        self._cov = np.ascontiguousarray(cov_full, dtype=np.float64)
        self.plane_exp_ = None if plane_exp is None else np.ascontiguousarray(plane_exp, dtype=np.int64).reshape(-1)
        self.dtype_ = dtype
        self.n_components = int(self.weights_.size)

    @classmethod
    def from_params(cls, weights, means, covariances, covariance_type: str = "full", plane_exp=None, dtype: str = "float32", **kw):
        """A model from weights (k,), means (k, F) and covariances (scikit-learn's shape for the type), in feature units.
        plane_exp: the exponents predictions scale the planes by (default: from every raster's own extrema)."""
        means = np.array(means, dtype=np.float64, ndmin=2)
        k, F = means.shape
        weights = np.asarray(weights, np.float64).reshape(-1)
        if weights.size != k or not np.all(np.isfinite(weights)) or np.any(weights <= 0) or abs(weights.sum() - 1.0) > 1e-8:
            raise ValueError(f"GaussianMixtureModel: weights must be {k} positive probabilities that sum to 1")
        if F > MAX_FEATURES:
            raise ValueError(f"GaussianMixtureModel: {F} features, at most {MAX_FEATURES}")
        if dtype not in ("float32", "uint8"):
            raise ValueError(f"GaussianMixtureModel: dtype {dtype!r}, must be 'float32' or 'uint8'")
        self = cls(n_components=k, covariance_type=covariance_type, **kw)
        full = cls._full_cov(covariances, k, F, covariance_type)
        kernel_model(weights, means, full, None, 0, covariance_type)   # refuses a covariance that is not positive definite
        self._set(weights, means, full, plane_exp, dtype)
        self.converged_, self.n_iter_, self.lower_bound_, self.history_ = False, 0, float("nan"), []
        return self

    # ---- the raster ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _raster(features, mask, ctx, sweep):
        if not isinstance(features, np.ndarray) and len(features) > 0:
            kinds = {("uint8" if "uint8" in str(p.dtype) else "float") for p in features}
            if len(kinds) > 1:
                raise ValueError("gmm: planes must all be float32 or all uint8, not a mixture of the two")
        r = ISO._Raster(features, mask, ctx, sweep, name="gmm", device_sweep="gmm_sweep")
        check_q(q_for(r.n), r.n, r.u8)
        return r

    @staticmethod
    def _exponents(r, ranges):
        if r.u8:
            return None
        if ranges is None:
            rg = r.extrema()
        else:
            rg = np.asarray(ranges, np.float64)
            if rg.shape != (r.F, 2) or not np.all(np.isfinite(rg)):
                raise ValueError(f"gmm: ranges must be {r.F} finite (lo, hi) pairs")
        return np.array([SIG.exponent_for(m) for m in np.abs(rg).max(axis=1)], np.int64)

    def _const(self, plane_exp) -> float:
        """What turns the kernel's ll (u units, no 2 pi) into a log-density in feature units."""
        F = self.n_features_in_
        return -0.5 * F * LN_2PI + (0.0 if plane_exp is None else math.log(2.0) * float(np.sum(plane_exp)))

    def _kernel_model(self, r, ranges=None):
        self._check_fitted()
        if r.F != self.n_features_in_:
            raise ValueError(f"GaussianMixtureModel: {r.F} planes, the model has {self.n_features_in_} features")
        if ("uint8" if r.u8 else "float32") != self.dtype_:
            raise ValueError(f"GaussianMixtureModel: {'uint8' if r.u8 else 'float32'} planes, the model is for {self.dtype_} planes")
        pe = None if r.u8 else (self.plane_exp_ if (self.plane_exp_ is not None and ranges is None) else self._exponents(r, ranges))
        return kernel_model(self.weights_, self.means_, self._cov, pe, q_for(r.n), self.covariance_type), pe

    # ---- fitting ------------------------------------------------------------------------------------------------------------
    def _initial(self, r, pe):
        k, F = self.n_components, r.F
        init = self.init
        if isinstance(init, tuple) and len(init) == 3:
            w, mu, cov = init
            mu = np.array(mu, dtype=np.float64, ndmin=2)
            if mu.shape != (k, F):
                raise ValueError(f"gmm: init means {mu.shape}, {k} components over {F} planes are {(k, F)}")
            w = np.asarray(w, np.float64).reshape(-1)
            if w.size != k or np.any(~(w > 0)) or abs(w.sum() - 1.0) > 1e-8:
                raise ValueError(f"gmm: init weights must be {k} positive probabilities that sum to 1")
            return w, mu, self._full_cov(cov, k, F, self.covariance_type), []
        if isinstance(init, str):
            if not r.on_device:
                raise ValueError(f"gmm: init {init!r} runs on the GPU; a host sweep takes a label array or explicit parameters")
            torch = __import__("torch")
            if init == "kmeans":
                from .kmeans_model import KMeansModel
                planes = r.planes if not r.u8 else [p.to(torch.float32) for p in r.planes]
                seed = 42 if self.random_state is None else int(self.random_state)
                _, lab = KMeansModel.fit(planes, k, seed=seed, ctx=r.ctx, mask=r.mask)
                lab = torch.where(lab < 0, torch.full_like(lab, 255), lab).to(torch.uint8)
            else:
                # k_max = k: ISODATA never returns more clusters than components; where it settles on fewer, the components
                # without a cluster are dropped and recorded like any component without weight
                lab = ISO.isodata(r.planes, k_target=k, k_max=k, mask=r.mask, ctx=r.ctx).labels
        else:
            lab = init
        QK = SIG.q_for(r.n)
        if r.on_device:
            torch = __import__("torch")
            if not hasattr(lab, "data_ptr"):
                a = np.asarray(lab).reshape(-1)
                if a.size != r.n:
                    raise ValueError(f"gmm: {a.size} initial labels, the planes have {r.n} pixels")
                a = np.where((a >= 0) & (a < k), a, 255).astype(np.uint8)
                lab = r.ctx.to_device(a)
            lab = lab.reshape(-1)
            if lab.dtype != torch.uint8:
                lab = torch.where((lab >= 0) & (lab < k), lab, torch.full_like(lab, 255)).to(torch.uint8)
            table, _ = r.ctx.class_moments(r.planes, lab, 256, pe, 0 if r.u8 else QK, ignore=255, mask=r.mask)
            rows = _rows(table)[:k]
        else:
            rows = _hard_table_host(r.planes, lab, k, pe, 0 if r.u8 else QK, r.mask)
        e = np.zeros(F, np.int64) if pe is None else pe
        kept, w, mu, cov = m_step(rows, F, 0 if r.u8 else QK, e, False, self.covariance_type, self.reg_covar)
        return w, mu, cov, [j for j in range(k) if j not in kept]

    def fit(self, features, mask=None, ranges=None, ctx=None, sweep=None, keep_tables: bool = False) -> GMMResult:
        """EM over uint8 or float32 planes (a sequence of host or device planes, or an (F, H, W) / (F, n) array; float64 is cast
        to float32).  mask: non-zero = counted; ranges: (F, 2) per-plane (lo, hi) that size the fixed point (default the planes'
        extrema); sweep: a callable with Context.gmm_sweep's signature on host arrays (the tests' restatement), default the GPU;
        keep_tables: tables_ keeps every iteration's integer table (rows of Python ints), for diagnosis."""
        r = self._raster(features, mask, ctx, sweep)
        F = r.F
        pe = self._exponents(r, ranges)
        e = np.zeros(F, np.int64) if pe is None else pe
        Q = q_for(r.n)
        QM = 0 if r.u8 else Q
        diag = self.covariance_type in ("diag", "spherical")
        weights, means, cov, dropped0 = self._initial(r, pe)
        self._set(weights, means, cov, pe, "uint8" if r.u8 else "float32")
        const = self._const(pe)
        history, tables = [], []
        prev, lb = -math.inf, float("nan")
        self.converged_ = False
        n_iter = 0
        for it in range(1, self.max_iter + 1):
            n_iter = it
            km = kernel_model(self.weights_, self.means_, self._cov, pe, Q, self.covariance_type)
            o = r.sweep(r.planes, km, mask=r.mask, want_table=True)
            if o["n_counted"] == 0:
                raise ValueError("gmm: no pixel entered the sweep (every pixel masked, left out or without a finite density)")
            rows = _rows(o["table"])
            if keep_tables:
                tables.append(rows)
            lb = float(Fraction(o["ll_sum"], o["n_counted"] << Q))
            kept, w, mu, cov = m_step(rows, F, QM, e, diag, self.covariance_type, self.reg_covar)
            self._set(w, mu, cov, pe, self.dtype_)
            history.append(dict(lower_bound=lb + const, n_far=int(o["n_far"]), weights=[float(v) for v in w],
                                dropped=[j for j in range(len(rows)) if j not in kept] + (dropped0 if it == 1 else [])))
            if abs(lb - prev) < self.tol:
                self.converged_ = True
                break
            prev = lb
        self.n_iter_, self.lower_bound_, self.history_ = n_iter, lb + const, history
        self.tables_ = tables if keep_tables else None
        km = kernel_model(self.weights_, self.means_, self._cov, pe, Q, self.covariance_type)
        o = r.sweep(r.planes, km, mask=r.mask, want_table=False, want_labels=True)
        return GMMResult(r.labels_out(o["labels"]), self, self.weights_.copy(), history, int(o["n_left_out"]))

    # ---- prediction ---------------------------------------------------------------------------------------------------------
    def _sweep(self, features, mask, ctx, sweep, ranges=None, **want):
        r = self._raster(features, mask, ctx, sweep)
        km, pe = self._kernel_model(r, ranges)
        return r, pe, r.sweep(r.planes, km, mask=r.mask, want_table=False, **want)

    def predict(self, features, mask=None, ctx=None, sweep=None):
        """uint8 labels, component + 1, 0 where the mask is 0 or the pixel is left out.  Host planes give a host array of the
        planes' shape, device planes a flat device plane."""
        r, _, o = self._sweep(features, mask, ctx, sweep, want_labels=True)
        return r.labels_out(o["labels"])

    def predict_with_posterior(self, features, mask=None, ctx=None, sweep=None):
        """(labels, posterior of the label float32, log-likelihood float32 in feature units), one sweep."""
        r, pe, o = self._sweep(features, mask, ctx, sweep, want_labels=True, want_posterior=True, want_loglik=True)
        return r.labels_out(o["labels"]), r.labels_out(o["posterior"]), r.labels_out(o["loglik"] + float(self._const(pe)))

    def predict_proba(self, features, mask=None, ctx=None, sweep=None):
        """(k, ...) float32: every component's responsibility at every pixel, NaN where the pixel is not counted."""
        r, _, o = self._sweep(features, mask, ctx, sweep, want_proba=True)
        p = o["proba"]
        if r.on_device and r.device_in:
            return p
        p = p.cpu().numpy() if hasattr(p, "data_ptr") else p
        return p.reshape((self.n_components,) + tuple(r.shape))

    def score_samples(self, features, mask=None, ctx=None, sweep=None):
        """float64 log-density of every pixel in feature units (the float32 map plus the constants), NaN where not counted."""
        r, pe, o = self._sweep(features, mask, ctx, sweep, want_loglik=True)
        ll = o["loglik"]
        ll = ll.cpu().numpy() if hasattr(ll, "data_ptr") else ll
        return ll.astype(np.float64).reshape(r.shape) + self._const(pe)

    def _score(self, features, mask, ctx, sweep):
        r, pe, o = self._sweep(features, mask, ctx, sweep)
        n = o["n_counted"]
        if n <= 0:
            raise ValueError("gmm: no pixel entered the sweep")
        return float(Fraction(o["ll_sum"], n << q_for(r.n))) + self._const(pe), n

    def score(self, features, mask=None, ctx=None, sweep=None) -> float:
        """The mean log-likelihood per counted pixel, from the exact integer ll_sum."""
        return self._score(features, mask, ctx, sweep)[0]

    def n_parameters(self) -> int:
        self._check_fitted()
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    def bic(self, features, mask=None, ctx=None, sweep=None) -> float:
        s, n = self._score(features, mask, ctx, sweep)
        return -2.0 * s * n + self.n_parameters() * math.log(n)

    def aic(self, features, mask=None, ctx=None, sweep=None) -> float:
        s, n = self._score(features, mask, ctx, sweep)
        return -2.0 * s * n + 2.0 * self.n_parameters()

    # ---- files and other libraries --------------------------------------------------------------------------------------------
    def save(self, path) -> str:
        self._check_fitted()
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, format=np.array(_FORMAT_NAME), version=np.int64(FORMAT_VERSION), covariance_type=np.array(self.covariance_type),
                 weights=self.weights_, means=self.means_, covariances=self._cov, has_exp=np.int64(self.plane_exp_ is not None),
                 plane_exp=np.zeros(0, np.int64) if self.plane_exp_ is None else self.plane_exp_, dtype=np.array(self.dtype_),
                 tol=np.float64(self.tol), reg_covar=np.float64(self.reg_covar), max_iter=np.int64(self.max_iter),
                 converged=np.int64(bool(getattr(self, "converged_", False))), n_iter=np.int64(getattr(self, "n_iter_", 0)),
                 lower_bound=np.float64(getattr(self, "lower_bound_", float("nan"))))
        return path

    @classmethod
    def load(cls, path) -> "GaussianMixtureModel":
        with np.load(str(path), allow_pickle=False) as z:
            if "format" not in z.files or str(z["format"]) != _FORMAT_NAME:
                raise ValueError(f"GaussianMixtureModel.load: {path} is not a Gaussian mixture model file")
            if int(z["version"]) > FORMAT_VERSION:
                raise ValueError(f"GaussianMixtureModel.load: {path} has format version {int(z['version'])}, this build reads {FORMAT_VERSION}")
            ct = str(z["covariance_type"])
            self = cls(n_components=int(z["weights"].size), covariance_type=ct, tol=float(z["tol"]), reg_covar=float(z["reg_covar"]),
                       max_iter=int(z["max_iter"]))
            self._set(z["weights"], z["means"], z["covariances"], z["plane_exp"] if int(z["has_exp"]) else None, str(z["dtype"]))
            self.converged_, self.n_iter_, self.lower_bound_, self.history_ = bool(int(z["converged"])), int(z["n_iter"]), float(z["lower_bound"]), []
            return self

    def _whiten_x(self):
        """(W (k, F, F) in feature units, ln |S| (k,))."""
        k, F = self.means_.shape
        diag = self.covariance_type in ("diag", "spherical")
        W, ld = np.zeros((k, F, F)), np.zeros(k)
        for j in range(k):
            if self.covariance_type == "tied" and j > 0:
                W[j], ld[j] = W[0], ld[0]
            else:
                W[j], ld[j] = cholesky_whiten(self._cov[j], f"component {j}", diag)
        return W, ld

    def to_sklearn(self):
        """A sklearn.mixture.GaussianMixture with weights_, means_, covariances_, precisions_cholesky_ and precisions_ set."""
        from sklearn.mixture import GaussianMixture
        self._check_fitted()
        ct = self.covariance_type
        gm = GaussianMixture(n_components=self.n_components, covariance_type=ct, tol=self.tol, reg_covar=self.reg_covar, max_iter=self.max_iter)
        W, _ = self._whiten_x()
        gm.weights_, gm.means_, gm.covariances_ = self.weights_.copy(), self.means_.copy(), self.covariances_
        if ct == "full":
            gm.precisions_cholesky_ = np.ascontiguousarray(np.transpose(W, (0, 2, 1)))
            gm.precisions_ = np.stack([p @ p.T for p in gm.precisions_cholesky_])
        elif ct == "tied":
            gm.precisions_cholesky_ = np.ascontiguousarray(W[0].T)
            gm.precisions_ = gm.precisions_cholesky_ @ gm.precisions_cholesky_.T
        else:
            d = np.diagonal(W, axis1=1, axis2=2)
            gm.precisions_cholesky_ = d.copy() if ct == "diag" else d[:, 0].copy()
            gm.precisions_ = gm.precisions_cholesky_ ** 2
        gm.converged_ = bool(getattr(self, "converged_", False))
        gm.n_iter_ = int(getattr(self, "n_iter_", 0))
        gm.lower_bound_ = float(getattr(self, "lower_bound_", float("nan")))
        gm.n_features_in_ = self.n_features_in_
        return gm

    @classmethod
    def from_sklearn(cls, gm, plane_exp=None, dtype: str = "float32") -> "GaussianMixtureModel":
        self = cls.from_params(gm.weights_, gm.means_, gm.covariances_, gm.covariance_type, plane_exp=plane_exp, dtype=dtype, tol=gm.tol,
                               reg_covar=gm.reg_covar, max_iter=gm.max_iter)
        self.converged_ = bool(getattr(gm, "converged_", False))
        self.n_iter_ = int(getattr(gm, "n_iter_", 0))
        self.lower_bound_ = float(getattr(gm, "lower_bound_", float("nan")))
        return self

    def to_gaussian_classifier(self):
        """The mixture as a K22 'ml' model (rsseg.gaussian.GaussianClassifier): component j is class value j + 1, the weights
        are the priors.  Its labels are this model's wherever every pixel lies within the ranges."""
        from .gaussian import GaussianClassifier
        self._check_fitted()
        W, ld = self._whiten_x()
        offset = np.array([ld[j] - 2.0 * math.log(self.weights_[j]) for j in range(self.n_components)])
        return GaussianClassifier.from_params(self.means_, pack_lower(W), offset, np.arange(1, self.n_components + 1), method="ml",
                                              priors=self.weights_)

    def history_json(self) -> str:
        return json.dumps(dict(covariance_type=self.covariance_type, n_components=self.n_components, converged=bool(self.converged_),
                               n_iter=int(self.n_iter_), lower_bound=float(self.lower_bound_), history=self.history_), indent=1)


def select_components(features, ks, criterion: str = "bic", mask=None, ranges=None, ctx=None, sweep=None, **kw):
    """Fits a mixture for every k of ks (the other arguments are GaussianMixtureModel's) -> (table: a list of dict(k, bic, aic,
    lower_bound, n_iter, converged), the model with the smallest criterion)."""
    if criterion not in ("bic", "aic"):
        raise ValueError(f"select_components: criterion {criterion!r}, must be 'bic' or 'aic'")
    table, best = [], None
    for k in ks:
        m = GaussianMixtureModel(n_components=int(k), **kw)
        m.fit(features, mask=mask, ranges=ranges, ctx=ctx, sweep=sweep)
        s, n = m._score(features, mask, ctx, sweep)
        row = dict(k=int(k), bic=-2.0 * s * n + m.n_parameters() * math.log(n), aic=-2.0 * s * n + 2.0 * m.n_parameters(),
                   lower_bound=m.lower_bound_, n_iter=m.n_iter_, converged=m.converged_)
        table.append(row)
        if best is None or row[criterion] < best[0]:
            best = (row[criterion], m)
    if best is None:
        raise ValueError("select_components: ks is empty")
    return table, best[1]
