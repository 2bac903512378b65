"""
Class signatures (K24, csrc/k24_moments.hip; no counterpart in the reference): each class's pixel count, mean vector and
covariance matrix over the feature planes, taken from a label raster on the device, and what is read off them.

  class_moments(features, labels)  ->  ClassMoments     one keyed Gram pass (Context.class_moments): exact integer sums
  ClassMoments.mean / cov / pooled_cov                    from the integers, in rational arithmetic, rounded to float64 once
  ClassMoments.merge / save / load                        stripes, tiles and scenes add; a signature file is an .npz
  separability(moments, kind)                             Jeffries-Matusita, Bhattacharyya, (transformed) divergence
  GaussianClassifier.fit_moments(moments)                 the K22 models trained without a host sample matrix (rsseg/gaussian.py)

The table (include/rsseg.h, rsseg_class_moments; restated in tests/moments_ref.py) holds per label
  column 0 the count n,  column 1 + f  S_f = sum rint(u_f 2^Q),  column 1 + F + tri(a, b)  S_ab = sum rint(u_a u_b 2^Q)
with u_f = x_f 2^plane_exp[f] in [-1, 1].  Every term is off by at most half a unit of 2^-Q, so
  cov_ab = (S_ab - S_a S_b / (n 2^Q)) / (2^Q (n - ddof)) 2^-(e_a + e_b)
is within 1.5 n / (n - ddof) units of 2^-Q 2^-(e_a + e_b) of the exact covariance of the float32 inputs.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Optional, Sequence

import numpy as np

KINDS = ("jm", "bhattacharyya", "td", "divergence")
MAX_CLASSES = 256
Q_CAP = 44


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .runtime import default_context
    return default_context()


def n_columns(F: int) -> int:
    return 1 + F + F * (F + 1) // 2


def tri_index(F: int):
    """(a, b) of the columns 1 + F ... of the table: the row-major upper triangle."""
    return np.triu_indices(F)


def exponent_for(max_abs: float) -> int:
    """plane_exp of a plane whose largest finite |x| is max_abs: -ceil(log2(max_abs)), 0 for an all-zero plane, so that
    |x| 2^plane_exp <= 1."""
    max_abs = float(max_abs)
    if not math.isfinite(max_abs) or max_abs < 0:
        raise ValueError(f"class_moments: the largest |x| of a plane is {max_abs!r}")
    if max_abs == 0.0:
        return 0
    m, e = math.frexp(max_abs)   # max_abs = m 2^e, 0.5 <= m < 1
    return -(e - 1 if m == 0.5 else e)


def q_for(n_total: int) -> int:
    """Q = min(44, 61 - ceil(log2(n))): n 2^Q stays below 2^62."""
    n_total = max(int(n_total), 1)
    return min(Q_CAP, 61 - (n_total - 1).bit_length())


class ClassMoments:
    """The moment table of a label raster.  table: int64 (n_labels, 1 + F + F (F + 1) / 2), row = label value; plane_exp (F,)
    ints and Q as the kernel took them (all 0 for uint8 planes); classes: the label values with a non-zero count;
    n_left_out: counted pixels that entered no column because a value was infinite or beyond the planes' stated range."""

    def __init__(self, table, plane_exp, Q: int, n_left_out: int = 0):
        table = np.ascontiguousarray(table, dtype=np.int64)
        if table.ndim != 2:
            raise ValueError("ClassMoments: the table must be (n_labels, columns)")
        pe = np.ascontiguousarray(plane_exp, dtype=np.int64).reshape(-1)
        if table.shape[1] != n_columns(pe.size):
            raise ValueError(f"ClassMoments: {table.shape[1]} columns do not belong to {pe.size} planes")
        self.table, self.plane_exp, self.Q, self.n_left_out = table, pe, int(Q), int(n_left_out)

    # ---- what the table holds -----------------------------------------------------------------------------------------
    @property
    def n_features(self) -> int:
        return int(self.plane_exp.size)

    @property
    def counts(self) -> np.ndarray:
        """Pixels per label value: int64 (n_labels,)."""
        return self.table[:, 0].copy()

    @property
    def classes(self) -> np.ndarray:
        return np.flatnonzero(self.table[:, 0] > 0)

    def _row(self, c: int):
        row = [int(v) for v in self.table[int(c)]]
        F = self.n_features
        return row[0], row[1:1 + F], row[1 + F:]

    def mean(self) -> np.ndarray:
        """(len(classes), F) float64: S_f / (n 2^Q) 2^-e_f, rounded once."""
        F = self.n_features
        out = np.zeros((self.classes.size, F))
        for j, c in enumerate(self.classes):
            n, s, _ = self._row(c)
            for f in range(F):
                out[j, f] = float(Fraction(s[f], n << self.Q) / Fraction(2) ** int(self.plane_exp[f]))
        return out

    def _scatter(self, c: int):
        """The exact centred sums of products of class c in units of 2^-2Q 2^-(e_a + e_b) / n: S_ab n 2^Q - S_a S_b, as ints."""
        n, s, p = self._row(c)
        a, b = tri_index(self.n_features)
        return n, [p[i] * (n << self.Q) - s[ai] * s[bi] for i, (ai, bi) in enumerate(zip(a.tolist(), b.tolist()))]

    def _unit(self, i: int, a, b) -> Fraction:
        return Fraction(2) ** (-2 * self.Q - int(self.plane_exp[a[i]]) - int(self.plane_exp[b[i]]))

    def _full(self, tri_vals) -> np.ndarray:
        F = self.n_features
        a, b = tri_index(F)
        m = np.zeros((F, F))
        m[a, b] = tri_vals
        m[b, a] = tri_vals
        return m

    def cov(self, ddof: int = 1) -> np.ndarray:
        """(len(classes), F, F) float64 covariances, np.cov's for ddof=1; a class of n <= ddof pixels gets NaN."""
        F = self.n_features
        a, b = tri_index(F)
        out = np.full((self.classes.size, F, F), np.nan)
        for j, c in enumerate(self.classes):
            n, sc = self._scatter(c)
            if n - ddof <= 0:
                continue
            den = n * (n - ddof)
            out[j] = self._full([float(Fraction(v, den) * self._unit(i, a, b)) for i, v in enumerate(sc)])
        return out

    def pooled_cov(self) -> np.ndarray:
        """(F, F): the pooled within-class covariance, sum_c (n_c - 1) cov_c / (N - k)."""
        F = self.n_features
        a, b = tri_index(F)
        N, k = int(self.table[:, 0].sum()), self.classes.size
        if N - k < 1:
            raise ValueError(f"ClassMoments.pooled_cov: {N} pixels of {k} classes leave nothing for the pooled covariance")
        tot = [Fraction(0)] * a.size
        for c in self.classes:
            n, sc = self._scatter(c)
            for i, v in enumerate(sc):
                tot[i] += Fraction(v, n)
        return self._full([float(t / (N - k) * self._unit(i, a, b)) for i, t in enumerate(tot)])

    def std(self) -> np.ndarray:
        """(len(classes), F): the square roots of the variances (ddof=1)."""
        return np.sqrt(np.maximum(np.diagonal(self.cov(), axis1=1, axis2=2), 0.0))

    # ---- accumulation and files -----------------------------------------------------------------------------------------
    def merge(self, other: "ClassMoments") -> "ClassMoments":
        """The moments of both rasters together: the tables add.  Both must have been taken with the same plane_exp and Q
        (class_moments(..., ranges=, n_total=))."""
        if self.n_features != other.n_features or np.any(self.plane_exp != other.plane_exp):
            raise ValueError("ClassMoments.merge: the two tables were taken with different plane exponents (pass the same ranges=)")
        if self.Q != other.Q:
            raise ValueError(f"ClassMoments.merge: the two tables were taken with Q = {self.Q} and Q = {other.Q} (pass the same n_total=)")
        rows = max(self.table.shape[0], other.table.shape[0])
        t = np.zeros((rows, self.table.shape[1]), np.int64)
        t[:self.table.shape[0]] += self.table
        t[:other.table.shape[0]] += other.table
        return ClassMoments(t, self.plane_exp, self.Q, self.n_left_out + other.n_left_out)

    def save(self, path) -> str:
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, table=self.table, plane_exp=self.plane_exp, Q=np.int64(self.Q), n_left_out=np.int64(self.n_left_out))
        return path

    @classmethod
    def load(cls, path) -> "ClassMoments":
        with np.load(str(path), allow_pickle=False) as z:
            return cls(z["table"], z["plane_exp"], int(z["Q"]), int(z["n_left_out"]))


# ---- the pass over the raster (GPU) -------------------------------------------------------------------------------------
def plane_extrema(ctx, planes: Sequence) -> np.ndarray:
    """(F, 2) float64: the smallest and largest finite value of each float32 device plane (0, 0 when it has none), by the
    library's order statistics (K1); a plane with NaN or infinite values is compacted to its finite pixels first (K19)."""
    n = planes[0].numel()
    out = np.zeros((len(planes), 2))
    if n == 0:
        return out
    for g0 in range(0, len(planes), 8):
        grp = list(planes[g0:g0 + 8])
        v, nn = ctx.order_stats_multi(grp, [[0, n - 1]] * len(grp))
        for i, p in enumerate(grp):
            lo, hi = float(v[i, 0]), float(v[i, 1])
            if nn[i] or not (math.isfinite(lo) and math.isfinite(hi)):
                mask, nv = ctx.valid_mask([p], nan=True, inf=True)
                if nv == 0:
                    lo = hi = 0.0
                else:
                    w, _ = ctx.order_stats(ctx.compact(ctx.compact_plan(mask), [p])[0], [0, nv - 1])
                    lo, hi = float(w[0]), float(w[1])
            out[g0 + i] = lo, hi
    return out


def _to_planes(ctx, features):
    """flat device planes of one dtype (float32 or uint8) and the raster's pixel count"""
    if isinstance(features, np.ndarray):
        if features.ndim != 3:
            raise ValueError("class_moments: features must be a 3-D array (height, width, n_features) or a sequence of device planes")
        dt = np.uint8 if features.dtype == np.uint8 else np.float32
        return [ctx.to_device(np.ascontiguousarray(features[:, :, f], dtype=dt).reshape(-1)) for f in range(features.shape[2])]
    planes = [p.reshape(-1) if hasattr(p, "data_ptr") else ctx.to_device(np.ascontiguousarray(p).reshape(-1)) for p in features]
    if not planes:
        raise ValueError("class_moments: no feature planes")
    return planes


def _to_labels(ctx, labels, n: int):
    if hasattr(labels, "data_ptr"):
        lab = labels.reshape(-1)
    else:
        a = np.asarray(labels)
        if a.dtype != np.uint8:
            if a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
                raise ValueError("class_moments: labels must be integers that fit int32")
            a = a.astype(np.int32)
        lab = ctx.to_device(np.ascontiguousarray(a).reshape(-1))
    if lab.numel() != n:
        raise ValueError(f"class_moments: {lab.numel()} labels, the planes have {n} pixels")
    return lab


def class_moments(features, labels, *, ignore: int = 0, mask=None, ranges=None, n_total: Optional[int] = None, ctx=None) -> ClassMoments:
    """The moments of the classes of a label raster over the feature planes, in one pass on the GPU.
    features: (H, W, F) array or a sequence of F device planes, float32 or uint8.  labels: uint8 or int32, host or device, the
    label value is the table's row (0 ... 255); pixels labelled `ignore` (default 0, -1: none) and pixels whose mask (None, or
    non-zero = counted) is 0 do not count.  NaN features read as 0.
    ranges: (F, 2) (lo, hi) or (F,) max |x| per plane: what sizes the fixed point instead of an extrema pass; n_total: the
    pixel count of everything that will be merged (default: this raster's).  Tables merge only when both were the same."""
    from .masked import mask_to_device
    ctx = _ctx(ctx)
    torch = __import__("torch")
    planes = _to_planes(ctx, features)
    F, n = len(planes), planes[0].numel()
    u8 = planes[0].dtype == torch.uint8
    lab = _to_labels(ctx, labels, n)
    dmask = None if mask is None else mask_to_device(ctx, mask, n)
    if lab.dtype == torch.uint8:
        h = ctx.hist_u8(lab) if n else np.zeros(256, np.int64)
        top = int(np.flatnonzero(h)[-1]) if h.any() else 0
    else:
        top = int(lab.max().item()) if n else 0
    n_classes = max(top, 0) + 1
    if u8:
        pe, Q = None, 0
    else:
        if ranges is None:
            mx = np.abs(plane_extrema(ctx, planes)).max(axis=1)
        else:
            r = np.asarray(ranges, np.float64)
            mx = np.abs(r).max(axis=1) if r.ndim == 2 else np.abs(r).reshape(-1)
            if mx.size != F:
                raise ValueError(f"class_moments: ranges for {mx.size} planes, the raster has {F}")
        pe = np.array([exponent_for(m) for m in mx], np.int64)
        Q = q_for(n if n_total is None else max(int(n_total), n))
    table, left = ctx.class_moments(planes, lab, n_classes, pe, Q, ignore=ignore, mask=dmask)
    return ClassMoments(table.cpu().numpy(), np.zeros(F, np.int64) if pe is None else pe, Q, left)


# ---- separability (host, float64) ---------------------------------------------------------------------------------------
def _signature(obj):
    """(classes, counts, mean (k, F), cov (k, F, F)) of a ClassMoments or of a dict with those keys"""
    if isinstance(obj, ClassMoments):
        return obj.classes, obj.counts[obj.classes], obj.mean(), obj.cov()
    mean = np.asarray(obj["mean"], np.float64)
    cov = np.asarray(obj["cov"], np.float64)
    classes = np.asarray(obj["classes"]) if "classes" in obj else np.arange(mean.shape[0])
    counts = np.asarray(obj["counts"]) if "counts" in obj else np.zeros(mean.shape[0], np.int64)
    if mean.ndim != 2 or cov.shape != (mean.shape[0], mean.shape[1], mean.shape[1]) or classes.shape != (mean.shape[0],):
        raise ValueError("separability: a signature is classes (k,), mean (k, F) and cov (k, F, F)")
    return classes, counts, mean, cov


def _spd(cov: np.ndarray, c) -> np.ndarray:
    """the Cholesky factor of a class covariance; ValueError naming the class when it has none"""
    bad = ValueError(f"separability: the covariance of class {c} is singular (constant or linearly dependent features, or too few pixels)")
    if not np.all(np.isfinite(cov)):
        raise bad
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise bad from None
    if np.any(np.diag(L) ** 2 <= cov.shape[0] * np.finfo(np.float64).eps * np.diag(cov)):
        raise bad
    return L


def separability(moments_or_signature, kind: str = "jm") -> np.ndarray:
    """The k x k float64 matrix of pairwise class separability (classes in ascending label order):
      'bhattacharyya'  B = 1/8 d' S^-1 d + 1/2 ln(|S| / sqrt(|S1| |S2|)),  S = (S1 + S2) / 2,  d = mu1 - mu2
      'jm'             2 (1 - exp(-B)), in [0, 2]
      'divergence'     D = 1/2 tr((S1 - S2)(S2^-1 - S1^-1)) + 1/2 tr((S1^-1 + S2^-1) d d')
      'td'             2000 (1 - exp(-D / 8)), in [0, 2000]
    A singular class covariance is a ValueError naming the class."""
    if kind not in KINDS:
        raise ValueError(f"separability: kind {kind!r}, must be one of {KINDS}")
    classes, _, mean, cov = _signature(moments_or_signature)
    k = len(classes)
    chol = [_spd(cov[j], classes[j]) for j in range(k)]
    logdet = [2.0 * float(np.sum(np.log(np.diag(L)))) for L in chol]
    out = np.zeros((k, k))
    if kind in ("td", "divergence"):
        inv = [np.linalg.inv(cov[j]) for j in range(k)]
    for i in range(k):
        for j in range(i + 1, k):
            d = mean[i] - mean[j]
            if kind in ("jm", "bhattacharyya"):
                S = 0.5 * (cov[i] + cov[j])
                Ls = np.linalg.cholesky(S)
                z = np.linalg.solve(Ls, d)
                ld = 2.0 * float(np.sum(np.log(np.diag(Ls))))
                v = 0.125 * float(z @ z) + 0.5 * (ld - 0.5 * (logdet[i] + logdet[j]))
                v = max(v, 0.0)
                if kind == "jm":
                    v = 2.0 * -math.expm1(-v)
            else:
                v = 0.5 * float(np.trace((cov[i] - cov[j]) @ (inv[j] - inv[i]))) + 0.5 * float(d @ (inv[i] + inv[j]) @ d)
                v = max(v, 0.0)
                if kind == "td":
                    v = 2000.0 * -math.expm1(-v / 8.0)
            out[i, j] = out[j, i] = v
    return out


def separability_report(moments_or_signature, kinds: Sequence[str] = ("jm", "td")) -> dict:
    """What the signatures stage writes (JSON-ready): per class the label, count, mean and standard deviation; per kind the
    matrix and the least separable pair of classes."""
    classes, counts, mean, cov = _signature(moments_or_signature)
    std = np.sqrt(np.maximum(np.diagonal(cov, axis1=1, axis2=2), 0.0))
    rep = dict(classes=[int(c) for c in classes],
               per_class=[dict(label=int(c), count=int(n), mean=mean[j].tolist(), std=std[j].tolist())
                          for j, (c, n) in enumerate(zip(classes, counts))])
    if isinstance(moments_or_signature, ClassMoments):
        rep["n_left_out"] = moments_or_signature.n_left_out
    for kind in kinds:
        m = separability(moments_or_signature, kind)
        entry = dict(matrix=m.tolist(), least_separable=None)
        if len(classes) > 1:
            iu = np.triu_indices(len(classes), 1)
            p = int(np.argmin(m[iu]))
            entry["least_separable"] = dict(classes=[int(classes[iu[0][p]]), int(classes[iu[1][p]])], value=float(m[iu][p]))
        rep[kind] = entry
    return rep
