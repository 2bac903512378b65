"""
ISODATA clustering (K26, csrc/k26_isodata.hip; no counterpart in the reference): k-means that finds the number of clusters
itself.  Every iteration is one pass over the raster on the GPU (Context.isodata_sweep: assign every pixel to the nearest
centre and take each cluster's count, sum and sum of squares per plane, as exact integers); everything else happens here, in
float64 and Python integers on the k x (1 + 2 F) table.  There is no per-pixel host work and no random number.

  isodata(features, k_target=7, ...)  ->  IsodataResult(labels, model, counts, history, n_left_out)
  IsodataModel.predict(other_features)           one labels-only sweep: cluster ids mean the same thing in every map
  IsodataModel.save(path) / IsodataModel.load    an .npz of plain arrays and strings, no pickle

The clustering space is the k-means path's: every plane divided by its range hi - lo (a constant plane gets weight 0), so
max_std and min_dist are fractions of a plane's range.  The kernel takes u_f = x_f 2^plane_exp[f] in [-1, 1] (K24's fixed
point, rsseg.signatures.exponent_for / q_for) and z_f = u_f weight[f] with weight[f] = 2^-plane_exp[f] / (hi - lo); centres are
kept in these weighted units.

Iteration it = 1 ... max_iter (Tou & Gonzalez, made deterministic):
  1  sweep
  2  drop every cluster with n_j < min_size (never the largest)
  3  centres = the means (from the integers, rounded once); sigma_jf = weight_f sqrt(population variance of u);
     D_j = sqrt(sum_f sigma_jf^2), the root-mean-square distance of the cluster's pixels to its centre (the textbook's mean
     distance would cost one more column and a square root per pixel); D = sqrt(sum n_j D_j^2 / sum n_j)
  4  unless it is the last iteration: the split step when k <= k_target / 2, or when it is odd and k < 2 k_target; else the
     merge step
  5  split, j ascending: f* = the lowest f with the largest sigma_jf; when sigma_jf* > max_std and (D_j > D and
     n_j > 2 (min_size + 1), or k <= k_target / 2) and the count is below k_max: c_j -> c_j - gamma sigma e_f*, and
     c_j + gamma sigma e_f* is appended
  6  merge (chosen, or the split step split nothing): the pairs i < j closer than min_dist, by (distance, i, j), at most
     max_pairs, a cluster in at most one; c_i = the count-weighted mean, j removed
  7  stop after max_iter, or when this iteration and the one before dropped, split and merged nothing and
     n_changed <= change * n_counted.  (Labels are renumbered whenever the set of centres changes, so n_changed means something
     only between two sweeps over the same set.)
One final sweep with the final centres gives the returned labels and counts.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import signatures as SIG

MAX_CLUSTERS = 64
MAX_FEATURES = 64
NO_LABEL = 255
FORMAT_VERSION = 1
_FORMAT_NAME = "rsseg.IsodataModel"


def _is_device(p) -> bool:
    return hasattr(p, "data_ptr")


def _host_planes(features, name: str = "isodata"):
    """features -> (list of flat host planes of one dtype (float32 or uint8), shape of one plane); name: the caller, as its
    errors call it"""
    if isinstance(features, np.ndarray):
        if features.ndim not in (2, 3):
            raise ValueError(f"{name}: features must be an (F, H, W) or (F, n) array or a sequence of planes")
        seq = [features[f] for f in range(features.shape[0])]
    else:
        seq = [p.cpu().numpy() if _is_device(p) else np.asarray(p) for p in features]
    if not seq:
        raise ValueError(f"{name}: no feature planes")
    u8 = all(p.dtype == np.uint8 for p in seq)
    for p in seq:
        if p.dtype != np.uint8 and p.dtype.kind != "f":
            raise ValueError(f"{name}: planes must be uint8, float32 or float64, not {p.dtype}")
        if p.shape != seq[0].shape:
            raise ValueError(f"{name}: the planes differ in shape")
    dt = np.uint8 if u8 else np.float32
    return [np.ascontiguousarray(p, dtype=dt).reshape(-1) for p in seq], seq[0].shape


class _Raster:
    """The planes, the mask and the label plane where the sweep wants them: on the device for Context.isodata_sweep, on the
    host for a sweep= callable.  name and device_sweep: the caller as its errors call it and the Context method that is its sweep
    (rsseg.gmm shares this class)."""

    def __init__(self, features, mask, ctx, sweep, name: str = "isodata", device_sweep: str = "isodata_sweep"):
        self.on_device = sweep is None
        self.device_in = not isinstance(features, np.ndarray) and len(features) > 0 and all(_is_device(p) for p in features)
        if self.on_device:
            self.ctx = SIG._ctx(ctx)
            self.sweep = getattr(self.ctx, device_sweep)
            if self.device_in:
                torch = __import__("torch")
                self.planes = [p.reshape(-1) for p in features]
                if any(p.dtype == torch.float64 for p in self.planes):
                    self.planes = [p.to(torch.float32) for p in self.planes]
                self.shape = tuple(features[0].shape)
                if any(p.dtype != self.planes[0].dtype or p.dtype not in (torch.float32, torch.uint8) or p.numel() != self.planes[0].numel()
                       for p in self.planes):
                    raise ValueError(f"{name}: planes must all be float32 or all uint8, of one size")
                self.u8 = self.planes[0].dtype == torch.uint8
            else:
                host, self.shape = _host_planes(features, name)
                self.u8 = host[0].dtype == np.uint8
                self.planes = [self.ctx.to_device(p) for p in host]
            self.n = int(self.planes[0].numel())
        else:
            self.ctx = None
            self.sweep = sweep
            self.planes, self.shape = _host_planes(features, name)
            self.u8 = self.planes[0].dtype == np.uint8
            self.n = int(self.planes[0].size)
        self.F = len(self.planes)
        if self.F > MAX_FEATURES:
            raise ValueError(f"{name}: {self.F} planes, at most {MAX_FEATURES}")
        self.mask = None
        if mask is not None:
            if self.on_device:
                from .masked import mask_to_device
                self.mask = mask_to_device(self.ctx, mask, self.n).reshape(-1)
            else:
                m = mask.cpu().numpy() if _is_device(mask) else np.asarray(mask)
                if m.size != self.n:
                    raise ValueError(f"mask: {m.size} elements, the planes have {self.n} pixels")
                self.mask = np.ascontiguousarray(m != 0, dtype=np.uint8).reshape(-1)

    def new_labels(self):
        if self.on_device:
            torch = __import__("torch")
            lab = self.ctx.empty(max(self.n, 1), torch.uint8)[:self.n]
            with torch.cuda.stream(self.ctx.torch_stream):   # ordered before the sweep that reads it
                lab.fill_(NO_LABEL)
            return lab
        return np.full(self.n, NO_LABEL, np.uint8)

    def extrema(self) -> np.ndarray:
        """(F, 2): the smallest and largest finite value of every plane over its counted pixels (0, 0 when it has none)"""
        out = np.zeros((self.F, 2))
        if self.n == 0:
            return out
        if not self.on_device:
            for f, p in enumerate(self.planes):
                v = p if self.mask is None else p[self.mask != 0]
                v = v[np.isfinite(v)] if v.dtype != np.uint8 else v
                if v.size:
                    out[f] = float(v.min()), float(v.max())
            return out
        planes = self.planes
        if self.mask is not None:   # the counted pixels alone (K19)
            plan = self.ctx.compact_plan(self.mask)
            if plan.n_valid == 0:
                return out
            planes = self.ctx.compact(plan, planes)
        if not self.u8:
            return SIG.plane_extrema(self.ctx, planes)
        for f, p in enumerate(planes):
            nz = np.flatnonzero(self.ctx.hist_u8(p))
            out[f] = float(nz[0]), float(nz[-1])
        return out

    def labels_out(self, labels):
        if self.on_device and self.device_in:
            return labels
        lab = labels.cpu().numpy() if _is_device(labels) else labels
        return lab.reshape(self.shape)



def _scaling(r: _Raster, ranges):
    """(ranges (F, 2), plane_exp or None, Q, weight (F,)) of a raster"""
    if ranges is None:
        rg = r.extrema()
    else:
        rg = np.asarray(ranges, np.float64)
        if rg.shape != (r.F, 2) or not np.all(np.isfinite(rg)) or np.any(rg[:, 1] < rg[:, 0]):
            raise ValueError(f"isodata: ranges must be {r.F} finite (lo, hi) pairs with lo <= hi")
    if r.u8:
        pe, Q = None, 0
        e = np.zeros(r.F, np.int64)
    else:
        e = np.array([SIG.exponent_for(m) for m in np.abs(rg).max(axis=1)], np.int64)
        pe, Q = e, SIG.q_for(r.n)
    weight = np.zeros(r.F)
    for f in range(r.F):
        span = float(rg[f, 1]) - float(rg[f, 0])
        if span > 0.0 and math.isfinite(span):
            weight[f] = math.ldexp(1.0, -int(e[f])) / span
    if not np.all(np.isfinite(weight)):
        raise ValueError("isodata: a plane's range is too small for a finite weight")
    return rg, pe, Q, weight


def _table_rows(table):
    t = table.cpu().numpy() if _is_device(table) else np.asarray(table)
    return [[int(v) for v in row] for row in t]


def _moments(row, F: int, Q: int, weight):
    """(n, centre (F,) in weighted units, sigma (F,)) of one table row: the mean is S_f / (n 2^Q) times the weight, rounded
    once; sigma_f = weight_f sqrt(max(0, S2_f n 2^Q - S_f^2) / (n 2^Q)^2), the quotient rounded once."""
    n = row[0]
    den = n << Q
    c = [float(Fraction(row[1 + f], den) * Fraction(float(weight[f]))) for f in range(F)]
    s = [float(weight[f]) * math.sqrt(float(Fraction(max(0, row[1 + F + f] * den - row[1 + f] ** 2), den * den))) for f in range(F)]
    return n, c, s


def _dist(a, b) -> float:
    d = 0.0
    for x, y in zip(a, b):
        t = x - y
        d = d + t * t
    return math.sqrt(d)


class IsodataModel:
    """Centres (k, F) in weighted units with what turns a plane value into them: weight (F,), plane_exp (F,) (zeros for uint8
    planes), Q, the ranges (F, 2) the weights came from, optional plane names, and the planes' dtype ('float32' or 'uint8')."""

    def __init__(self, centers, weight, plane_exp, Q: int, ranges, dtype: str, feature_names: Optional[Sequence[str]] = None):
        c = np.ascontiguousarray(centers, dtype=np.float64)
        if c.ndim != 2 or not 1 <= c.shape[0] <= MAX_CLUSTERS or c.shape[1] < 1:
            raise ValueError(f"IsodataModel: centers must be (k, F) with 1 <= k <= {MAX_CLUSTERS}")
        F = c.shape[1]
        self.centers = c
        self.weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        self.plane_exp = np.ascontiguousarray(plane_exp, dtype=np.int64).reshape(-1)
        self.ranges = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1, 2)
        if self.weight.size != F or self.plane_exp.size != F or self.ranges.shape[0] != F:
            raise ValueError(f"IsodataModel: {F} features in the centres, {self.weight.size} weights, {self.plane_exp.size} exponents, "
                             f"{self.ranges.shape[0]} ranges")
        if not (np.all(np.isfinite(c)) and np.all(np.isfinite(self.weight))):
            raise ValueError("IsodataModel: centres and weights must be finite")
        if dtype not in ("float32", "uint8"):
            raise ValueError(f"IsodataModel: dtype {dtype!r}, must be 'float32' or 'uint8'")
        self.Q, self.dtype = int(Q), dtype
        self.feature_names = None if feature_names is None else [str(s) for s in feature_names]
        if self.feature_names is not None and len(self.feature_names) != F:
            raise ValueError(f"IsodataModel: {len(self.feature_names)} feature names for {F} features")

    @property
    def n_clusters(self) -> int:
        return self.centers.shape[0]

    @property
    def n_features(self) -> int:
        return self.centers.shape[1]

    def centers_in_feature_units(self) -> np.ndarray:
        """(k, F): the centres as plane values, c / (weight 2^plane_exp); a plane of weight 0 (constant) shows its lo."""
        out = np.empty_like(self.centers)
        for f in range(self.n_features):
            w = self.weight[f] * math.ldexp(1.0, int(self.plane_exp[f]))
            out[:, f] = self.centers[:, f] / w if w != 0.0 else self.ranges[f, 0]
        return out

    def predict(self, features, mask=None, ctx=None, sweep=None):
        """The label (0 ... k - 1; 255 where the mask is 0 or a value lies beyond the model's ranges) of every pixel: one
        labels-only sweep.  Host planes give a host array of the planes' shape, device planes a flat device plane."""
        r = _Raster(features, mask, ctx, sweep)
        if r.F != self.n_features:
            raise ValueError(f"IsodataModel: {r.F} planes, the model was fitted on {self.n_features}")
        if ("uint8" if r.u8 else "float32") != self.dtype:
            raise ValueError(f"IsodataModel: {'uint8' if r.u8 else 'float32'} planes, the model was fitted on {self.dtype} planes")
        labels = r.new_labels()
        r.sweep(r.planes, labels, self.centers, self.weight, None if r.u8 else self.plane_exp, 0 if r.u8 else SIG.q_for(r.n), mask=r.mask,
                want_table=False)
        return r.labels_out(labels)

    def save(self, path) -> str:
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, format=np.array(_FORMAT_NAME), version=np.int64(FORMAT_VERSION), centers=self.centers, weight=self.weight,
                 plane_exp=self.plane_exp, Q=np.int64(self.Q), ranges=self.ranges, dtype=np.array(self.dtype),
                 feature_names=np.array(self.feature_names if self.feature_names is not None else [], dtype=str),
                 has_names=np.int64(self.feature_names is not None))
        return path

    @classmethod
    def load(cls, path) -> "IsodataModel":
        with np.load(str(path), allow_pickle=False) as z:
            if "format" not in z.files or str(z["format"]) != _FORMAT_NAME:
                raise ValueError(f"IsodataModel.load: {path} is not an ISODATA model file")
            if int(z["version"]) > FORMAT_VERSION:
                raise ValueError(f"IsodataModel.load: {path} has format version {int(z['version'])}, this build reads {FORMAT_VERSION}")
            names = [str(s) for s in z["feature_names"]] if int(z["has_names"]) else None
            return cls(z["centers"], z["weight"], z["plane_exp"], int(z["Q"]), z["ranges"], str(z["dtype"]), names)


class IsodataResult(NamedTuple):
    labels: object        # uint8, 0 ... k - 1, 255 = not counted or left out: a host array of the planes' shape, or a flat device plane
    model: IsodataModel
    counts: np.ndarray    # int64 (k,): the pixels of every cluster
    history: list         # per iteration: dict(k, dropped, split, merged, n_changed)
    n_left_out: int       # counted pixels with a value beyond the ranges (none with the default ranges)


def isodata(features, *, k_target: int = 7, k_init: Optional[int] = None, k_max: Optional[int] = None, min_size: Optional[int] = None,
            max_std: float = 0.06, min_dist: float = 0.1, max_pairs: int = 2, max_iter: int = 20, change: float = 0.0,
            gamma: float = 0.5, init="diagonal", mask=None, ranges=None, feature_names=None, ctx=None, sweep=None) -> IsodataResult:
    """ISODATA over uint8 or float32 planes (a sequence of host or device planes, or an (F, H, W) / (F, n) array; float64 is
    cast to float32).  See the module text for the iteration.
    k_target: the number of clusters aimed at; k_init (default k_target): the initial number; k_max (default
    min(64, max(2 k_target, k_init))): splitting stops there; min_size (default max(1, n_counted // 1000)); max_std, min_dist: in
    units of a plane's range; init: 'diagonal' (k_init centres along mean +- sigma of the scene, from one sweep with k = 1) or a
    (k_init, F) array in plane values; mask: non-zero = counted; ranges: (F, 2) per-plane (lo, hi), default the planes' extrema;
    sweep: a callable with Context.isodata_sweep's signature on host arrays (the tests' restatement), default the GPU."""
    k_target = int(k_target)
    if not 1 <= k_target <= MAX_CLUSTERS:
        raise ValueError(f"isodata: k_target={k_target}, must be 1 ... {MAX_CLUSTERS}")
    init_arr = None
    if not isinstance(init, str):
        init_arr = np.asarray(init, np.float64)
        if init_arr.ndim != 2 or not np.all(np.isfinite(init_arr)):
            raise ValueError("isodata: init must be 'diagonal' or a finite (k_init, F) array")
        if k_init is not None and int(k_init) != init_arr.shape[0]:
            raise ValueError(f"isodata: k_init={k_init} but init holds {init_arr.shape[0]} centres")
        k_init = init_arr.shape[0]
    elif init != "diagonal":
        raise ValueError(f"isodata: init {init!r}, must be 'diagonal' or an array of centres")
    k_init = k_target if k_init is None else int(k_init)
    if not 1 <= k_init <= MAX_CLUSTERS:
        raise ValueError(f"isodata: k_init={k_init}, must be 1 ... {MAX_CLUSTERS}")
    k_max = min(MAX_CLUSTERS, max(2 * k_target, k_init)) if k_max is None else int(k_max)
    if not max(k_init, 1) <= k_max <= MAX_CLUSTERS:
        raise ValueError(f"isodata: k_max={k_max}, must be k_init ... {MAX_CLUSTERS}")
    if min_size is not None and int(min_size) < 1:
        raise ValueError(f"isodata: min_size={min_size}, must be >= 1")
    max_iter, max_pairs = int(max_iter), int(max_pairs)
    if max_iter < 1:
        raise ValueError(f"isodata: max_iter={max_iter}, must be >= 1")
    if max_pairs < 0:
        raise ValueError(f"isodata: max_pairs={max_pairs}, must be >= 0")
    for name, v in (("max_std", max_std), ("min_dist", min_dist), ("change", change), ("gamma", gamma)):
        if not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"isodata: {name}={v!r}, must be finite and >= 0")
    max_std, min_dist, change, gamma = float(max_std), float(min_dist), float(change), float(gamma)

    r = _Raster(features, mask, ctx, sweep)
    F = r.F
    if init_arr is not None and init_arr.shape[1] != F:
        raise ValueError(f"isodata: init has {init_arr.shape[1]} features, the raster {F} planes")
    rg, pe, Q, weight = _scaling(r, ranges)
    e = np.zeros(F, np.int64) if pe is None else pe
    labels = r.new_labels()

    def run(centers, want_table=True):
        table, changed, left = r.sweep(r.planes, labels, np.array(centers, np.float64).reshape(len(centers), F), weight, pe, Q, mask=r.mask,
                                       want_table=want_table)
        return (_table_rows(table) if want_table else None), int(changed), int(left)

    if init_arr is None:
        rows, _, _ = run([[0.0] * F])
        if rows[0][0] > 0:
            _, mu, sd = _moments(rows[0], F, Q, weight)
        else:
            mu, sd = [0.0] * F, [0.0] * F
        centers = [[mu[f] + sd[f] * ((2.0 * j) / (k_init - 1) - 1.0) if k_init > 1 else mu[f] for f in range(F)] for j in range(k_init)]
        labels = r.new_labels()   # the next sweep's n_changed starts from no assignment
    else:
        centers = [[math.ldexp(float(init_arr[j, f]), int(e[f])) * float(weight[f]) for f in range(F)] for j in range(k_init)]
    for c in centers:
        if not all(math.isfinite(v) for v in c):
            raise ValueError("isodata: an initial centre is not finite in the clustering space")

    history = []
    quiet_before = False
    for it in range(1, max_iter + 1):
        rows, n_changed, _ = run(centers)
        k = len(centers)
        counts = [row[0] for row in rows]
        n_counted = sum(counts)
        msize = max(1, n_counted // 1000) if min_size is None else int(min_size)
        # 2: drop
        largest = max(range(k), key=lambda j: (counts[j], -j))
        keep = [j for j in range(k) if counts[j] >= msize or j == largest]
        dropped = k - len(keep)
        # 3: update
        cen, sig, cnt = [], [], []
        for j in keep:
            if counts[j] > 0:
                _, c, s = _moments(rows[j], F, Q, weight)
            else:
                c, s = list(centers[j]), [0.0] * F
            cen.append(c)
            sig.append(s)
            cnt.append(counts[j])
        k = len(cen)
        Dj = [math.sqrt(sum(v * v for v in s)) for s in sig]
        tot = sum(cnt)
        D = math.sqrt(sum(n * d * d for n, d in zip(cnt, Dj)) / tot) if tot > 0 else 0.0
        n_split = n_merged = 0
        if it < max_iter:
            # 4, 5: split
            do_split = 2 * k <= k_target or (it % 2 == 1 and k < 2 * k_target)
            if do_split:
                few = 2 * k <= k_target
                for j in range(k):
                    if len(cen) >= k_max:
                        break
                    fs = max(range(F), key=lambda f: (sig[j][f], -f))
                    s = sig[j][fs]
                    if s > max_std and ((Dj[j] > D and cnt[j] > 2 * (msize + 1)) or few):
                        up = list(cen[j])
                        up[fs] = cen[j][fs] + gamma * s
                        cen[j][fs] = cen[j][fs] - gamma * s
                        cen.append(up)
                        n_split += 1
            # 6: merge
            if not do_split or n_split == 0:
                pairs = sorted((d, i, j) for i in range(k) for j in range(i + 1, k) for d in [_dist(cen[i], cen[j])] if d < min_dist)
                used, gone = set(), []
                for d, i, j in pairs:
                    if n_merged >= max_pairs or k - n_merged <= 1:
                        break
                    if i in used or j in used:
                        continue
                    used.update((i, j))
                    ni, nj = cnt[i], cnt[j]
                    if ni + nj > 0:
                        cen[i] = [(ni * a + nj * b) / (ni + nj) for a, b in zip(cen[i], cen[j])]
                    else:
                        cen[i] = [(a + b) / 2.0 for a, b in zip(cen[i], cen[j])]
                    cnt[i] = ni + nj
                    gone.append(j)
                    n_merged += 1
                cen = [c for j, c in enumerate(cen) if j not in gone]
        centers = cen
        history.append(dict(k=len(centers), dropped=dropped, split=n_split, merged=n_merged, n_changed=n_changed))
        quiet = dropped == 0 and n_split == 0 and n_merged == 0
        if quiet and quiet_before and n_changed <= change * n_counted:
            break
        quiet_before = quiet

    rows, _, n_left = run(centers)
    model = IsodataModel(np.array(centers, np.float64).reshape(len(centers), F), weight, e, Q, rg, "uint8" if r.u8 else "float32", feature_names)
    return IsodataResult(r.labels_out(labels), model, np.array([row[0] for row in rows], np.int64), history, n_left)
