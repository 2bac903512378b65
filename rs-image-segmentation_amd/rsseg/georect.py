"""
Geometric correction from ground control points (K21) — beyond the reference, whose geometric_correction(bands_data, gcps)
ignores its GCPs and warps with the identity matrix (modules/features/preprocessing.py:77-102).

The host part fits the transform in float64 and composes it with the output grid; the device part (rsseg_warp_poly,
csrc/k21_warp.hip) resamples every band in one launch.

    gcps = parse_gcps("scene.gcp")                    # pixel line x y, one GCP per line
    t = fit_gcp_transform(gcps, order=1)              # forward and backward least-squares polynomials, residuals, RMSE
    Ho, Wo, out_transform = output_grid(t, (H, W))    # a north-up grid over the forward image of the source's border
    plan = warp_plan(t, (Ho, Wo), out_transform, (H, W))
    planes, mask, n_valid = warp_planes(ctx, bands, (H, W), plan, method="bilinear")

Coordinates follow GDAL: pixel / line are measured from the outer corner of the top-left pixel (the first pixel's centre is
(0.5, 0.5)), x / y are map coordinates, and transforms are in rasterio order (a, b, c, d, e, f): x = a * px + b * py + c,
y = d * px + e * py + f.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

METHODS = ("nearest", "bilinear", "cubic")
N_TERMS = {1: 3, 2: 6}


def parse_gcps(text_or_path) -> np.ndarray:
    """(N, 4) float64 array of `pixel line x y` rows.  The argument is a path, or the text itself (anything holding a
    newline, or that names no file).  Values are separated by whitespace or commas; `#` starts a comment."""
    s = os.fspath(text_or_path) if not isinstance(text_or_path, str) else text_or_path
    if "\n" not in s and os.path.exists(s):
        with open(s, "r", encoding="utf-8") as f:
            s = f.read()
    rows = []
    for no, line in enumerate(s.splitlines(), 1):
        body = line.split("#", 1)[0].replace(",", " ").split()
        if not body:
            continue
        if len(body) != 4:
            raise ValueError(f"parse_gcps: line {no}: {len(body)} values, expected 4 (pixel line x y): {line.strip()!r}")
        try:
            vals = [float(v) for v in body]
        except ValueError:
            raise ValueError(f"parse_gcps: line {no}: not a number in {line.strip()!r}") from None
        if not all(math.isfinite(v) for v in vals):
            raise ValueError(f"parse_gcps: line {no}: non-finite value in {line.strip()!r}")
        rows.append(vals)
    return np.array(rows, np.float64).reshape(-1, 4)


def poly_terms(a, b, order: int) -> np.ndarray:
    """The design matrix of the polynomial in (a, b): columns 1, a, b and for order 2 also a*a, a*b, b*b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cols = [np.ones_like(a), a, b]
    if order == 2:
        cols += [a * a, a * b, b * b]
    return np.stack(cols, axis=-1)


def _normalisation(a: np.ndarray, b: np.ndarray) -> Tuple[float, float, float, float]:
    """(centre a, centre b, scale a, scale b): the mean and the largest deviation from it (1 when all values are equal)."""
    ca, cb = float(a.mean()), float(b.mean())
    sa, sb = float(np.abs(a - ca).max()), float(np.abs(b - cb).max())
    return ca, cb, sa if sa > 0 else 1.0, sb if sb > 0 else 1.0


@dataclass
class GcpTransform:
    """Least-squares polynomials in both directions.  forward: (pixel, line) -> (x, y); backward: (x, y) -> (pixel, line).
    Each is evaluated on normalised inputs (v - centre) / scale: fwd_norm / bwd_norm = (centre a, centre b, scale a, scale b);
    fwd / bwd: (2, n_terms) coefficients of poly_terms.  residuals: (N, 2) backward(x, y) - (pixel, line) per GCP, in source
    pixels; rmse: sqrt(mean(dp^2 + dl^2))."""
    order: int
    fwd: np.ndarray
    fwd_norm: Tuple[float, float, float, float]
    bwd: np.ndarray
    bwd_norm: Tuple[float, float, float, float]
    residuals: np.ndarray
    rmse: float

    @staticmethod
    def _eval(coef, norm, a, b, order):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        t = poly_terms((a - norm[0]) / norm[2], (b - norm[1]) / norm[3], order)
        return t @ coef[0], t @ coef[1]

    def forward(self, pixel, line):
        return self._eval(self.fwd, self.fwd_norm, pixel, line, self.order)

    def backward(self, x, y):
        return self._eval(self.bwd, self.bwd_norm, x, y, self.order)

    def to_json(self) -> str:
        return json.dumps({"order": self.order, "fwd": self.fwd.tolist(), "fwd_norm": list(self.fwd_norm), "bwd": self.bwd.tolist(),
                           "bwd_norm": list(self.bwd_norm), "residuals": self.residuals.tolist(), "rmse": self.rmse})

    @classmethod
    def from_json(cls, text: str) -> "GcpTransform":
        d = json.loads(text)
        return cls(int(d["order"]), np.array(d["fwd"], np.float64), tuple(d["fwd_norm"]), np.array(d["bwd"], np.float64),
                   tuple(d["bwd_norm"]), np.array(d["residuals"], np.float64).reshape(-1, 2), float(d["rmse"]))


def _lstsq(a, b, ta, tb, order: int, what: str):
    norm = _normalisation(a, b)
    A = poly_terms((a - norm[0]) / norm[2], (b - norm[1]) / norm[3], order)
    sol, _, rank, _ = np.linalg.lstsq(A, np.stack([ta, tb], axis=1), rcond=None)
    if rank < A.shape[1]:
        raise ValueError(f"fit_gcp_transform: the {what} design matrix is rank-deficient (rank {rank} of {A.shape[1]}): the GCPs are "
                         "collinear or coincide")
    return np.ascontiguousarray(sol.T), norm


def fit_gcp_transform(gcps, order: int = 1) -> GcpTransform:
    """Least-squares polynomial of order 1 (3 coefficients per axis, >= 3 GCPs) or 2 (6 per axis, >= 6 GCPs) in both
    directions, np.linalg.lstsq in float64 on centred and scaled coordinates."""
    if order not in N_TERMS:
        raise ValueError(f"fit_gcp_transform: order = {order!r} is not 1 or 2")
    g = np.asarray(gcps, np.float64)
    if g.ndim != 2 or g.shape[1] != 4:
        raise ValueError(f"fit_gcp_transform: gcps must be an (N, 4) array of pixel, line, x, y, not {g.shape}")
    if not np.isfinite(g).all():
        raise ValueError("fit_gcp_transform: gcps holds a non-finite value")
    if g.shape[0] < N_TERMS[order]:
        raise ValueError(f"fit_gcp_transform: too few GCPs: {g.shape[0]} given, order {order} needs at least {N_TERMS[order]}")
    px, ln, x, y = g.T
    fwd, fwd_norm = _lstsq(px, ln, x, y, order, "forward")
    bwd, bwd_norm = _lstsq(x, y, px, ln, order, "backward")
    t = GcpTransform(order, fwd, fwd_norm, bwd, bwd_norm, np.zeros((0, 2)), 0.0)
    bp, bl = t.backward(x, y)
    t.residuals = np.stack([bp - px, bl - ln], axis=1)
    t.rmse = float(np.sqrt(np.mean(np.sum(t.residuals * t.residuals, axis=1))))
    return t


def output_grid(transform: GcpTransform, src_shape, pixel_size: Optional[float] = None):
    """(Ho, Wo, out_transform): a north-up grid (a, 0, c, 0, -a, f) that covers the forward image of the source's border.
    Order 1 maps the four corners, order 2 samples the border at every pixel edge.  pixel_size defaults to the square
    root of |det| of the forward polynomial's linear part at the source's centre."""
    H, W = int(src_shape[0]), int(src_shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"output_grid: src_shape = {tuple(src_shape)}: both sides must be at least 1")
    if transform.order == 1:
        bp, bl = np.array([0.0, W, 0.0, W]), np.array([0.0, 0.0, H, H])
    else:
        ex, ey = np.arange(W + 1, dtype=np.float64), np.arange(H + 1, dtype=np.float64)
        bp = np.concatenate([ex, ex, np.zeros(H + 1), np.full(H + 1, float(W))])
        bl = np.concatenate([np.zeros(W + 1), np.full(W + 1, float(H)), ey, ey])
    x, y = transform.forward(bp, bl)
    if pixel_size is None:
        # the Jacobian of forward at the centre, by the polynomial's own derivative
        cp, cl, sp, sl = transform.fwd_norm
        a, b = (W / 2 - cp) / sp, (H / 2 - cl) / sl
        da = np.array([0.0, 1.0, 0.0] + ([2 * a, b, 0.0] if transform.order == 2 else [])) / sp
        db = np.array([0.0, 0.0, 1.0] + ([0.0, a, 2 * b] if transform.order == 2 else [])) / sl
        J = np.array([[transform.fwd[0] @ da, transform.fwd[0] @ db], [transform.fwd[1] @ da, transform.fwd[1] @ db]])
        pixel_size = math.sqrt(abs(float(np.linalg.det(J))))
    ps = float(pixel_size)
    if not (math.isfinite(ps) and ps > 0):
        raise ValueError(f"output_grid: pixel_size = {pixel_size!r} must be finite and > 0")
    xmin, xmax, ymin, ymax = float(x.min()), float(x.max()), float(y.min()), float(y.max())
    Wo, Ho = max(1, math.ceil((xmax - xmin) / ps)), max(1, math.ceil((ymax - ymin) / ps))
    return Ho, Wo, (ps, 0.0, xmin, 0.0, -ps, ymax)


@dataclass
class WarpPlan:
    """What rsseg_warp_poly takes: coef = (p0..p5, q0..q5), the source pixel / line as polynomials of the centred output pixel
    coordinates X = (c + 0.5) - cx, Y = (r + 0.5) - cy with terms 1, X, Y, X*X, X*Y, Y*Y."""
    coef: np.ndarray
    cx: float
    cy: float
    out_shape: Tuple[int, int]
    src_shape: Tuple[int, int]
    out_transform: Tuple[float, float, float, float, float, float]


def _lin_mul(l, m):
    """The product of two linear forms l0 + l1 X + l2 Y as coefficients of 1, X, Y, X*X, X*Y, Y*Y."""
    return np.array([l[0] * m[0], l[0] * m[1] + l[1] * m[0], l[0] * m[2] + l[2] * m[0], l[1] * m[1], l[1] * m[2] + l[2] * m[1], l[2] * m[2]])


def warp_plan(transform: GcpTransform, out_shape, out_transform, src_shape) -> WarpPlan:
    """Composes the backward polynomial with out_transform, in float64, into one polynomial per source axis over the
    centred output pixel coordinates (cx = Wo / 2, cy = Ho / 2).  For order 1 the quadratic coefficients are 0."""
    Ho, Wo = int(out_shape[0]), int(out_shape[1])
    a, b, c, d, e, f = (float(v) for v in out_transform)
    cx, cy = Wo / 2, Ho / 2
    mx, my, sx, sy = transform.bwd_norm
    # the normalised map coordinates as linear forms of (X, Y)
    xn = np.array([(a * cx + b * cy + c - mx) / sx, a / sx, b / sx])
    yn = np.array([(d * cx + e * cy + f - my) / sy, d / sy, e / sy])
    lin = lambda l: np.array([l[0], l[1], l[2], 0.0, 0.0, 0.0])
    terms = [np.array([1.0, 0, 0, 0, 0, 0]), lin(xn), lin(yn)]
    if transform.order == 2:
        terms += [_lin_mul(xn, xn), _lin_mul(xn, yn), _lin_mul(yn, yn)]
    T = np.stack(terms)   # (n_terms, 6)
    coef = np.concatenate([transform.bwd[0] @ T, transform.bwd[1] @ T]).astype(np.float64)
    if not np.isfinite(coef).all():
        raise ValueError("warp_plan: the composed coefficients are not finite")
    return WarpPlan(coef, cx, cy, (Ho, Wo), (int(src_shape[0]), int(src_shape[1])), (a, b, c, d, e, f))


def _torch_dtype(dt):
    torch = __import__("torch")
    if dt is None or isinstance(dt, torch.dtype):
        return dt
    return getattr(torch, np.dtype(dt).name)


def warp_planes(ctx, planes: Sequence, src_shape, plan: WarpPlan, method: str = "nearest", fill=0, out_dtype=None, want_mask: bool = True):
    """Resamples the planes (host arrays or device tensors of one dtype, src_shape pixels each, at most 16) by `plan` on
    the device: (flat device planes of plan.out_shape, uint8 device mask or None, n_valid).  out_dtype: None (the planes'
    dtype), float32 or float64, as a NumPy or torch dtype."""
    from .runtime import default_context
    torch = __import__("torch")
    ctx = ctx or default_context()
    H, W = int(src_shape[0]), int(src_shape[1])
    if (H, W) != tuple(plan.src_shape):
        raise ValueError(f"warp_planes: src_shape {(H, W)} is not the plan's {tuple(plan.src_shape)}")
    dev = []
    for i, p in enumerate(planes):
        if not isinstance(p, torch.Tensor):
            a = np.ascontiguousarray(p)
            if a.dtype == np.int64 or a.dtype.kind not in "iuf" or not hasattr(torch, a.dtype.name):
                raise ValueError(f"warp_planes: planes[{i}] is {a.dtype.name}: uint8, int16, uint16, int32, float32 or float64 are taken")
            p = ctx.to_device(a)
        if p.numel() != H * W:
            raise ValueError(f"warp_planes: planes[{i}] holds {p.numel()} pixels, src_shape {(H, W)} has {H * W}")
        dev.append(p.reshape(-1))
    Ho, Wo = plan.out_shape
    return ctx.warp_poly(dev, H, W, plan.coef, plan.cx, plan.cy, Ho, Wo, method=method, fill=fill, out_dtype=_torch_dtype(out_dtype),
                         want_mask=want_mask)


def geometric_correction_gcps(bands_data, gcps, order: int = 1, method: str = "nearest", pixel_size: Optional[float] = None):
    """Host in, host out: the bands (2-D arrays of one dtype and shape) rectified by the transform fitted to `gcps`
    ((N, 4) pixel, line, x, y) onto output_grid's north-up grid.  Returns (bands, out_transform, valid_mask, transform);
    pixels outside the source are 0 and 0 in valid_mask (uint8)."""
    bands = [np.asarray(b) for b in bands_data]
    if not bands or any(b.ndim != 2 or b.shape != bands[0].shape for b in bands):
        raise ValueError("geometric_correction_gcps: bands_data must hold 2-D bands of one shape")
    t = fit_gcp_transform(gcps, order)
    H, W = bands[0].shape
    Ho, Wo, out_transform = output_grid(t, (H, W), pixel_size)
    plan = warp_plan(t, (Ho, Wo), out_transform, (H, W))
    outs, mask, _ = warp_planes(None, bands, (H, W), plan, method=method)
    return [o.cpu().numpy().reshape(Ho, Wo) for o in outs], out_transform, mask.cpu().numpy().reshape(Ho, Wo), t


def correction_record(transform: GcpTransform, plan: WarpPlan, method: str, n_valid: int) -> dict:
    """What the preprocessing stage writes beside its output (OUT_geometric_correction.json)."""
    return {"order": transform.order, "method": method, "forward": transform.fwd.tolist(), "forward_norm": list(transform.fwd_norm),
            "backward": transform.bwd.tolist(), "backward_norm": list(transform.bwd_norm), "residuals": transform.residuals.tolist(),
            "rmse": transform.rmse, "output_shape": list(plan.out_shape), "output_transform": list(plan.out_transform),
            "warp_coef": plan.coef.tolist(), "n_valid": int(n_valid)}
