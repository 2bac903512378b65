"""NumPy restatement of K21 (rsseg_warp_poly, include/rsseg.h), operation for operation: what the kernel is equal to, bit for
bit.  Every arithmetic step below is one float64 NumPy operation on whole arrays, in the order the kernel performs it."""
from __future__ import annotations

import numpy as np

METHODS = ("nearest", "bilinear", "cubic")
INT_RANGE = {np.dtype(np.uint8): (0.0, 255.0), np.dtype(np.int16): (-32768.0, 32767.0), np.dtype(np.uint16): (0.0, 65535.0),
             np.dtype(np.int32): (-2147483648.0, 2147483647.0)}


def source_coords(coef, cx, cy, Ho, Wo):
    """(u, v): the source position of every output pixel, in pixel-corner coordinates."""
    p = [np.float64(x) for x in np.asarray(coef, np.float64).reshape(12)]
    X = (np.arange(Wo, dtype=np.float64)[None, :] + 0.5) - np.float64(cx)
    Y = (np.arange(Ho, dtype=np.float64)[:, None] + 0.5) - np.float64(cy)
    X, Y = np.broadcast_arrays(X, Y)
    XX, XY, YY = X * X, X * Y, Y * Y
    with np.errstate(all="ignore"):
        u = ((((p[0] + p[1] * X) + p[2] * Y) + p[3] * XX) + p[4] * XY) + p[5] * YY
        v = ((((p[6] + p[7] * X) + p[8] * Y) + p[9] * XX) + p[10] * XY) + p[11] * YY
    return u, v


def keys_near(t):
    t2 = t * t
    t3 = t2 * t
    return (1.5 * t3 - 2.5 * t2) + 1.0


def keys_far(t):
    t2 = t * t
    t3 = t2 * t
    return ((-0.5 * t3 + 2.5 * t2) - 4.0 * t) + 2.0


def keys_weights(t):
    """The four weights of the taps i = -1, 0, 1, 2 for the fraction t in [0, 1): they lie at |t - i| = t + 1, t, 1 - t, 2 - t."""
    return [keys_far(t + 1.0), keys_near(t), keys_near(1.0 - t), keys_far(2.0 - t)]


def finish(val, out_dtype, saturate=True):
    """float64 -> the output dtype: integers rint (half to even) and saturate, float32 is one cast."""
    dt = np.dtype(out_dtype)
    if dt in INT_RANGE:
        lo, hi = INT_RANGE[dt]
        r = np.rint(val)
        if not saturate:
            return r
        return np.clip(r, lo, hi).astype(dt)
    return val.astype(dt)


def warp(planes, coef, cx, cy, Ho, Wo, method="nearest", fill=0, out_dtype=None, saturate=True):
    """planes: (H, W) arrays of one dtype.  Returns (list of (Ho, Wo) arrays, uint8 mask, n_valid).  saturate=False (tests
    only): integer results come back as the rounded float64 before the clip."""
    planes = [np.asarray(p) for p in planes]
    H, W = planes[0].shape
    dt = np.dtype(planes[0].dtype if out_dtype is None else out_dtype)
    u, v = source_coords(coef, cx, cy, Ho, Wo)
    with np.errstate(invalid="ignore"):
        ok = (u >= 0.0) & (u < np.float64(W)) & (v >= 0.0) & (v < np.float64(H))
    uu, vv = u[ok], v[ok]   # invalid coordinates are never converted
    fx, fy = uu - 0.5, vv - 0.5
    outs = []
    if method == "nearest":
        x = np.clip(np.floor(fx + 0.5).astype(np.int64), 0, W - 1)
        y = np.clip(np.floor(fy + 0.5).astype(np.int64), 0, H - 1)
    elif method in ("bilinear", "cubic"):
        bx, by = np.floor(fx), np.floor(fy)
        tx, ty = fx - bx, fy - by
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        if method == "cubic":
            wx, wy = keys_weights(tx), keys_weights(ty)
    else:
        raise ValueError(f"unknown method {method!r}")
    for g in planes:
        full = not saturate and dt in INT_RANGE
        o = np.full((Ho, Wo), fill, dtype=np.float64 if full else dt)
        with np.errstate(all="ignore"):
            if method == "nearest":
                val = g[y, x]
                o[ok] = val if val.dtype == dt else val.astype(dt)
            elif method == "bilinear":
                x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
                y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
                g00, g01 = g[y0, x0].astype(np.float64), g[y0, x1].astype(np.float64)
                g10, g11 = g[y1, x0].astype(np.float64), g[y1, x1].astype(np.float64)
                ux = 1.0 - tx
                top = g00 * ux + g01 * tx
                bot = g10 * ux + g11 * tx
                o[ok] = finish(top * (1.0 - ty) + bot * ty, dt, saturate)
            else:
                xs = [np.clip(ix - 1 + i, 0, W - 1) for i in range(4)]
                ys = [np.clip(iy - 1 + j, 0, H - 1) for j in range(4)]
                acc = np.zeros(uu.shape, np.float64)
                for j in range(4):
                    row = np.zeros(uu.shape, np.float64)
                    for i in range(4):
                        row = row + wx[i] * g[ys[j], xs[i]].astype(np.float64)
                    acc = acc + wy[j] * row
                o[ok] = finish(acc, dt, saturate)
        outs.append(o)
    return outs, ok.astype(np.uint8), int(ok.sum())


def affine_coef(A, Ho, Wo):
    """coef, cx, cy of the backward affine A = [[a, b, c], [d, e, f]] that maps output pixel-corner coordinates
    (c + 0.5, r + 0.5) to source ones: u = a * x + b * y + c.  Re-centred on (Wo / 2, Ho / 2) as warp_plan does."""
    A = np.asarray(A, np.float64)
    cx, cy = Wo / 2, Ho / 2
    p = [A[0, 2] + A[0, 0] * cx + A[0, 1] * cy, A[0, 0], A[0, 1], 0.0, 0.0, 0.0]
    q = [A[1, 2] + A[1, 0] * cx + A[1, 1] * cy, A[1, 0], A[1, 1], 0.0, 0.0, 0.0]
    return np.array(p + q, np.float64), cx, cy
