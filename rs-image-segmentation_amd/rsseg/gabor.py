"""
The Gabor bank of the reference's calculate_gabor_features (indices.py:346-399) on K17 (csrc/k17_correlate.hip).

cv2 is not a dependency: cv2.getGaborKernel is restated here from its documentation (float64 arithmetic, rounded to float32,
stored mirrored), cv2.filter2D as its direct path (include/rsseg.h, rsseg_correlate_u8_f32).  Both restatements are
"unverified-here" in the sense of SURVEY.md §8c; DESIGN.md §4 states the contract.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _lib as L

MAX_KSIZE = 15


def tile_shape() -> Tuple[int, int]:
    """(rows, columns) of the output tile one K17 workgroup owns, asked of the library."""
    th, tw = C.c_int(0), C.c_int(0)
    L.load().rsseg_correlate_tile(C.byref(th), C.byref(tw))
    return th.value, tw.value


def gabor_kernel(ksize: int, sigma: float, theta: float, lambd: float, gamma: float, psi: float = 0.0) -> np.ndarray:
    """cv2.getGaborKernel((ksize, ksize), sigma, theta, lambd, gamma, psi, CV_32F): computed in float64, rounded to float32,
    the value of (x, y) stored at [m - y, m - x]."""
    m = ksize // 2
    c, s = np.cos(np.float64(theta)), np.sin(np.float64(theta))
    ex, ey = -0.5 / (np.float64(sigma) * sigma), -0.5 / ((np.float64(sigma) / gamma) * (np.float64(sigma) / gamma))
    cscale = np.pi * 2.0 / np.float64(lambd)
    y, x = np.mgrid[-m:m + 1, -m:m + 1].astype(np.float64)
    xr = x * c + y * s
    yr = -x * s + y * c
    v = np.exp(ex * xr * xr + ey * yr * yr) * np.cos(cscale * xr + psi)
    return np.ascontiguousarray(v[::-1, ::-1]).astype(np.float32)


def bank_ksize(scale: float) -> int:
    """The reference's kernel size for a scale (indices.py:375-379): 5 * scale truncated, made odd upwards, at least 5."""
    return max(int(5 * scale) | 1, 5)


def gabor_plan(num_scales: int = 4, num_orientations: int = 6) -> List[Tuple[int, np.ndarray]]:
    """[(ksize, taps[nf, ksize, ksize] float32), ...]: one entry per scale in the reference's order, its orientations in the
    reference's order.  The scales are np.logspace(-1, 0.5, num_scales) and the orientations np.arange(0, pi, pi /
    num_orientations) (indices.py:365-366: those two expressions decide the float64 values, so they are the reference's);
    sigma = scale, lambd = 10 * scale, gamma = 0.5, psi = 0 (indices.py:381-389)."""
    thetas = np.arange(0, np.pi, np.pi / num_orientations)
    plan = []
    for s in np.logspace(-1, 0.5, num=num_scales):
        k = bank_ksize(s)
        plan.append((k, np.stack([gabor_kernel(k, s, t, 10 * s, 0.5, 0.0) for t in thetas]).reshape(len(thetas), k, k)))
    return plan


def gabor_bank(ctx, q_u8, h: int, w: int, num_scales: int = 4, num_orientations: int = 6):
    """The min-max normalised responses of the bank on the uint8 device plane q_u8: a list of flat float32 device planes, one
    per filter, scales outer and orientations inner."""
    planes = []
    for ksize, taps in gabor_plan(num_scales, num_orientations):
        if len(taps):
            planes += ctx.filter_bank_norm(q_u8, h, w, taps)
    return planes
