"""NumPy restatement of the Gabor bank (cv2.getGaborKernel, cv2.filter2D's direct path, the min-max normalisation), written
apart from rsseg/gabor.py so that the two can disagree.  OpenCV is not a dependency of the project: the library semantics are
restated from its documentation (unverified-here)."""
import math

import numpy as np


def gabor_kernel_ref(ksize, sigma, theta, lambd, gamma, psi=0.0):
    """Scalar loop: v(x, y) = exp(-xr^2 / (2 sx^2) - yr^2 / (2 sy^2)) * cos(2 pi xr / lambd + psi) in float64, stored as float32
    at [m - y, m - x]."""
    m = ksize // 2
    sx, sy = float(sigma), float(sigma) / float(gamma)
    ct, st = math.cos(float(theta)), math.sin(float(theta))
    k = np.zeros((ksize, ksize), np.float32)
    for y in range(-m, m + 1):
        for x in range(-m, m + 1):
            xr = x * ct + y * st
            yr = y * ct - x * st
            g = math.exp(-(xr * xr) / (2.0 * sx * sx) - (yr * yr) / (2.0 * sy * sy))
            k[m - y, m - x] = np.float32(g * math.cos(2.0 * math.pi * xr / float(lambd) + psi))
    return k


def bank_params(num_scales=4, num_orientations=6):
    """[(ksize, sigma, theta, lambd, gamma)] in the reference's order: scales outer, orientations inner."""
    out = []
    for scale in np.logspace(-1, 0.5, num=num_scales):
        ksize = int(5 * scale)
        ksize += 1 - ksize % 2
        ksize = max(ksize, 5)
        for theta in np.arange(0, np.pi, np.pi / num_orientations):
            out.append((ksize, scale, theta, 10 * scale, 0.5))
    return out


def reflect101(i, n):
    """BORDER_REFLECT_101 index, reflected as often as needed; an axis of one element reads that element."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i = abs(i) % p
    return p - i if i >= n else i


def pad101(u8, m):
    h, w = u8.shape
    ys = [reflect101(y, h) for y in range(-m, h + m)]
    xs = [reflect101(x, w) for x in range(-m, w + m)]
    return u8[np.ix_(ys, xs)]


def correlate_ref(u8, taps, dtype=np.float32):
    """r[y, x] = sum_i sum_j k[i, j] * u8[y + i - m, x + j - m], taps in row-major order, every product and every sum
    rounded to `dtype`, started from +0.  float32 is the contract; float64 the yardstick."""
    k = np.asarray(taps)
    m = k.shape[0] // 2
    h, w = u8.shape
    p = pad101(np.asarray(u8), m).astype(dtype)
    acc = np.zeros((h, w), dtype)
    for i in range(k.shape[0]):
        for j in range(k.shape[1]):
            acc = acc + dtype(k[i, j]) * p[i:i + h, j:j + w]
    return acc


def gamma_bound(u8, taps):
    """gamma_n * sum |k * x| per pixel, gamma_n = n u / (1 - n u), u = 2^-24, n the non-zero taps: the float32 rounding
    bound of a recursive sum of n products (Higham, Accuracy and Stability of Numerical Algorithms, §3.1)."""
    k = np.asarray(taps, np.float64)
    n = int(np.count_nonzero(k))
    u = 2.0 ** -24
    g = n * u / (1.0 - n * u)
    return g * correlate_ref(u8, np.abs(k), np.float64)


def normalise_ref(r):
    """(r - min) / (max - min + 1e-10), float32 throughout."""
    r = np.asarray(r, np.float32)
    mn, mx = r.min(), r.max()
    den = np.float32(np.float32(mx - mn) + np.float32(1e-10))
    return (r - mn) / den


def bank_ref(u8, num_scales=4, num_orientations=6):
    return [normalise_ref(correlate_ref(u8, gabor_kernel_ref(*p), np.float32)) for p in bank_params(num_scales, num_orientations)]
