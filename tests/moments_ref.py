"""NumPy / Python-int restatement of K24 (rsseg_class_moments, include/rsseg.h): the per-label moment table.

A pixel is counted when its mask byte is non-zero (mask None: all) and its label differs from `ignore` (-1: no label is
ignored); a counted label outside 0 ... n_classes - 1 is a ValueError.
float32 planes: v_f = the value, NaN read as +0; u_f = v_f * 2^plane_exp[f] in float64 (exact); a counted pixel with any
|u_f| > 1 (+-inf included) enters no column and is counted in n_left_out.  Otherwise row `label` takes
  column 0 += 1;  column 1 + f += rint(u_f * 2^Q);  column 1 + F + tri(a, b) += rint((u_a * 2^Q) * u_b), a <= b row-major
where (u_a * 2^Q) * u_b is ONE float64 multiplication of two values with 24-bit significands, hence exact, and np.rint rounds
it once to nearest-even.  uint8 planes: the plain integers v_f and v_a * v_b (plane_exp None, Q 0).
The sums are Python ints."""
import numpy as np


def n_columns(F: int) -> int:
    return 1 + F + F * (F + 1) // 2


def moments_table(planes, labels, n_classes, plane_exp=None, Q=0, ignore=-1, mask=None):
    """planes: (F, n) float32 or uint8; labels: (n,) integers; -> (int64 table (n_classes, columns), n_left_out)."""
    planes = np.asarray(planes)
    F, n = planes.shape
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    assert labels.size == n and 0 <= Q <= 50 and (n << Q) < 2 ** 62
    counted = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    if ignore != -1:
        counted &= labels != ignore
    if np.any(counted & ((labels < 0) | (labels >= n_classes))):
        raise ValueError("a counted label outside 0 ... n_classes - 1")
    if planes.dtype == np.uint8:
        assert plane_exp is None and Q == 0
        u = planes.astype(np.float64)
        plane_exp = np.zeros(F, np.int64)
    else:
        assert planes.dtype == np.float32
        x = planes.astype(np.float64)
        x[np.isnan(x)] = 0.0
        with np.errstate(over="ignore"):
            u = np.ldexp(x, np.asarray(plane_exp, np.int64).reshape(F, 1))
    if planes.dtype == np.uint8:
        out_of_range = np.zeros(n, bool)
    else:
        out_of_range = np.any(~(np.abs(u) <= 1.0), axis=0)
    n_left = int((counted & out_of_range).sum())
    keep = np.flatnonzero(counted & ~out_of_range)
    u, lab = u[:, keep], labels[keep]
    y = np.vstack([np.ones((1, keep.size)), u])   # the augmented vector (1, u): the columns are the upper triangle of y y'
    a, b = np.triu_indices(F + 1)
    table = np.zeros((n_classes, n_columns(F)), np.int64)
    two_q = float(2 ** Q)
    for c in np.unique(lab):
        yc = y[:, lab == c]
        t = np.rint((yc[a] * two_q) * yc[b]).astype(np.int64).astype(object)   # (columns, pixels of the class), exact integers
        sums = [int(v) for v in t.sum(axis=1)]                                  # Python-int sums
        sums[0] >>= Q                                                           # y_0 y_0 2^Q = 2^Q per pixel: the count
        table[c] = sums
    return table, n_left


def exact_cov(X, ddof=1):
    """The exact rational covariance of the rows of X (n, F) float32, as Fractions: (F, F) nested lists."""
    from fractions import Fraction
    X = np.asarray(X)
    n, F = X.shape
    cols = [[Fraction(float(v)) for v in X[:, f]] for f in range(F)]
    s = [sum(c, Fraction(0)) for c in cols]
    out = [[None] * F for _ in range(F)]
    for a in range(F):
        for b in range(a, F):
            sab = sum((p * q for p, q in zip(cols[a], cols[b])), Fraction(0))
            out[a][b] = out[b][a] = (sab - s[a] * s[b] / n) / (n - ddof)
    return out
