"""K25 restated in NumPy (include/rsseg.h: rsseg_segment_features; rsseg/objects.py: training_segments): what the kernel's table
is equal to, bit for bit.  Every column is an integer sum, minimum or maximum over the counted pixels of a segment."""
import numpy as np

GEO = 11
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def effective_labels(seg, mask=None):
    """the label where it is >= 1 and the mask byte is non-zero, else 0"""
    seg = np.asarray(seg).astype(np.int64)
    eff = np.where(seg >= 1, seg, 0)
    if mask is not None:
        eff = np.where(np.asarray(mask) != 0, eff, 0)
    return eff


def perimeter_sides(eff):
    """per pixel, how many of its four neighbours lie outside the image or hold another effective label (0 for label 0)"""
    H, W = eff.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = eff
    sides = np.zeros((H, W), np.int64)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        sides += pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] != eff
    return np.where(eff > 0, sides, 0)


def fixed40(x):
    """llrint(x * 2^40): the product is exact in float64 for a float32 x"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * np.float64(2.0 ** 40)).astype(np.int64)


def sq_fixed24(x):
    """llrint(x * x * 2^24): the square of a float32 is exact in float64, one rounding"""
    d = np.asarray(x, np.float32).astype(np.float64)
    return np.rint(d * d * np.float64(2.0 ** 24)).astype(np.int64)


def object_table_ref(seg, planes=(), mask=None, n_segments=None, geometry=True):
    """int64 [(n + 1), 11 + 4 P]"""
    seg = np.asarray(seg)
    H, W = seg.shape
    n = int(seg.max()) if n_segments is None else int(n_segments)
    eff = effective_labels(seg, mask)
    v = eff > 0
    l = eff[v]
    yy, xx = np.mgrid[0:H, 0:W]
    y, x = yy[v].astype(np.int64), xx[v].astype(np.int64)
    out = np.zeros((n + 1, GEO + 4 * len(planes)), np.int64)
    out[:, 6], out[:, 7], out[:, 8], out[:, 9] = H, -1, W, -1
    np.add.at(out[:, 0], l, 1)
    if geometry:
        for col, val in ((1, y), (2, x), (3, y * y), (4, x * x), (5, y * x), (10, perimeter_sides(eff)[v])):
            np.add.at(out[:, col], l, val)
        np.minimum.at(out[:, 6], l, y)
        np.maximum.at(out[:, 7], l, y)
        np.minimum.at(out[:, 8], l, x)
        np.maximum.at(out[:, 9], l, x)
    for i, p in enumerate(planes):
        p = np.asarray(p)
        if p.dtype == np.uint8:
            q = p[v].astype(np.int64)
            q2 = q * q
        else:
            q, q2 = fixed40(p[v]), sq_fixed24(p[v])
        c = GEO + 4 * i
        out[:, c + 2], out[:, c + 3] = I64_MAX, I64_MIN
        np.add.at(out[:, c], l, q)
        np.add.at(out[:, c + 1], l, q2)
        np.minimum.at(out[:, c + 2], l, q)
        np.maximum.at(out[:, c + 3], l, q)
    return out


def training_segments_ref(seg, roi, mask=None, n_segments=None):
    """(idx, y): the segments with a counted pixel of roi > 0, and their majority ROI class (ties: the smallest label)"""
    eff = effective_labels(seg, mask)
    roi = np.asarray(roi).astype(np.int64)
    n = int(np.asarray(seg).max()) if n_segments is None else int(n_segments)
    votes = np.zeros((n + 1, 256), np.int64)
    v = (eff > 0) & (roi > 0)
    np.add.at(votes, (eff[v], roi[v]), 1)
    idx = np.flatnonzero(votes.max(axis=1) > 0)
    return idx.astype(np.int64), votes[idx].argmax(axis=1).astype(np.uint8)   # argmax: the first maximum
