"""K19 restated in NumPy (include/rsseg.h, rsseg_valid_mask / rsseg_compact_planes / rsseg_expand_plane), and the scenes and
masks the CPU and GPU tests of the masked classifiers share."""
import numpy as np

VALID_NAN, VALID_INF, VALID_VALUE = 1, 2, 4


def compact(plane, mask):
    """plane[mask != 0]: the valid pixels in raster order."""
    return np.ascontiguousarray(np.asarray(plane).reshape(-1)[np.asarray(mask).reshape(-1) != 0])


def expand(compacted, mask, fill):
    """out[i] = compacted[rank(i)] where the mask is set, `fill` elsewhere; flat, in the compacted plane's dtype."""
    m = np.asarray(mask).reshape(-1) != 0
    compacted = np.asarray(compacted)
    full = np.empty(m.size, compacted.dtype)
    full[m] = compacted
    return np.where(m, full, np.asarray(fill, compacted.dtype))


def nodata_as(nodata, dtype):
    """`nodata` cast to the planes' type; None when the type cannot hold it (it then matches nothing)."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.uint8(nodata) if 0 <= nodata <= 255 and float(nodata).is_integer() else None
    return dtype.type(nodata)


def valid_mask(planes, flags, nodata=0.0, and_mask=None):
    """uint8 0 / 1: a pixel is valid iff no plane holds NaN (VALID_NAN), +-inf (VALID_INF) or the nodata value (VALID_VALUE)
    there, and and_mask (when given) is non-zero there."""
    ok = np.ones(np.asarray(planes[0]).size, bool)
    for p in planes:
        p = np.asarray(p).reshape(-1)
        if p.dtype.kind == "f":
            if flags & VALID_NAN:
                ok &= ~np.isnan(p)
            if flags & VALID_INF:
                ok &= ~np.isinf(p)
        if flags & VALID_VALUE:
            v = nodata_as(nodata, p.dtype)
            if v is not None:
                ok &= ~(p == v)
    if and_mask is not None:
        ok &= np.asarray(and_mask).reshape(-1) != 0
    return ok.astype(np.uint8)


# ---- scenes ------------------------------------------------------------------------------------------------------
def collar_and_holes(h, w, border, hole_share, seed):
    """A nodata collar `border` pixels wide plus a share of random holes: (h, w) uint8, 1 = valid."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    m[border:h - border, border:w - border] = 1
    m[rng.random((h, w)) < hole_share] = 0
    return m


def blob_scene(dtype=np.float32):
    """48 x 64 pixels, four well separated blobs in 5 features, a collar plus 5 % holes (1792 valid, 1280 nodata); the nodata
    pixels hold NaN, as rsseg.stages reads a GeoTIFF's nodata.  Fitted over all pixels (NaN -> 0), one of the four clusters goes
    to the nodata pixels alone and two blobs are merged; fitted over the valid pixels, all four are found (441 / 465 / 480 / 406).  Returns (planes [(48, 64)] * 5, mask (48, 64) uint8)."""
    h, w, F, k = 48, 64, 5, 4
    rng = np.random.default_rng(7)
    centres = rng.uniform(-4.0, 4.0, (k, F)) + 6.0 * np.eye(k, F)
    which = rng.integers(0, k, h * w)
    X = (centres[which] + 0.3 * rng.standard_normal((h * w, F))).astype(dtype)
    mask = collar_and_holes(h, w, 6, 0.05, 11)
    X[mask.reshape(-1) == 0] = np.nan
    return [np.ascontiguousarray(X[:, f]).reshape(h, w) for f in range(F)], mask
