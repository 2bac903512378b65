"""
Superpixels and object-based class maps on the GPU (K23, csrc/k23_slic.hip).  This goes beyond the reference, which has no
segmentation step: slic() cuts a feature stack into superpixels, segment_means() describes them, object_majority() /
object_classify() vote a per-pixel class map into one class per object, paint() writes a per-segment table back to the raster.

A segment map is (H, W) int32: 0 where the pixel is masked, 1 ... n_segments elsewhere, numbered in the order of the
segments' first pixel.  Every function takes NumPy arrays or device tensors and returns NumPy, or with device=True device
tensors.  Semantics: include/rsseg.h (rsseg_slic_u8, rsseg_segment_*), restated in NumPy in tests/slic_ref.py; the results are
equal to that restatement bit for bit.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from .postclass import check_class_map
from .runtime import Context, RssegUnsupported, default_context

MAX_PLANES = 16
FIXED_ONE = float(2 ** 40)       # the quantum of the float32 sums is 2^-40
FIXED_LIMIT = float(2 ** 11)     # |x| below this is summed exactly
FIXED_AREA_LIMIT = float(2 ** 23)  # area * max|x| below this keeps a segment's sum inside int64


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _check_count(v, name: str, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or int(v) != v or int(v) < 0:
        raise ValueError(f"{what}: {name}={v!r} is not a non-negative integer")
    return int(v)


def _check_nodata(nodata, what: str) -> int:
    if nodata is None:
        return -1
    if isinstance(nodata, (bool, np.bool_)) or int(nodata) != nodata or not 0 <= int(nodata) <= 255:
        raise ValueError(f"{what}: nodata={nodata!r} is neither None nor an integer in 0..255")
    return int(nodata)


def _context(ctx: Optional[Context], what: str) -> Context:
    ctx = ctx or default_context()
    if ctx.world > 1:
        raise RssegUnsupported(f"{what}: the raster and its segment map must be whole on one GPU (this context has {ctx.world} ranks); "
                               "superpixels and their sums cross stripes")
    return ctx


def _plane_list(x, name: str, what: str):
    """A stack as a list of (H, W) planes: a sequence of 2-D planes or one (P, H, W) array / tensor."""
    if _is_tensor(x) or isinstance(x, np.ndarray):
        if x.ndim == 2:
            return [x]
        if x.ndim == 3:
            return [x[i] for i in range(x.shape[0])]
        raise ValueError(f"{what}: {name} must be (H, W), (P, H, W) or a list of (H, W) planes, got shape {tuple(x.shape)}")
    planes = list(x)
    for i, p in enumerate(planes):
        if not (_is_tensor(p) or isinstance(p, np.ndarray)) or p.ndim != 2:
            raise ValueError(f"{what}: {name}[{i}] is not an (H, W) array")
    return planes


def _check_shapes(planes, name: str, what: str, shape=None):
    if not planes and shape is None:
        raise ValueError(f"{what}: {name} is empty")
    shape = tuple(planes[0].shape) if shape is None else tuple(shape)
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what}: {name} is empty: shape {shape}")
    for i, p in enumerate(planes):
        if tuple(p.shape) != shape:
            raise ValueError(f"{what}: {name}[{i}] has shape {tuple(p.shape)}, expected {shape}")
    if shape[0] * shape[1] > 2 ** 31 - 1:
        raise ValueError(f"{what}: {name} holds more than 2^31 - 1 pixels")
    return shape


def _is_u8(p) -> bool:
    import torch
    return p.dtype == (torch.uint8 if _is_tensor(p) else np.uint8)


def _dev_flat(ctx: Context, p, dtype):
    """The plane as a flat device tensor of `dtype` (a torch dtype)."""
    import torch
    if _is_tensor(p):
        return p.to(ctx.device).contiguous().reshape(-1).to(dtype)
    np_dt = {torch.uint8: np.uint8, torch.float32: np.float32, torch.int32: np.int32}[dtype]
    return ctx.to_device(np.ascontiguousarray(p, dtype=np_dt).reshape(-1))


def _check_mask(mask, shape, what: str):
    if mask is None:
        return None
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: mask has shape {tuple(mask.shape)}, expected {tuple(shape)}")
    return mask


def _dev_mask(ctx: Context, mask):
    import torch
    if mask is None:
        return None
    if _is_tensor(mask):
        return (mask.to(ctx.device) != 0).to(torch.uint8).contiguous().reshape(-1)
    return ctx.to_device((np.asarray(mask) != 0).astype(np.uint8).reshape(-1))


def check_segments(segments, what: str = "segments"):
    """The segment map as something uploadable: (H, W) integers, none negative.  Returns it (int32 where it is a NumPy array)."""
    if _is_tensor(segments):
        import torch
        if segments.dim() != 2 or segments.numel() == 0:
            raise ValueError(f"{what}: segments must be a non-empty (H, W) map, got shape {tuple(segments.shape)}")
        if segments.dtype.is_floating_point or segments.dtype.is_complex or segments.dtype == torch.bool:
            raise ValueError(f"{what}: segments must hold integer labels, got {segments.dtype}")
        return segments
    a = np.asarray(segments)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"{what}: segments must be a non-empty (H, W) map, got shape {a.shape}")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: segments must hold integer labels, got dtype {a.dtype}")
    if int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 1:
        raise ValueError(f"{what}: segments holds a label outside 0 ... 2^31 - 1")
    return np.ascontiguousarray(a, dtype=np.int32)


def _upload_segments(ctx: Context, seg, n_segments):
    """(flat int32 device plane, H, W, n_segments)"""
    import torch
    h, w = int(seg.shape[0]), int(seg.shape[1])
    d = _dev_flat(ctx, seg, torch.int32)
    if n_segments is None:
        n_segments = int(d.max())
    return d, h, w, int(n_segments)


def slic_step(shape, n_segments: int) -> int:
    """The grid step that gives about n_segments superpixels on an image of this shape."""
    return max(2, int(round(math.sqrt(shape[0] * shape[1] / n_segments))))


def _check_slic(step, n_segments, compactness, max_iter, min_area, shape):
    if (step is None) == (n_segments is None):
        raise ValueError("slic: give exactly one of step and n_segments")
    if step is None:
        if isinstance(n_segments, (bool, np.bool_)) or int(n_segments) != n_segments or int(n_segments) < 1:
            raise ValueError(f"slic: n_segments={n_segments!r} is not a positive integer")
        step = slic_step(shape, int(n_segments))
        step = min(step, 4096)
    if isinstance(step, (bool, np.bool_)) or int(step) != step or not 2 <= int(step) <= 4096:
        raise ValueError(f"slic: step={step!r} is not an integer in 2..4096")
    step = int(step)
    if isinstance(compactness, (bool, np.bool_)) or not np.isfinite(compactness) or compactness < 0:
        raise ValueError(f"slic: compactness={compactness!r} is not a finite non-negative number")
    max_iter = _check_count(max_iter, "max_iter", "slic")
    min_area = max(1, step * step // 4) if min_area is None else _check_count(min_area, "min_area", "slic")
    return step, float(compactness), min(max_iter, 2 ** 31 - 1), min(min_area, 2 ** 31 - 1)


def slic_weight(compactness: float, step: int) -> float:
    """The weight of the squared pixel distance beside the squared colour distance: (m * m) / (S * S), in float64."""
    return (float(compactness) * float(compactness)) / (float(step) * float(step))


def quantise_planes(ctx: Context, planes: Sequence, ranges=None):
    """The planes slic() segments, as flat uint8 device planes: uint8 planes as they are, float planes through
    Context.normalize_quantize_u8(plane, lo, hi, 255.0) with lo / hi = ranges[p] or the plane's finite min / max."""
    import torch
    out = []
    for i, p in enumerate(planes):
        if _is_u8(p):
            out.append(_dev_flat(ctx, p, torch.uint8))
            continue
        dt = p.dtype
        if not (dt.is_floating_point if _is_tensor(p) else np.issubdtype(dt, np.floating)):
            raise ValueError(f"slic: features[{i}] must be uint8 or floating point, got {dt}")
        d = _dev_flat(ctx, p, torch.float32)
        if ranges is not None and ranges[i] is not None:
            lo, hi = float(ranges[i][0]), float(ranges[i][1])
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError(f"slic: ranges[{i}]={ranges[i]!r} is not a finite (lo, hi) with lo <= hi")
        else:
            fin = d[torch.isfinite(d)]
            lo, hi = (float(fin.min()), float(fin.max())) if fin.numel() else (0.0, 0.0)
        out.append(ctx.normalize_quantize_u8(d, lo, hi, 255.0))
    return out


def slic(features, step: Optional[int] = None, n_segments: Optional[int] = None, compactness: float = 10.0, max_iter: int = 10,
         min_area: Optional[int] = None, mask=None, ranges=None, ctx: Optional[Context] = None, device: bool = False,
         return_stats: bool = False):
    """SLIC superpixels of a feature stack (1 ... 16 planes: a list of (H, W) planes or a (P, H, W) array).
    step: the grid step S in pixels, or n_segments: about how many superpixels are wanted (S = max(2, round(sqrt(H W / n)))).
    compactness m: the squared pixel distance weighs (m / S)^2 beside the squared distance of the 8-bit features.
    max_iter: assignment iterations at most (they stop when one changes no label); 0 leaves the grid cells.
    min_area: connected pieces smaller than this are merged into a neighbour (default S * S // 4; <= 1: none).
    mask: (H, W), non-zero = valid; masked pixels get segment 0 and take no part.
    ranges: per float plane (lo, hi) to quantise with instead of its own finite min / max (None entries: its own).
    Returns the (H, W) int32 segment map; with return_stats also {"n_segments", "n_iter", "n_regrown", "step", "compactness",
    "min_area", "max_iter"}."""
    planes = _plane_list(features, "features", "slic")
    shape = _check_shapes(planes, "features", "slic")
    if len(planes) > MAX_PLANES:
        raise ValueError(f"slic: features holds {len(planes)} planes, at most {MAX_PLANES} are segmented at once")
    if ranges is not None and len(ranges) != len(planes):
        raise ValueError(f"slic: ranges has {len(ranges)} entries for {len(planes)} planes")
    step, m, max_iter, min_area = _check_slic(step, n_segments, compactness, max_iter, min_area, shape)
    mask = _check_mask(mask, shape, "slic")
    ctx = _context(ctx, "slic")
    q = quantise_planes(ctx, planes, ranges)
    labels, ns, ni, nr = ctx.slic_u8(q, shape[0], shape[1], step, slic_weight(m, step), max_iter, min_area, mask=_dev_mask(ctx, mask))
    out = labels.reshape(shape) if device else labels.cpu().numpy().reshape(shape)
    if return_stats:
        return out, {"n_segments": int(ns), "n_iter": int(ni), "n_regrown": int(nr), "step": step, "compactness": m, "min_area": min_area,
                     "max_iter": max_iter}
    return out


def _check_float_domain(ctx: Context, d, name: str, dmask, max_area: int):
    """The exact-sum domain of a float32 plane: no NaN, |x| < 2^11, largest area * max|x| < 2^23 (valid pixels only)."""
    import torch
    v = d if dmask is None else d[dmask != 0]
    if v.numel() == 0:
        return
    if bool(torch.isnan(v).any()):
        raise ValueError(f"segment_means: {name} holds NaN; mask those pixels out with mask=")
    big = float(v.abs().max())
    if not big < FIXED_LIMIT:
        raise ValueError(f"segment_means: {name} holds |x| = {big:g}, the exact sums need |x| < 2^11")
    if not max_area * big < FIXED_AREA_LIMIT:
        raise ValueError(f"segment_means: {name}: the largest segment ({max_area} pixels) times max|x| = {big:g} is not below 2^23")


def segment_sums(segments, planes=(), mask=None, n_segments: Optional[int] = None, ctx: Optional[Context] = None):
    """int64 NumPy table [(n_segments + 1), 3 + P]: per segment the pixel count, sum y, sum x and the sum of every plane (uint8
    planes as integers, float planes as llrint(x * 2^40)); row 0 is zero.  Planes are checked as segment_means checks them."""
    import torch
    seg = check_segments(segments, "segment_sums")
    pls = _plane_list(planes, "planes", "segment_sums") if (_is_tensor(planes) or isinstance(planes, np.ndarray) or len(planes)) else []
    shape = _check_shapes(pls, "planes", "segment_sums", shape=seg.shape)
    mask = _check_mask(mask, shape, "segment_sums")
    ctx = _context(ctx, "segment_sums")
    d_seg, h, w, ns = _upload_segments(ctx, seg, n_segments)
    dmask = _dev_mask(ctx, mask)
    base = ctx.segment_sums(d_seg, h, w, ns, (), mask=dmask)
    cols = [base.cpu().numpy()]
    max_area = int(cols[0][:, 0].max())
    for p0 in range(0, len(pls), MAX_PLANES):
        for is_u8 in (True, False):
            idx = [i for i in range(p0, min(p0 + MAX_PLANES, len(pls))) if _is_u8(pls[i]) == is_u8]
            if not idx:
                continue
            dev = [_dev_flat(ctx, pls[i], torch.uint8 if is_u8 else torch.float32) for i in idx]
            if not is_u8:
                for i, d in zip(idx, dev):
                    _check_float_domain(ctx, d, f"planes[{i}]", dmask, max_area)
            t = ctx.segment_sums(d_seg, h, w, ns, dev, mask=dmask).cpu().numpy()
            cols.append((idx, t[:, 3:]))
    out = np.zeros((ns + 1, 3 + len(pls)), np.int64)
    out[:, :3] = cols[0]
    for idx, t in cols[1:]:
        out[:, [3 + i for i in idx]] = t
    return out


def segment_means(segments, planes, mask=None, n_segments: Optional[int] = None, ctx: Optional[Context] = None, return_geometry: bool = False):
    """float64 [(n_segments + 1), P]: the mean of every plane over every segment's (valid) pixels; row 0 and segments without a
    valid pixel are NaN.  The means are exact ratios: uint8 planes are summed as integers, float planes as integers of
    2^-40, which needs |x| < 2^11, the largest segment's area * max|x| < 2^23 and no NaN among the valid pixels (ValueError
    naming the plane; mask= takes pixels out).  return_geometry: also (area int64, centroid y, centroid x)."""
    pls = _plane_list(planes, "planes", "segment_means")
    sums = segment_sums(segments, pls, mask=mask, n_segments=n_segments, ctx=ctx)
    area = sums[:, 0]
    scale = np.array([1.0 if _is_u8(p) else FIXED_ONE for p in pls], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = sums[:, 3:].astype(np.float64) / scale[None, :] / area.astype(np.float64)[:, None]
        if return_geometry:
            return means, (area.copy(), sums[:, 1] / area.astype(np.float64), sums[:, 2] / area.astype(np.float64))
    return means


def object_majority(segments, class_map, nodata: Optional[int] = 0, fill: Optional[int] = None, n_segments: Optional[int] = None,
                    ctx: Optional[Context] = None, device: bool = False):
    """uint8 table [n_segments + 1]: every segment's most frequent class (ties: the smallest label).  Pixels of class `nodata`
    do not vote (None: every value votes); a segment without a voter, and entry 0, get `fill` (default: nodata, or 0)."""
    import torch
    seg = check_segments(segments, "object_majority")
    cm = check_class_map(class_map)
    if tuple(cm.shape) != tuple(seg.shape):
        raise ValueError(f"object_majority: class_map has shape {tuple(cm.shape)}, segments {tuple(seg.shape)}")
    nd = _check_nodata(nodata, "object_majority")
    if fill is not None and (isinstance(fill, (bool, np.bool_)) or int(fill) != fill or not 0 <= int(fill) <= 255):
        raise ValueError(f"object_majority: fill={fill!r} is neither None nor an integer in 0..255")
    fl = max(nd, 0) if fill is None else int(fill)
    ctx = _context(ctx, "object_majority")
    d_seg, h, w, ns = _upload_segments(ctx, seg, n_segments)
    table = ctx.segment_majority_u8(d_seg, ns, _dev_flat(ctx, cm, torch.uint8), ignore=nd, fill=fl)
    return table if device else table.cpu().numpy()


def paint(segments, table, n_segments: Optional[int] = None, ctx: Optional[Context] = None, device: bool = False):
    """(H, W) raster out[y, x] = table[segments[y, x]] for a uint8, int32 or float32 table of n_segments + 1 entries (entry 0 is
    what the masked pixels get)."""
    import torch
    seg = check_segments(segments, "paint")
    if _is_tensor(table):
        t = table
        if t.dim() != 1 or t.dtype not in (torch.uint8, torch.int32, torch.float32):
            raise ValueError(f"paint: table must be 1-D uint8, int32 or float32, got {t.dtype} of shape {tuple(t.shape)}")
    else:
        t = np.asarray(table)
        if t.ndim != 1 or t.dtype not in (np.uint8, np.int32, np.float32):
            raise ValueError(f"paint: table must be 1-D uint8, int32 or float32, got {t.dtype} of shape {t.shape}")
    ctx = _context(ctx, "paint")
    d_seg, h, w, ns = _upload_segments(ctx, seg, n_segments)
    if int(t.shape[0]) != ns + 1:
        raise ValueError(f"paint: table has {int(t.shape[0])} entries, the map's {ns} segments need {ns + 1}")
    dt = t.to(ctx.device).contiguous() if _is_tensor(t) else ctx.to_device(t)
    out = ctx.segment_paint(d_seg, ns, dt)
    return out.reshape(h, w) if device else out.cpu().numpy().reshape(h, w)


def object_classify(segments, class_map, nodata: Optional[int] = 0, ctx: Optional[Context] = None, device: bool = False):
    """The object-based class map: every pixel gets its segment's majority class of class_map; masked pixels (segment 0) and
    segments without a voter get `nodata` (0 when nodata is None)."""
    ctx = _context(ctx, "object_classify")
    seg = check_segments(segments, "object_classify")
    import torch
    d_seg, h, w, ns = _upload_segments(ctx, seg, None)
    table = object_majority(d_seg.reshape(h, w), class_map, nodata=nodata, n_segments=ns, ctx=ctx, device=True)
    out = ctx.segment_paint(d_seg, ns, table)
    return out.reshape(h, w) if device else out.cpu().numpy().reshape(h, w)
