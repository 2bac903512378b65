"""
Clean-up of a per-pixel class map on the GPU (K20, csrc/k20_postclass.hip): majority filter, multi-class sieve, and the usual
recipe of the two.  This goes beyond the reference, which cleans only the binary masks of its rule-based path
(advanced_post_processing, mirrored by K12); there is nothing of it in modules/.

A class map is (H, W) with byte values; 0 is unclassified / nodata by the project's convention (run_kmeans_stage, the masked
maps of K19), which is what `nodata=0` means below.  Every function takes a NumPy array or a device tensor and returns a NumPy
(H, W) uint8 map, or with device=True the (H, W) uint8 device tensor.  Semantics: include/rsseg.h (rsseg_majority_u8,
rsseg_sieve_u8), restated in NumPy in tests/postclass_ref.py.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .runtime import Context, RssegUnsupported, default_context

WINDOWS = (3, 5, 7, 9, 11, 13, 15)


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def check_class_map(class_map):
    """The map as something uploadable: a C-contiguous (H, W) uint8 array (or the device tensor, as uint8).  Integer maps of
    another dtype pass when every value lies in 0..255 (KMeans' int32 labels); a float map, another rank or a value outside
    is a ValueError naming what is wrong."""
    if _is_tensor(class_map):
        import torch
        t = class_map
        if t.dim() != 2:
            raise ValueError(f"class_map must be (H, W), got a tensor of shape {tuple(t.shape)}")
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"class_map must hold integer labels, got {t.dtype}")
        if t.dtype != torch.uint8 and t.numel():
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi > 255:
                raise ValueError(f"class_map value {lo if lo < 0 else hi} is outside 0..255")
        return t.contiguous().to(torch.uint8)
    a = np.asarray(class_map)
    if a.ndim != 2:
        raise ValueError(f"class_map must be (H, W), got shape {a.shape}")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"class_map must hold integer labels, got dtype {a.dtype}")
    if a.size == 0:
        raise ValueError(f"class_map is empty: shape {a.shape}")
    if a.dtype != np.uint8:
        lo, hi = int(a.min()), int(a.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"class_map value {lo if lo < 0 else hi} is outside 0..255")
    return np.ascontiguousarray(a, dtype=np.uint8)


def _check_nodata(nodata, what: str) -> int:
    if nodata is None:
        return -1
    if isinstance(nodata, (bool, np.bool_)) or int(nodata) != nodata or not 0 <= int(nodata) <= 255:
        raise ValueError(f"{what}: nodata={nodata!r} is neither None nor an integer in 0..255")
    return int(nodata)


def _check_window(window, what: str) -> int:
    if window not in WINDOWS:
        raise ValueError(f"{what}: window={window!r} is not an odd number in 3..15")
    return int(window)


def _check_count(v, name: str, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or int(v) != v or int(v) < 0:
        raise ValueError(f"{what}: {name}={v!r} is not a non-negative integer")
    return int(v)


def _context(ctx: Optional[Context], what: str) -> Context:
    ctx = ctx or default_context()
    if ctx.world > 1:
        raise RssegUnsupported(f"{what}: the class map must be whole on one GPU (this context has {ctx.world} ranks); windows and "
                               "components cross stripes")
    return ctx


def _upload(ctx: Context, m):
    """(flat uint8 device plane that the caller may NOT write, H, W)"""
    h, w = (int(m.shape[0]), int(m.shape[1]))
    if _is_tensor(m):
        if m.numel() == 0:
            raise ValueError(f"class_map is empty: shape {tuple(m.shape)}")
        return m.to(ctx.device).reshape(-1), h, w
    return ctx.to_device(m.reshape(-1)), h, w


def _result(t, h: int, w: int, device: bool):
    return t.reshape(h, w) if device else t.cpu().numpy().reshape(h, w)


def _group_mask(counts: np.ndarray, *not_voting: int) -> int:
    """bit g: a label of 8g .. 8g + 7 occurs and votes"""
    c = counts.copy()
    for v in not_voting:
        if v >= 0:
            c[v] = 0
    return int(sum(1 << g for g in range(32) if c[8 * g:8 * g + 8].any()))


def _majority_passes(ctx: Context, cur, h: int, w: int, k: int, passes: int, ignore: int, fill: int, group_mask: int):
    """Up to `passes` ordinary majority passes over two buffers, stopping once a pass changes nothing.
    (plane, n_changed per pass run, n_unfilled of the last pass or None)."""
    import torch
    changed, unfilled, spare = [], None, None
    for _ in range(passes):
        out = spare if spare is not None else ctx.empty(h * w, torch.uint8)
        out, nc, unfilled = ctx.majority_u8(cur, h, w, k, ignore=ignore, fill=fill, group_mask=group_mask, out=out)
        # the input plane of the first pass is the caller's: it is never written
        spare = cur if changed else None
        cur = out
        changed.append(int(nc))
        if nc == 0:
            break
    return cur, changed, unfilled


def majority_filter(class_map, window: int = 3, nodata: Optional[int] = 0, fill_nodata: bool = False, iterations: int = 1,
                    ctx: Optional[Context] = None, return_stats: bool = False, device: bool = False):
    """window x window majority (mode) filter.  The window is clipped to the image; the winner is the label with the most
    votes, a tie goes to the centre's own label when it is among the maxima and else to the smallest tied label.
    nodata: pixels of this value never vote; None: every value votes.  fill_nodata=False: they also stay as they are;
    True: a nodata pixel takes its window's winner when the window holds a voter.
    iterations: passes, stopped early once a pass changes nothing.
    return_stats: also {"iterations": passes run, "n_changed": [per pass], "n_unfilled": nodata pixels left by the last pass
    (fill_nodata only, else 0)}."""
    m = check_class_map(class_map)
    k = _check_window(window, "majority_filter")
    nd = _check_nodata(nodata, "majority_filter")
    passes = _check_count(iterations, "iterations", "majority_filter")
    ctx = _context(ctx, "majority_filter")
    cur, h, w = _upload(ctx, m)
    ignore, fill = (-1, nd) if fill_nodata else (nd, -1)
    gm = _group_mask(ctx.hist_u8(cur), nd) if passes > 1 else 0    # one histogram serves every pass: no pass adds a label
    cur, changed, unfilled = _majority_passes(ctx, cur, h, w, k, passes, ignore, fill, gm)
    if not changed:
        cur = cur.clone()
    out = _result(cur, h, w, device)
    if return_stats:
        return out, {"iterations": len(changed), "n_changed": changed, "n_unfilled": int(unfilled or 0) if fill_nodata and nd >= 0 else 0}
    return out


def sieve(class_map, min_area: int, connectivity: int = 8, nodata: Optional[int] = 0, ctx: Optional[Context] = None,
          return_stats: bool = False, device: bool = False):
    """Every connected component (same label, 8- or 4-neighbours, label != nodata) of fewer than min_area pixels becomes
    nodata; min_area <= 1 changes nothing.  nodata=None is a ValueError: there would be nothing to write.
    return_stats: also {"n_removed": pixels of the removed components}."""
    m = check_class_map(class_map)
    if nodata is None:
        raise ValueError("sieve: nodata=None leaves no value to write removed components as")
    nd = _check_nodata(nodata, "sieve")
    area = _check_count(min_area, "min_area", "sieve")
    if connectivity not in (4, 8):
        raise ValueError(f"sieve: connectivity={connectivity!r} is neither 4 nor 8")
    ctx = _context(ctx, "sieve")
    cur, h, w = _upload(ctx, m)
    out, removed = ctx.sieve_u8(cur, h, w, min(area, 2 ** 31 - 1), connectivity, ignore=nd, removed_value=nd)
    res = _result(out, h, w, device)
    return (res, {"n_removed": int(removed)}) if return_stats else res


def hole_value(counts: np.ndarray, nodata: int) -> int:
    """The temporary value clean_class_map marks removed pixels with: the largest byte value that neither occurs in the map
    nor is nodata."""
    for v in range(255, -1, -1):
        if counts[v] == 0 and v != nodata:
            return v
    raise RssegUnsupported("clean_class_map: the map uses every byte value, none is left to mark removed pixels with")


def clean_class_map(class_map, min_area: int = 0, window: int = 3, nodata: int = 0, max_fill_iterations: int = 64,
                    majority_iterations: int = 0, connectivity: int = 8, ctx: Optional[Context] = None, return_stats: bool = False,
                    device: bool = False):
    """The usual clean-up of a classifier's map, in this order:
      1. sieve: components of fewer than min_area pixels are marked with a temporary hole value (hole_value);
      2. the holes are grown over from their surroundings: window x window majority passes that write hole pixels only, until
         none is left, a pass fills none, or max_fill_iterations passes have run; what is left becomes nodata.  True nodata
         pixels never vote and are never filled;
      3. majority_iterations ordinary majority passes (stopped once one changes nothing).
    return_stats: also {"removed": pixels sieved out, "filled": of those, given a label again, "left_as_nodata": the others,
    "fill_iterations": passes of step 2, "changed": [pixels changed by every pass of step 3]}."""
    m = check_class_map(class_map)
    if nodata is None:
        raise ValueError("clean_class_map: nodata=None leaves no value to write removed components as")
    nd = _check_nodata(nodata, "clean_class_map")
    k = _check_window(window, "clean_class_map")
    area = _check_count(min_area, "min_area", "clean_class_map")
    max_fill = _check_count(max_fill_iterations, "max_fill_iterations", "clean_class_map")
    passes = _check_count(majority_iterations, "majority_iterations", "clean_class_map")
    if connectivity not in (4, 8):
        raise ValueError(f"clean_class_map: connectivity={connectivity!r} is neither 4 nor 8")
    ctx = _context(ctx, "clean_class_map")
    import torch
    src, h, w = _upload(ctx, m)
    counts = ctx.hist_u8(src)
    hole = hole_value(counts, nd)
    gm = _group_mask(counts, nd)      # the sieve and the passes add no label but the hole, which never votes
    cur, removed = ctx.sieve_u8(src, h, w, min(area, 2 ** 31 - 1), connectivity, ignore=nd, removed_value=hole)
    unfilled, fill_iterations, spare = int(removed), 0, None
    while unfilled > 0 and fill_iterations < max_fill:
        out = spare if spare is not None else ctx.empty(h * w, torch.uint8)
        out, _, left = ctx.majority_u8(cur, h, w, k, ignore=nd, fill=hole, fill_only=True, group_mask=gm, out=out)
        cur, spare = out, cur
        fill_iterations += 1
        stalled = left >= unfilled
        unfilled = int(left)
        if stalled:
            break
    if unfilled:
        ctx.replace_u8(cur, hole, nd)
    cur, changed, _ = _majority_passes(ctx, cur, h, w, k, passes, nd, -1, gm)
    res = _result(cur, h, w, device)
    if return_stats:
        return res, {"removed": int(removed), "filled": int(removed) - unfilled, "left_as_nodata": unfilled, "fill_iterations": fill_iterations,
                     "changed": changed}
    return res


def class_counts(class_map) -> dict:
    """{label: pixels} of the labels that occur, as JSON wants them (string keys in the file, int here)."""
    c = np.bincount(np.asarray(class_map, dtype=np.uint8).reshape(-1), minlength=256)
    return {int(v): int(c[v]) for v in np.flatnonzero(c)}
