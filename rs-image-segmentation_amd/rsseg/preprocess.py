"""
Stage 1 of the reference on the device: scripts/1_preprocessing.py:25-85 with modules/features/preprocessing.py:54-154.

A raw DN raster is read once on the host, crosses PCIe in its own dtype, and K15 (rsseg_preprocess_u8) turns it into the
uint8 planes the reference writes: radiometric calibration with the reference's seven gains and biases, the identity warp,
and the min-max stretch with astype(np.uint8).  The planes stay in HBM, so the feature stage can take them directly
(rsseg.stages --raw).  On disk the product is what the reference's save_processed_image writes: a Float32 GeoTIFF of the
uint8 values with the input's georeferencing.  The figures of scripts/1 are out of scope: the visualisation directory is
created and nothing is drawn.

    python -m rsseg.preprocess RAW.tif OUT.tif [--viz-dir DIR]

Beyond the reference (whose geometric_correction ignores its GCPs): with --gcps FILE the DN planes are first rectified on the
device by the polynomial fitted to the ground control points (rsseg/georect.py, K21) and then go through K15 unchanged.

    python -m rsseg.preprocess RAW.tif OUT.tif --gcps FILE [--warp-order 1|2] [--resampling nearest|bilinear|cubic] [--pixel-size S]
"""
from __future__ import annotations

import os
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .runtime import Context, RssegUnsupported, default_context

# radiometric_calibration's constants (preprocessing.py:65-66), one per TM band
GAIN = [0.671339, 1.322205, 1.043976, 0.876024, 0.120354, 0.055376, 0.065551]
BIAS = [-2.19, -4.16, -2.21, -2.39, -0.49, 1.18, -0.22]

DN_DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64)


def check_dn_dtype(dtype, what: str = "preprocessing") -> np.dtype:
    """The DN dtypes K15 reads; anything else (int64, int8, uint32, bool, ...) is refused by name."""
    dt = np.dtype(dtype)
    if dt not in [np.dtype(d) for d in DN_DTYPES]:
        raise RssegUnsupported(f"{what}: {dt.name} bands are not supported (uint8, int16, uint16, int32, float32 or float64)")
    return dt


def radiance_range(dn_range: np.ndarray, dtype, gain: Optional[Sequence[float]] = None,
                   bias: Optional[Sequence[float]] = None) -> List[Tuple[float, float]]:
    """np.min / np.max of each band's radiance from the whole raster's DN range {min, max, NaN count} (what the kernels
    derive on the device): gain * DN + bias in the radiance dtype, NaN when the band holds a NaN."""
    rt = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    out = []
    for i, (mn, mx, nan) in enumerate(np.asarray(dn_range, np.float64)):
        lo, hi = rt(mn), rt(mx)
        if gain is not None:
            with np.errstate(over="ignore", invalid="ignore"):
                lo, hi = rt(gain[i]) * lo + rt(bias[i]), rt(gain[i]) * hi + rt(bias[i])
        if nan > 0:
            lo = hi = rt(np.nan)
        out.append((lo, hi))
    return out


def warn_degenerate(dn_range: np.ndarray, dtype, gain=None, bias=None, stacklevel: int = 3) -> List[int]:
    """One RuntimeWarning per band whose stretch divides NaN or inf (a band with a NaN, a constant band, an infinite radiance
    range): NumPy warns there and its cast gives 0, so the band comes out all zero.  Returns those bands."""
    bad = []
    for i, (lo, hi) in enumerate(radiance_range(dn_range, dtype, gain, bias)):
        with np.errstate(all="ignore"):
            den = hi - lo
            ok = np.isfinite(den) and den > 0 and np.isfinite(den * type(den)(255.0))
        if not ok:
            bad.append(i)
            warnings.warn(f"band {i}: radiance range [{lo}, {hi}] ({int(dn_range[i][2])} NaN): the 8-bit stretch divides "
                          f"{hi} - {lo} = {den}, and NaN / inf cast to uint8 give 0", RuntimeWarning, stacklevel=stacklevel)
    return bad


def preprocess_to_device(ctx: Optional[Context], dn_planes: Sequence, want_range: bool = False, warn: bool = True):
    """Stage 1 of n <= 7 DN bands (host arrays or device tensors of one dtype and shape) -> the uint8 device planes (flat),
    bit-exact with radiometric_calibration -> geometric_correction -> image_enhancement -> astype(np.uint8).  More than 7
    bands raise IndexError, as gain[i] does in the reference.  `warn` (the default) reads the per-band range back — the one
    host wait — and warns for every band that comes out all zero; with warn=False and want_range=False nothing waits."""
    torch = __import__("torch")
    ctx = ctx or default_context()
    planes = list(dn_planes)
    if len(planes) > len(GAIN):
        raise IndexError("list index out of range")   # gain[7] in radiometric_calibration (preprocessing.py:71)
    if not planes:
        return ([], np.zeros((0, 3))) if want_range else []
    dev = []
    for p in planes:
        if isinstance(p, torch.Tensor):
            check_dn_dtype(str(p.dtype).split(".")[-1])
            dev.append(p.reshape(-1))
        else:
            a = np.ascontiguousarray(p)
            check_dn_dtype(a.dtype)
            dev.append(ctx.to_device(a.reshape(-1)))
    if any(d.dtype != dev[0].dtype or d.numel() != dev[0].numel() for d in dev):
        raise ValueError("preprocess_to_device: the bands must share one dtype and shape")
    nb = len(dev)
    if dev[0].numel() == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    need_range = want_range or warn
    res = ctx.preprocess_u8(dev, GAIN[:nb], BIAS[:nb], want_range=need_range)
    outs, rng = res if need_range else (res, None)
    if warn:
        warn_degenerate(rng, str(dev[0].dtype).split(".")[-1], GAIN[:nb], BIAS[:nb])
    return (outs, rng) if want_range else outs


# ---- the georeferencing of load_tm_image / save_processed_image ------------------------------------------------------
DEFAULT_GEOTRANSFORM = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)   # what GDAL reports for a file without georeferencing


def gdal_geotransform(transform) -> tuple:
    """rasterio order (a, b, c, d, e, f) -> GDAL's (c, a, b, f, d, e); None -> GDAL's default."""
    if transform is None:
        return DEFAULT_GEOTRANSFORM
    a, b, c, d, e, f = (float(v) for v in transform)
    return (c, a, b, f, d, e)


def rasterio_transform(geotransform) -> Optional[tuple]:
    """GDAL's (c, a, b, f, d, e) -> rasterio order; GDAL's default (no georeferencing) -> None."""
    gt = tuple(float(v) for v in geotransform)
    if len(gt) != 6:
        raise ValueError(f"geotransform must have 6 values, not {len(gt)}")
    if gt == DEFAULT_GEOTRANSFORM:
        return None
    c, a, b, f, d, e = gt
    return (a, b, c, d, e, f)


def projection_string(epsg: Optional[int]) -> str:
    """'' when the file names no coordinate system, else 'EPSG:<code>' (there is no WKT without GDAL)."""
    return "" if epsg is None else f"EPSG:{int(epsg)}"


def parse_projection(projection) -> Tuple[Optional[int], Optional[bool]]:
    """(EPSG code or None, geographic or None) of '', 'EPSG:n', or a WKT whose last AUTHORITY is EPSG."""
    import re
    p = (projection or "").strip()
    if not p:
        return None, None
    m = re.fullmatch(r"(?i)epsg:(\d+)", p)
    if m:
        return int(m.group(1)), None
    auth = re.findall(r'AUTHORITY\[\s*"([^"]+)"\s*,\s*"?(\d+)"?\s*\]', p)
    if auth and auth[-1][0].upper() == "EPSG":
        head = p.split("[", 1)[0].strip().upper()
        geographic = True if head in ("GEOGCS", "GEOGCRS") else (False if head in ("PROJCS", "PROJCRS") else None)
        return int(auth[-1][1]), geographic
    raise RssegUnsupported(f"projection {p[:80]!r}: only '', 'EPSG:<code>' or a WKT whose last AUTHORITY is EPSG can be written")


def write_processed_tif(path: str, bands_u8: Sequence[np.ndarray], transform=None, epsg: Optional[int] = None,
                        geographic: Optional[bool] = None) -> str:
    """save_processed_image's file: a GTiff of Float32 samples, one uncompressed band after the other, with the
    transform and EPSG code carried over."""
    from .tiff import write_tiff
    arr = np.stack([np.asarray(b).astype(np.float32) for b in bands_u8])
    write_tiff(path, arr, transform=transform, epsg=epsg, geographic=geographic)
    return path


def warp_dn_planes(ctx: Optional[Context], dn_planes: Sequence, src_shape, gcps, warp_order: int = 1, resampling: str = "nearest",
                   pixel_size: Optional[float] = None):
    """The DN planes rectified on the device by the transform fitted to `gcps` (a path, the text of a GCP file, or an (N, 4)
    array): (device planes, mask, n_valid, transform, plan).  nearest keeps the DN dtype; bilinear and cubic write float64
    for integer DN (K15 then computes the radiance in float64, as it does for integer DN) and float DN keep their dtype.
    Pixels outside the source are 0 DN."""
    from . import georect as G
    g = G.parse_gcps(gcps) if isinstance(gcps, (str, os.PathLike)) else np.asarray(gcps, np.float64)
    t = G.fit_gcp_transform(g, warp_order)
    ho, wo, out_transform = G.output_grid(t, src_shape, pixel_size)
    plan = G.warp_plan(t, (ho, wo), out_transform, src_shape)
    planes = list(dn_planes)
    dt = check_dn_dtype(str(planes[0].dtype).split(".")[-1])
    out_dtype = np.float64 if resampling != "nearest" and dt.kind in "iu" else None
    outs, mask, n_valid = G.warp_planes(ctx, planes, src_shape, plan, method=resampling, fill=0, out_dtype=out_dtype)
    return outs, mask, n_valid, t, plan


def run_preprocessing_stage(input_file, output_file, visualization_output_dir, ctx: Optional[Context] = None, return_device: bool = False,
                            gcps=None, warp_order: int = 1, resampling: str = "nearest", pixel_size: Optional[float] = None,
                            nodata: Optional[float] = None):
    """scripts/1_preprocessing.py:25-85: raw DN GeoTIFF -> calibrated, stretched, Float32 GeoTIFF; returns output_file.
    return_device: (output_file, uint8 device planes, (H, W), georef) instead, for a caller that goes on on the device.

    gcps (beyond the reference; a GCP file, its text or an (N, 4) array of pixel, line, x, y): the DN planes are rectified
    first (warp_dn_planes) and then calibrated and stretched as they are.  Calibration is linear per band, so this is the
    reference's calibrate -> warp -> stretch up to rounding, and exactly that for `nearest`.  The pixels outside the source
    are 0 DN and take part in the stretch, as the constant border of cv2.warpAffine would.  The output carries the
    rectified grid's transform; OUT_valid.npy (the uint8 mask, 1 = sampled) and OUT_geometric_correction.json (order, method,
    coefficients, per-GCP residuals, RMSE, output shape and transform, n_valid) are written beside it, and return_device
    gives (output_file, planes, (Ho, Wo), georef, mask) with georef["transform"] the new one.  nodata (with gcps and
    return_device): the returned mask is also 0 where a warped DN band equals `nodata` or holds a NaN (Context.valid_mask
    with the warp's mask as and_mask; 16- and 32-bit integer DN are compared as float32); the file keeps the warp's mask."""
    from .tiff import read_tiff, read_tiff_georef
    print("开始数据预处理阶段...")
    print(f"输入文件: {input_file}")
    print(f"输出文件: {output_file}")
    os.makedirs(os.path.dirname(output_file) or ".", exist_ok=True)
    os.makedirs(visualization_output_dir, exist_ok=True)
    arr = read_tiff(input_file)
    geo = read_tiff_georef(input_file)
    h, w = arr.shape[1:]
    dn = [arr[i] for i in range(arr.shape[0])]
    mask = None
    if gcps is not None:
        import json
        from .georect import correction_record
        if len(dn) > len(GAIN):
            raise IndexError("list index out of range")   # gain[7], before any work
        dn, mask, n_valid, t, plan = warp_dn_planes(ctx, dn, (h, w), gcps, warp_order, resampling, pixel_size)
        h, w = plan.out_shape
        geo = dict(geo, transform=tuple(plan.out_transform))
        stem = os.path.splitext(output_file)[0]
        np.save(stem + "_valid.npy", mask.cpu().numpy().reshape(h, w))
        with open(stem + "_geometric_correction.json", "w", encoding="utf-8") as f:
            json.dump(correction_record(t, plan, resampling, n_valid), f, indent=1)
        if nodata is not None and return_device:
            torch = __import__("torch")
            c = ctx or default_context()
            cmp = [p if p.dtype in (torch.uint8, torch.float32, torch.float64) else p.to(torch.float32) for p in dn]
            mask, _ = c.valid_mask(cmp, nan=True, nodata=nodata, and_mask=mask)
        print(f"几何校正: order {t.order}, {resampling}, RMSE {t.rmse:.4f} px, {h} x {w}, {n_valid} valid pixels")
    planes = preprocess_to_device(ctx, dn)
    write_processed_tif(output_file, [p.cpu().numpy().reshape(h, w) for p in planes], geo["transform"], geo["epsg"])
    print(f"已保存处理后的影像到: {output_file}")
    print("数据预处理阶段完成")
    if return_device:
        return (output_file, planes, (h, w), geo) + (() if mask is None else (mask,))
    return output_file


def add_gcp_arguments(ap) -> None:
    """The geometric-correction options shared by `python -m rsseg.preprocess` and `python -m rsseg.stages --raw`."""
    ap.add_argument("--gcps", default=None, metavar="FILE", help="ground control points, one `pixel line x y` per line: rectify the DN "
                    "planes on the GPU before calibration (beyond the reference, which ignores its GCPs)")
    ap.add_argument("--warp-order", type=int, choices=(1, 2), default=1, help="polynomial order of the GCP transform (default 1)")
    ap.add_argument("--resampling", choices=("nearest", "bilinear", "cubic"), default="nearest", help="interpolator of the warp (default nearest)")
    ap.add_argument("--pixel-size", type=float, default=None, help="output pixel size in map units (default: from the transform)")


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rsseg.preprocess",
                                 description="stage 1 (scripts/1): radiometric calibration and 8-bit stretch of a raw DN GeoTIFF on the GPU")
    ap.add_argument("input_file")
    ap.add_argument("output_file")
    ap.add_argument("--viz-dir", default=None, help="visualisation directory (created; nothing is drawn). Default: next to OUT")
    add_gcp_arguments(ap)
    a = ap.parse_args(argv)
    viz = a.viz_dir or (os.path.dirname(a.output_file) or ".")
    run_preprocessing_stage(a.input_file, a.output_file, viz, gcps=a.gcps, warp_order=a.warp_order, resampling=a.resampling,
                            pixel_size=a.pixel_size)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
