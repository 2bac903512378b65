"""
Drop-in counterpart of the reference's modules/features/preprocessing.py (load_tm_image, radiometric_calibration,
geometric_correction, image_enhancement, save_processed_image, :19-154), the module scripts/1_preprocessing.py
star-imports.  Calibration and the 8-bit stretch run on the GPU (K15: rsseg_radiometric, rsseg_preprocess_u8) and equal
NumPy's results bit for bit; the rasters are read and written by rsseg/tiff.py instead of GDAL.

Two deviations, both documented in INTEGRATION.md:
  * geometric_correction returns copies.  cv2.warpAffine with the identity matrix is the identity for finite input; its
    zero-weight bilinear taps would spread a NaN or inf to the left and upper neighbours, which is not reproduced.  Stage 1's
    output does not change: a band with a NaN or inf radiance comes out all zero either way.
  * The projection is '' when the file names no coordinate system and 'EPSG:<code>' otherwise (no WKT without GDAL);
    save_processed_image takes '', 'EPSG:<code>' or a WKT whose last AUTHORITY is EPSG.
`gdal` and `cv2` are library names of the reference's module and are not provided, as plt / cv2 are not by the other
mirrors.
"""
from __future__ import annotations

import numpy as np

from rsseg import preprocess as PP
from rsseg.runtime import default_context

__all__ = ["load_tm_image", "radiometric_calibration", "geometric_correction", "image_enhancement", "save_processed_image", "np"]


def _ctx():
    return default_context()


def load_tm_image(file_path):
    """(list of 2-D arrays in the file's dtype, GDAL-order geotransform, projection) — (0, 1, 0, 0, 0, 1) and '' for a file
    without georeferencing, as GDAL reports them."""
    from rsseg.tiff import read_tiff, read_tiff_georef
    try:
        arr = read_tiff(file_path)
        geo = read_tiff_georef(file_path)
    except (OSError, ValueError) as e:
        raise Exception("无法打开文件: " + file_path) from e
    bands_count, height, width = arr.shape
    geotransform = PP.gdal_geotransform(geo["transform"])
    projection = PP.projection_string(geo["epsg"])
    bands_data = [np.ascontiguousarray(arr[i]) for i in range(bands_count)]
    print(f"成功加载影像, 尺寸: {width}x{height}, 波段数: {bands_count}")
    return bands_data, geotransform, projection


def radiometric_calibration(bands_data):
    """gain[i] * band + bias[i] per band on the GPU: float64, or float32 for float32 bands (NumPy 2 promotion).  An eighth
    band raises IndexError like the reference's gain[i]."""
    ctx = _ctx()
    calibrated_bands = []
    for i, band_data in enumerate(bands_data):
        g, b = PP.GAIN[i], PP.BIAS[i]
        a = np.asarray(band_data)
        PP.check_dn_dtype(a.dtype, "radiometric_calibration")
        out = ctx.radiometric(ctx.to_device(a.reshape(-1)), g, b)
        calibrated_bands.append(out.cpu().numpy().reshape(a.shape))
    return calibrated_bands


def geometric_correction(bands_data, gcps):
    """The reference's identity cv2.warpAffine (gcps ignored): copies of the 2-D bands."""
    corrected_bands = []
    for band_data in bands_data:
        height, width = band_data.shape
        corrected_bands.append(np.array(band_data, copy=True))
    return corrected_bands


def image_enhancement(bands_data):
    """Linear stretch to uint8 per band on the GPU: ((band - min) * 255.0 / (max - min)).astype(np.uint8) in the band's
    dtype, with NumPy's RuntimeWarning (and its all-zero result) for a constant band, a band with a NaN, or an infinite
    range."""
    ctx = _ctx()
    enhanced_bands = []
    for band_data in bands_data:
        a = np.asarray(band_data)
        dt = PP.check_dn_dtype(a.dtype, "image_enhancement")
        if a.size == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        (q,), rng = ctx.preprocess_u8([ctx.to_device(a.reshape(-1))], want_range=True)
        if dt.kind == "i" and rng[0, 1] - rng[0, 0] > np.iinfo(dt).max:
            # NumPy forms band - min in the band's own integer type, which wraps here
            raise PP.RssegUnsupported(f"image_enhancement: the range of this {dt.name} band overflows {dt.name} in band - min")
        PP.warn_degenerate(rng, dt)
        enhanced_bands.append(q.cpu().numpy().reshape(a.shape))
    return enhanced_bands


def save_processed_image(bands_data, geotransform, projection, output_path):
    """A Float32 GeoTIFF of the bands with the geotransform (GDAL order) and projection ('', 'EPSG:<code>' or a WKT whose last
    AUTHORITY is EPSG) carried over."""
    epsg, geographic = PP.parse_projection(projection)
    PP.write_processed_tif(output_path, bands_data, PP.rasterio_transform(geotransform), epsg, geographic)
    print(f"已保存处理后的影像到: {output_path}")
