"""K21 on the GPU (rsseg_warp_poly through Context.warp_poly) against tests/warp_ref.py: integer planes bit for bit, float
planes bit for bit where they are no NaN and NaN where the restatement is NaN, the mask and n_valid exact.  A workgroup's
tile is 4 rows by 64 threads; for nearest a thread owns 4 (1-byte output) or 2 (2-byte output) adjacent pixels and stores
them as one dword, else one pixel."""
import json
import os

import numpy as np
import pytest

import warp_ref as R

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64)
SRC, OUT = (37, 53), (41, 67)
AFFINE = [[0.93, 0.11, -3.2], [-0.08, 0.97, 2.6]]
N = int(os.environ.get("RSSEG_FUZZ_N", "0"))
SEED0 = int(os.environ.get("RSSEG_FUZZ_SEED0", "0"))


def random_plane(rs, shape, dtype):
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return rs.randint(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dt)
    return (rs.standard_normal(shape) * 1000.0).astype(dt)


def torch_dtype(dt):
    import torch
    return None if dt is None else getattr(torch, np.dtype(dt).name)


def same_bits(got, want):
    """integers equal; floats: NaN where the restatement is NaN, the same bits elsewhere (so -0.0 is not 0.0)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(got.view(u)[~nan], want.view(u)[~nan])


def check(ctx, planes, coef, cx, cy, Ho, Wo, method, fill=0, out_dtype=None, want_mask=True, valid_share=None):
    H, W = planes[0].shape
    want, wmask, wn = R.warp(planes, coef, cx, cy, Ho, Wo, method=method, fill=fill, out_dtype=out_dtype)
    if valid_share is not None:
        assert valid_share[0] <= wmask.mean() <= valid_share[1], wmask.mean()   # both branches run
    dev = [ctx.to_device(p.reshape(-1)) for p in planes]
    outs, mask, nv = ctx.warp_poly(dev, H, W, coef, cx, cy, Ho, Wo, method=method, fill=fill, out_dtype=torch_dtype(out_dtype),
                                   want_mask=want_mask)
    assert len(outs) == len(planes)
    for b, (o, w) in enumerate(zip(outs, want)):
        got = o.cpu().numpy().reshape(Ho, Wo)
        if not same_bits(got, w):
            bad = np.argwhere(~((got == w) | (np.isnan(got.astype(np.float64)) & np.isnan(w.astype(np.float64)))))
            raise AssertionError((planes[0].dtype.name, method, (H, W), (Ho, Wo), "band", b, len(bad), bad[:5].tolist(),
                                  [(got[tuple(i)], w[tuple(i)]) for i in bad[:5]]))
    if want_mask:
        assert np.array_equal(mask.cpu().numpy().reshape(Ho, Wo), wmask)
    else:
        assert mask is None
    assert nv == wn
    return want, wmask, wn


def order2_coef(Ho, Wo):
    coef, cx, cy = R.affine_coef(AFFINE, Ho, Wo)
    coef = coef.copy()
    coef[3:6] = [1.5e-3, -0.8e-3, 0.6e-3]
    coef[9:12] = [-0.7e-3, 1.1e-3, 0.9e-3]
    return coef, cx, cy


# ---- main sweep ----
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_sweep_dtypes_and_methods(ctx, dtype, method):
    rs = np.random.RandomState(11)
    planes = [random_plane(rs, SRC, dtype) for _ in range(2)]
    check(ctx, planes, *R.affine_coef(AFFINE, *OUT), *OUT, method, valid_share=(0.2, 0.95))
    check(ctx, planes, *order2_coef(*OUT), *OUT, method, valid_share=(0.2, 0.95))


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("out_dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dtype", [np.uint8, np.int16], ids=lambda d: np.dtype(d).name)
def test_float_output_from_integer_planes(ctx, dtype, out_dtype, method):
    planes = [random_plane(np.random.RandomState(12), SRC, dtype)]
    want, _, _ = check(ctx, planes, *R.affine_coef(AFFINE, *OUT), *OUT, method, out_dtype=out_dtype, valid_share=(0.2, 0.95))
    assert want[0].dtype == out_dtype


@pytest.mark.parametrize("dtype,out_dtype", [(np.float32, np.float64), (np.float64, np.float32), (np.int32, np.float32), (np.uint16, np.float64)])
def test_float_output_from_the_other_planes(ctx, dtype, out_dtype):
    planes = [random_plane(np.random.RandomState(13), SRC, dtype)]
    for method in R.METHODS:
        check(ctx, planes, *R.affine_coef(AFFINE, *OUT), *OUT, method, out_dtype=out_dtype)


# ---- seams ----
@pytest.mark.parametrize("Ho", [1, 3, 9])
@pytest.mark.parametrize("Wo", [63, 64, 65, 257])
def test_tile_seams(ctx, Wo, Ho):
    rs = np.random.RandomState(Wo * 16 + Ho)
    A = [[SRC[1] / Wo * 1.1, 0.02, -1.0], [0.01, SRC[0] / Ho * 1.1, -0.7]]
    for dtype in (np.uint8, np.uint16, np.float32):
        planes = [random_plane(rs, SRC, dtype)]
        for method in R.METHODS:
            check(ctx, planes, *R.affine_coef(A, Ho, Wo), Ho, Wo, method, valid_share=(0.5, 0.99))


@pytest.mark.parametrize("Wo", [65, 66, 67, 129, 130, 131, 258, 259])
def test_dword_store_tails(ctx, Wo):
    """a 1-, 2- and 3-pixel tail behind the last whole dword of a row, for 1- and 2-byte outputs; with an odd width every
    second row's dwords start at an odd address"""
    rs = np.random.RandomState(Wo)
    Ho = 6
    A = [[SRC[1] / Wo, 0.0, 0.0], [0.0, SRC[0] / Ho * 1.2, 0.0]]
    for dtype in (np.uint8, np.int16, np.uint16):
        planes = [random_plane(rs, SRC, dtype), random_plane(rs, SRC, dtype)]
        for method in ("nearest", "bilinear"):
            check(ctx, planes, *R.affine_coef(A, Ho, Wo), Ho, Wo, method, fill=3)


@pytest.mark.parametrize("src_shape", [(1, 1), (2, 2), (1, 40)])
def test_tiny_sources_every_tap_clamps(ctx, src_shape):
    rs = np.random.RandomState(5)
    H, W = src_shape
    Ho, Wo = 7, 70
    A = [[W / Wo * 1.3, 0.0, -0.15 * W], [0.0, H / Ho * 1.3, -0.15 * H]]
    for dtype in (np.uint8, np.int32, np.float64):
        planes = [random_plane(rs, src_shape, dtype)]
        for method in R.METHODS:
            check(ctx, planes, *R.affine_coef(A, Ho, Wo), Ho, Wo, method, valid_share=(0.3, 0.9))


def test_one_by_one_output(ctx):
    rs = np.random.RandomState(6)
    for dtype in DTYPES:
        planes = [random_plane(rs, SRC, dtype)]
        for method in R.METHODS:
            _, mask, nv = check(ctx, planes, *R.affine_coef([[1, 0, 20.3], [0, 1, 11.7]], 1, 1), 1, 1, method)
            assert nv == 1
            check(ctx, planes, *R.affine_coef([[1, 0, -20.3], [0, 1, 11.7]], 1, 1), 1, 1, method, fill=9)


@pytest.mark.parametrize("dtype,offsets", [(np.uint8, (1, 2, 3)), (np.uint16, (1,)), (np.int16, (1,))])
def test_output_plane_at_an_odd_element_offset(ctx, dtype, offsets):
    import torch
    rs = np.random.RandomState(8)
    planes = [random_plane(rs, SRC, dtype)]
    Ho, Wo = 5, 68
    coef, cx, cy = R.affine_coef(AFFINE, Ho, Wo)
    dev = [ctx.to_device(p.reshape(-1)) for p in planes]
    for method in ("nearest", "bilinear"):
        want, wmask, wn = R.warp(planes, coef, cx, cy, Ho, Wo, method=method, fill=1)
        for off in offsets:
            buf = torch.full((Ho * Wo + 8,), 77, dtype=torch_dtype(dtype), device=dev[0].device)
            out = buf[off:off + Ho * Wo]
            assert out.data_ptr() == buf.data_ptr() + off * buf.element_size()
            outs, mask, nv = ctx.warp_poly(dev, *SRC, coef, cx, cy, Ho, Wo, method=method, fill=1, out=[out])
            h = buf.cpu().numpy()
            assert np.array_equal(h[off:off + Ho * Wo].reshape(Ho, Wo), want[0]), (method, off)
            assert (h[:off] == 77).all() and (h[off + Ho * Wo:] == 77).all()      # nothing written outside the plane
            assert np.array_equal(mask.cpu().numpy().reshape(Ho, Wo), wmask) and nv == wn


# ---- bands ----
@pytest.mark.parametrize("nb", [1, 7, 16])
def test_band_counts(ctx, nb):
    rs = np.random.RandomState(nb)
    for dtype, method in ((np.uint8, "nearest"), (np.uint8, "bilinear"), (np.uint16, "cubic"), (np.float32, "bilinear"), (np.int16, "nearest")):
        planes = [random_plane(rs, SRC, dtype) for _ in range(nb)]
        check(ctx, planes, *R.affine_coef(AFFINE, *OUT), *OUT, method)
    check(ctx, planes, *R.affine_coef(AFFINE, *OUT), *OUT, "nearest", want_mask=False)


def test_seventeen_planes_are_refused(ctx):
    planes = [ctx.to_device(np.zeros(SRC, np.uint8).reshape(-1)) for _ in range(17)]
    with pytest.raises(ValueError, match="planes.*17"):
        ctx.warp_poly(planes, *SRC, *R.affine_coef(AFFINE, *OUT), *OUT)


# ---- extremes ----
def test_source_entirely_off_the_grid(ctx):
    rs = np.random.RandomState(9)
    for dtype, fill in ((np.uint8, 0), (np.int16, -5), (np.float32, np.nan), (np.float64, 2.5)):
        planes = [random_plane(rs, SRC, dtype)]
        for method in R.METHODS:
            want, mask, nv = check(ctx, planes, *R.affine_coef([[1, 0, 1000.0], [0, 1, -1000.0]], *OUT), *OUT, method, fill=fill)
            assert nv == 0 and not mask.any()


@pytest.mark.parametrize("scale,out", [(3.0, (13, 19)), (0.25, (150, 214))])
def test_downscale_by_3_and_upscale_by_4(ctx, scale, out):
    rs = np.random.RandomState(10)
    A = [[scale, 0.0, 0.2], [0.0, scale, -0.3]]
    for dtype in (np.uint8, np.int16, np.float32):
        planes = [random_plane(rs, SRC, dtype)]
        for method in R.METHODS:
            check(ctx, planes, *R.affine_coef(A, *out), *out, method, valid_share=(0.5, 1.0))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16], ids=lambda d: np.dtype(d).name)
def test_cubic_overshoot_saturates(ctx, dtype):
    lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
    src = np.full((12, 16), lo, dtype)
    src[:, 8:] = hi
    src[6:, :] = src[6:, ::-1]
    Ho, Wo = 40, 60
    A = [[16 / Wo, 0.01, 0.0], [0.02, 12 / Ho, 0.0]]
    coef, cx, cy = R.affine_coef(A, Ho, Wo)
    (raw,), _, _ = R.warp([src], coef, cx, cy, Ho, Wo, method="cubic", saturate=False)
    assert raw.min() < lo and raw.max() > hi          # the unclamped restatement leaves the range
    (want,), _, _ = check(ctx, [src], coef, cx, cy, Ho, Wo, "cubic")
    assert want.min() == lo and want.max() == hi


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_and_inf_pixels(ctx, dtype):
    rs = np.random.RandomState(14)
    src = random_plane(rs, SRC, dtype)
    src[5, 7] = np.nan
    src[20, 30] = np.inf
    src[21, 31] = -np.inf
    src[30, 10:12] = [np.inf, -np.inf]
    src[0, 0] = np.nan
    src[2, 3] = -0.0
    for method in R.METHODS:
        (want,), _, _ = check(ctx, [src], *R.affine_coef(AFFINE, *OUT), *OUT, method)
        assert np.isnan(want).any() and np.isinf(want).any()
        check(ctx, [src], *R.affine_coef([[1, 0, 0], [0, 1, 0]], *SRC), *SRC, method)


def test_fill_values(ctx):
    """fill must be a value of an integer output dtype: anything else is refused, not saturated (a fill the caller did not ask
    for would be indistinguishable from data); a float output takes any fill, float32 rounds it once"""
    rs = np.random.RandomState(15)
    coef, cx, cy = R.affine_coef(AFFINE, *OUT)
    for dtype, fill in ((np.uint8, 255), (np.uint8, 200.0), (np.int16, -32768), (np.uint16, 65535), (np.int32, -2147483648), (np.float32, 0.1),
                        (np.float32, np.inf), (np.float64, -1e300)):
        want, mask, _ = check(ctx, [random_plane(rs, SRC, dtype)], coef, cx, cy, *OUT, "bilinear", fill=fill)
        assert (want[0][mask == 0] == np.dtype(dtype).type(fill)).all()
    check(ctx, [random_plane(rs, SRC, np.uint8)], coef, cx, cy, *OUT, "bilinear", fill=-7.5, out_dtype=np.float32)
    for dtype, fill in ((np.uint8, 256), (np.uint8, -1), (np.uint8, 1.5), (np.int16, 32768), (np.uint16, -1), (np.int32, 2147483648.0),
                        (np.uint8, np.nan), (np.int16, np.inf)):
        with pytest.raises(ValueError, match="fill"):
            ctx.warp_poly([ctx.to_device(random_plane(rs, SRC, dtype).reshape(-1))], *SRC, coef, cx, cy, *OUT, fill=fill)


# ---- refusals ----
def test_refusals_name_the_argument(ctx):
    import torch
    coef, cx, cy = R.affine_coef(AFFINE, *OUT)
    u8 = ctx.to_device(np.zeros(SRC, np.uint8).reshape(-1))
    with pytest.raises(ValueError, match="planes.*int64"):
        ctx.warp_poly([ctx.to_device(np.zeros(SRC, np.int64).reshape(-1))], *SRC, coef, cx, cy, *OUT)
    with pytest.raises(ValueError, match="method.*'lanczos'"):
        ctx.warp_poly([u8], *SRC, coef, cx, cy, *OUT, method="lanczos")
    for i, bad in ((0, np.nan), (4, np.inf), (11, -np.inf)):
        c = coef.copy()
        c[i] = bad
        with pytest.raises(ValueError, match=rf"coef\[{i}\]"):
            ctx.warp_poly([u8], *SRC, c, cx, cy, *OUT)
    with pytest.raises(ValueError, match="coef.*12"):
        ctx.warp_poly([u8], *SRC, coef[:6], cx, cy, *OUT)
    with pytest.raises(ValueError, match="cx"):
        ctx.warp_poly([u8], *SRC, coef, np.nan, cy, *OUT)
    with pytest.raises(ValueError, match="planes.*H \\* W"):
        ctx.warp_poly([u8, ctx.to_device(np.zeros((37, 52), np.uint8).reshape(-1))], *SRC, coef, cx, cy, *OUT)
    with pytest.raises(ValueError, match="planes.*dtype"):
        ctx.warp_poly([u8, ctx.to_device(np.zeros(SRC, np.int16).reshape(-1))], *SRC, coef, cx, cy, *OUT)
    with pytest.raises(ValueError, match="out_dtype"):
        ctx.warp_poly([u8], *SRC, coef, cx, cy, *OUT, out_dtype=torch.int16)
    with pytest.raises(ValueError, match="Ho"):
        ctx.warp_poly([u8], *SRC, coef, cx, cy, 0, 5)
    with pytest.raises(ValueError, match="out must"):
        ctx.warp_poly([u8], *SRC, coef, cx, cy, *OUT, out=[torch.empty(5, dtype=torch.uint8, device=u8.device)])
    with pytest.raises(ValueError, match="planes is empty"):
        ctx.warp_poly([], *SRC, coef, cx, cy, *OUT)


def test_a_context_with_a_communication_path_is_refused():
    from rsseg.runtime import Context, RssegUnsupported
    c = Context(0, use_dist=False)
    try:
        c.warp_poly([c.to_device(np.zeros(SRC, np.uint8).reshape(-1))], *SRC, *R.affine_coef(AFFINE, *OUT), *OUT)
        c.install_comm_hook(0, 1, lambda *a: None)     # one rank, identity reductions: a path all the same
        with pytest.raises(RssegUnsupported, match="one GPU"):
            c.warp_poly([c.to_device(np.zeros(SRC, np.uint8).reshape(-1))], *SRC, *R.affine_coef(AFFINE, *OUT), *OUT)
    finally:
        c.close()


def test_profiler_name(ctx):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        ctx.warp_poly([ctx.to_device(np.zeros(SRC, np.uint8).reshape(-1))], *SRC, *R.affine_coef(AFFINE, *OUT), *OUT)
        ms, launches = ctx.prof_get("warp")
        assert launches == 1 and ms > 0
    finally:
        ctx.prof_enable(False)


# ---- the public interface and the chain ----
FWD = [[30.0, 2.5, 500000.0], [1.5, -30.0, 4200000.0]]


def scene_gcps(H, W, n=9, seed=0, noise=4.0):
    rs = np.random.RandomState(seed)
    pts = np.stack([rs.uniform(0, W, n), rs.uniform(0, H, n)], 1)
    xy = pts @ np.array(FWD)[:, :2].T + np.array(FWD)[:, 2] + rs.normal(0, noise, (n, 2))
    return np.concatenate([pts, xy], 1)


def write_gcps(path, g):
    with open(path, "w") as f:
        f.write("# pixel line x y\n")
        for row in g:
            f.write(", ".join(repr(float(v)) for v in row) + "\n")


def host_plan(g, shape, order=1, pixel_size=None):
    from rsseg import georect as G
    t = G.fit_gcp_transform(g, order)
    Ho, Wo, tr = G.output_grid(t, shape, pixel_size)
    return t, G.warp_plan(t, (Ho, Wo), tr, shape)


@pytest.mark.parametrize("order", [1, 2])
def test_warp_planes_and_geometric_correction_gcps(ctx, order):
    from rsseg import georect as G
    rs = np.random.RandomState(20)
    H, W = 45, 61
    g = scene_gcps(H, W, 12, seed=order)
    bands = [random_plane(rs, (H, W), np.uint16) for _ in range(3)]
    t, plan = host_plan(g, (H, W), order)
    Ho, Wo = plan.out_shape
    for method in R.METHODS:
        want, wmask, wn = R.warp(bands, plan.coef, plan.cx, plan.cy, Ho, Wo, method=method)
        assert 0.5 < wmask.mean() < 1.0
        outs, mask, nv = G.warp_planes(ctx, bands, (H, W), plan, method=method)            # host arrays in
        assert all(np.array_equal(o.cpu().numpy().reshape(Ho, Wo), w) for o, w in zip(outs, want)) and nv == wn
        outs, mask, nv = G.warp_planes(ctx, [ctx.to_device(b) for b in bands], (H, W), plan, method=method, out_dtype=np.float64,
                                       want_mask=False)                                    # device tensors in
        want64, _, _ = R.warp(bands, plan.coef, plan.cx, plan.cy, Ho, Wo, method=method, out_dtype=np.float64)
        assert mask is None and all(same_bits(o.cpu().numpy().reshape(Ho, Wo), w) for o, w in zip(outs, want64))
        got, tr, gmask, gt = G.geometric_correction_gcps(bands, g, order=order, method=method)
        assert tr == plan.out_transform and gt.rmse == t.rmse and np.array_equal(gmask, wmask)
        assert all(np.array_equal(a, w) for a, w in zip(got, want))
    with pytest.raises(ValueError, match="src_shape"):
        G.warp_planes(ctx, bands, (H, W + 1), plan)
    with pytest.raises(ValueError, match=r"planes\[0\].*int64"):
        G.warp_planes(ctx, [bands[0].astype(np.int64)], (H, W), plan)


def test_mirror_geometric_correction_still_ignores_its_gcps():
    from modules.features.preprocessing import geometric_correction
    b = [np.arange(12, dtype=np.uint8).reshape(3, 4)]
    out = geometric_correction(b, scene_gcps(3, 4))
    assert np.array_equal(out[0], b[0]) and out[0] is not b[0]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=lambda d: np.dtype(d).name)
def test_stage_with_gcps_equals_the_mirrors_host_chain(ctx, dtype, tmp_path):
    """nearest: warping DN and calibrating after is calibrate -> warp -> stretch exactly"""
    from modules.features.preprocessing import image_enhancement, radiometric_calibration
    from rsseg.preprocess import run_preprocessing_stage
    from rsseg.tiff import read_tiff, read_tiff_georef, write_tiff
    rs = np.random.RandomState(21)
    H, W = 50, 70
    top = 255 if dtype == np.uint8 else 4095
    dn = np.stack([rs.randint(1, top + 1, (H, W)).astype(dtype) for _ in range(7)])
    raw = str(tmp_path / "raw.tif")
    write_tiff(raw, dn, transform=(1.0, 0.0, 0.0, 0.0, -1.0, 0.0), epsg=32649)
    g = scene_gcps(H, W, 10, seed=3)
    t, plan = host_plan(g, (H, W))
    Ho, Wo = plan.out_shape
    out = str(tmp_path / "o" / "pre.tif")
    path, planes, shape, geo, mask = run_preprocessing_stage(raw, out, str(tmp_path / "o"), ctx=ctx, return_device=True, gcps=g)
    assert path == out and shape == (Ho, Wo) and geo["transform"] == plan.out_transform and geo["epsg"] == 32649
    warped, wmask, wn = R.warp(list(dn), plan.coef, plan.cx, plan.cy, Ho, Wo, method="nearest")
    assert 0.5 < wmask.mean() < 1.0 and np.array_equal(mask.cpu().numpy().reshape(Ho, Wo), wmask)
    want = image_enhancement(radiometric_calibration(warped))
    for p, w in zip(planes, want):
        assert np.array_equal(p.cpu().numpy().reshape(Ho, Wo), w)
    assert np.array_equal(read_tiff(out), np.stack(want).astype(np.float32))
    assert read_tiff_georef(out)["transform"] == plan.out_transform


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_stage_mask_with_a_nodata_value(ctx, dtype, tmp_path):
    """return_device with nodata: the warp's mask AND 'no warped DN band equals nodata'"""
    from rsseg.preprocess import run_preprocessing_stage
    from rsseg.tiff import write_tiff
    rs = np.random.RandomState(23)
    H, W = 40, 48
    dn = np.stack([rs.randint(1, 200, (H, W)).astype(dtype) for _ in range(3)])
    dn[0, 5:12, 7:20] = 0
    dn[2, 30:33, 40:48] = 0
    raw = str(tmp_path / "raw.tif")
    write_tiff(raw, dn)
    g = scene_gcps(H, W, 8, seed=6)
    t, plan = host_plan(g, (H, W))
    Ho, Wo = plan.out_shape
    warped, wmask, _ = R.warp(list(dn), plan.coef, plan.cx, plan.cy, Ho, Wo)
    want = wmask & np.all(np.stack(warped) != 0, axis=0)
    assert 0 < want.sum() < wmask.sum() < wmask.size
    out = str(tmp_path / "o" / "pre.tif")
    _, _, shape, _, mask = run_preprocessing_stage(raw, out, str(tmp_path / "o"), ctx=ctx, return_device=True, gcps=g, nodata=0)
    assert shape == (Ho, Wo) and np.array_equal(mask.cpu().numpy().reshape(Ho, Wo), want)
    assert np.array_equal(np.load(str(tmp_path / "o" / "pre_valid.npy")), wmask)      # the file keeps the warp's mask


@pytest.mark.parametrize("resampling,order", [("nearest", 1), ("bilinear", 2), ("cubic", 1)])
def test_preprocess_cli_with_gcps(ctx, tmp_path, resampling, order):
    from rsseg import preprocess
    from rsseg.tiff import read_tiff, read_tiff_georef, write_tiff
    rs = np.random.RandomState(22)
    H, W = 40, 56
    dn = np.stack([rs.randint(0, 256, (H, W)).astype(np.uint8) for _ in range(7)])
    raw, gfile, out = str(tmp_path / "raw.tif"), str(tmp_path / "scene.gcp"), str(tmp_path / "out" / "OUT.tif")
    write_tiff(raw, dn, epsg=32649)
    g = scene_gcps(H, W, 12, seed=4)
    write_gcps(gfile, g)
    assert preprocess.main([raw, out, "--gcps", gfile, "--warp-order", str(order), "--resampling", resampling, "--pixel-size", "25"]) == 0
    t, plan = host_plan(g, (H, W), order, 25.0)
    Ho, Wo = plan.out_shape
    assert read_tiff_georef(out)["transform"] == plan.out_transform and plan.out_transform[0] == 25.0
    assert read_tiff(out).shape == (7, Ho, Wo)
    _, wmask, wn = R.warp([dn[0]], plan.coef, plan.cx, plan.cy, Ho, Wo, method=resampling)
    assert np.array_equal(np.load(str(tmp_path / "out" / "OUT_valid.npy")), wmask)
    rec = json.load(open(str(tmp_path / "out" / "OUT_geometric_correction.json")))
    assert rec["rmse"] == t.rmse and rec["n_valid"] == wn and rec["order"] == order and rec["method"] == resampling
    assert rec["output_shape"] == [Ho, Wo] and tuple(rec["output_transform"]) == plan.out_transform
    assert np.array_equal(np.array(rec["residuals"]), t.residuals) and np.array_equal(np.array(rec["backward"]), t.bwd)
    if resampling != "nearest":
        # integer DN are interpolated into float64 planes, which K15 calibrates and stretches as NumPy does
        warped, _, _ = R.warp(list(dn), plan.coef, plan.cx, plan.cy, Ho, Wo, method=resampling, out_dtype=np.float64)
        from test_preprocess_host import restate_stage1
        want = restate_stage1(warped)
        assert np.array_equal(read_tiff(out), np.stack(want).astype(np.float32))


def test_stages_raw_gcps_kmeans_mask_nodata(ctx, golden_dir, tmp_path):
    from rsseg import stages
    from rsseg.tiff import read_tiff_georef, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 200:296, 300:396]
    assert dn.shape == (7, 96, 96)
    raw, gfile, out = str(tmp_path / "raw.tif"), str(tmp_path / "scene.gcp"), str(tmp_path / "out")
    write_tiff(raw, dn, epsg=32649)
    g = scene_gcps(96, 96, 9, seed=5)
    write_gcps(gfile, g)
    assert stages.main([raw, out, "--raw", "--gcps", gfile, "--classify", "kmeans", "--mask-nodata"]) == 0
    t, plan = host_plan(g, (96, 96))
    Ho, Wo = plan.out_shape
    _, wmask, wn = R.warp([dn[0]], plan.coef, plan.cx, plan.cy, Ho, Wo)
    assert 0.5 < wmask.mean() < 1.0
    assert np.array_equal(np.load(os.path.join(out, "feature_outputs", "valid_mask.npy")), wmask)
    cm = np.load(os.path.join(out, "segmentation_results", "classification_kmeans.npy"))
    assert cm.shape == (Ho, Wo) and np.array_equal(cm == 0, wmask == 0)
    assert read_tiff_georef(os.path.join(out, "preprocessed", "raw_preprocessed.tif"))["transform"] == plan.out_transform
    # without --mask-nodata the collar is classified as data
    out2 = str(tmp_path / "out2")
    assert stages.main([raw, out2, "--raw", "--gcps", gfile, "--classify", "kmeans"]) == 0
    cm2 = np.load(os.path.join(out2, "segmentation_results", "classification_kmeans.npy"))
    assert cm2.shape == (Ho, Wo) and (cm2 > 0).all()


# ---- seeded random family ----
def random_case(seed):
    rs = np.random.RandomState(1000 + seed)
    H, W, Ho, Wo = (int(v) for v in rs.randint(1, 131, 4))
    dtype = DTYPES[rs.randint(len(DTYPES))]
    method = R.METHODS[rs.randint(3)]
    nb = int(rs.randint(1, 5))
    # a well-conditioned backward map: the output rectangle onto roughly the source, rotated and sheared a little
    ang = rs.uniform(-0.3, 0.3)
    sx, sy = W / Wo * rs.uniform(0.7, 1.4), H / Ho * rs.uniform(0.7, 1.4)
    L = np.array([[np.cos(ang) * sx, -np.sin(ang) * sy + rs.uniform(-0.1, 0.1) * sx], [np.sin(ang) * sx, np.cos(ang) * sy]])
    centre = np.array([W / 2 + rs.uniform(-0.2, 0.2) * W, H / 2 + rs.uniform(-0.2, 0.2) * H])
    off = centre - L @ np.array([Wo / 2, Ho / 2])
    coef, cx, cy = R.affine_coef(np.concatenate([L, off[:, None]], 1), Ho, Wo)
    if rs.rand() < 0.5:   # order 2: up to a fifth of the source's side of bend at the output's corner
        coef = coef.copy()
        coef[3:6] = rs.uniform(-1, 1, 3) * 0.2 * W / max(Wo / 2, Ho / 2) ** 2
        coef[9:12] = rs.uniform(-1, 1, 3) * 0.2 * H / max(Wo / 2, Ho / 2) ** 2
    planes = [random_plane(rs, (H, W), dtype) for _ in range(nb)]
    out_dtype = [None, None, np.float32, np.float64][rs.randint(4)]
    fill = 0 if rs.rand() < 0.5 else int(rs.randint(0, 100))
    return planes, coef, cx, cy, Ho, Wo, method, fill, out_dtype


@pytest.mark.parametrize("seed", list(range(SEED0, SEED0 + (N or 12))))
def test_random_family(ctx, seed):
    planes, coef, cx, cy, Ho, Wo, method, fill, out_dtype = random_case(seed)
    check(ctx, planes, coef, cx, cy, Ho, Wo, method, fill=fill, out_dtype=out_dtype)
