"""Host side of K21 (rsseg/georect.py) and the NumPy restatement of the kernel (tests/warp_ref.py), without a GPU: the GCP
fit against np.linalg.lstsq and an independent restatement of residuals and RMSE, its refusals, the GCP parser, the output
grid, the JSON round trip; the restatement against scipy.ndimage.map_coordinates and its own properties."""
import numpy as np
import pytest

import warp_ref as R
from rsseg import georect as G

EPS = np.finfo(np.float64).eps
# the shapes and the backward affine of the GPU sweep (tests/test_gpu_warp.py)
SRC, OUT = (37, 53), (41, 67)
AFFINE = [[0.93, 0.11, -3.2], [-0.08, 0.97, 2.6]]


def affine_gcps(A, pts):
    """GCPs that the forward affine A = [[a, b, c], [d, e, f]] maps exactly: x = a * pixel + b * line + c."""
    pts = np.asarray(pts, np.float64)
    A = np.asarray(A, np.float64)
    xy = pts @ A[:, :2].T + A[:, 2]
    return np.concatenate([pts, xy], axis=1)


FWD = [[30.0, 2.5, 500000.0], [1.5, -30.0, 4200000.0]]


# ---- fit ----
def test_three_exact_gcps_recover_the_affine():
    g = affine_gcps(FWD, [[10.5, 20.5], [400.5, 35.5], [120.5, 300.5]])
    t = G.fit_gcp_transform(g, 1)
    px, ln = np.array([0.0, 512.0, 77.25]), np.array([0.0, 3.0, 410.5])
    x, y = t.forward(px, ln)
    want = np.stack([px, ln], 1) @ np.array(FWD)[:, :2].T + np.array(FWD)[:, 2]
    assert np.allclose(x, want[:, 0], rtol=0, atol=1e-6) and np.allclose(y, want[:, 1], rtol=0, atol=1e-6)   # 1e-6 m at 4.2e6: 2e-13 relative
    bp, bl = t.backward(want[:, 0], want[:, 1])
    assert np.allclose(bp, px, rtol=0, atol=1e-8) and np.allclose(bl, ln, rtol=0, atol=1e-8)
    assert t.rmse < 1e-9 and np.abs(t.residuals).max() < 1e-9


def noisy_gcps(n, seed, order=1):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(0, 600, (n, 2))
    g = affine_gcps(FWD, pts)
    if order == 2:
        g[:, 2] += 1e-3 * (pts[:, 0] - 300) ** 2 - 2e-3 * (pts[:, 0] - 300) * (pts[:, 1] - 300)
        g[:, 3] += 5e-4 * (pts[:, 1] - 300) ** 2
    g[:, 2:] += rs.normal(0, 12.0, (n, 2))
    return g


@pytest.mark.parametrize("order,n", [(1, 12), (2, 6), (2, 15)])
def test_fit_equals_lstsq_on_the_normalised_design(order, n):
    g = noisy_gcps(n, 7 + n, order)
    t = G.fit_gcp_transform(g, order)
    for coef, norm, (a, b), (ta, tb) in ((t.fwd, t.fwd_norm, (g[:, 0], g[:, 1]), (g[:, 2], g[:, 3])),
                                         (t.bwd, t.bwd_norm, (g[:, 2], g[:, 3]), (g[:, 0], g[:, 1]))):
        an, bn = (a - norm[0]) / norm[2], (b - norm[1]) / norm[3]
        assert np.abs(an).max() <= 1.0 and np.abs(bn).max() <= 1.0          # centred and scaled
        cols = [np.ones(n), an, bn] + ([an * an, an * bn, bn * bn] if order == 2 else [])
        A = np.stack(cols, 1)
        assert coef.shape == (2, A.shape[1])
        for row, target in zip(coef, (ta, tb)):
            want = np.linalg.lstsq(A, target, rcond=None)[0]
            assert np.allclose(row, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    # residuals and RMSE restated: evaluate the backward polynomial by hand
    mx, my, sx, sy = t.bwd_norm
    xn, yn = (g[:, 2] - mx) / sx, (g[:, 3] - my) / sy
    terms = [np.ones(n), xn, yn] + ([xn * xn, xn * yn, yn * yn] if order == 2 else [])
    bp = sum(c * v for c, v in zip(t.bwd[0], terms))
    bl = sum(c * v for c, v in zip(t.bwd[1], terms))
    res = np.stack([bp - g[:, 0], bl - g[:, 1]], 1)
    assert np.allclose(t.residuals, res, rtol=0, atol=1e-9)
    assert t.residuals.shape == (n, 2)
    assert abs(t.rmse - np.sqrt(np.mean(res[:, 0] ** 2 + res[:, 1] ** 2))) < 1e-9
    if n > G.N_TERMS[order]:
        assert 0.05 < t.rmse < 5.0    # 12 m of noise on 30 m pixels
    else:
        assert t.rmse < 1e-6          # as many points as coefficients: the fit interpolates


def test_fit_refusals_name_the_cause():
    g = noisy_gcps(12, 1)
    with pytest.raises(ValueError, match="too few GCPs"):
        G.fit_gcp_transform(g[:2], 1)
    with pytest.raises(ValueError, match="too few GCPs"):
        G.fit_gcp_transform(g[:5], 2)
    with pytest.raises(ValueError, match="order"):
        G.fit_gcp_transform(g, 3)
    with pytest.raises(ValueError, match="order"):
        G.fit_gcp_transform(g, 0)
    line = affine_gcps(FWD, [[i * 10.0, i * 20.0] for i in range(8)])
    with pytest.raises(ValueError, match="rank-deficient"):
        G.fit_gcp_transform(line, 1)
    with pytest.raises(ValueError, match="rank-deficient"):
        G.fit_gcp_transform(line, 2)
    bad = g.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        G.fit_gcp_transform(bad, 1)
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        G.fit_gcp_transform(g[:, :3], 1)


def test_parse_gcps(tmp_path):
    text = "# pixel line x y\n10.5 20.5 500315.0 4199400.5\n\n  400.5, 35.5, 512103.75, 4199535.75  # corner\n120.5,300.5\t504366.25 4191165.75\n"
    want = np.array([[10.5, 20.5, 500315.0, 4199400.5], [400.5, 35.5, 512103.75, 4199535.75], [120.5, 300.5, 504366.25, 4191165.75]])
    got = G.parse_gcps(text)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    p = tmp_path / "scene.gcp"
    p.write_text(text)
    assert np.array_equal(G.parse_gcps(str(p)), want)
    assert np.array_equal(G.parse_gcps(p), want)
    assert G.parse_gcps("# nothing\n").shape == (0, 4)
    with pytest.raises(ValueError, match="line 2.*3 values"):
        G.parse_gcps("1 2 3 4\n1 2 3\n")
    with pytest.raises(ValueError, match="line 3.*5 values"):
        G.parse_gcps("1 2 3 4\n# c\n1 2 3 4 5\n")
    with pytest.raises(ValueError, match="line 1.*non-finite"):
        G.parse_gcps("1 2 inf 4\n")
    with pytest.raises(ValueError, match="line 2.*non-finite"):
        G.parse_gcps("1 2 3 4\n1 nan 3 4\n")
    with pytest.raises(ValueError, match="line 1.*not a number"):
        G.parse_gcps("1 2 three 4\n")


@pytest.mark.parametrize("order", [1, 2])
def test_output_grid_contains_the_corners_and_is_north_up(order):
    g = noisy_gcps(15, 3, order)
    t = G.fit_gcp_transform(g, order)
    H, W = 480, 640
    Ho, Wo, tr = G.output_grid(t, (H, W))
    a, b, c, d, e, f = tr
    assert b == 0.0 and d == 0.0 and a > 0 and e == -a
    x, y = t.forward(np.array([0.0, W, 0.0, W]), np.array([0.0, 0.0, H, H]))
    assert (x >= c).all() and (x <= c + a * Wo).all() and (y <= f).all() and (y >= f - a * Ho).all()
    assert abs(a - 30.0) < 1.0                                        # |det| of FWD's linear part is 903.75: sqrt = 30.06
    assert (c + a * (Wo - 1) < x.max()) and (f - a * (Ho - 1) > y.min())   # and no wider than it must be
    Ho2, Wo2, tr2 = G.output_grid(t, (H, W), pixel_size=60.0)
    assert tr2[0] == 60.0 and tr2[4] == -60.0 and abs(Wo2 - Wo * a / 60.0) <= 1 and abs(Ho2 - Ho * a / 60.0) <= 1
    with pytest.raises(ValueError, match="pixel_size"):
        G.output_grid(t, (H, W), pixel_size=0.0)


@pytest.mark.parametrize("order", [1, 2])
def test_json_round_trip_is_bitwise(order):
    t = G.fit_gcp_transform(noisy_gcps(15, 5, order), order)
    u = G.GcpTransform.from_json(t.to_json())
    assert u.order == t.order and u.rmse == t.rmse and u.fwd_norm == t.fwd_norm and u.bwd_norm == t.bwd_norm
    for a, b in ((t.fwd, u.fwd), (t.bwd, u.bwd), (t.residuals, u.residuals)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("order", [1, 2])
def test_warp_plan_composes_backward_with_the_grid(order):
    """the plan's polynomials give, at every output pixel, what backward(out_transform(pixel centre)) gives"""
    t = G.fit_gcp_transform(noisy_gcps(15, 9, order), order)
    H, W = 120, 160
    Ho, Wo, tr = G.output_grid(t, (H, W))
    plan = G.warp_plan(t, (Ho, Wo), tr, (H, W))
    assert plan.coef.shape == (12,) and plan.cx == Wo / 2 and plan.cy == Ho / 2 and plan.out_shape == (Ho, Wo)
    if order == 1:
        assert not plan.coef[3:6].any() and not plan.coef[9:12].any()
    u, v = R.source_coords(plan.coef, plan.cx, plan.cy, Ho, Wo)
    cc, rr = np.meshgrid(np.arange(Wo) + 0.5, np.arange(Ho) + 0.5)
    bp, bl = t.backward(tr[0] * cc + tr[1] * rr + tr[2], tr[3] * cc + tr[4] * rr + tr[5])
    assert np.abs(u - bp).max() < 1e-7 and np.abs(v - bl).max() < 1e-7   # pixels; float64 at 1e6 m with 30 m pixels resolves 1e-11
    # the rectified grid covers the source: most source pixels are sampled
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    assert 0.5 < ok.mean() <= 1.0


def test_command_line_options():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["raw.tif", "out", "--raw", "--gcps", "scene.gcp", "--classify", "kmeans", "--mask-nodata"])
    assert (a.gcps, a.warp_order, a.resampling, a.pixel_size, a.mask_nodata) == ("scene.gcp", 1, "nearest", None, stages.MASK_NODATA_FROM_TAG)
    a = stages.parse_args(ap, ["raw.tif", "out", "--raw", "--gcps", "g", "--warp-order", "2", "--resampling", "cubic", "--pixel-size", "28.5"])
    assert (a.warp_order, a.resampling, a.pixel_size) == (2, "cubic", 28.5)
    for argv in (["img.tif", "out", "--gcps", "g"],                                        # GCPs rectify the raw raster only
                 ["raw.tif", "out", "--raw", "--classify", "kmeans", "--mask-nodata", "0"],   # as before: not without --gcps
                 ["raw.tif", "out", "--raw", "--gcps", "g", "--warp-order", "3"],
                 ["raw.tif", "out", "--raw", "--gcps", "g", "--resampling", "lanczos"]):
        with pytest.raises(SystemExit):
            stages.parse_args(stages.build_parser(), argv)
    assert stages.parse_args(stages.build_parser(), ["img.tif", "out"]).gcps is None


# ---- the restatement against SciPy ----
def sweep_case(dtype=np.float64, seed=0):
    rs = np.random.RandomState(seed)
    src = (rs.rand(*SRC) * 200.0 - 20.0).astype(dtype)
    coef, cx, cy = R.affine_coef(AFFINE, *OUT)
    return src, coef, cx, cy


def test_restatement_against_scipy():
    import scipy.ndimage as ndi
    src, coef, cx, cy = sweep_case()
    u, v = R.source_coords(coef, cx, cy, *OUT)
    (near,), mask, nv = R.warp([src], coef, cx, cy, *OUT, method="nearest")
    (bil,), mask2, _ = R.warp([src], coef, cx, cy, *OUT, method="bilinear")
    ok = mask.astype(bool)
    assert np.array_equal(mask, mask2) and nv == ok.sum()
    share = ok.mean()
    print(f"valid share {share:.3f}")
    assert 0.2 <= share <= 0.95
    coords = np.stack([v[ok] - 0.5, u[ok] - 0.5])
    want0 = ndi.map_coordinates(src, coords, order=0, mode="nearest")
    assert int((near[ok] != want0).sum()) == 0
    want1 = ndi.map_coordinates(src, coords, order=1, mode="nearest")
    diff = np.abs(bil[ok] - want1).max()
    bound = 8 * EPS * np.abs(src).max()
    print(f"bilinear: max |diff| {diff:.3e} = {diff / (EPS * np.abs(src).max()):.2f} eps max|v|, bound {bound:.3e}")
    assert diff <= bound
    assert (near[~ok] == 0).all() and (bil[~ok] == 0).all()


# ---- properties of the restatement ----
def test_cubic_reproduces_a_quadratic_surface():
    H, W = 24, 31
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = lambda x, y: 3.0 + 0.5 * x - 0.25 * y + 0.02 * x * x - 0.03 * x * y + 0.01 * y * y
    src = f(xx, yy)
    Ho, Wo = 29, 37
    coef, cx, cy = R.affine_coef([[0.71, 0.13, 2.4], [-0.09, 0.66, 3.3]], Ho, Wo)
    u, v = R.source_coords(coef, cx, cy, Ho, Wo)
    (got,), mask, _ = R.warp([src], coef, cx, cy, Ho, Wo, method="cubic")
    fx, fy = u - 0.5, v - 0.5
    inner = mask.astype(bool) & (np.floor(fx) >= 1) & (np.floor(fx) + 2 <= W - 1) & (np.floor(fy) >= 1) & (np.floor(fy) + 2 <= H - 1)
    assert inner.sum() > 300
    err = np.abs(got[inner] - f(fx[inner], fy[inner])).max()
    print(f"cubic on a quadratic: max error {err:.3e}, max|v| {np.abs(src).max():.3f}")
    assert err <= 1e-9 * np.abs(src).max()
    # and the weights are a partition of unity with Keys' values at the knots
    t = np.linspace(0, 1, 17, endpoint=False)
    assert np.abs(sum(R.keys_weights(t)) - 1.0).max() < 1e-15
    assert [float(w) for w in R.keys_weights(np.float64(0.0))] == [0.0, 1.0, 0.0, 0.0]
    assert np.allclose([float(w) for w in R.keys_weights(np.float64(0.5))], [-0.0625, 0.5625, 0.5625, -0.0625], rtol=0, atol=1e-16)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
@pytest.mark.parametrize("method", R.METHODS)
def test_identity_and_integer_shift(dtype, method):
    rs = np.random.RandomState(4)
    src = (rs.rand(19, 23) * 250).astype(dtype)
    coef, cx, cy = R.affine_coef([[1, 0, 0], [0, 1, 0]], 19, 23)
    (got,), mask, nv = R.warp([src], coef, cx, cy, 19, 23, method=method)
    assert got.dtype == src.dtype and np.array_equal(got, src) and mask.all() and nv == src.size
    coef, cx, cy = R.affine_coef([[1, 0, 3], [0, 1, -2]], 19, 23)   # out(r, c) = src(r - 2, c + 3)
    (got,), mask, nv = R.warp([src], coef, cx, cy, 19, 23, method=method, fill=7)
    want = np.full_like(src, 7)
    want[2:, :20] = src[:17, 3:]
    wmask = np.zeros((19, 23), np.uint8)
    wmask[2:, :20] = 1
    assert np.array_equal(got, want) and np.array_equal(mask, wmask) and nv == 17 * 20


def test_half_pixel_shift_rounds_ties_to_even():
    src = np.array([[0, 1, 2, 5, 6, 9, 10, 13]], np.uint8)
    coef, cx, cy = R.affine_coef([[1, 0, 0.5], [0, 1, 0]], 1, 7)   # between neighbours: means 0.5 1.5 3.5 5.5 7.5 9.5 11.5
    (got,), mask, _ = R.warp([src], coef, cx, cy, 1, 7, method="bilinear")
    assert mask.all() and got.tolist() == [[0, 2, 4, 6, 8, 10, 12]]
    (raw,), _, _ = R.warp([src], coef, cx, cy, 1, 7, method="bilinear", out_dtype=np.float64)
    assert raw.tolist() == [[0.5, 1.5, 3.5, 5.5, 7.5, 9.5, 11.5]]
