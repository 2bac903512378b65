"""K15 on the GPU: stage 1 (radiometric calibration, identity warp, 8-bit stretch) against the NumPy restatement of
tests/test_preprocess_host.py, bit for bit, for every DN dtype; degenerate bands; refusals; the bundled scene through the
feature stack and the forest; the --raw command; a row-sharded raster; the full 16384^2 x 7 size."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from test_preprocess_host import BIAS, GAIN, restate_stage1

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int16, np.uint16, np.int32, np.float32, np.float64]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bands(rng, dt, n, nb, narrow):
    dt = np.dtype(dt)
    out = []
    for i in range(nb):
        if dt.kind in "ui":
            info = np.iinfo(dt)
            lo, hi = (int(info.min), int(info.max)) if not narrow else (int(max(info.min, -40)) + 60, int(max(info.min, -40)) + 60 + 11 + i)
            b = rng.integers(lo, hi, n, endpoint=True, dtype=np.int64)
            if not narrow and n >= 2:          # the type's extremes, somewhere in the band
                b[rng.integers(0, n)] = lo
                b[rng.integers(0, n)] = hi
            out.append(b.astype(dt))
        else:
            if narrow:
                b = 100.0 + rng.random(n) * (0.5 + i)
            else:
                b = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)
            out.append(b.astype(dt))
    return out


def _quiet(fn, *a):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*a)


@pytest.mark.parametrize("n", [1, 15, 17, 1000, 65536 + 7])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_stage1_bitexact_every_dtype(ctx, dt, n):
    from rsseg.preprocess import preprocess_to_device
    rng = np.random.default_rng(n * 7 + DTYPES.index(dt))
    for nb in (1, 5, 7):
        for narrow in (False, True):
            bands = _bands(rng, dt, n, nb, narrow)
            want = _quiet(restate_stage1, bands)
            got = _quiet(preprocess_to_device, ctx, bands)
            for i in range(nb):
                g = got[i].cpu().numpy()
                assert g.dtype == np.uint8 and np.array_equal(g, want[i]), (nb, narrow, i, int((g != want[i]).sum()))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_mirror_functions_bitexact(dt):
    from modules.features.preprocessing import geometric_correction, image_enhancement, radiometric_calibration
    rng = np.random.default_rng(5)
    bands = [b.reshape(37, 53) for b in _bands(rng, dt, 37 * 53, 7, False)]
    cal = radiometric_calibration(bands)
    for i, (c, b) in enumerate(zip(cal, bands)):
        w = GAIN[i] * b + BIAS[i]
        assert c.dtype == w.dtype == (np.float32 if dt == np.float32 else np.float64) and c.shape == b.shape
        assert np.array_equal(c, w, equal_nan=True), i
    cor = geometric_correction(cal, [])
    enh = _quiet(image_enhancement, cor)
    want = _quiet(restate_stage1, cal, GAIN, BIAS, False)
    for e, w in zip(enh, want):
        assert e.dtype == np.uint8 and e.shape == (37, 53) and np.array_equal(e, w)
    # image_enhancement on the DN themselves (the stretch alone, in the band's dtype)
    if np.dtype(dt).kind in "uf" or dt == np.int16:
        small = [((b.astype(np.float64) % 1000)).astype(dt) for b in bands] if np.dtype(dt).kind == "i" else bands
        assert all(np.array_equal(e, w) for e, w in zip(_quiet(image_enhancement, small), _quiet(restate_stage1, small, GAIN, BIAS, False)))


def _degenerate_cases():
    n = 301
    base = (np.arange(n) % 97).astype(np.float64)
    nan = base.copy()
    nan[150] = np.nan
    pinf = base.copy()
    pinf[3] = np.inf
    ninf = base.copy()
    ninf[7] = -np.inf
    over = (np.arange(n) % 5).astype(np.float32)
    over[10] = np.float32(3.0e38)    # finite DN; 1.322205 * 3e38 overflows float32 -> radiance inf
    return {"constant_u8": [np.full(n, 77, np.uint8)], "constant_f32": [np.full(n, -2.5, np.float32)],
            "nan_f64": [nan], "nan_f32": [nan.astype(np.float32)], "pinf_f64": [pinf], "ninf_f32": [ninf.astype(np.float32)],
            "overflow_f32": [(np.arange(n) % 7).astype(np.float32), over]}


@pytest.mark.parametrize("case", list(_degenerate_cases()))
def test_degenerate_bands_come_out_as_numpy_gives_them(ctx, case):
    from rsseg.preprocess import preprocess_to_device
    bands = _degenerate_cases()[case]
    with warnings.catch_warnings(record=True) as wn, np.errstate(all="warn"):
        warnings.simplefilter("always")
        want = restate_stage1(bands)
    assert any(issubclass(w.category, RuntimeWarning) for w in wn)         # NumPy warns on this band
    with pytest.warns(RuntimeWarning, match=f"band {len(bands) - 1}:") as rec:
        got = preprocess_to_device(ctx, bands)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1   # one per degenerate band
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    assert not want[-1].any()


def test_refusals(ctx):
    import torch
    from modules.features.preprocessing import image_enhancement, radiometric_calibration
    from rsseg import _lib as L
    from rsseg.preprocess import preprocess_to_device
    from rsseg.runtime import RssegUnsupported
    eight = [np.zeros(64, np.uint8)] * 8
    with pytest.raises(IndexError):
        preprocess_to_device(ctx, eight)
    with pytest.raises(IndexError):
        radiometric_calibration(eight)
    for dt in (np.int64, np.int8, np.uint32):
        with pytest.raises(RssegUnsupported, match=np.dtype(dt).name):
            preprocess_to_device(ctx, [np.zeros(64, dt)])
        with pytest.raises(RssegUnsupported, match=np.dtype(dt).name):
            radiometric_calibration([np.zeros((8, 8), dt)])
        with pytest.raises(RssegUnsupported, match=np.dtype(dt).name):
            image_enhancement([np.zeros((8, 8), dt)])
    with pytest.raises(ValueError, match="int64"):
        ctx.preprocess_u8([ctx.to_device(np.zeros(64, np.int64))])
    # the C entry names an unsupported dtype too
    x, o = ctx.to_device(np.zeros(64, np.int64)), torch.empty(64, dtype=torch.uint8, device=ctx.device)
    rc = ctx.lib.rsseg_preprocess_u8(ctx.h, ctx._pp([x]), L.I64, 1, 64, None, None, ctx._pp([o]), None)
    assert rc == -1 and b"int64" in ctx.lib.rsseg_last_error(ctx.h)
    p = ctx.to_device(np.arange(64, dtype=np.uint8))
    for g, b in ((0.0, 1.0), (-0.5, 1.0), (np.inf, 0.0), (np.nan, 0.0), (1.0, np.nan), (1.0, -np.inf)):
        with pytest.raises(ValueError, match="gain"):
            ctx.preprocess_u8([p], [g], [b])
    with pytest.raises(ValueError):
        ctx.radiometric(p, 1.0, np.inf)


def test_bundled_scene_end_to_end(ctx, oracle, golden_dir):
    from rsseg import pipeline as P
    from rsseg.preprocess import preprocess_to_device
    scene = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    dn = scene["dn"]
    want = oracle.stage1_preprocess(dn)
    planes = preprocess_to_device(ctx, [dn[i] for i in range(7)])
    for p, w in zip(planes, want):
        assert p.dtype.itemsize == 1 and np.array_equal(p.cpu().numpy().reshape(600, 600).astype(np.float32), w)
    stack, _ = P.feature_stack19(ctx, planes, 600, 600)
    f = dict(np.load(os.path.join(golden_dir, "rf_samples_model_flat.npz")))
    ctx.forest_load(f)
    cm = ctx.forest_predict(P.stack19_forest_planes(ctx, stack)).cpu().numpy().reshape(600, 600)
    assert float(np.mean(cm == scene["class_map"])) >= 0.999
    for (x, y), lab in zip(scene["sample_coords"], scene["sample_labels"]):
        assert cm[y, x] == lab


def _tree_files(d):
    out = {}
    for sub in ("feature_outputs", "segmentation_results"):
        for root, _, files in os.walk(os.path.join(d, sub)):
            for fn in files:
                if fn.endswith(".npy"):
                    p = os.path.join(root, fn)
                    out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_stages_raw_cli_equals_the_two_step_run(ctx, oracle, golden_dir, tmp_path):
    from rsseg import stages
    from rsseg.tiff import read_tiff, read_tiff_georef, write_tiff
    g = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    raw = str(tmp_path / "AA.tif")
    write_tiff(raw, g["dn"], transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    np.save(tmp_path / "roi.npy", g["roi_mask"])
    out = str(tmp_path / "out")
    assert stages.main([raw, out, "--raw", "--classify", "kmeans", "--evaluate", str(tmp_path / "roi.npy")]) == 0
    tile = os.path.join(out, "preprocessed", "AA_preprocessed.tif")
    arr = read_tiff(tile)
    assert arr.dtype == np.float32 and np.array_equal(arr, np.stack(oracle.stage1_preprocess(g["dn"])))
    geo = read_tiff_georef(tile)
    assert geo["transform"] == (30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0) and geo["epsg"] == 32649
    assert (tmp_path / "out" / "evaluation_results" / "evaluation_report.txt").exists()
    out2 = str(tmp_path / "out2")
    assert stages.main([tile, out2, "--classify", "kmeans"]) == 0
    a, b = _tree_files(out), _tree_files(out2)
    assert len(a) >= 4 and a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT]))
    t3 = str(tmp_path / "cli" / "AA_pre.tif")
    r = subprocess.run([sys.executable, "-m", "rsseg.preprocess", raw, t3], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(t3, "rb").read() == open(tile, "rb").read()


@pytest.mark.parametrize("world", [2, 3])
def test_row_sharded_stripes_equal_the_single_rank_result(ctx, world):
    from test_gpu_eval import _ThreadWorld
    from rsseg.preprocess import preprocess_to_device
    from rsseg.runtime import Context
    H, W = 97, 131
    rng = np.random.default_rng(world)
    bands = [rng.integers(1000, 3000, (H, W)).astype(np.uint16) for _ in range(5)]
    for b in bands:                     # the raster's min only in rank 0's stripe, its max only in the last stripe
        b[2, 5] = 7
        b[H - 3, W - 2] = 60000
    fb = [rng.standard_normal((H, W)).astype(np.float32) for _ in range(3)]
    fb[0][1, 1], fb[0][H - 1, 3] = -500.0, 800.0
    fb[2][H // 2, 0] = np.nan           # a NaN in one stripe: every rank's band comes out all zero
    want_u = [p.cpu().numpy().reshape(H, W) for p in preprocess_to_device(ctx, bands)]
    with pytest.warns(RuntimeWarning):
        want_f = [p.cpu().numpy().reshape(H, W) for p in preprocess_to_device(ctx, fb)]
    tw = _ThreadWorld(world)
    got = [None] * world

    def rank_main(r):
        c = Context(0, use_dist=False)
        c.install_comm_hook(r, world, tw.hook(r))
        r0, r1 = r * H // world, (r + 1) * H // world
        u, rng_u = preprocess_to_device(c, [b[r0:r1] for b in bands], want_range=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f = preprocess_to_device(c, [b[r0:r1] for b in fb])
        got[r] = (r0, r1, [p.cpu().numpy().reshape(r1 - r0, W) for p in u], [p.cpu().numpy().reshape(r1 - r0, W) for p in f], rng_u)
        c.close()

    tw.run(rank_main)
    assert tw.calls == 2 * 3
    for r0, r1, u, f, rng_u in got:
        assert np.array_equal(rng_u[:, :2], np.array([[7.0, 60000.0]] * 5))
        for i in range(5):
            assert np.array_equal(u[i], want_u[i][r0:r1]), (r0, i)
        for i in range(3):
            assert np.array_equal(f[i], want_f[i][r0:r1]), (r0, i)
        assert not f[2].any()


def test_at_size_16384_u8_against_torch_float64(ctx):
    import torch
    from rsseg.preprocess import preprocess_to_device
    N, nb = 16384 * 16384, 7
    g = torch.Generator(device=ctx.device).manual_seed(1)
    dn = [torch.randint(3 + i, 250 - i, (N,), generator=g, device=ctx.device, dtype=torch.uint8) for i in range(nb)]
    out = preprocess_to_device(ctx, dn, want_range=True, warn=False)   # warm: workspace and pinned staging sized
    torch.cuda.synchronize()
    ctx.host_syncs(reset=True)
    out = preprocess_to_device(ctx, dn, warn=False)
    assert ctx.host_syncs() == 0
    out2, rng = preprocess_to_device(ctx, dn, want_range=True, warn=False)
    assert ctx.host_syncs() == 1
    for i in range(nb):
        r = GAIN[i] * dn[i].to(torch.float64)
        r = r + BIAS[i]
        mn, mx = r.min(), r.max()
        v = ((r - mn) * 255.0) / (mx - mn)
        want = torch.where((v >= 0) & (v < 256), v.trunc(), torch.zeros_like(v)).to(torch.uint8)
        assert torch.equal(out[i], want) and torch.equal(out2[i], want), i
        assert rng[i, 0] == float(dn[i].min()) and rng[i, 1] == float(dn[i].max()) and rng[i, 2] == 0
        del r, v, want
