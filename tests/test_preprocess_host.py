"""Stage 1 (scripts/1_preprocessing.py, modules/features/preprocessing.py) without a GPU: the mirror's names and signatures,
the NumPy restatement the GPU tests compare against, the georeferencing of load_tm_image / save_processed_image, and the
--raw flag of rsseg.stages.

tests/golden/preprocessing_names.json holds identifiers only.  It was produced once with the functions of oracle/gen_names.py
over the reference's two files, from the repository root, with the reference's checkout as the argument:

    python -c "import json, sys; sys.path.insert(0, 'oracle'); import gen_names as G; R = sys.argv[1]; \
      m = R + '/modules/features/preprocessing.py'; s = R + '/scripts/1_preprocessing.py'; \
      json.dump({'_about': \"identifiers only; produced by oracle/gen_names.py's functions from the reference's files with ast (no import)\", \
                 'modules.features.preprocessing': {'public_names': G.module_public_names(m), 'signatures': G.module_signatures(m)}, \
                 'scripts/1_preprocessing.py': {'star_import_of': 'modules.features.preprocessing', 'free_names': G.script_free_names(s)}}, \
                open('tests/golden/preprocessing_names.json', 'w'), indent=1, sort_keys=True)" REFERENCE_CHECKOUT
"""
import inspect
import json
import os

import numpy as np
import pytest

GAIN = [0.671339, 1.322205, 1.043976, 0.876024, 0.120354, 0.055376, 0.065551]
BIAS = [-2.19, -4.16, -2.21, -2.39, -0.49, 1.18, -0.22]
OUT_OF_SCOPE_LIBRARY_NAMES = {"gdal", "cv2"}


def restate_stage1(bands, gain=GAIN, bias=BIAS, calibrate=True):
    """preprocessing.py:65-72 and :115-118 restated: radiance = gain[i] * band + bias[i] with NumPy 2's promotion (float64
    for integer and float64 DN, float32 for float32 DN), the identity warp, then the stretch in the radiance's dtype and
    astype(np.uint8).  Warnings are NumPy's own."""
    out = []
    for i, b in enumerate(bands):
        r = gain[i] * b + bias[i] if calibrate else b
        mn, mx = np.min(r), np.max(r)
        out.append(((r - mn) * 255.0 / (mx - mn)).astype(np.uint8))
    return out


def _names():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "preprocessing_names.json")))


def test_star_import_resolves_every_name_scripts1_uses():
    spec = _names()
    s1 = spec["scripts/1_preprocessing.py"]
    assert s1["star_import_of"] == "modules.features.preprocessing"
    wanted = set(s1["free_names"])
    assert {"load_tm_image", "radiometric_calibration", "geometric_correction", "image_enhancement", "save_processed_image", "np"} <= wanted
    ns = {}
    exec("from modules.features.preprocessing import *", ns)   # noqa: S102 — what scripts/1 does
    missing = sorted(n for n in wanted - OUT_OF_SCOPE_LIBRARY_NAMES if n not in ns)
    assert not missing, missing
    assert ns["np"] is np
    public = spec["modules.features.preprocessing"]["public_names"]
    for n, kind in public.items():
        if kind == "function":
            assert callable(ns[n]) and ns[n].__module__ == "modules.features.preprocessing", n
        elif n not in OUT_OF_SCOPE_LIBRARY_NAMES:
            assert n in ns, n
    from modules.utils.set_chinese_font import set_chinese_font   # scripts/1:20
    assert set_chinese_font() is None


def test_mirror_signatures_equal_the_reference():
    import modules.features.preprocessing as M
    sigs = _names()["modules.features.preprocessing"]["signatures"]
    assert len(sigs) == 5
    for name, want in sigs.items():
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(M, name)).parameters.values()]
        assert got == want, name


def test_restatement_equals_the_oracle_on_the_bundled_scene(oracle, golden_dir):
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"]
    want = oracle.stage1_preprocess(dn)
    got = restate_stage1([dn[i] for i in range(dn.shape[0])])
    assert len(got) == len(want) == 7
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and np.array_equal(g.astype(np.float32), w)


def test_restatement_follows_numpy2_promotion():
    x32 = np.array([0.0, 1.5, 3.25, 100.0], np.float32)
    r = GAIN[0] * x32 + BIAS[0]
    assert r.dtype == np.float32
    assert np.array_equal(r, np.float32(GAIN[0]) * x32 + np.float32(BIAS[0]))
    assert (GAIN[0] * np.arange(4, dtype=np.int16) + BIAS[0]).dtype == np.float64
    with pytest.warns(RuntimeWarning):
        z = restate_stage1([np.full((3, 3), 7, np.uint8)])[0]
    assert not z.any()
    with pytest.warns(RuntimeWarning):
        assert np.array_equal(np.array([np.nan, np.inf]).astype(np.uint8), [0, 0])


def _tif(tmp_path, name, arr, **kw):
    from rsseg.tiff import write_tiff
    p = str(tmp_path / name)
    write_tiff(p, arr, **kw)
    return p


def test_load_tm_image_without_georeferencing(tmp_path, capsys):
    from modules.features.preprocessing import load_tm_image
    a = (np.arange(3 * 20 * 30) % 251).astype(np.uint8).reshape(3, 20, 30)
    bands, gt, proj = load_tm_image(_tif(tmp_path, "plain.tif", a))
    assert gt == (0.0, 1.0, 0.0, 0.0, 0.0, 1.0) and proj == ""
    assert len(bands) == 3 and all(b.dtype == np.uint8 and b.shape == (20, 30) for b in bands)
    assert np.array_equal(np.stack(bands), a)
    assert "成功加载影像, 尺寸: 30x20, 波段数: 3" in capsys.readouterr().out
    with pytest.raises(Exception, match="无法打开文件: "):
        load_tm_image(str(tmp_path / "missing.tif"))


def test_load_tm_image_with_transform_and_epsg(tmp_path):
    from modules.features.preprocessing import load_tm_image
    a = np.arange(2 * 8 * 9, dtype=np.int16).reshape(2, 8, 9) - 50
    t = (30.0, 0.0, 500000.0, 0.0, -30.0, 4100000.0)
    bands, gt, proj = load_tm_image(_tif(tmp_path, "geo.tif", a, transform=t, epsg=32650))
    assert gt == (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0)   # GDAL order (c, a, b, f, d, e)
    assert proj == "EPSG:32650"
    assert bands[1].dtype == np.int16 and np.array_equal(bands[1], a[1])


@pytest.mark.parametrize("projection, epsg", [("", None), ("EPSG:32650", 32650),
                                              ('PROJCS["WGS 84 / UTM zone 50N",GEOGCS["WGS 84",AUTHORITY["EPSG","4326"]],'
                                               'UNIT["metre",1],AUTHORITY["EPSG","32650"]]', 32650)])
def test_save_processed_image_round_trips(tmp_path, capsys, projection, epsg):
    from modules.features.preprocessing import load_tm_image, save_processed_image
    from rsseg.tiff import _open, read_tiff, read_tiff_georef
    bands = [(np.arange(12 * 17) * (i + 3) % 256).astype(np.uint8).reshape(12, 17) for i in range(3)]
    gt = (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0) if epsg else (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    p = str(tmp_path / "out.tif")
    assert save_processed_image(bands, gt, projection, p) is None
    assert f"已保存处理后的影像到: {p}" in capsys.readouterr().out
    _, _, tags = _open(p)
    assert tags[339][0] == 3 and tags[258][0] == 32      # SampleFormat IEEE float, 32 bits: GDT_Float32
    arr = read_tiff(p)
    assert arr.dtype == np.float32 and np.array_equal(arr, np.stack(bands).astype(np.float32))
    back, gt2, proj2 = load_tm_image(p)
    assert gt2 == gt and proj2 == ("" if epsg is None else f"EPSG:{epsg}")
    assert read_tiff_georef(p)["epsg"] == epsg


def test_save_processed_image_refuses_a_projection_it_cannot_name(tmp_path):
    from modules.features.preprocessing import save_processed_image
    from rsseg.runtime import RssegUnsupported
    with pytest.raises(RssegUnsupported, match="EPSG"):
        save_processed_image([np.zeros((2, 2), np.uint8)], (0.0, 1.0, 0.0, 0.0, 0.0, 1.0), 'LOCAL_CS["x"]', str(tmp_path / "x.tif"))


def test_geometric_correction_returns_copies():
    from modules.features.preprocessing import geometric_correction
    b = [np.arange(6, dtype=np.float64).reshape(2, 3)]
    out = geometric_correction(b, [])
    assert np.array_equal(out[0], b[0]) and out[0] is not b[0] and out[0].dtype == b[0].dtype
    out[0][0, 0] = 99
    assert b[0][0, 0] == 0
    with pytest.raises(ValueError):
        geometric_correction([np.zeros(3)], [])


def test_stages_raw_flag_parses():
    from rsseg import stages
    ap = stages.build_parser()
    a = stages.parse_args(ap, ["raw.tif", "out", "--raw", "--classify", "kmeans", "--evaluate", "roi.npy"])
    assert a.raw and a.classify == "kmeans" and a.evaluate == "roi.npy" and not a.no_preprocessing
    assert not stages.parse_args(ap, ["img.tif", "out"]).raw
    assert inspect.signature(stages.run_scripts_2_3).parameters["raw"].default is False
    with pytest.raises(SystemExit):
        stages.parse_args(ap, ["raw.tif", "out", "--raw", "--evaluate", "roi.npy"])


def test_preprocess_cli_parses_and_keeps_the_reference_signature():
    from rsseg import preprocess as PP
    assert list(inspect.signature(PP.run_preprocessing_stage).parameters)[:3] == ["input_file", "output_file", "visualization_output_dir"]
    assert PP.GAIN == GAIN and PP.BIAS == BIAS
    assert PP.gdal_geotransform(None) == (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    assert PP.rasterio_transform(PP.gdal_geotransform((30.0, 0.0, 5.0, 0.0, -30.0, 7.0))) == (30.0, 0.0, 5.0, 0.0, -30.0, 7.0)
    from rsseg.runtime import RssegUnsupported
    for dt in (np.int64, np.int8, np.uint32, np.bool_):
        with pytest.raises(RssegUnsupported, match=np.dtype(dt).name):
            PP.check_dn_dtype(dt)
