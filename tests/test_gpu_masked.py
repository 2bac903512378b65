"""The classifiers on the valid pixels of a raster (rsseg.masked over K19): the masked KMeans fit against the CPU oracle and
against the unmasked fit on NumPy-compacted planes, KMeansModel with a mask, the masked forest against the unmasked walk, and
`python -m rsseg.stages --mask-nodata`.  No tolerances: compaction is data movement and everything downstream is an existing
bit-exact path on a smaller input."""
import json
import os

import numpy as np
import pytest

import compact_ref as CR

pytestmark = pytest.mark.gpu


def scene(name, golden_dir):
    """(planes [(H, W)], mask (H, W) uint8, k)"""
    if name.startswith("blobs"):
        planes, mask = CR.blob_scene(np.float32 if name.endswith("32") else np.float64)
        return planes, mask, 4
    st = np.load(os.path.join(golden_dir, "crop96.npz"))["stack19"]
    dt = np.float32 if name.endswith("32") else np.float64
    return [np.ascontiguousarray(st[:, :, i], dtype=dt) for i in range(19)], CR.collar_and_holes(96, 96, 7, 0.05, 23), 6


SCENES = ["blobs-float32", "blobs-float64", "crop96-float32", "crop96-float64"]


@pytest.mark.parametrize("name", SCENES)
def test_masked_kmeans_equals_the_fit_on_compacted_planes(ctx, oracle, golden_dir, name):
    from rsseg.masked import kmeans_fit_predict_masked
    planes, mask, k = scene(name, golden_dir)
    m = mask != 0
    comp = [CR.compact(p, mask) for p in planes]
    want, info = oracle.kmeans_fit_planes(comp, k)
    labels, meta = kmeans_fit_predict_masked(planes, mask, k, ctx=ctx)
    assert labels.shape == mask.shape and labels.dtype == np.int32 and meta["n_valid"] == int(m.sum())
    # the criterion of tests/test_gpu_fuzz.py for the unmasked fit: seeds, iterations, relocations, labels
    assert np.array_equal(meta["init_indices"], info["init_indices"])
    assert meta["n_iter"] == info["n_iter"] and meta["relocated"] == info["relocated"]
    assert np.array_equal(labels[m], want) and np.all(labels[~m] == -1)
    # the model, bitwise, against the unmasked call on the NumPy-compacted planes
    plain_labels, plain = ctx.kmeans_fit_predict([ctx.to_device(c) for c in comp], k)
    for key in ("centers", "scale", "min"):
        assert np.asarray(meta[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    assert np.array_equal(plain_labels.cpu().numpy(), labels[m])
    # device planes and a device mask of arbitrary non-zero bytes in -> a flat device tensor out
    dev = [ctx.to_device(np.ascontiguousarray(p).reshape(-1)) for p in planes]
    lab2, _ = kmeans_fit_predict_masked(dev, ctx.to_device((mask.reshape(-1) * 255).astype(np.uint8)), k, fill=-3, ctx=ctx)
    assert np.array_equal(lab2.cpu().numpy(), np.where(m.reshape(-1), labels.reshape(-1), -3))


@pytest.mark.parametrize("name", ["blobs-float32", "crop96-float64"])
def test_kmeans_model_with_a_mask(ctx, golden_dir, name):
    from rsseg.kmeans_model import KMeansModel
    planes, mask, k = scene(name, golden_dir)
    m = mask != 0
    comp = [CR.compact(p, mask) for p in planes]
    model, labels = KMeansModel.fit(planes, k, ctx=ctx, mask=mask)
    plain, plain_labels = KMeansModel.fit(comp, k, ctx=ctx)
    assert model.n_samples_fit_ == int(m.sum()) and np.array_equal(labels[m], plain_labels) and np.all(labels[~m] == -1)
    for a in ("cluster_centers_", "scale_", "min_"):
        assert getattr(model, a).tobytes() == getattr(plain, a).tobytes(), a
    # another scene for the sweep: the planes shifted a little, nodata as NaN under the mask
    other = [np.where(m, p * p.dtype.type(0.97) + p.dtype.type(0.01), p.dtype.type(np.nan)) for p in planes]
    ocomp = [CR.compact(p, mask) for p in other]
    want_l, want_d = model.predict_with_distance(ocomp, ctx=ctx)
    want_s = model.summary(ocomp, ctx=ctx)
    lab, dist = model.predict_with_distance(other, ctx=ctx, mask=mask)
    assert lab.shape == mask.shape and np.array_equal(lab[m], want_l) and np.all(lab[~m] == -1)
    assert dist.dtype == want_d.dtype and np.array_equal(dist[m], want_d) and np.all(np.isnan(dist[~m]))
    assert np.array_equal(model.predict(other, ctx=ctx, mask=mask), lab)
    s = model.summary(other, ctx=ctx, mask=mask)
    assert np.array_equal(s["counts"], want_s["counts"]) and int(s["counts"].sum()) == int(m.sum()) == s["n_valid"]
    assert s["inertia"] == want_s["inertia"] and s["overflow"] == want_s["overflow"] and s["score"] == -s["inertia"]


def test_masked_errors(ctx):
    from rsseg.masked import kmeans_fit_predict_masked
    planes, mask = CR.blob_scene(np.float32)
    with pytest.raises(ValueError, match="no valid pixels"):
        kmeans_fit_predict_masked(planes, np.zeros_like(mask), 4, ctx=ctx)
    three = np.zeros_like(mask)
    three[10, 10:13] = 1
    with pytest.raises(ValueError, match=r"n_samples=3 should be >= n_clusters=4"):
        kmeans_fit_predict_masked(planes, three, 4, ctx=ctx)


def test_masked_forest_equals_the_unmasked_walk(ctx, golden_dir):
    from rsseg import forest as FO
    from rsseg.masked import forest_predict_masked
    from modules.features.extract import supervised_classification_predict
    flat = dict(np.load(os.path.join(golden_dir, "rf_samples_model_flat.npz")))
    stack = np.load(os.path.join(golden_dir, "crop96.npz"))["stack19"].copy()
    mask = CR.collar_and_holes(96, 96, 7, 0.05, 23)
    m = mask != 0
    stack[~m] = np.nan                       # nodata as the stage reads it
    stack[20, 30, 4] = np.nan                # and a NaN at a valid pixel: it counts as 0, as in the unmasked path
    assert m[20, 30]
    import rsseg.runtime as rt
    prev, rt._default_ctx = rt._default_ctx, ctx
    try:
        want_lab = supervised_classification_predict(stack, flat)
    finally:
        rt._default_ctx = prev
    want_p, want_c = FO.image_proba_and_confidence(flat, np.nan_to_num(stack, nan=0.0), ctx=ctx)
    lab = forest_predict_masked(flat, stack, mask, ctx=ctx)
    assert lab.shape == (96, 96) and lab.dtype == want_lab.dtype and np.array_equal(lab[m], want_lab[m]) and np.all(lab[~m] == 0)
    assert set(np.unique(lab[m])) <= {1, 2, 3}
    assert np.all(forest_predict_masked(flat, stack, mask, fill=-1, ctx=ctx)[~m] == -1)
    proba, conf = FO.image_proba_and_confidence(flat, stack, ctx=ctx, mask=mask)
    assert proba.shape == want_p.shape and proba.dtype == np.float64 and conf.shape == (96, 96)
    assert np.array_equal(proba[m], want_p[m]) and np.array_equal(conf[m], want_c[m])
    assert not proba[~m].any() and not conf[~m].any()


def test_stage_mask_nodata(ctx, golden_dir, tmp_path):
    """python -m rsseg.stages image.tif out --classify kmeans --mask-nodata on a GeoTIFF with a nodata tag and a collar."""
    from rsseg import stages
    from rsseg.tiff import read_tiff, read_tiff_georef, write_tiff
    dn = np.load(os.path.join(golden_dir, "scene_aa.npz"))["dn"][:, 100:196, 200:328].copy()
    assert dn.dtype == np.uint8 and dn.shape[1:] == (96, 128)
    dn[dn == 0] = 1                                        # 0 is the nodata value: no valid pixel holds it
    collar = np.ones((96, 128), bool)
    collar[9:90, 11:120] = False
    collar[40:44, 60:70] = True                            # and a hole
    dn[:, collar] = 0
    dn[2, 50, 50] = 0                                      # one band without data is enough
    collar[50, 50] = True
    tr = (30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0)
    tagged, untagged = str(tmp_path / "tagged.tif"), str(tmp_path / "untagged.tif")
    write_tiff(tagged, dn, transform=tr, epsg=32649, nodata=0)
    write_tiff(untagged, dn, transform=tr, epsg=32649)
    assert read_tiff_georef(tagged)["nodata"] == 0.0 and read_tiff_georef(untagged)["nodata"] is None

    def run(image, out, *opts):
        assert stages.main([image, str(tmp_path / out), "--classify", "kmeans", "--n-clusters", "5", *opts]) == 0
        sdir = tmp_path / out / "segmentation_results"
        return np.load(sdir / "classification_kmeans.npy"), sdir, tmp_path / out / "feature_outputs"

    cm, sdir, fdir = run(tagged, "masked", "--mask-nodata")
    assert cm.dtype == np.uint8 and np.array_equal(cm == 0, collar)                # 0 exactly on the collar ...
    assert set(np.unique(cm[~collar])) == {1, 2, 3, 4, 5}                           # ... and 1 .. k elsewhere
    vm = np.load(fdir / "valid_mask.npy")
    assert vm.dtype == np.uint8 and vm.shape == (96, 128) and np.array_equal(vm != 0, ~collar)
    tif = str(sdir / "kmeans_classification_map.tif")
    assert read_tiff_georef(tif)["nodata"] == 0.0 and np.array_equal(read_tiff(tif)[0], cm)
    # the value on the command line instead of the tag: the same map
    cm2, _, fdir2 = run(untagged, "masked_value", "--mask-nodata", "0")
    assert np.array_equal(cm2, cm) and np.array_equal(np.load(fdir2 / "valid_mask.npy"), vm)
    # without the option the classification is what it was: every pixel in a cluster, no mask file; and the option does not
    # touch feature extraction (the feature files of both runs are the same bytes)
    cm3, sdir3, fdir3 = run(untagged, "plain")
    assert cm3.min() >= 1 and not (fdir3 / "valid_mask.npy").exists()
    for name in ("all_hierarchical_features.npy", "level1_features.npy", "level2_features.npy"):
        assert (fdir3 / name).read_bytes() == (fdir2 / name).read_bytes(), name
    # the 19-feature stage on the same stack: 0 exactly where the mask is 0
    hier = np.load(fdir3 / "all_hierarchical_features.npy")
    cm4 = stages.run_kmeans_stage(hier, 5, ctx=ctx, valid_mask=vm)
    assert np.array_equal(cm4 == 0, collar) and set(np.unique(cm4[~collar])) == {1, 2, 3, 4, 5}
    # neither a tag nor a value
    with pytest.raises(SystemExit) as e:
        stages.main([untagged, str(tmp_path / "none"), "--classify", "kmeans", "--mask-nodata"])
    assert "no GDAL_NODATA tag" in str(e.value.code)
