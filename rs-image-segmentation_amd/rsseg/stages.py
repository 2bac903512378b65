"""
Counterparts of the two stage functions that bracket the hot path:

  run_feature_extraction_stage   reference scripts/2_feature_extraction.py:27-133
  run_classification_stage       reference scripts/3_classification.py:267-505 (KMeans and forest branches)

They keep the reference's return values and on-disk layout (.npy of the (H, W, C) float64 stacks,
scripts/2:193-214; pickle with 'hierarchical_features' / 'all_extracted_features_dict' / 'dimensions',
scripts/2:222-232; label maps as .npy), but run the whole chain on the device with ONE upload of the
bands and one download per product, instead of a host round trip per function as the per-function
mirrors in modules/ do.  Plotting (scripts/2:131, 267-385; scripts/3:491) is out of scope.
"""
from __future__ import annotations

import json
import os
import pickle
from dataclasses import dataclass, replace
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import pipeline as P
from .runtime import Context, RssegUnsupported, default_context


def run_feature_extraction_stage(bands_data: Sequence[np.ndarray], preprocessing: bool = True, texture_band_index: int = 3,
                                 ctx: Optional[Context] = None) -> Tuple[Dict, Dict]:
    """bands_data: list of >= 5 (H, W) arrays in TM band order.  `texture_band_index` is accepted and
    ignored exactly as in the reference (NIR = bands[3] is hard-wired, scripts/2:84)."""
    ctx = ctx or default_context()
    h, w = np.asarray(bands_data[0]).shape
    # 8-bit rasters cross PCIe as one byte per pixel and STAY one byte per pixel in HBM (Context.upload_band): the order
    # statistics, index and PCA kernels read the uint8 planes directly; anything else is float32 as in the reference
    arrs = [np.asarray(b) for b in bands_data if b is not None]
    all_u8 = all(a.dtype == np.uint8 for a in arrs)
    dev = [ctx.upload_band(a) if all_u8 else ctx.upload_f32(a) for a in arrs]
    return _feature_extraction_on_device(ctx, dev, h, w, preprocessing)


def _feature_extraction_on_device(ctx: Context, dev: Sequence, h: int, w: int, preprocessing: bool = True) -> Tuple[Dict, Dict]:
    """run_feature_extraction_stage from the bands' flat device planes (uint8 or float32): what --raw hands over from stage 1
    without a host round trip."""
    planes, ex = P.feature_stack19(ctx, dev, h, w, preprocessing=bool(preprocessing))   # False: bands taken as given (scripts/2:43-50)

    def host(t):
        return t.cpu().numpy().reshape(h, w)

    # features_dict in the reference's insertion order (scripts/2:62-106; the members of the nested dicts in the order
    # indices.py builds them): the order is part of the interface, because unsupervised_kmeans_classification's default
    # key selection stacks the 2-D members in dict order (extract.py:516-522, 568)
    from . import _lib as L
    fd: Dict[str, object] = {k: host(v) for k, v in ex["indices"].items()}
    fd["pca_result"] = [host(p) for p in ex["pca"]]
    fd["variance_ratio"] = ex["pca_ratio"]
    fd["glcm_features"] = {k: host(v) for k, v in ex["glcm"].items()}
    nir2, q255 = ex["nir2"], ex["q255"]  # the re-normalised NIR band and its uint8 image (indices.py:412-415)
    lbp = ctx.lbp_uniform(q255, h, w, 24, 3).cpu().numpy().reshape(h, w).astype(np.float64)
    fd["lbp_feature"] = lbp / lbp.max()
    ms: Dict[str, np.ndarray] = {}
    for k in (1, 3, 5, 7):                # per scale: mean, variance, std_dev, entropy for scales <= 5 (indices.py:535-560)
        if k == 1:                        # cv2.blur with a 1 x 1 kernel is the identity: variance and std are exactly 0
            ms["mean_scale_1"] = host(nir2)
            ms["variance_scale_1"] = np.zeros((h, w), np.float32)
            ms["std_dev_scale_1"] = np.zeros((h, w), np.float32)
        else:
            ms[f"mean_scale_{k}"] = host(ctx.box_mean(nir2, h, w, k, L.BORDER_REFLECT101))
            ms[f"variance_scale_{k}"] = host(ctx.local_var(nir2, h, w, k))
            ms[f"std_dev_scale_{k}"] = host(planes[17]) if k == 5 else host(ctx.local_std(nir2, h, w, k))
        if k <= 5:
            e = ctx.rank_entropy(q255, h, w, k).cpu().numpy().reshape(h, w)
            ms[f"entropy_scale_{k}"] = e / np.max(e)
    fd["multi_scale_features"] = ms
    ops = (("erosion", L.MORPH_ERODE), ("dilation", L.MORPH_DILATE), ("opening", L.MORPH_OPEN), ("closing", L.MORPH_CLOSE),
           ("gradient", L.MORPH_GRADIENT))
    fd["morphological_features"] = {f"{name}_{k}": ctx.morph(q255, h, w, k, op).cpu().numpy().reshape(h, w) / 255.0
                                    for k in (3, 5, 7) for name, op in ops}
    g5 = ctx.gaussian_blur_u8(q255, h, w, 5).cpu().numpy().reshape(h, w) / 255.0
    g15 = ctx.gaussian_blur_u8(q255, h, w, 15).cpu().numpy().reshape(h, w) / 255.0
    dog = g5 - g15
    fd["filter_features"] = {"gaussian_5": g5, "gaussian_15": g15, "dog": (dog - dog.min()) / (dog.max() - dog.min() + 1e-10),
                             "laplacian": host(ctx.laplacian_norm(q255, h, w)), "sobel_mag": host(planes[18])}
    stack = P.stack19_to_host(planes, h, w)
    hier = {"level_1": np.ascontiguousarray(stack[:, :, :14]), "level_2": np.ascontiguousarray(stack[:, :, 14:]), "all": stack}
    return fd, hier


def save_feature_outputs(output_dir: str, features_dict: Dict, hierarchical_features: Dict, height: int, width: int,
                         transform=None, crs=None) -> Dict[str, str]:
    """File names and contents of scripts/2:193-258: the three .npy stacks, the pickle, and the full stack as
    all_hierarchical_features.tif (one band per feature, float64, georeferenced with `transform` / `crs`, LZW in
    256 x 256 tiles as the reference asks rasterio for; BigTIFF once the stack passes 4 GB).
    `crs`: an EPSG integer, 'EPSG:xxxx', or an object with to_epsg()."""
    os.makedirs(output_dir, exist_ok=True)
    paths = {"level1": os.path.join(output_dir, "level1_features.npy"),
             "level2": os.path.join(output_dir, "level2_features.npy"),
             "all": os.path.join(output_dir, "all_hierarchical_features.npy"),
             "pkl": os.path.join(output_dir, "all_features_and_metadata.pkl"),
             "tif": os.path.join(output_dir, "all_hierarchical_features.tif")}
    np.save(paths["level1"], hierarchical_features["level_1"])
    np.save(paths["level2"], hierarchical_features["level_2"])
    np.save(paths["all"], hierarchical_features["all"])
    with open(paths["pkl"], "wb") as f:
        pickle.dump({"hierarchical_features": hierarchical_features, "all_extracted_features_dict": features_dict,
                     "dimensions": (height, width), "geo_transform": transform, "crs": crs}, f)
    from .tiff import write_tiff
    write_tiff(paths["tif"], np.moveaxis(hierarchical_features["all"], -1, 0), transform=transform, epsg=_epsg_of(crs),
               geographic=_is_geographic(crs), compress="lzw", tiled=True)
    return paths


def _epsg_of(crs) -> Optional[int]:
    if crs is None:
        return None
    if hasattr(crs, "to_epsg"):
        return crs.to_epsg()
    if isinstance(crs, str) and crs.upper().startswith("EPSG:"):
        return int(crs.split(":")[1])
    return int(crs)


def _is_geographic(crs) -> Optional[bool]:
    g = getattr(crs, "is_geographic", None)   # rasterio.crs.CRS
    return bool(g) if g is not None else None


def save_class_map_tif(class_map: np.ndarray, out_tif: str, transform=None, crs=None) -> str:
    """Convenience form of modules.features.extract.save_classification_as_geotiff (reference extract.py:778-833) for callers
    that hold transform / crs instead of a feature dictionary."""
    from modules.features.extract import save_classification_as_geotiff
    a = np.asarray(class_map)
    save_classification_as_geotiff(a, {"transform": transform, "crs": crs, "height": a.shape[0], "width": a.shape[1]}, out_tif)
    return out_tif


def run_kmeans_stage(hierarchical_all: np.ndarray, n_clusters: int = 7, ctx: Optional[Context] = None, *, valid_mask=None) -> np.ndarray:
    """KMeans branch of run_classification_stage on the 19-feature stack: labels + 1 as uint8
    (scripts/3:390-394, 509-538: final_map = labels + 1, saved as uint8 with nodata 0).
    valid_mask ((H, W), non-zero = valid): the fit sees the valid pixels only and the class map is 0 at the others."""
    ctx = ctx or default_context()
    h, w, c = hierarchical_all.shape
    dt = np.float32 if hierarchical_all.dtype == np.float32 else np.float64
    dev = [ctx.to_device(np.ascontiguousarray(hierarchical_all[:, :, i], dtype=dt).reshape(-1)) for i in range(c)]
    if valid_mask is not None:
        from .masked import kmeans_fit_predict_masked
        labels, _ = kmeans_fit_predict_masked(dev, _check_valid_mask(valid_mask, (h, w)), n_clusters, ctx=ctx)
    else:
        labels, _ = ctx.kmeans_fit_predict(dev, n_clusters)
    return (labels.cpu().numpy().reshape(h, w) + 1).astype(np.uint8)


def _check_valid_mask(valid_mask, shape):
    if valid_mask is None:
        return None
    m = np.asarray(valid_mask)
    if m.shape != tuple(shape):
        raise ValueError(f"valid_mask: shape {m.shape}, the raster is {tuple(shape)}")
    return m


RF_MODEL_FILE = "random_forest_model.joblib"   # scripts/3_classification.py:459
GAUSS_METHODS = ("maximum_likelihood", "mahalanobis", "minimum_distance")   # rsseg.gaussian.STAGE_METHODS


@dataclass(frozen=True)
class ClassifyRequest:
    """What one run of the classification stage is asked for: the arguments of run_classification_stage and of its three
    siblings, with run_classification_stage's defaults.  A branch of _classify reads its own fields and ignores the others."""
    method: str = "rule_based"
    n_clusters: int = 7
    use_hierarchical_all: bool = True
    classifier: object = None
    feature_keys: Optional[Sequence[str]] = None
    labeled_roi_file: str = "labeled_roi.tif"
    strict_reference: bool = False
    valid_mask: object = None                  # (H, W), non-zero = valid: class 0 at the other pixels
    confidence: bool = False                   # forest: ClassifyProducts.proba and .confidence
    importance_mask: object = None             # forest: an (H, W) label mask -> .importance and .feature_names
    save_kmeans_model: Optional[str] = None    # kmeans: .kmeans_model, the model of the fit that made the labels, saved there
    ml_threshold: Optional[float] = None       # GAUSS_METHODS
    rule_image: bool = False                   # GAUSS_METHODS: .dist2 and .margin
    fit_on_device: bool = False                # GAUSS_METHODS


@dataclass
class ClassifyProducts:
    """What a branch of _classify made beside the class map; None: not made.  _run_classification writes what is there."""
    kmeans_model: object = None
    proba: Optional[np.ndarray] = None         # (H, W, C)
    confidence: Optional[np.ndarray] = None    # (H, W)
    gauss_model: object = None
    dist2: Optional[np.ndarray] = None
    margin: Optional[np.ndarray] = None
    importance: Optional[Dict[str, object]] = None
    feature_names: Optional[Sequence[str]] = None


def run_classification_stage(feature_file_path, method='rule_based', output_dir="segmentation_outputs", use_hierarchical_all=True, *,
                             n_clusters: int = 7, classifier=None, feature_keys=None, labeled_roi_file: str = "labeled_roi.tif",
                             strict_reference: bool = False, ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """run_classification_stage (scripts/3_classification.py:267-505): the reference's name, positional order and defaults
    (`method='rule_based'`, `output_dir="segmentation_outputs"`, `use_hierarchical_all=True`); what follows the `*` are
    keyword-only additions.  Loads and normalises the feature file (extract.py:32-295), dispatches on `method`:

      'rule_based'     thresholds + morphology + area filter (scripts/3:335-375).  The rules read 'ndvi', 'ndwi', 'mndwi',
                       'ndbi' (extract.py:406-505); stage 2's pickle stores them under 'all_extracted_features_dict_<index>'
                       after normalisation, and those are used when the plain keys are absent.
      'kmeans'         scripts/3:377-398: the keys ['ndvi', 'ndwi', 'ndbi', 'texture_mean', 'hierarchical_all'] that exist, 7
                       clusters (`n_clusters`), labels + 1.  On a stage-2 pickle none of them exists (the keys are prefixed,
                       SURVEY.md 3.2); the reference then announces "将使用自动选择" (automatic selection) but hands over the
                       EMPTY list, on which unsupervised_kmeans_classification raises (extract.py:533).  This driver does what
                       the message says: `feature_keys_to_use=None`, i.e. every 2-D plane of the dictionary (55 on a stage-2
                       pickle).  `feature_keys` overrides the selection; `strict_reference=True` hands over the empty list
                       as the reference does, i.e. raises its ValueError.
      'random_forest'  scripts/3:401-488, inference part: the feature array is 'hierarchical_all' (also under stage 2's key
                       'hierarchical_features_all') when `use_hierarchical_all`, else every 2-D plane of the image's shape
                       stacked (:425-437); the classifier is `classifier` when given, else <output_dir>/random_forest_model.joblib
                       when it exists and its n_features_in_ matches (:459-475); otherwise the forest is fitted from
                       `labeled_roi_file` (prepare_training_samples + train_random_forest_classifier, :450-475: K16 on the GPU,
                       the same trees scikit-learn grows) and cached as that joblib file.  Without a model and without the label raster the stage
                       reports that and returns None (the reference insists on the label raster even when the cache exists, :405-409).
      'maximum_likelihood', 'mahalanobis', 'minimum_distance'   (beyond the reference) rsseg.gaussian.GaussianClassifier, K22:
                       trained from `labeled_roi_file` on the feature array the forest branch takes, applied to every pixel
                       on the GPU; also writes <output_dir>/<method>_model.npz (GaussianClassifier.save).

    Writes <output_dir>/classification_<method>.npy and, when the feature file carries transform / crs / width / height
    (scripts/3:495-498), <output_dir>/<method>_classification_map.tif (uint8 labels, nodata 0, LZW tiles); the PNG of
    scripts/3:491 is plotting (out of scope).  The reference returns None; this returns the label map as well (None on the
    reference's error paths, which print and return).  run_forest_confidence_stage is the 'random_forest' branch with the
    class probabilities and the confidence map written beside the class map, run_masked_classification_stage the same
    dispatch on the valid pixels of a scene with nodata."""
    req = ClassifyRequest(method=method, n_clusters=n_clusters, use_hierarchical_all=use_hierarchical_all, classifier=classifier,
                          feature_keys=feature_keys, labeled_roi_file=labeled_roi_file, strict_reference=strict_reference)
    return _run_classification(feature_file_path, output_dir, req, ctx)


def run_masked_classification_stage(feature_file_path, method='rule_based', output_dir="segmentation_outputs", use_hierarchical_all=True, *,
                                    valid_mask=None, n_clusters: int = 7, classifier=None, feature_keys=None,
                                    labeled_roi_file: str = "labeled_roi.tif", strict_reference: bool = False, confidence: bool = False,
                                    ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """run_classification_stage with valid_mask ((H, W), non-zero = valid; rsseg.masked): the classifier sees the valid pixels
    only — KMeans is fitted on them alone, the forest walks its trees for them alone — and the class map is 0 at the others,
    which is what the GeoTIFF's nodata 0 says.  The rule-based map is painted 0 there.  Feature extraction came first and is
    not masked.  valid_mask=None is run_classification_stage itself.  confidence (method 'random_forest'): the files of
    run_forest_confidence_stage as well, with probability rows of 0 and confidence 0 at the masked pixels.  (A function of its
    own, like run_forest_confidence_stage: the signatures of run_classification_stage and run_forest_confidence_stage are the
    reference's plus a fixed set of keyword-only additions.)"""
    req = ClassifyRequest(method=method, n_clusters=n_clusters, use_hierarchical_all=use_hierarchical_all, classifier=classifier,
                          feature_keys=feature_keys, labeled_roi_file=labeled_roi_file, strict_reference=strict_reference,
                          valid_mask=valid_mask, confidence=bool(confidence))
    return _run_classification(feature_file_path, output_dir, req, ctx)


IMPORTANCE_FILE = "rf_permutation_importance.json"
IMPORTANCE_REPEATS, IMPORTANCE_SEED = 5, 42


def run_forest_importance_stage(feature_file_path, roi_mask, output_dir="segmentation_outputs", use_hierarchical_all=True, *,
                                classifier=None, labeled_roi_file: str = "labeled_roi.tif", confidence: bool = False,
                                ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """run_classification_stage(feature_file_path, 'random_forest', ...) (run_forest_confidence_stage with `confidence`) with
    the permutation importance of the forest's features over the labelled pixels of `roi_mask` ((H, W) integers, 0 = no
    label): every file of that call, unchanged, and beside them <output_dir>/rf_permutation_importance.json with
    feature_names, importances_mean, importances_std, importances (F x n_repeats), baseline_score, n_samples, n_repeats (5)
    and random_state (42) — rsseg.forest_importance.permutation_importance_image, equal to scikit-learn's
    permutation_importance.  The ranking is printed as train_random_forest_classifier prints its importances.  Returns the
    label map."""
    req = ClassifyRequest(method="random_forest", use_hierarchical_all=use_hierarchical_all, classifier=classifier,
                          labeled_roi_file=labeled_roi_file, confidence=confidence, importance_mask=np.asarray(roi_mask))
    return _run_classification(feature_file_path, output_dir, req, ctx)


def run_forest_confidence_stage(feature_file_path, output_dir="segmentation_outputs", use_hierarchical_all=True, *, classifier=None,
                                labeled_roi_file: str = "labeled_roi.tif", ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """run_classification_stage(feature_file_path, 'random_forest', ...) with confidence: every file of that call, unchanged,
    and beside them <output_dir>/rf_class_probabilities.npy, (H, W, C) float64 = the forest's predict_proba of every pixel in
    the order of classes_, <output_dir>/rf_confidence.npy, (H, W) float64 = the largest of them, and, with complete
    metadata, <output_dir>/random_forest_confidence_map.tif (float64, LZW tiles).  Returns the label map.  (A function of
    its own: the signature of run_classification_stage is the reference's plus a fixed set of keyword-only additions.)
    On a scene with nodata: run_masked_classification_stage(..., 'random_forest', valid_mask=..., confidence=True)."""
    req = ClassifyRequest(method="random_forest", use_hierarchical_all=use_hierarchical_all, classifier=classifier,
                          labeled_roi_file=labeled_roi_file, confidence=True)
    return _run_classification(feature_file_path, output_dir, req, ctx)


KMEANS_SUMMARY_FILE = "kmeans_model_summary.json"


def run_kmeans_model_stage(feature_file_path, model_path, output_dir="segmentation_outputs", *, feature_keys=None,
                           ctx: Optional[Context] = None, valid_mask=None) -> Optional[np.ndarray]:
    """The 'kmeans' branch of run_classification_stage with a SAVED model (rsseg.kmeans_model.KMeansModel.save) instead of a
    fit: the feature file is loaded and normalised the same way, the planes are selected as the fitted path selects them
    (`feature_keys` as there; the model refuses another number of planes or, when it stores names, other planes), and the
    model labels them, so that the cluster ids of this map are those of every other map of the model.  Writes
    <output_dir>/classification_kmeans.npy (labels + 1 as uint8, the fitted path's layout), kmeans_classification_map.tif with
    complete metadata, kmeans_distance.npy ((H, W), the distance of every pixel to its centre in the planes' dtype) and
    kmeans_model_summary.json (counts per cluster, inertia, the overflow flag, the model file's name).  Returns the class map.
    valid_mask ((H, W), non-zero = valid): only the valid pixels are labelled; the class map is 0 and the distance NaN at the
    others, counts and inertia cover the valid pixels, and the summary also carries n_valid."""
    from .kmeans_model import KMeansModel
    model = KMeansModel.load(model_path)
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        return None
    keys = _kmeans_keys(feats, feature_keys, False)
    planes, shape = model.select_planes(feats, keys)
    ctx = ctx or default_context()
    dev = [ctx.to_device(np.ascontiguousarray(p, dtype=model.dtype).reshape(-1)) for p in _planes_in(planes, model.dtype)]
    extra = {}
    if valid_mask is not None:
        from .masked import kmeans_predict_masked
        labels, dist, summary, n_valid = kmeans_predict_masked(ctx, dev, _check_valid_mask(valid_mask, shape),
                                                               model.cluster_centers_.astype(np.float64), model.scale_.astype(np.float64),
                                                               model.min_.astype(np.float64), want_distance=True, want_summary=True)
        extra = {"n_valid": n_valid}
    else:
        labels, dist, summary = ctx.kmeans_predict(dev, model.cluster_centers_.astype(np.float64), model.scale_.astype(np.float64),
                                                   model.min_.astype(np.float64), want_distance=True, want_summary=True)
    out = (labels.cpu().numpy().reshape(shape) + 1).astype(np.uint8)
    np.save(os.path.join(output_dir, "classification_kmeans.npy"), out)
    _save_class_tif(out, feats, output_dir, "kmeans")
    np.save(os.path.join(output_dir, "kmeans_distance.npy"), dist.cpu().numpy().reshape(shape))
    inertia = summary["inertia"]
    _write_json(os.path.join(output_dir, KMEANS_SUMMARY_FILE),
                {"model": os.path.basename(str(model_path)), "n_clusters": model.n_clusters, "n_features": model.n_features_in_,
                 "counts": summary["counts"].tolist(), "inertia": inertia if np.isfinite(inertia) else None,
                 "overflow": bool(summary["overflow"]), **extra})
    return out


def _planes_in(planes, dt):
    """The selected planes must already be of the model's dtype class (float32 iff every plane is float32, as the fit stacks them)."""
    got = np.result_type(*[np.asarray(p).dtype for p in planes])
    got = np.dtype(np.float32) if got == np.float32 else np.dtype(np.float64)
    if got != np.dtype(dt):
        raise ValueError(f"KMeansModel: the selected planes stack to {got.name}, the model was fitted in {np.dtype(dt).name}")
    return planes


def _kmeans_keys(feats, feature_keys, strict_reference):
    """The key selection of the 'kmeans' branch (scripts/3:377-391; see run_classification_stage)."""
    wanted = ["ndvi", "ndwi", "ndbi", "texture_mean", "hierarchical_all"] if feature_keys is None else list(feature_keys)
    valid = [k for k in wanted if isinstance(feats.get(k), np.ndarray) and feats[k].ndim in (2, 3)]
    if not valid:
        print(f"警告: 为KMeans指定的特征键 {wanted} 在数据中均不可用，将使用自动选择。")
    return valid if (valid or strict_reference) else None      # the reference passes [] and raises (scripts/3:391, extract.py:533)


def _save_class_tif(out, feats, output_dir, method):
    from modules.features.extract import save_classification_as_geotiff
    if all(feats.get(k) is not None for k in ("transform", "crs", "width", "height")):   # scripts/3:495-498
        save_classification_as_geotiff(out, feats, os.path.join(output_dir, f"{method}_classification_map.tif"))
    else:
        print("警告: 元数据不完整，无法将分类结果保存为带地理参考的GeoTIFF。")


def _load_normalised(feature_file_path, output_dir):
    """The feature file as scripts/3:295-311 loads and checks it -> the normalised dictionary, or None after the reference's message."""
    from modules.features.extract import load_features, normalize_features_structure
    os.makedirs(output_dir, exist_ok=True)
    try:
        raw = load_features(feature_file_path)
        if not raw:
            print("加载原始特征失败。")
            return None
        feats = normalize_features_structure(raw)
        skip = ("transform", "crs", "width", "height", "dimensions", "geo_transform", "hierarchical_level_1", "hierarchical_level_2",
                "hierarchical_all")
        has_arrays = any(isinstance(v, np.ndarray) and v.ndim >= 2 for k, v in feats.items() if k not in skip)
        has_all = isinstance(feats.get("hierarchical_all"), np.ndarray) and feats["hierarchical_all"].ndim == 3
        has_dims = isinstance(feats.get("height"), int) and isinstance(feats.get("width"), int)
        if not (has_arrays or has_all) or not has_dims:
            print("错误：规范化后的特征不包含有效的图像数组数据（单个特征或hierarchical_all）或尺寸信息。")
            print(f"规范化后的键: {list(feats.keys())}")
            return None
    except Exception as e:  # noqa: BLE001 — scripts/3:307-311 prints and returns
        print(f"加载或规范化特征失败: {e}")
        return None
    return feats


def _run_classification(feature_file_path, output_dir, req: ClassifyRequest, ctx: Optional[Context]) -> Optional[np.ndarray]:
    """The classification stage behind run_classification_stage and its siblings: load, _classify, write the map and its products."""
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        return None
    if req.valid_mask is not None:
        req = replace(req, valid_mask=_check_valid_mask(req.valid_mask, (feats["height"], feats["width"])))
    from . import runtime as _rt
    prev_ctx = _rt._default_ctx
    if ctx is not None:   # the mirrors run on the process-wide context: lend them this one for the duration of the call
        _rt._default_ctx = ctx
    try:
        out, made = _classify(feats, output_dir, req)
    finally:
        _rt._default_ctx = prev_ctx
    if out is None:
        return None
    method = req.method
    np.save(os.path.join(output_dir, f"classification_{method}.npy"), out)
    _save_class_tif(out, feats, output_dir, method)
    if made.kmeans_model is not None:
        print(f"KMeans模型保存至: {made.kmeans_model.save(req.save_kmeans_model)}")
    if made.proba is not None:
        np.save(os.path.join(output_dir, "rf_class_probabilities.npy"), made.proba)
        np.save(os.path.join(output_dir, "rf_confidence.npy"), made.confidence)
        if all(feats.get(k) is not None for k in ("transform", "crs", "width", "height")):
            from .tiff import write_tiff
            write_tiff(os.path.join(output_dir, f"{method}_confidence_map.tif"), made.confidence, transform=feats["transform"],
                       epsg=_epsg_of(feats["crs"]), geographic=_is_geographic(feats["crs"]), compress="lzw", tiled=True)
    if made.gauss_model is not None:
        print(f"{method} 模型保存至: {made.gauss_model.save(os.path.join(output_dir, f'{method}_model.npz'))}")
    if made.dist2 is not None:
        np.save(os.path.join(output_dir, f"{method}_dist2.npy"), made.dist2)
        np.save(os.path.join(output_dir, f"{method}_margin.npy"), made.margin)
    if made.importance is not None:
        _save_importance(os.path.join(output_dir, IMPORTANCE_FILE), made.importance, made.feature_names)
    return out


def _save_importance(path: str, imp, names) -> None:
    _write_json(path, {"feature_names": list(names), "importances_mean": imp["importances_mean"].tolist(),
                       "importances_std": imp["importances_std"].tolist(), "importances": imp["importances"].tolist(),
                       "baseline_score": imp["baseline_score"], "n_samples": imp["n_samples"], "n_repeats": IMPORTANCE_REPEATS,
                       "random_state": IMPORTANCE_SEED})
    mean = imp["importances_mean"]
    print(f"随机森林置换特征重要性 ({imp['n_samples']} 个标注像素, 基准准确率 {imp['baseline_score']:.4f}):")
    for i in np.argsort(mean)[::-1]:
        print(f"    特征 '{names[i]}': {mean[i]:.4f}")


def _classify(feats, output_dir, req: ClassifyRequest) -> Tuple[Optional[np.ndarray], ClassifyProducts]:
    """The dispatch of scripts/3_classification.py:335-488 on a normalised feature dictionary -> (label map or None, what the
    branch made beside it).  req.valid_mask is None or an (H, W) array already checked against the features' shape."""
    branch = _BRANCHES.get(req.method)
    if branch is None:
        print(f"错误: 不支持的分割方法 '{req.method}'")
        return None, ClassifyProducts()
    return branch(feats, output_dir, req)


def _classify_rules(feats, output_dir, req):
    from modules.features.extract import rule_based_classification
    rules = {}
    for k in ("ndvi", "ndwi", "mndwi", "ndbi"):
        v = feats.get(k)
        if v is None:
            v = feats.get(f"all_extracted_features_dict_{k}")
        if v is not None:
            rules[k] = v
    rules["height"], rules["width"] = feats["height"], feats["width"]
    out = rule_based_classification(rules)
    if req.valid_mask is not None and out is not None:
        out = np.where(req.valid_mask != 0, out, 0).astype(out.dtype)
    return out, ClassifyProducts()


def _classify_kmeans(feats, output_dir, req):
    from modules.features.extract import unsupervised_kmeans_classification
    keys = _kmeans_keys(feats, req.feature_keys, req.strict_reference)
    if req.save_kmeans_model:   # the same call on the same planes, its model kept
        from .kmeans_model import KMeansModel
        model, labels = KMeansModel.fit_features(feats, req.n_clusters, keys, mask=req.valid_mask)
        return (labels + 1).astype(np.uint8), ClassifyProducts(kmeans_model=model)
    if req.valid_mask is not None:   # labels -1 at the masked pixels: class 0
        from modules.features.extract import _select_planes
        from .masked import kmeans_fit_predict_masked
        planes, _ = _select_planes(feats, keys)
        labels, _ = kmeans_fit_predict_masked([np.asarray(p) for p in planes], req.valid_mask, int(req.n_clusters))
        return (labels.reshape(feats["height"], feats["width"]) + 1).astype(np.uint8), ClassifyProducts()
    return (unsupervised_kmeans_classification(feats, req.n_clusters, keys) + 1).astype(np.uint8), ClassifyProducts()   # scripts/3:394


def _classify_gaussian(feats, output_dir, req):
    from modules.features.extract import prepare_training_samples
    shape = (feats["height"], feats["width"])
    roi_file = req.labeled_roi_file
    arr, names = _supervised_feature_array(feats, req.use_hierarchical_all, shape)
    if arr is None:
        return None, ClassifyProducts()
    if not os.path.exists(roi_file):
        print(f"错误: 监督分类所需的标签ROI文件 '{roi_file}' 未找到。")
        return None, ClassifyProducts()
    from .gaussian import STAGE_METHODS, GaussianClassifier
    if req.fit_on_device:   # the classes' moments from the raster on the GPU (K24): no host sample matrix
        from .tiff import read_tiff
        roi = read_tiff(roi_file)[0]
        if roi.shape != shape:
            raise ValueError(f"标签ROI文件 '{roi_file}' (形状 {roi.shape}) 尺寸与特征数据 (期望的2D形状 {shape}) 不匹配。")
        clf = GaussianClassifier(STAGE_METHODS[req.method], threshold=req.ml_threshold).fit_image(arr, roi, device=True)
    else:
        X, y = prepare_training_samples(arr, roi_file)
        clf = GaussianClassifier(STAGE_METHODS[req.method], threshold=req.ml_threshold).fit(X, y)
    rule = bool(req.rule_image)
    res = clf.predict_image(arr, mask=req.valid_mask, want_dist2=rule, want_margin=rule)
    if rule:
        return res[0], ClassifyProducts(gauss_model=clf, dist2=res[1], margin=res[2])
    return res, ClassifyProducts(gauss_model=clf)


def _classify_forest(feats, output_dir, req):
    from modules.features.extract import prepare_training_samples, supervised_classification_predict, train_random_forest_classifier
    classifier, roi_file, valid_mask, made = req.classifier, req.labeled_roi_file, req.valid_mask, ClassifyProducts()
    arr, names = _supervised_feature_array(feats, req.use_hierarchical_all, (feats["height"], feats["width"]))
    if arr is None:
        return None, made
    model_path = os.path.join(output_dir, RF_MODEL_FILE)
    try:
        import joblib
        if classifier is None and os.path.exists(model_path):
            print(f"加载已训练的随机森林模型: {model_path}")
            classifier = joblib.load(model_path)
        nf = getattr(classifier, "n_features_in_", None)
        if classifier is not None and nf is not None and nf != arr.shape[-1]:
            print(f"警告: 加载的分类器需要 {nf} 个特征，但准备的数据有 {arr.shape[-1]} 个。正在重新训练模型。")
            classifier = None
        if classifier is None:      # scripts/3:450-475: fit on the host from the label raster, cache the model
            if not os.path.exists(roi_file):
                print(f"错误: 监督分类所需的标签ROI文件 '{roi_file}' 未找到 (也没有可用的模型 '{model_path}')。")
                return None, made
            X, y = prepare_training_samples(arr, roi_file)
            classifier = train_random_forest_classifier(X, y, feature_names_for_training=names)
            joblib.dump(classifier, model_path)
            print(f"随机森林模型训练并保存至: {model_path}")
        if valid_mask is not None:
            from .masked import forest_predict_masked
            out = forest_predict_masked(classifier, arr, valid_mask, 0)
        else:
            out = supervised_classification_predict(arr, classifier)
        if req.confidence:   # the same pixels as the label map saw: NaN -> 0 (extract.py:690-719)
            from .forest import image_proba_and_confidence
            if valid_mask is not None:
                made.proba, made.confidence = image_proba_and_confidence(classifier, arr, mask=valid_mask)
            else:
                made.proba, made.confidence = image_proba_and_confidence(classifier, np.nan_to_num(arr, nan=0.0))
        if req.importance_mask is not None:
            from .forest_importance import permutation_importance_image
            made.importance = permutation_importance_image(classifier, arr, req.importance_mask,
                                                           n_repeats=IMPORTANCE_REPEATS, random_state=IMPORTANCE_SEED)
            made.feature_names = names
        return out, made
    except RssegUnsupported:
        raise
    except Exception as e:  # noqa: BLE001 — scripts/3:482-486 prints and returns
        print(f"随机森林分类过程中发生错误: {e}")
        return None, ClassifyProducts()


_BRANCHES = {"rule_based": _classify_rules, "kmeans": _classify_kmeans, **dict.fromkeys(GAUSS_METHODS, _classify_gaussian),
             **dict.fromkeys(("random_forest", "rf", "supervised"), _classify_forest)}


def _supervised_feature_array(feats, use_hierarchical_all, shape):
    """The feature array of the supervised branches (scripts/3:413-437) -> ((H, W, F) array, feature names), or (None, []) after
    the reference's message."""
    arr, names = None, []
    if use_hierarchical_all:
        for key in ("hierarchical_all", "hierarchical_features_all"):
            v = feats.get(key)
            if isinstance(v, np.ndarray) and v.ndim == 3 and v.shape[:2] == shape:
                arr = v
                names = [f"hierarchical_feature_{i + 1}" for i in range(v.shape[-1])]
                break
    if arr is None:   # scripts/3:425-437: every 2-D plane of the image's shape, in dict order
        names = [k for k, v in feats.items() if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape == shape]
        if not names:
            print("错误: 为随机森林指定的特征键在数据中均不可用或不是匹配图像形状的2D数组。")
            return None, []
        arr = np.stack([feats[k] for k in names], axis=-1)
    return arr, names


def _supervised_stack(feature_file_path, output_dir, who):
    """The feature file's (H, W, F) stack as the supervised classifiers read it -> ((H, W), stack, feature names); a file without one
    is refused in the name of the stage `who`.  output_dir exists afterwards (_load_normalised makes it)."""
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        raise ValueError(f"{who}: {feature_file_path} holds no feature stack")
    shape = (int(feats["height"]), int(feats["width"]))
    arr, names = _supervised_feature_array(feats, True, shape)
    if arr is None:
        raise ValueError(f"{who}: {feature_file_path} holds no plane of shape {shape}")
    return shape, arr, names


def _write_class_tif(path, class_map, transform, crs) -> None:
    """A class map beside the raw one: uint8, nodata 0, LZW tiles; georeferenced when transform and crs are given."""
    from .tiff import write_tiff
    write_tiff(path, class_map, transform=transform, epsg=_epsg_of(crs), geographic=_is_geographic(crs), nodata=0, compress="lzw", tiled=True)


def _write_json(path, obj) -> None:
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)


# --------------------------------------------------------------------------------------------------
# one-command driver shaped like the two scripts' __main__ blocks (scripts/2_feature_extraction.py:137-262,
# scripts/3_classification.py:545-632):   python -m rsseg.stages <image.tif> <output_dir> [--classify kmeans]
# --------------------------------------------------------------------------------------------------
def run_scripts_2_3(image_path: str, output_dir: str, classify: Optional[str] = None, preprocessing: bool = True, n_clusters: int = 7,
                    ctx: Optional[Context] = None, evaluate: Optional[str] = None, raw: bool = False,
                    confidence: bool = False, importance: Optional[str] = None) -> Dict[str, object]:
    """Reads the GeoTIFF's bands as float32 with nodata -> NaN (scripts/2:154-161), runs the feature stage, writes
    <output_dir>/feature_outputs/{level1,level2,all_hierarchical}_features.npy, all_features_and_metadata.pkl and
    all_hierarchical_features.tif (scripts/2:193-258), then — `classify` in {'kmeans', 'rule_based', 'random_forest'} —
    the classification stage on that pickle into <output_dir>/segmentation_results (scripts/3:548-551), and — `evaluate` naming a
    ROI mask (.npy / .tif) — the accuracy assessment of that class map (scripts/4) into <output_dir>/evaluation_results.
    raw: the image is a raw DN raster: stage 1 (scripts/1) runs first on the device and writes the reference's product,
    <output_dir>/preprocessed/<stem>_preprocessed.tif, and its uint8 planes go to the feature stage without leaving HBM.
    confidence: with classify='random_forest', the class probabilities and the confidence map beside the class map
    (run_forest_confidence_stage).
    importance: with classify='random_forest', a ROI mask (.npy / .tif, read as `evaluate` reads its mask): the permutation
    importance of the forest's features over its labelled pixels, written as segmentation_results/rf_permutation_importance.json
    (run_forest_importance_stage)."""
    opts = RunOptions(classify=classify, preprocessing=preprocessing, n_clusters=n_clusters, evaluate=evaluate, raw=raw, confidence=confidence,
                      importance=importance)
    return _run_scripts_2_3(image_path, output_dir, opts, ctx)


MASK_NODATA_FROM_TAG = "tag"   # --mask-nodata without a value


def resolve_mask_nodata(option, tag) -> Optional[float]:
    """The nodata value --mask-nodata masks by: `option` is None (not asked for: None comes back), MASK_NODATA_FROM_TAG (the
    file's GDAL_NODATA tag `tag`; SystemExit with a message when the file has none) or the value given on the command line."""
    if option is None:
        return None
    if option != MASK_NODATA_FROM_TAG:
        return float(option)
    if tag is None:
        raise SystemExit("--mask-nodata: the image carries no GDAL_NODATA tag; name the value: --mask-nodata VALUE")
    return float(tag)


def nodata_valid_mask(ctx: Context, arr: np.ndarray, nodata: float) -> Tuple[np.ndarray, int]:
    """'Every band holds data' on the device (Context.valid_mask): pixel (y, x) of the (bands, H, W) raster is valid iff no band
    equals `nodata` there (8-bit bands compared as bytes, every other dtype as the float32 the feature stage reads) or holds a
    NaN.  Returns ((H, W) uint8 of 0 / 1, valid count)."""
    dt = np.uint8 if arr.dtype == np.uint8 else np.float32
    dev = [ctx.to_device(np.ascontiguousarray(arr[i], dtype=dt).reshape(-1)) for i in range(arr.shape[0])]
    mask, n_valid = ctx.valid_mask(dev, nan=True, nodata=nodata)
    return mask.cpu().numpy().reshape(arr.shape[1:]), n_valid


POSTCLASS_STATS_FILE = "postclass_stats.json"


def run_postclass_stage(class_map, output_dir: str, method: str, min_area: int = 0, window: int = 0, majority_iterations: int = 1, *,
                        nodata: int = 0, transform=None, crs=None, ctx: Optional[Context] = None) -> Tuple[np.ndarray, Dict[str, object]]:
    """Clean-up of a finished class map (rsseg.postclass.clean_class_map; no counterpart in the reference): components of fewer
    than min_area pixels are removed and grown over from their surroundings, then — window != 0 — majority_iterations passes of
    a window x window majority filter run.  window = 0: no majority pass, the holes are filled with a 3 x 3 window.
    Writes, beside the raw map's files that stay as they are: <output_dir>/classification_<method>_clean.npy,
    <method>_classification_map_clean.tif (uint8, nodata 0, LZW tiles; georeferenced when transform and crs are given) and
    postclass_stats.json (the parameters, clean_class_map's statistics, pixels per class before and after).
    Returns (clean map, that dictionary)."""
    from . import postclass as PC
    raw = PC.check_class_map(class_map)
    if _is_device_tensor(raw):
        raw = raw.cpu().numpy()
    clean, st = PC.clean_class_map(raw, min_area=min_area, window=window or 3, nodata=nodata, majority_iterations=majority_iterations if window else 0,
                                   ctx=ctx, return_stats=True)
    os.makedirs(output_dir, exist_ok=True)
    np.save(os.path.join(output_dir, f"classification_{method}_clean.npy"), clean)
    _write_class_tif(os.path.join(output_dir, f"{method}_classification_map_clean.tif"), clean, transform, crs)
    stats: Dict[str, object] = {"method": method, "min_area": int(min_area), "window": int(window or 3),
                                "majority_iterations": int(majority_iterations if window else 0), "nodata": int(nodata), **st,
                                "class_counts_before": {str(k): v for k, v in PC.class_counts(raw).items()},
                                "class_counts_after": {str(k): v for k, v in PC.class_counts(clean).items()}}
    _write_json(os.path.join(output_dir, POSTCLASS_STATS_FILE), stats)
    return clean, stats


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


SEGMENT_STATS_FILE = "segment_stats.json"
SIGNATURES_OF_MAP = "class-map"   # --signatures without a value: the classes of the raw class map just produced


def run_signatures_stage(feature_file_path, label_map, output_dir: str, method: str, *, valid_mask=None, ignore: int = 0,
                         ctx: Optional[Context] = None):
    """Class signatures of a label raster over the feature stack (rsseg.signatures, K24; no counterpart in the reference): the
    count, mean vector and covariance matrix of every class of `label_map` (an (H, W) uint8 class map, or an ROI raster of
    training classes; `ignore`, default 0, labels nothing), taken in one pass on the GPU, and their pairwise separability.
    The planes are the (H, W, F) stack of the feature file the supervised classifiers read (hierarchical_all, else every 2-D
    plane), as float32.  valid_mask: pixels outside it are not counted.
    Writes <output_dir>/signatures_<method>.npz (ClassMoments.save: the integer table, so that signature files of several
    scenes merge) and separability_<method>.json (separability_report: Jeffries-Matusita and transformed divergence, the least
    separable pair, per class the count, mean and standard deviation; a class whose covariance is singular is named under
    "error" in place of the matrices).  Returns (ClassMoments, that dictionary)."""
    from . import signatures as SIG
    shape, arr, names = _supervised_stack(feature_file_path, output_dir, "run_signatures_stage")
    lab = label_map.cpu().numpy() if _is_device_tensor(label_map) else np.asarray(label_map)
    if lab.shape != shape:
        raise ValueError(f"run_signatures_stage: the label raster is {lab.shape}, the features are {shape}")
    if lab.dtype != np.uint8:
        l64 = np.nan_to_num(lab.astype(np.float64), nan=0.0)
        if np.any(l64 != np.floor(l64)) or np.any(l64 < 0) or np.any(l64 > 255):
            raise ValueError("run_signatures_stage: the labels must be integers in 0..255")
        lab = l64.astype(np.uint8)
    valid_mask = _check_valid_mask(valid_mask, shape)
    mom = SIG.class_moments(np.asarray(arr, np.float32) if arr.dtype != np.uint8 else arr, lab, ignore=ignore, mask=valid_mask, ctx=ctx)
    mom.save(os.path.join(output_dir, f"signatures_{method}.npz"))
    try:
        report = SIG.separability_report(mom)
    except ValueError as e:   # a singular class: the per-class figures still stand
        report = SIG.separability_report(mom, kinds=())
        report["error"] = str(e)
    report = {"method": method, "feature_names": list(names), **report}
    _write_json(os.path.join(output_dir, f"separability_{method}.json"), report)
    return mom, report


def run_segment_stage(feature_file_path, class_map, output_dir: str, method: str, step: int, compactness: float = 10.0, iterations: int = 10,
                      object_based: bool = False, *, valid_mask=None, nodata: int = 0, transform=None, crs=None,
                      ctx: Optional[Context] = None) -> Tuple[np.ndarray, Dict[str, object], Optional[np.ndarray]]:
    """Superpixels of the feature stack (rsseg.segment.slic; no counterpart in the reference) and, with object_based, the class
    map voted per superpixel.  The planes are the (H, W, F) stack of the feature file the supervised classifiers read
    (hierarchical_all, else every 2-D plane); a stack of more than 16 planes is segmented on its first 16 (segment_stats.json
    names how many).  valid_mask: pixels outside it belong to no segment and stay `nodata` in the object map.
    Writes, beside the raw map's files that stay as they are: <output_dir>/segments.npy (int32, 0 = masked), segment_stats.json
    (the parameters, n_segments, n_iter, n_regrown, the smallest / median / largest area) and, with object_based,
    classification_<method>_objects.npy and <method>_classification_map_objects.tif (uint8, nodata 0, LZW tiles).
    Returns (segments, that dictionary, object map or None)."""
    from . import segment as SG
    _, arr, names = _supervised_stack(feature_file_path, output_dir, "run_segment_stage")
    used = min(arr.shape[-1], SG.MAX_PLANES)
    if used < arr.shape[-1]:
        print(f"segments: the feature stack has {arr.shape[-1]} planes, the first {used} are segmented ({', '.join(names[:used])})")
    planes = [np.ascontiguousarray(arr[..., i]) for i in range(used)]
    segments, st = SG.slic(planes, step=step, compactness=compactness, max_iter=iterations, mask=valid_mask, ctx=ctx, return_stats=True)
    area = np.bincount(segments.reshape(-1), minlength=st["n_segments"] + 1)[1:]
    stats: Dict[str, object] = {"method": method, **st, "planes_in_stack": int(arr.shape[-1]), "planes_used": int(used),
                                "masked_pixels": int((segments == 0).sum()),
                                "area_min": int(area.min()) if area.size else 0, "area_median": float(np.median(area)) if area.size else 0.0,
                                "area_max": int(area.max()) if area.size else 0, "object_based": bool(object_based)}
    np.save(os.path.join(output_dir, "segments.npy"), segments)
    objects = None
    if object_based:
        objects = SG.object_classify(segments, class_map, nodata=nodata, ctx=ctx)
        np.save(os.path.join(output_dir, f"classification_{method}_objects.npy"), objects)
        _write_class_tif(os.path.join(output_dir, f"{method}_classification_map_objects.tif"), objects, transform, crs)
        stats["pixels_changed_by_objects"] = int((objects != np.asarray(class_map)).sum())
    _write_json(os.path.join(output_dir, SEGMENT_STATS_FILE), stats)
    return segments, stats, objects


OBJECT_FEATURES_FILE = "object_features.npz"


def run_object_features_stage(feature_file_path, segments, output_dir: str, method: str, *, labeled_roi_file: str = "labeled_roi.tif",
                              valid_mask=None, transform=None, crs=None, ctx: Optional[Context] = None):
    """Object-based supervised classification from object features (rsseg.objects.classify_objects, K25; no counterpart in the
    reference): every segment of `segments` (run_segment_stage's map) is described by the mean and the standard deviation of
    the planes run_segment_stage segments (the first 16 of the feature file's (H, W, F) stack, as float32), the segments that
    hold pixels of the ROI raster train `method` ('random_forest', 'maximum_likelihood', 'mahalanobis' or 'minimum_distance'),
    every segment is labelled and painted back.  valid_mask: pixels outside it are not counted and stay 0.
    Writes, beside the raw map's files that stay as they are: <output_dir>/object_features.npz (table, X, columns),
    classification_<method>_object_features.npy, <method>_classification_map_object_features.tif (uint8, nodata 0, LZW tiles)
    and an "object_features" entry in segment_stats.json (n_train, classes, columns).
    Returns (object map, rsseg.objects.ObjectClassification, that entry)."""
    from . import objects as OB
    from . import segment as SG
    from .tiff import read_tiff
    if method not in OB.FOREST_METHODS and method not in OB.GAUSS_METHODS:
        raise ValueError(f"run_object_features_stage: method {method!r} is not a supervised classifier")
    shape, arr, names = _supervised_stack(feature_file_path, output_dir, "run_object_features_stage")
    if tuple(np.asarray(segments).shape) != shape:
        raise ValueError(f"run_object_features_stage: the segment map is {tuple(np.asarray(segments).shape)}, the features are {shape}")
    if not os.path.exists(labeled_roi_file):
        raise FileNotFoundError(f"标签ROI文件未找到: {labeled_roi_file}")
    roi = read_tiff(labeled_roi_file)
    roi = roi[0] if roi.ndim == 3 else roi
    if roi.shape != shape:
        raise ValueError(f"标签ROI文件 '{labeled_roi_file}' (形状 {roi.shape}) 尺寸与特征数据 (期望的2D形状 {shape}) 不匹配。")
    valid_mask = _check_valid_mask(valid_mask, shape)
    used = min(arr.shape[-1], SG.MAX_PLANES)
    planes = [np.ascontiguousarray(arr[..., i]) if arr.dtype == np.uint8 else np.ascontiguousarray(arr[..., i], dtype=np.float32) for i in range(used)]
    of = OB.object_features(segments, planes, names=names[:used], stats=("mean", "std"), shape=False, mask=valid_mask, ctx=ctx)
    res = OB.classify_objects(segments, planes, roi, method=method, mask=valid_mask, features=of, ctx=ctx)
    class_map = res.class_map
    if valid_mask is not None:   # a segment map made under another mask: its pixels outside this one stay 0 all the same
        class_map = np.where(np.asarray(valid_mask) != 0, class_map, 0).astype(np.uint8)
    np.savez(os.path.join(output_dir, OBJECT_FEATURES_FILE), table=of.table, X=of.X, columns=np.array(of.columns))
    np.save(os.path.join(output_dir, f"classification_{method}_object_features.npy"), class_map)
    _write_class_tif(os.path.join(output_dir, f"{method}_classification_map_object_features.tif"), class_map, transform, crs)
    entry: Dict[str, object] = {"method": method, "n_train": int(res.train_idx.size), "classes": [int(c) for c in np.unique(res.train_y)],
                                "columns": list(res.columns), "planes_used": int(used)}
    spath = os.path.join(output_dir, SEGMENT_STATS_FILE)
    stats = {}
    if os.path.exists(spath):
        with open(spath) as f:
            stats = json.load(f)
    stats["object_features"] = entry
    _write_json(spath, stats)
    return class_map, res, entry


REGION_GRAPH_FILE = "region_graph.npz"
REGION_STATS_FILE = "regions_stats.json"


def run_region_merge_stage(feature_file_path, segments, output_dir: str, *, threshold=None, scales=None, criterion: str = "ward", min_area: int = 0,
                           n_regions: Optional[int] = None, class_map=None, method: Optional[str] = None, valid_mask=None, transform=None,
                           crs=None, ctx: Optional[Context] = None):
    """Region merging of a segment map (rsseg.regions.merge_regions, K27; no counterpart in the reference) on the planes
    run_segment_stage segmented: the first 16 of the feature file's (H, W, F) stack.  valid_mask: pixels outside it belong to no
    region and stay 0.
    Writes, beside the earlier files that stay as they are: <output_dir>/regions.npy (int32, 0 = masked), or regions_<i>.npy per
    scale (i = 0 ...); region_graph.npz (the graph of the final regions, RegionGraph.save); regions_stats.json (the parameters,
    segments_in, regions_out and the smallest / median / largest area per map, rounds, merges); and, with class_map and method,
    classification_<method>_regions.npy and <method>_classification_map_regions.tif: the class map voted per region of the
    (last) map (rsseg.segment.object_classify; uint8, nodata 0, LZW tiles).
    Returns (rsseg.regions.RegionMerge, that dictionary, region class map or None)."""
    from . import regions as RG
    from . import segment as SG
    if (class_map is None) != (method is None):
        raise ValueError("run_region_merge_stage: class_map and method go together")
    shape, arr, names = _supervised_stack(feature_file_path, output_dir, "run_region_merge_stage")
    segments = np.asarray(segments)
    if tuple(segments.shape) != shape:
        raise ValueError(f"run_region_merge_stage: the segment map is {tuple(segments.shape)}, the features are {shape}")
    valid_mask = _check_valid_mask(valid_mask, shape)
    used = min(arr.shape[-1], SG.MAX_PLANES)
    planes = [np.ascontiguousarray(arr[..., i]) for i in range(used)]
    res = RG.merge_regions(segments, planes, threshold=threshold, scales=scales, criterion=criterion, min_area=min_area, n_regions=n_regions,
                           mask=valid_mask, ctx=ctx)

    def areas(labels):
        area = np.bincount(labels.reshape(-1))[1:]
        return {"regions_out": int(area.size), "area_min": int(area.min()) if area.size else 0,
                "area_median": float(np.median(area)) if area.size else 0.0, "area_max": int(area.max()) if area.size else 0}

    maps = res.scale_labels if scales is not None else [res.labels]
    for i, labels in enumerate(maps):
        np.save(os.path.join(output_dir, f"regions_{i}.npy" if scales is not None else "regions.npy"), labels.astype(np.int32))
    res.graph.save(os.path.join(output_dir, REGION_GRAPH_FILE))
    stats: Dict[str, object] = {"criterion": criterion, "threshold": None if threshold is None else float(threshold),
                                "scales": None if scales is None else [float(t) for t in scales], "n_regions": n_regions, "min_area": int(min_area),
                                "planes_in_stack": int(arr.shape[-1]), "planes_used": int(used), "segments_in": int((res.parent > 0).sum()),
                                "regions_out": int(res.n_regions), "rounds": int(res.history["round"].max()) if res.history.size else 0,
                                "merges": int(res.history.size), "maps": [areas(m) for m in maps]}
    regions_cm = None
    if class_map is not None:
        regions_cm = SG.object_classify(res.labels, class_map, nodata=0, ctx=ctx)
        np.save(os.path.join(output_dir, f"classification_{method}_regions.npy"), regions_cm)
        _write_class_tif(os.path.join(output_dir, f"{method}_classification_map_regions.tif"), regions_cm, transform, crs)
        stats["method"] = method
        stats["pixels_changed_by_regions"] = int((regions_cm != np.asarray(class_map)).sum())
    _write_json(os.path.join(output_dir, REGION_STATS_FILE), stats)
    return res, stats, regions_cm


SVM_MODEL_FILE = "svm_model.npz"


def run_svm_stage(feature_file_path, output_dir, *, labeled_roi_file="labeled_roi.tif", kernel="rbf", C=1.0, gamma="scale", degree=3, coef0=0.0,
                  model_path=None, rule_image=False, valid_mask=None, ctx: Optional[Context] = None):
    """Support vector machine classification (rsseg.svm.SVMClassifier, K28; no counterpart in the reference) of the (H, W, F)
    feature stack the forest branch takes: trained on the pixels labeled_roi_file labels (0 = unlabelled; class labels 1..255),
    or, with model_path, a saved model applied as it is.  valid_mask: pixels outside it stay class 0.
    Writes, beside the earlier files that stay as they are: <output_dir>/classification_svm.npy (uint8), svm_classification_map.tif
    (when the metadata is complete), svm_model.npz and, with rule_image, svm_margin.npy (float32: the smallest |decision| among
    the winner's pairs, NaN where nothing was classified).  Returns the class map."""
    from .svm import SVMClassifier
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        raise ValueError(f"run_svm_stage: {feature_file_path} holds no feature stack")
    shape = (int(feats["height"]), int(feats["width"]))
    arr, _ = _supervised_feature_array(feats, True, shape)
    if arr is None:
        raise ValueError(f"run_svm_stage: {feature_file_path} holds no plane of shape {shape}")
    valid_mask = _check_valid_mask(valid_mask, shape)
    if model_path is not None:
        clf = SVMClassifier.load(model_path)
    else:
        from .tiff import read_tiff
        if not os.path.exists(labeled_roi_file):
            raise FileNotFoundError(f"run_svm_stage: the label raster '{labeled_roi_file}' was not found")
        roi = read_tiff(labeled_roi_file)
        roi = roi[0] if roi.ndim == 3 else roi
        if roi.shape != shape:
            raise ValueError(f"run_svm_stage: the label raster is {roi.shape}, the features are {shape}")
        clf = SVMClassifier(kernel=kernel, C=C, gamma=gamma, degree=degree, coef0=coef0).fit_image(arr, roi)
    if clf.classes_.min() < 1 or clf.classes_.max() > 255:
        raise ValueError("run_svm_stage: class labels must be integers in 1..255 (0 is 'unclassified' in the class map)")
    res = clf.predict_image(arr, mask=valid_mask, want_margin=bool(rule_image), ctx=ctx)
    out = (res[0] if rule_image else res).astype(np.uint8)
    np.save(os.path.join(output_dir, "classification_svm.npy"), out)
    _save_class_tif(out, feats, output_dir, "svm")
    print(f"svm 模型保存至: {clf.save(os.path.join(output_dir, SVM_MODEL_FILE))}")
    if rule_image:
        np.save(os.path.join(output_dir, "svm_margin.npy"), res[1])
    return out


MLP_MODEL_FILE = "mlp_model.npz"


def run_mlp_stage(feature_file_path, output_dir, *, labeled_roi_file="labeled_roi.tif", hidden_layer_sizes=(100,), activation="relu", alpha=1e-4,
                  max_iter=500, random_state=42, model_path=None, rule_image=False, valid_mask=None, ctx: Optional[Context] = None):
    """Neural-network classification (rsseg.mlp.NeuralNetClassifier, K30; no counterpart in the reference) of the (H, W, F)
    feature stack the forest branch takes: trained on the pixels labeled_roi_file labels (0 = unlabelled; class labels 1..255),
    or, with model_path, a saved model applied as it is.  valid_mask: pixels outside it stay class 0.
    Writes, beside the earlier files that stay as they are: <output_dir>/classification_mlp.npy (uint8), mlp_classification_map.tif
    (when the metadata is complete), mlp_model.npz and, with rule_image, mlp_margin.npy (float32: the winner's logit minus the
    runner-up's) and mlp_confidence.npy (float32: the winner's probability), both NaN where nothing was classified.  Returns the
    class map."""
    from .mlp import NeuralNetClassifier
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        raise ValueError(f"run_mlp_stage: {feature_file_path} holds no feature stack")
    shape = (int(feats["height"]), int(feats["width"]))
    arr, _ = _supervised_feature_array(feats, True, shape)
    if arr is None:
        raise ValueError(f"run_mlp_stage: {feature_file_path} holds no plane of shape {shape}")
    valid_mask = _check_valid_mask(valid_mask, shape)
    if model_path is not None:
        clf = NeuralNetClassifier.load(model_path)
    else:
        from .tiff import read_tiff
        if not os.path.exists(labeled_roi_file):
            raise FileNotFoundError(f"run_mlp_stage: the label raster '{labeled_roi_file}' was not found")
        roi = read_tiff(labeled_roi_file)
        roi = roi[0] if roi.ndim == 3 else roi
        if roi.shape != shape:
            raise ValueError(f"run_mlp_stage: the label raster is {roi.shape}, the features are {shape}")
        clf = NeuralNetClassifier(hidden_layer_sizes=hidden_layer_sizes, activation=activation, alpha=alpha, max_iter=max_iter,
                                  random_state=random_state).fit_image(arr, roi)
    if clf.classes_.min() < 1 or clf.classes_.max() > 255:
        raise ValueError("run_mlp_stage: class labels must be integers in 1..255 (0 is 'unclassified' in the class map)")
    res = clf.predict_image(arr, mask=valid_mask, want_margin=bool(rule_image), want_conf=bool(rule_image), ctx=ctx)
    out = (res[0] if rule_image else res).astype(np.uint8)
    np.save(os.path.join(output_dir, "classification_mlp.npy"), out)
    _save_class_tif(out, feats, output_dir, "mlp")
    print(f"mlp 模型保存至: {clf.save(os.path.join(output_dir, MLP_MODEL_FILE))}")
    if rule_image:
        np.save(os.path.join(output_dir, "mlp_margin.npy"), res[1])
        np.save(os.path.join(output_dir, "mlp_confidence.npy"), res[2])
    return out


ISODATA_HISTORY_FILE = "isodata_history.json"
ISODATA_DEFAULTS = dict(init_clusters=None, max_std=0.06, min_dist=0.1, min_size=None, iterations=20, change=0.0)


def isodata_planes(feats, feature_keys=None):
    """The planes run_isodata_stage clusters -> (list of (H, W) planes, all uint8 or all float32, their names): the (H, W, F)
    stack the Gaussian methods, SLIC and the signatures read (hierarchical_all, else every 2-D plane), or, with feature_keys,
    those entries of the feature dictionary (2-D planes, 3-D stacks plane by plane)."""
    shape = (int(feats["height"]), int(feats["width"]))
    if feature_keys is None:
        arr, names = _supervised_feature_array(feats, True, shape)
        if arr is None:
            return None, []
        planes = [arr[..., i] for i in range(arr.shape[-1])]
    else:
        planes, names = [], []
        for k in feature_keys:
            v = feats.get(k)
            if not isinstance(v, np.ndarray) or v.ndim not in (2, 3) or v.shape[:2] != shape:
                raise ValueError(f"run_isodata_stage: feature {k!r} is not a plane or a stack of shape {shape}")
            if v.ndim == 2:
                planes.append(v)
                names.append(str(k))
            else:
                planes += [v[..., i] for i in range(v.shape[-1])]
                names += [f"{k}_{i + 1}" for i in range(v.shape[-1])]
    dt = np.uint8 if all(p.dtype == np.uint8 for p in planes) else np.float32
    return [np.ascontiguousarray(p, dtype=dt) for p in planes], names


def run_isodata_stage(feature_file_path, output_dir="segmentation_outputs", *, n_clusters: int = 7, init_clusters: Optional[int] = None,
                      max_std: float = 0.06, min_dist: float = 0.1, min_size: Optional[int] = None, iterations: int = 20,
                      change: float = 0.0, model_path: Optional[str] = None, feature_keys=None, valid_mask=None,
                      ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """ISODATA clustering of the feature stack (rsseg.isodata, K26; no counterpart in the reference): n_clusters is the number
    aimed at (k_target), the other parameters are rsseg.isodata.isodata's.  model_path: a saved model (IsodataModel.save) is
    applied and nothing is fitted, so that the cluster ids of this map are those of every other map of the model.
    valid_mask ((H, W), non-zero = valid): only the valid pixels are clustered; the class map is 0 at the others.
    Writes <output_dir>/classification_isodata.npy (labels + 1 as uint8, 0 = nodata, the k-means layout),
    isodata_classification_map.tif with complete metadata, isodata_model.npz and isodata_history.json (the parameters, the
    per-iteration history, the pixels per cluster, n_left_out).  Returns the class map."""
    from . import isodata as ISO
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        return None
    shape = (int(feats["height"]), int(feats["width"]))
    planes, names = isodata_planes(feats, feature_keys)
    if planes is None:
        return None
    valid_mask = _check_valid_mask(valid_mask, shape)
    if model_path:
        model = ISO.IsodataModel.load(model_path)
        if model.feature_names is not None and model.feature_names != list(names):
            raise ValueError(f"IsodataModel: the model was fitted on {model.feature_names}, the feature file offers {list(names)}")
        labels = model.predict(planes, mask=valid_mask, ctx=ctx)
        counts = np.bincount(labels.reshape(-1), minlength=256)[:model.n_clusters]
        record = {"model": os.path.basename(str(model_path)), "fitted": False, "history": [], "n_left_out": int((labels == ISO.NO_LABEL).sum())
                  - (0 if valid_mask is None else int((np.asarray(valid_mask) == 0).sum()))}
    else:
        res = ISO.isodata(planes, k_target=n_clusters, k_init=init_clusters, min_size=min_size, max_std=max_std, min_dist=min_dist,
                          max_iter=iterations, change=change, mask=valid_mask, feature_names=names, ctx=ctx)
        model, labels, counts = res.model, res.labels, res.counts
        record = {"fitted": True, "history": res.history, "n_left_out": int(res.n_left_out)}
    out = np.where(labels == ISO.NO_LABEL, 0, labels.astype(np.int32) + 1).astype(np.uint8).reshape(shape)
    np.save(os.path.join(output_dir, "classification_isodata.npy"), out)
    _save_class_tif(out, feats, output_dir, "isodata")
    model.save(os.path.join(output_dir, "isodata_model.npz"))
    _write_json(os.path.join(output_dir, ISODATA_HISTORY_FILE),
                {"k_target": int(n_clusters), "init_clusters": init_clusters, "max_std": max_std, "min_dist": min_dist, "min_size": min_size,
                 "iterations": int(iterations), "change": change, "n_clusters": int(model.n_clusters), "feature_names": list(names),
                 "counts": [int(c) for c in counts], **record})
    return out


GMM_HISTORY_FILE = "gmm_history.json"
GMM_DEFAULTS = dict(covariance="full", iterations=100, tol=1e-3, reg_covar=1e-6, posterior=False, model_path=None)


def run_gmm_stage(feature_file_path, output_dir="segmentation_outputs", *, n_clusters: int = 7, covariance: str = "full", iterations: int = 100,
                  tol: float = 1e-3, reg_covar: float = 1e-6, posterior: bool = False, model_path: Optional[str] = None, feature_keys=None,
                  valid_mask=None, random_state: int = 42, ctx: Optional[Context] = None) -> Optional[np.ndarray]:
    """Gaussian mixture clustering of the feature stack (rsseg.gmm, K29; no counterpart in the reference) over the planes
    run_isodata_stage clusters (isodata_planes): n_clusters components of the given covariance type, started from a k-means
    label map.  model_path: a saved model (GaussianMixtureModel.save) is applied and nothing is fitted.
    valid_mask ((H, W), non-zero = valid): only the valid pixels are clustered; the class map is 0 at the others.
    Writes <output_dir>/classification_gmm.npy (component + 1 as uint8, 0 = nodata, the k-means layout),
    gmm_classification_map.tif with complete metadata, gmm_model.npz and gmm_history.json; with posterior also gmm_posterior.npy
    (the label's posterior probability) and gmm_loglik.npy (the log-density), float32, NaN at nodata.  Returns the class map."""
    from . import gmm as GMM
    feats = _load_normalised(feature_file_path, output_dir)
    if feats is None:
        return None
    shape = (int(feats["height"]), int(feats["width"]))
    planes, names = isodata_planes(feats, feature_keys)
    if planes is None:
        return None
    valid_mask = _check_valid_mask(valid_mask, shape)
    if model_path:
        model = GMM.GaussianMixtureModel.load(model_path)
        n_clusters = model.n_components   # the model's own count: --n-clusters plays no part
        record = {"model": os.path.basename(str(model_path)), "fitted": False, "history": []}
    else:
        model = GMM.GaussianMixtureModel(n_components=n_clusters, covariance_type=covariance, tol=tol, reg_covar=reg_covar, max_iter=iterations,
                                         init="kmeans", random_state=random_state)
        res = model.fit(planes, mask=valid_mask, ctx=ctx)
        record = {"fitted": True, "history": res.history, "converged": bool(model.converged_), "n_iter": int(model.n_iter_),
                  "lower_bound": float(model.lower_bound_)}
    labels, post, loglik = model.predict_with_posterior(planes, mask=valid_mask, ctx=ctx)
    out = np.ascontiguousarray(labels, dtype=np.uint8).reshape(shape)
    n_valid = out.size if valid_mask is None else int((np.asarray(valid_mask) != 0).sum())
    np.save(os.path.join(output_dir, "classification_gmm.npy"), out)
    _save_class_tif(out, feats, output_dir, "gmm")
    model.save(os.path.join(output_dir, "gmm_model.npz"))
    if posterior:
        np.save(os.path.join(output_dir, "gmm_posterior.npy"), np.asarray(post, np.float32).reshape(shape))
        np.save(os.path.join(output_dir, "gmm_loglik.npy"), np.asarray(loglik, np.float32).reshape(shape))
    _write_json(os.path.join(output_dir, GMM_HISTORY_FILE),
                {"n_clusters": int(n_clusters), "covariance": model.covariance_type, "iterations": int(iterations), "tol": tol,
                 "reg_covar": reg_covar, "n_components": int(model.n_components), "feature_names": list(names),
                 "weights": [float(w) for w in model.weights_], "counts": [int(c) for c in np.bincount(out.reshape(-1), minlength=256)[1:model.n_components + 1]],
                 "n_left_out": n_valid - int((out != 0).sum()), **record})
    return out


@dataclass(frozen=True)
class RunOptions:
    """What one run of the driver is asked for beside the image, the output directory and the context: run_scripts_2_3's arguments
    (described there) and the further options of the command line, with the defaults of a call that names none of them.
    gcps (with raw; beyond the reference): stage 1 rectifies the DN planes first (rsseg.georect, K21) and the feature stage goes
    on from the warped planes with the new shape and georeferencing.  With mask_nodata the warp's validity mask is AND-ed into
    the nodata mask of the warped DN planes (a bare --mask-nodata on a file without a GDAL_NODATA tag masks by the warp alone);
    without it the collar outside the source is classified as data, as it would be after a cv2.warpAffine.
    segment, signatures and object_features run under the same valid mask as the classifier; the object-based map and the
    object-features map are evaluated into <output_dir>/evaluation_results_objects and evaluation_results_object_features."""
    classify: Optional[str] = None
    preprocessing: bool = True
    n_clusters: int = 7
    evaluate: Optional[str] = None
    raw: bool = False
    confidence: bool = False
    importance: Optional[str] = None
    kmeans_model: Optional[str] = None   # classify='kmeans': apply this saved model and fit nothing (run_kmeans_model_stage)
    save_kmeans_model: Optional[str] = None   # classify='kmeans': fit as always and also write the model there (KMeansModel.save; the same class map)
    # None, MASK_NODATA_FROM_TAG or a value (resolve_mask_nodata): the classifier sees only the pixels where every band holds data;
    # the mask is also written as <output_dir>/feature_outputs/valid_mask.npy and the class map is 0 elsewhere
    mask_nodata: object = None
    sieve: int = 0
    majority: int = 0
    majority_iterations: int = 1
    gcps: Optional[str] = None
    warp_order: int = 1
    resampling: str = "nearest"
    pixel_size: Optional[float] = None
    ml_threshold: Optional[float] = None   # classify in GAUSS_METHODS: the chi-square quantile beyond which a pixel stays unclassified
    rule_image: bool = False   # classify in GAUSS_METHODS: the rule images <method>_dist2.npy / <method>_margin.npy beside the class map
    segment: int = 0   # a grid step: run_segment_stage on the feature file, with the three options that follow
    compactness: float = 10.0
    segment_iterations: int = 10
    object_based: bool = False
    signatures: Optional[str] = None   # SIGNATURES_OF_MAP or an ROI raster's path: run_signatures_stage on the raw class map, or on the ROI's training classes
    fit_on_device: bool = False   # classify in GAUSS_METHODS: the model is fitted from moments taken on the GPU (fit_image(..., device=True))
    object_features: bool = False   # with segment and a supervised classify: run_object_features_stage on the segments, with ./labeled_roi.tif
    # classify='isodata': run_isodata_stage's keyword arguments beside n_clusters (init_clusters, max_std, min_dist, min_size, iterations,
    # change, model_path); the valid mask goes to the sweep as it is
    isodata: Optional[Dict[str, object]] = None


@dataclass(frozen=True)
class GmmRunOptions(RunOptions):
    """RunOptions of a --classify gmm run: run_gmm_stage's keyword arguments beside n_clusters (covariance, iterations, tol,
    reg_covar, posterior, model_path).  Every other run keeps the plain RunOptions."""
    gmm: Optional[Dict[str, object]] = None


def request_from_options(o: RunOptions, method: str, valid_mask, load_roi) -> ClassifyRequest:
    """The request of the driver's classification step: every option goes to the method it belongs to and to no other.  The
    --importance ROI is read here, by load_roi (ClassificationEvaluator._load) and so before the classification starts, for
    'random_forest' without a valid mask only: a masked run ignores `importance` (the command line refuses the combination)."""
    forest, gauss = method == "random_forest", method in GAUSS_METHODS
    importance_mask = np.asarray(load_roi(o.importance)) if forest and o.importance and valid_mask is None else None
    return ClassifyRequest(method=method, n_clusters=o.n_clusters, valid_mask=valid_mask, confidence=forest and bool(o.confidence),
                           importance_mask=importance_mask, save_kmeans_model=o.save_kmeans_model if method == "kmeans" else None,
                           ml_threshold=o.ml_threshold if gauss else None, rule_image=gauss and bool(o.rule_image),
                           fit_on_device=gauss and bool(o.fit_on_device))


def _evaluate_into(ev, class_map, roi_path, out_dir):   # -> (metrics, cluster mapping)
    return ev.evaluate_maps(class_map, ev.load_roi_mask(roi_path), out_dir)


def _run_scripts_2_3(image_path, output_dir, o: RunOptions, ctx: Optional[Context]) -> Dict[str, object]:
    """run_scripts_2_3 with every option of the command line (RunOptions)."""
    valid_mask = None
    if o.raw:
        from .preprocess import run_preprocessing_stage
        pdir = os.path.join(output_dir, "preprocessed")
        stem = os.path.splitext(os.path.basename(image_path))[0]
        ppath = os.path.join(pdir, f"{stem}_preprocessed.tif")
        if o.gcps is None:
            ppath, dev, (h, w), geo = run_preprocessing_stage(image_path, ppath, pdir, ctx=ctx, return_device=True)
        else:
            nodata = None
            if o.mask_nodata is not None:
                from .tiff import read_tiff_georef
                tag = read_tiff_georef(image_path)["nodata"]
                nodata = None if o.mask_nodata == MASK_NODATA_FROM_TAG and tag is None else resolve_mask_nodata(o.mask_nodata, tag)
            ppath, dev, (h, w), geo, wmask = run_preprocessing_stage(image_path, ppath, pdir, ctx=ctx, return_device=True, gcps=o.gcps,
                                                                     warp_order=o.warp_order, resampling=o.resampling, pixel_size=o.pixel_size,
                                                                     nodata=nodata)
            if o.mask_nodata is not None:
                valid_mask = wmask.cpu().numpy().reshape(h, w)
                print(f"valid pixels: {int(valid_mask.sum())} of {valid_mask.size} (warp mask"
                      + ("" if nodata is None else f" and nodata {nodata:g}") + ")")
        fd, hier = _feature_extraction_on_device(ctx or default_context(), dev, h, w, o.preprocessing)
    else:
        from .tiff import read_tiff, read_tiff_georef
        arr = read_tiff(image_path)
        geo = read_tiff_georef(image_path)
        nodata = resolve_mask_nodata(o.mask_nodata, geo["nodata"])
        if nodata is not None:
            valid_mask, n_valid = nodata_valid_mask(ctx or default_context(), arr, nodata)
            print(f"valid pixels: {n_valid} of {valid_mask.size} (nodata {nodata:g})")
        bands = []
        for i in range(arr.shape[0]):
            b = arr[i] if arr.dtype == np.uint8 and geo["nodata"] is None else arr[i].astype(np.float32)
            # with a valid mask the mask carries the nodata meaning and the bands keep their values: a NaN in a band makes
            # robust_normalize's percentiles NaN and PCA refuses the stack (scikit-learn's "Input X contains NaN"), so a scene
            # with nodata pixels never reached the classifier
            if geo["nodata"] is not None and valid_mask is None:
                b[b == geo["nodata"]] = np.nan
            bands.append(b)
        h, w = arr.shape[1:]
        fd, hier = run_feature_extraction_stage(bands, preprocessing=o.preprocessing, ctx=ctx)
    crs = None if geo["epsg"] is None else f"EPSG:{geo['epsg']}"
    fdir = os.path.join(output_dir, "feature_outputs")
    paths = save_feature_outputs(fdir, fd, hier, h, w, geo["transform"], crs)
    res: Dict[str, object] = {"paths": paths, "shape": (h, w)}
    if o.raw:
        res["preprocessed"] = ppath
    if valid_mask is not None:
        res["valid_mask_path"] = os.path.join(fdir, "valid_mask.npy")
        np.save(res["valid_mask_path"], valid_mask)
    if not o.classify:
        return res
    from .evaluate import ClassificationEvaluator
    classify, evaluate = o.classify, o.evaluate
    sdir = os.path.join(output_dir, "segmentation_results")
    if classify == "isodata":
        cm = run_isodata_stage(paths["pkl"], sdir, n_clusters=o.n_clusters, valid_mask=valid_mask, ctx=ctx, **(o.isodata or {}))
    elif classify == "gmm":
        cm = run_gmm_stage(paths["pkl"], sdir, n_clusters=o.n_clusters, valid_mask=valid_mask, ctx=ctx, **(getattr(o, "gmm", None) or {}))
    elif classify == "kmeans" and o.kmeans_model:
        cm = run_kmeans_model_stage(paths["pkl"], o.kmeans_model, sdir, ctx=ctx, valid_mask=valid_mask)
    else:
        cm = _run_classification(paths["pkl"], sdir, request_from_options(o, classify, valid_mask, ClassificationEvaluator._load), ctx)
    res["class_map"], res["segmentation_dir"] = cm, sdir
    if cm is None:   # the classifier printed why it made no map: nothing follows
        return res
    georef = dict(transform=geo["transform"], crs=crs, ctx=ctx)
    if evaluate:
        ev = ClassificationEvaluator(ctx)
        res["evaluation_dir"] = edir = os.path.join(output_dir, "evaluation_results")
        res["metrics"], res["cluster_mapping"] = _evaluate_into(ev, cm, evaluate, edir)
    if o.sieve or o.majority:
        # sieve / majority: the cleaned map beside the raw one (whose files and evaluation stay byte for byte what they are)
        res["class_map_clean"], res["postclass_stats"] = run_postclass_stage(cm, sdir, classify, o.sieve, o.majority, o.majority_iterations, **georef)
        if evaluate:
            res["evaluation_dir_clean"] = cdir = os.path.join(output_dir, "evaluation_results_clean")
            res["metrics_clean"], _ = _evaluate_into(ev, res["class_map_clean"], evaluate, cdir)
    if o.signatures:
        sig_labels = cm if o.signatures == SIGNATURES_OF_MAP else ClassificationEvaluator._load(o.signatures)
        res["signatures"], res["separability"] = run_signatures_stage(paths["pkl"], sig_labels, sdir, classify, valid_mask=valid_mask, ctx=ctx)
    if o.segment:
        # superpixels, and the class map voted per superpixel, beside the raw map (whose files stay byte for byte what they are)
        res["segments"], res["segment_stats"], res["class_map_objects"] = run_segment_stage(
            paths["pkl"], cm, sdir, classify, o.segment, o.compactness, o.segment_iterations, o.object_based, valid_mask=valid_mask, **georef)
        if evaluate and o.object_based:
            res["evaluation_dir_objects"] = odir = os.path.join(output_dir, "evaluation_results_objects")
            res["metrics_objects"], _ = _evaluate_into(ev, res["class_map_objects"], evaluate, odir)
        if o.object_features:
            res["class_map_object_features"], res["object_classification"], res["object_features_stats"] = run_object_features_stage(
                paths["pkl"], res["segments"], sdir, classify, labeled_roi_file="labeled_roi.tif", valid_mask=valid_mask, **georef)
            if evaluate:
                res["evaluation_dir_object_features"] = fdir_ = os.path.join(output_dir, "evaluation_results_object_features")
                res["metrics_object_features"], _ = _evaluate_into(ev, res["class_map_object_features"], evaluate, fdir_)
    return res


def parse_args(ap, argv=None):
    a = ap.parse_args(argv)
    if a.evaluate and not a.classify:
        ap.error("--evaluate needs --classify")
    if a.confidence and a.classify != "random_forest":
        ap.error("--confidence needs --classify random_forest")
    if a.importance and a.classify != "random_forest":
        ap.error("--importance needs --classify random_forest")
    if (a.kmeans_model or a.save_kmeans_model) and a.classify != "kmeans":
        ap.error("--kmeans-model / --save-kmeans-model need --classify kmeans")
    if a.kmeans_model and a.save_kmeans_model:
        ap.error("--kmeans-model applies a saved model and fits nothing: it does not go with --save-kmeans-model")
    iso_given = [f"--isodata-{k.replace('_', '-')}" for k in ISODATA_DEFAULTS if getattr(a, f"isodata_{k}") is not None] + (
        ["--isodata-model"] if a.isodata_model else [])
    if iso_given and a.classify != "isodata":
        ap.error(f"{' / '.join(iso_given)} need --classify isodata")
    if a.classify == "isodata":
        if not 1 <= a.n_clusters <= 64:
            ap.error("--classify isodata takes --n-clusters in 1..64")
        if a.isodata_init_clusters is not None and not 1 <= a.isodata_init_clusters <= 64:
            ap.error("--isodata-init-clusters takes a count in 1..64")
        if a.isodata_min_size is not None and a.isodata_min_size < 1:
            ap.error("--isodata-min-size takes a positive pixel count")
        if a.isodata_iterations is not None and a.isodata_iterations < 1:
            ap.error("--isodata-iterations takes a positive count")
        for k in ("max_std", "min_dist", "change"):
            v = getattr(a, f"isodata_{k}")
            if v is not None and not (v >= 0.0 and v < float("inf")):
                ap.error(f"--isodata-{k.replace('_', '-')} takes a finite non-negative number")
    if a.classify == "gmm" and not 1 <= a.n_clusters <= 32:
        ap.error("--classify gmm takes --n-clusters in 1..32")
    if (a.ml_threshold is not None or a.rule_image) and a.classify not in GAUSS_METHODS:
        ap.error("--ml-threshold / --rule-image need --classify maximum_likelihood, mahalanobis or minimum_distance")
    if a.ml_threshold is not None and not (0.0 < a.ml_threshold < 1.0):
        ap.error("--ml-threshold takes a probability in (0, 1)")
    if (a.signatures is not None or a.fit_on_device) and not a.classify:
        ap.error("--signatures / --fit-on-device need --classify")
    if a.fit_on_device and a.classify not in GAUSS_METHODS:
        ap.error("--fit-on-device needs --classify maximum_likelihood, mahalanobis or minimum_distance")
    if a.mask_nodata is not None and not a.classify:
        ap.error("--mask-nodata needs --classify")
    if a.gcps and not a.raw:
        ap.error("--gcps needs --raw: the ground control points rectify the raw DN raster in stage 1")
    if a.mask_nodata is not None and ((a.raw and not a.gcps) or a.importance):
        ap.error("--mask-nodata does not go with --raw or --importance")
    if (a.sieve or a.majority) and not a.classify:
        ap.error("--sieve / --majority need --classify")
    if a.sieve < 0:
        ap.error("--sieve takes a non-negative pixel count")
    if a.majority and a.majority not in (3, 5, 7, 9, 11, 13, 15):
        ap.error("--majority takes an odd window in 3..15")
    if a.majority_iterations < 0:
        ap.error("--majority-iterations takes a non-negative count")
    if a.segment and not a.classify:
        ap.error("--segment needs --classify")
    if a.segment and not 2 <= a.segment <= 4096:
        ap.error("--segment takes a grid step in 2..4096")
    if (a.object_based or a.compactness is not None or a.segment_iterations is not None) and not a.segment:
        ap.error("--compactness / --segment-iterations / --object-based need --segment")
    if a.object_features and not (a.segment and a.classify in ("random_forest", *GAUSS_METHODS)):
        ap.error("--object-features needs --segment and --classify random_forest, maximum_likelihood, mahalanobis or minimum_distance")
    if a.compactness is not None and not (a.compactness >= 0.0 and a.compactness < float("inf")):
        ap.error("--compactness takes a finite non-negative number")
    if a.segment_iterations is not None and a.segment_iterations < 0:
        ap.error("--segment-iterations takes a non-negative count")
    return a


def build_parser():
    import argparse
    # the options of --classify gmm have a parser of their own (build_gmm_parser); its help is printed below this parser's
    gmm_help = build_gmm_parser().format_help()
    ap = argparse.ArgumentParser(prog="python -m rsseg.stages", formatter_class=argparse.RawDescriptionHelpFormatter,
                                 description="feature extraction (scripts/2) and optionally classification (scripts/3) of one GeoTIFF on the GPU",
                                 epilog="options of --classify gmm:\n" + gmm_help[gmm_help.index("\n  --gmm-covariance") + 1:])
    ap.add_argument("image")
    ap.add_argument("output_dir")
    ap.add_argument("--classify", choices=["kmeans", "isodata", "gmm", "rule_based", "random_forest", *GAUSS_METHODS])
    ap.add_argument("--n-clusters", type=int, default=7)
    ap.add_argument("--no-preprocessing", action="store_true")
    ap.add_argument("--evaluate", metavar="ROI_MASK", help="accuracy assessment (scripts/4) of the class map against this ROI mask (.npy / .tif)")
    ap.add_argument("--raw", action="store_true",
                    help="the image is a raw DN raster: run stage 1 (scripts/1) on the GPU first, writing OUTPUT_DIR/preprocessed/<stem>_preprocessed.tif")
    ap.add_argument("--confidence", action="store_true",
                    help="with --classify random_forest: also write rf_class_probabilities.npy (H, W, C), rf_confidence.npy and a confidence GeoTIFF")
    ap.add_argument("--importance", metavar="ROI_MASK",
                    help="with --classify random_forest: permutation importance of the features over this ROI mask's labelled pixels "
                         "(.npy / .tif) -> rf_permutation_importance.json")
    ap.add_argument("--save-kmeans-model", metavar="PATH",
                    help="with --classify kmeans: fit as always and also write the fitted model (an .npz, rsseg.kmeans_model.KMeansModel)")
    ap.add_argument("--kmeans-model", metavar="PATH",
                    help="with --classify kmeans: apply this saved model instead of fitting -> the class map with the model's cluster ids, "
                         "kmeans_distance.npy and kmeans_model_summary.json")
    ap.add_argument("--ml-threshold", type=float, default=None, metavar="P",
                    help="with --classify maximum_likelihood / mahalanobis / minimum_distance: a pixel farther from its class than the "
                         "chi-square quantile P (0 < P < 1, F degrees of freedom) stays unclassified (0)")
    ap.add_argument("--rule-image", action="store_true",
                    help="with --classify maximum_likelihood / mahalanobis / minimum_distance: also write <method>_dist2.npy (squared distance "
                         "to the winning class) and <method>_margin.npy (runner-up minus winner)")
    ap.add_argument("--fit-on-device", action="store_true",
                    help="with --classify maximum_likelihood / mahalanobis / minimum_distance: fit the model from class moments taken "
                         "from the ROI raster on the GPU (rsseg.signatures) instead of a host sample matrix")
    ap.add_argument("--signatures", nargs="?", const=SIGNATURES_OF_MAP, default=None, metavar="ROI_MASK",
                    help="with --classify: also write signatures_<method>.npz (per-class count, mean and covariance as an exact integer "
                         "table) and separability_<method>.json (Jeffries-Matusita, transformed divergence) of the classes of the raw "
                         "class map, or, with ROI_MASK (.npy / .tif), of that raster's training classes")
    def nodata_value(s):   # argparse hands a string `const` to `type` as well
        return s if s == MASK_NODATA_FROM_TAG else float(s)
    nodata_value.__name__ = "float"   # the word argparse's "invalid ... value" message uses
    ap.add_argument("--mask-nodata", nargs="?", type=nodata_value, const=MASK_NODATA_FROM_TAG, default=None, metavar="VALUE",
                    help="with --classify: classify only the pixels where every band holds data (differs from VALUE; without VALUE, "
                         "from the file's GDAL_NODATA tag); the class map is 0 elsewhere and the mask is written as "
                         "feature_outputs/valid_mask.npy")
    ap.add_argument("--sieve", type=int, default=0, metavar="MIN_AREA",
                    help="with --classify: also write a cleaned class map (classification_<method>_clean.npy, "
                         "<method>_classification_map_clean.tif, postclass_stats.json): same-class components of fewer than MIN_AREA "
                         "pixels are removed and grown over from their surroundings (rsseg.postclass)")
    ap.add_argument("--majority", type=int, default=0, metavar="K",
                    help="with --classify: K x K majority filter (K odd, 3..15) of the (sieved) class map, written as the cleaned map")
    ap.add_argument("--majority-iterations", type=int, default=1, metavar="N", help="with --majority: up to N passes (stopped once one changes nothing)")
    ap.add_argument("--segment", type=int, default=0, metavar="STEP",
                    help="with --classify: also cut the feature stack into SLIC superpixels on a grid of STEP pixels (rsseg.segment) -> "
                         "segments.npy (int32, 0 = masked) and segment_stats.json")
    ap.add_argument("--compactness", type=float, default=None, metavar="M",
                    help="with --segment: weight of the pixel distance beside the 8-bit feature distance (default 10)")
    ap.add_argument("--segment-iterations", type=int, default=None, metavar="N", help="with --segment: at most N assignment iterations (default 10)")
    ap.add_argument("--object-based", action="store_true",
                    help="with --segment: also write the class map voted per superpixel (classification_<method>_objects.npy, "
                         "<method>_classification_map_objects.tif)")
    ap.add_argument("--object-features", action="store_true",
                    help="with --segment and a supervised --classify: also describe every superpixel by the mean and spread of its "
                         "planes, train the classifier on the superpixels under ./labeled_roi.tif and label every superpixel "
                         "(rsseg.objects) -> object_features.npz, classification_<method>_object_features.npy, "
                         "<method>_classification_map_object_features.tif")
    ap.add_argument("--isodata-init-clusters", type=int, default=None, metavar="K",
                    help="with --classify isodata (--n-clusters is the number aimed at): the initial number of clusters (default --n-clusters)")
    ap.add_argument("--isodata-max-std", type=float, default=None, metavar="S",
                    help="with --classify isodata: a cluster wider than S along a plane, in units of the plane's range, may be split (default 0.06)")
    ap.add_argument("--isodata-min-dist", type=float, default=None, metavar="D",
                    help="with --classify isodata: two clusters closer than D, in units of a plane's range, may be merged (default 0.1)")
    ap.add_argument("--isodata-min-size", type=int, default=None, metavar="N",
                    help="with --classify isodata: a cluster of fewer than N pixels is dropped (default: a thousandth of the valid pixels)")
    ap.add_argument("--isodata-iterations", type=int, default=None, metavar="N", help="with --classify isodata: at most N iterations (default 20)")
    ap.add_argument("--isodata-change", type=float, default=None, metavar="FRACTION",
                    help="with --classify isodata: stop once at most this fraction of the pixels changes cluster (default 0)")
    ap.add_argument("--isodata-model", metavar="PATH",
                    help="with --classify isodata: apply this saved model (isodata_model.npz of an earlier run) instead of fitting")
    from .preprocess import add_gcp_arguments
    add_gcp_arguments(ap)   # with --raw
    return ap


def options_from_args(a) -> RunOptions:
    """The parsed command line (parse_args) as RunOptions.  The defaults the parser leaves at None, so that parse_args can tell
    a given option from one left out (--compactness, --segment-iterations, --isodata-*), are filled in here."""
    iso = None
    if a.classify == "isodata":
        iso = {k: (d if getattr(a, f"isodata_{k}") is None else getattr(a, f"isodata_{k}")) for k, d in ISODATA_DEFAULTS.items()}
        iso["model_path"] = a.isodata_model
    return RunOptions(classify=a.classify, preprocessing=not a.no_preprocessing, n_clusters=a.n_clusters, evaluate=a.evaluate, raw=a.raw,
                      confidence=a.confidence, importance=a.importance, kmeans_model=a.kmeans_model, save_kmeans_model=a.save_kmeans_model,
                      mask_nodata=a.mask_nodata, sieve=a.sieve, majority=a.majority, majority_iterations=a.majority_iterations, gcps=a.gcps,
                      warp_order=a.warp_order, resampling=a.resampling, pixel_size=a.pixel_size, ml_threshold=a.ml_threshold,
                      rule_image=a.rule_image, segment=a.segment, compactness=10.0 if a.compactness is None else a.compactness,
                      segment_iterations=10 if a.segment_iterations is None else a.segment_iterations, object_based=a.object_based,
                      signatures=a.signatures, fit_on_device=a.fit_on_device, object_features=a.object_features, isodata=iso)


def _print_report(res, a) -> None:
    """What the command line prints of _run_scripts_2_3's result."""
    sdir = res.get("segmentation_dir")

    def accuracy(of, key):
        if f"metrics{key}" in res:
            m = res[f"metrics{key}"]
            print(f"evaluation{of}: OA {m['overall_accuracy'] * 100:.2f}%, kappa {m['kappa_coefficient']:.4f} -> {res[f'evaluation_dir{key}']}")

    if a.raw:
        print(f"preprocessed: {res['preprocessed']}")
    for k, v in res["paths"].items():
        print(f"{k}: {v}")
    if not a.classify:
        return
    cm = res.get("class_map")
    print(f"class map: {None if cm is None else (cm.shape, np.unique(cm).tolist())} -> {sdir}")
    accuracy("", "")
    if "postclass_stats" in res:
        s = res["postclass_stats"]
        print(f"cleaned map: {s['removed']} pixels sieved out, {s['filled']} filled, {s['left_as_nodata']} left as nodata, "
              f"majority passes changed {s['changed']} -> {sdir}")
    accuracy(" of the cleaned map", "_clean")
    if "segment_stats" in res:
        s = res["segment_stats"]
        print(f"segments: {s['n_segments']} superpixels of {s['area_min']} .. {s['area_max']} pixels after {s['n_iter']} iterations, "
              f"{s['n_regrown']} pixels regrown -> {sdir}")
    if "separability" in res:
        s = res["separability"]
        worst = (s.get("jm") or {}).get("least_separable")
        print(f"signatures: {len(s['classes'])} classes"
              + (f", least separable {worst['classes']} (JM {worst['value']:.4f})" if worst else "") + f" -> {sdir}")
    accuracy(" of the object-based map", "_objects")
    if "object_features_stats" in res:
        s = res["object_features_stats"]
        print(f"object features: {len(s['columns'])} columns, {s['n_train']} training superpixels of classes {s['classes']} -> {sdir}")
    accuracy(" of the object-features map", "_object_features")


def build_gmm_parser():
    """The options of --classify gmm.  They are parsed on their own, before the driver's parser sees the rest of the command
    line (split_gmm_args), and travel in GmmRunOptions.gmm."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m rsseg.stages", add_help=False, allow_abbrev=False)
    ap.add_argument("--gmm-covariance", choices=["full", "tied", "diag", "spherical"], default=None,
                    help="with --classify gmm (--n-clusters is the number of components): the covariance type (default full)")
    ap.add_argument("--gmm-iterations", type=int, default=None, metavar="N", help="with --classify gmm: at most N EM iterations (default 100)")
    ap.add_argument("--gmm-tol", type=float, default=None, metavar="T",
                    help="with --classify gmm: stop once the mean log-likelihood moves by less than T (default 1e-3)")
    ap.add_argument("--gmm-reg-covar", type=float, default=None, metavar="R", help="with --classify gmm: added to the covariances' diagonals (default 1e-6)")
    ap.add_argument("--gmm-posterior", action="store_true", help="with --classify gmm: also write gmm_posterior.npy and gmm_loglik.npy")
    ap.add_argument("--gmm-model", metavar="PATH", help="with --classify gmm: apply this saved model (gmm_model.npz of an earlier run) instead of fitting")
    return ap


def split_gmm_args(argv):
    """(run_gmm_stage's keyword arguments or None when no --gmm-* option is given, the rest of the command line)"""
    ap = build_gmm_parser()
    g, rest = ap.parse_known_args(argv)
    given = [f"--gmm-{k.replace('_', '-')}" for k in ("covariance", "iterations", "tol", "reg_covar") if getattr(g, f"gmm_{k}") is not None] + (
        ["--gmm-posterior"] if g.gmm_posterior else []) + (["--gmm-model"] if g.gmm_model else [])
    if g.gmm_iterations is not None and g.gmm_iterations < 1:
        ap.error("--gmm-iterations takes a positive count")
    for k in ("tol", "reg_covar"):
        v = getattr(g, f"gmm_{k}")
        if v is not None and not (v >= 0.0 and v < float("inf")):
            ap.error(f"--gmm-{k.replace('_', '-')} takes a finite non-negative number")
    kw = {k: (d if getattr(g, f"gmm_{k}", None) is None else getattr(g, f"gmm_{k}")) for k, d in GMM_DEFAULTS.items() if k != "model_path"}
    kw["posterior"] = bool(g.gmm_posterior)
    kw["model_path"] = g.gmm_model
    return (kw if given else None), given, rest


def main(argv=None) -> int:
    import dataclasses
    import sys
    gmm, gmm_given, rest = split_gmm_args(sys.argv[1:] if argv is None else list(argv))
    ap = build_parser()
    a = parse_args(ap, rest)
    if gmm_given and a.classify != "gmm":
        ap.error(f"{' / '.join(gmm_given)} need --classify gmm")
    o = options_from_args(a)
    if a.classify == "gmm":
        o = GmmRunOptions(**{f.name: getattr(o, f.name) for f in dataclasses.fields(o)}, gmm=gmm or dict(GMM_DEFAULTS))
    res = _run_scripts_2_3(a.image, a.output_dir, o, None)
    _print_report(res, a)
    return 1 if a.classify and res.get("class_map") is None else 0


if __name__ == "__main__":
    raise SystemExit(main())
