"""The stage driver's plumbing without a GPU (rsseg.stages): every option of the command line reaches RunOptions, the driver's
classification request carries each option to the method it belongs to and to no other, and the two dataclasses keep the defaults
the functions they replace had.  The defaults are written out here; none is read from the code under test."""
import dataclasses
import inspect

import numpy as np
import pytest

from rsseg import stages as S

# dest -> (--classify method or None, arguments the option needs beside it, the option at a legal value that is not its default)
FLIPS = {
    "classify": (None, [], ["--classify", "kmeans"]),
    "n_clusters": ("kmeans", [], ["--n-clusters", "5"]),
    "no_preprocessing": (None, [], ["--no-preprocessing"]),
    "evaluate": ("kmeans", [], ["--evaluate", "roi.npy"]),
    "raw": (None, [], ["--raw"]),
    "confidence": ("random_forest", [], ["--confidence"]),
    "importance": ("random_forest", [], ["--importance", "roi.npy"]),
    "save_kmeans_model": ("kmeans", [], ["--save-kmeans-model", "model.npz"]),
    "kmeans_model": ("kmeans", [], ["--kmeans-model", "model.npz"]),
    "ml_threshold": ("maximum_likelihood", [], ["--ml-threshold", "0.9"]),
    "rule_image": ("mahalanobis", [], ["--rule-image"]),
    "fit_on_device": ("minimum_distance", [], ["--fit-on-device"]),
    "signatures": ("kmeans", [], ["--signatures"]),
    "mask_nodata": ("kmeans", [], ["--mask-nodata", "0"]),
    "sieve": ("kmeans", [], ["--sieve", "6"]),
    "majority": ("kmeans", [], ["--majority", "3"]),
    "majority_iterations": ("kmeans", ["--majority", "3"], ["--majority-iterations", "2"]),
    "segment": ("kmeans", [], ["--segment", "8"]),
    "compactness": ("kmeans", ["--segment", "8"], ["--compactness", "5"]),
    "segment_iterations": ("kmeans", ["--segment", "8"], ["--segment-iterations", "3"]),
    "object_based": ("kmeans", ["--segment", "8"], ["--object-based"]),
    "object_features": ("random_forest", ["--segment", "8"], ["--object-features"]),
    "isodata_init_clusters": ("isodata", [], ["--isodata-init-clusters", "5"]),
    "isodata_max_std": ("isodata", [], ["--isodata-max-std", "0.1"]),
    "isodata_min_dist": ("isodata", [], ["--isodata-min-dist", "0.2"]),
    "isodata_min_size": ("isodata", [], ["--isodata-min-size", "10"]),
    "isodata_iterations": ("isodata", [], ["--isodata-iterations", "5"]),
    "isodata_change": ("isodata", [], ["--isodata-change", "0.01"]),
    "isodata_model": ("isodata", [], ["--isodata-model", "isodata_model.npz"]),
    "gcps": (None, ["--raw"], ["--gcps", "gcps.txt"]),
    "warp_order": (None, ["--raw", "--gcps", "gcps.txt"], ["--warp-order", "2"]),
    "resampling": (None, ["--raw", "--gcps", "gcps.txt"], ["--resampling", "cubic"]),
    "pixel_size": (None, ["--raw", "--gcps", "gcps.txt"], ["--pixel-size", "30"]),
}
POSITIONALS = {"image", "output_dir"}   # these two go to _run_scripts_2_3 beside the options: test_main_hands_over_...


def _options(argv):
    return S.options_from_args(S.parse_args(S.build_parser(), argv))


def test_the_table_knows_every_dest_of_the_parser():
    dests = {a.dest for a in S.build_parser()._actions} - {"help"}
    assert dests == set(FLIPS) | POSITIONALS, sorted(dests ^ (set(FLIPS) | POSITIONALS))


@pytest.mark.parametrize("dest", sorted(FLIPS))
def test_every_dest_reaches_the_options(dest):
    method, beside, flag = FLIPS[dest]
    base = ["in.tif", "out"] + (["--classify", method] if method else []) + beside
    parser = S.build_parser()
    a0, a1 = S.parse_args(parser, base), S.parse_args(parser, base + flag)
    assert getattr(a0, dest) == parser.get_default(dest) and getattr(a1, dest) != parser.get_default(dest)
    o0, o1 = S.options_from_args(a0), S.options_from_args(a1)
    assert isinstance(o1, S.RunOptions) and o0 != o1
    assert o0 == _options(base)   # the same command line, the same options


def test_the_defaults_the_parser_leaves_open_are_filled_in():
    o = _options(["in.tif", "out", "--classify", "isodata", "--isodata-max-std", "0.1", "--isodata-model", "m.npz"])
    assert o.isodata == dict(init_clusters=None, max_std=0.1, min_dist=0.1, min_size=None, iterations=20, change=0.0, model_path="m.npz")
    assert (o.compactness, o.segment_iterations, o.preprocessing) == (10.0, 10, True)
    o = _options(["in.tif", "out", "--classify", "kmeans", "--segment", "8", "--compactness", "0", "--segment-iterations", "0", "--no-preprocessing"])
    assert o.isodata is None and (o.compactness, o.segment_iterations, o.preprocessing) == (0.0, 0, False)


def test_main_hands_over_the_positionals_and_the_options(monkeypatch, capsys):
    seen = []
    monkeypatch.setattr(S, "_run_scripts_2_3", lambda *args: seen.append(args) or {"paths": {"pkl": "somewhere"}})
    assert S.main(["scene.tif", "outdir", "--no-preprocessing"]) == 0
    assert seen == [("scene.tif", "outdir", _options(["scene.tif", "outdir", "--no-preprocessing"]), None)]
    assert capsys.readouterr().out == "pkl: somewhere\n"


# ---- the classification request of the driver -----------------------------------------------------------------------------
REQUEST_DEFAULTS = dict(method="rule_based", n_clusters=7, use_hierarchical_all=True, classifier=None, feature_keys=None,
                        labeled_roi_file="labeled_roi.tif", strict_reference=False, valid_mask=None, confidence=False, importance_mask=None,
                        save_kmeans_model=None, ml_threshold=None, rule_image=False, fit_on_device=False)
GAUSS = ("maximum_likelihood", "mahalanobis", "minimum_distance")
ROI = np.arange(12, dtype=np.int32).reshape(3, 4) % 3
MASK = np.ones((3, 4), np.uint8)
# every option that belongs to one method only, all set at once: each case below says which of them its method takes
EVERYTHING = dict(n_clusters=5, confidence=True, importance="roi.npy", save_kmeans_model="model.npz", ml_threshold=0.999, rule_image=True,
                  fit_on_device=True)


def _request(method, mask, **options):
    """-> (request, the paths the ROI loader was asked for); the loader is a stand-in, so nothing is read."""
    asked = []
    req = S.request_from_options(S.RunOptions(classify=method, **options), method, mask, lambda path: asked.append(path) or ROI)
    return req, asked


def _check(req, **expected):
    want = {**REQUEST_DEFAULTS, **expected}
    assert [f.name for f in dataclasses.fields(req)] == list(want)
    for name, value in want.items():
        got = getattr(req, name)
        if isinstance(value, np.ndarray):
            assert isinstance(got, np.ndarray) and np.array_equal(got, value), name
        else:
            assert got is value or (type(got) is type(value) and got == value), (name, got, value)


def test_request_random_forest_with_confidence():
    req, asked = _request("random_forest", None, confidence=True)
    _check(req, method="random_forest", confidence=True)
    assert asked == []
    req, asked = _request("random_forest", MASK, confidence=True, n_clusters=5)
    _check(req, method="random_forest", n_clusters=5, confidence=True, valid_mask=MASK)
    assert req.valid_mask is MASK and asked == []


@pytest.mark.parametrize("confidence", [False, True])
def test_request_random_forest_with_importance(confidence):
    req, asked = _request("random_forest", None, importance="roi.npy", confidence=confidence)
    _check(req, method="random_forest", confidence=confidence, importance_mask=ROI)
    assert asked == ["roi.npy"]
    req, asked = _request("random_forest", MASK, importance="roi.npy", confidence=confidence)   # a masked run ignores importance
    _check(req, method="random_forest", confidence=confidence, valid_mask=MASK)
    assert req.importance_mask is None and asked == []


@pytest.mark.parametrize("mask", [None, MASK])
def test_request_kmeans_with_save_kmeans_model(mask):
    req, asked = _request("kmeans", mask, save_kmeans_model="model.npz", n_clusters=4)
    _check(req, method="kmeans", n_clusters=4, save_kmeans_model="model.npz", valid_mask=mask)
    assert asked == []


@pytest.mark.parametrize("mask", [None, MASK])
@pytest.mark.parametrize("method", GAUSS)
def test_request_gaussian_options(method, mask):
    req, _ = _request(method, mask, ml_threshold=0.999, rule_image=True, fit_on_device=True)
    _check(req, method=method, ml_threshold=0.999, rule_image=True, fit_on_device=True, valid_mask=mask)
    req, _ = _request(method, mask)
    _check(req, method=method, valid_mask=mask)


def test_request_rule_based_takes_no_confidence():
    req, asked = _request("rule_based", None, confidence=True)
    _check(req, method="rule_based")
    assert req.confidence is False and asked == []


@pytest.mark.parametrize("mask", [None, MASK])
@pytest.mark.parametrize("method, takes", [("rule_based", {}), ("kmeans", dict(save_kmeans_model="model.npz")),
                                           ("random_forest", dict(confidence=True)),
                                           *[(m, dict(ml_threshold=0.999, rule_image=True, fit_on_device=True)) for m in GAUSS]])
def test_request_takes_only_what_belongs_to_the_method(method, takes, mask):
    req, asked = _request(method, mask, **EVERYTHING)
    if method == "random_forest" and mask is None:
        takes = dict(takes, importance_mask=ROI)
    _check(req, method=method, n_clusters=5, valid_mask=mask, **takes)
    assert asked == (["roi.npy"] if method == "random_forest" and mask is None else [])


# ---- defaults -------------------------------------------------------------------------------------------------------------
def _defaults(cls):
    return {f.name: f.default for f in dataclasses.fields(cls)}


def test_classify_request_has_the_defaults_of_run_classification_stage():
    assert _defaults(S.ClassifyRequest) == REQUEST_DEFAULTS
    assert S.ClassifyRequest.__dataclass_params__.frozen
    sig = inspect.signature(S.run_classification_stage).parameters   # and the literals above are the function's own
    shared = [n for n in REQUEST_DEFAULTS if n in sig]
    assert shared == ["method", "n_clusters", "use_hierarchical_all", "classifier", "feature_keys", "labeled_roi_file", "strict_reference"]
    assert {n: sig[n].default for n in shared} == {n: REQUEST_DEFAULTS[n] for n in shared}


def test_classify_products_start_empty():
    assert _defaults(S.ClassifyProducts) == dict.fromkeys(("kmeans_model", "proba", "confidence", "gauss_model", "dist2", "margin",
                                                           "importance", "feature_names"))


def test_run_options_have_the_defaults_the_driver_had():
    # the first seven had no default in the driver itself: run_scripts_2_3's; the other twenty are the driver's own
    assert _defaults(S.RunOptions) == dict(
        classify=None, preprocessing=True, n_clusters=7, evaluate=None, raw=False, confidence=False, importance=None,
        kmeans_model=None, save_kmeans_model=None, mask_nodata=None, sieve=0, majority=0, majority_iterations=1, gcps=None, warp_order=1,
        resampling="nearest", pixel_size=None, ml_threshold=None, rule_image=False, segment=0, compactness=10.0, segment_iterations=10,
        object_based=False, signatures=None, fit_on_device=False, object_features=False, isodata=None)
    assert S.RunOptions.__dataclass_params__.frozen
    sig = inspect.signature(S.run_scripts_2_3).parameters
    assert {n: p.default for n, p in sig.items() if p.default is not inspect.Parameter.empty} == dict(
        classify=None, preprocessing=True, n_clusters=7, ctx=None, evaluate=None, raw=False, confidence=False, importance=None)


def test_the_drivers_take_at_most_four_parameters():
    for fn in (S._run_scripts_2_3, S._run_classification, S._classify):
        assert len(inspect.signature(fn).parameters) <= 4, fn.__name__
