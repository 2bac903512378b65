"""The cases of tests/golden/indices_helpers.npz: the input dictionary, the calls, and the flat naming of nested results.
Shared by tests/make_indices_helpers_golden.py (which runs the reference) and the tests (which replay the calls on the mirror)."""
import json

import numpy as np


def flatten(obj, prefix=""):
    """{path: array} of a result: an array is '', member k of a dict 'k', member i of a list '#i', nested with '/'.  Order kept."""
    if isinstance(obj, np.ndarray):
        return {prefix.rstrip("/"): obj}
    out = {}
    items = obj.items() if isinstance(obj, dict) else ((f"#{i}", v) for i, v in enumerate(obj))
    for k, v in items:
        if isinstance(v, (np.ndarray, dict, list)):
            out.update(flatten(v, f"{prefix}{k}/"))
    return out


def unflatten(flat):
    """Inverse of flatten for the input dictionary (dicts of arrays, lists of arrays, nested once)."""
    out = {}
    for path, v in flat.items():
        parts = path.split("/")
        if len(parts) == 1:
            out[parts[0]] = v
        elif parts[1].startswith("#"):
            out.setdefault(parts[0], []).append(v)
        else:
            out.setdefault(parts[0], {})[parts[1]] = v
    return out


def input_dict():
    """A 12 x 10 feature dictionary: float32 index planes of large, middling and tiny variance, a constant plane, a float64
    plane, a list of principal components and a nested dict; and a label map for semantic_merge_water_classes."""
    rng = np.random.default_rng(20240611)
    h, w = 12, 10

    def plane(scale, shift=0.0, dtype=np.float32):
        return (shift + scale * rng.uniform(-1.0, 1.0, (h, w))).astype(dtype)

    D = {
        "ndvi": plane(1.0), "evi": plane(0.3), "msavi": plane(0.01, 0.3), "ndwi": plane(1.0, -0.1), "mndwi": plane(0.3, 0.2),
        "ndbi": plane(0.9), "bsi": plane(0.008),
        "constant": np.full((h, w), 0.25, np.float32),
        "lbp": plane(1.0, 2.0, np.float64),
        "pca_result": [plane(2.0), plane(0.3), plane(0.005), plane(1.5)],
        "glcm_features": {"contrast": plane(3.0, 3.0), "homogeneity": plane(0.004, 0.5), "energy": plane(0.3)},
        "tiny_list": [plane(0.002)],
    }
    seg = rng.integers(0, 5, (h, w)).astype(np.int32)
    return D, seg


# (function, positional arguments ('<D>': the dictionary, '<seg>': the label map), keyword arguments)
CALLS = [
    ("feature_selection_by_variance", ["<D>"], {}),
    ("feature_selection_by_variance", ["<D>"], {"threshold": 0.1}),
    ("feature_selection_by_variance", ["<D>", 0.0], {}),
    ("feature_fusion_for_segmentation", ["<D>"], {}),
    ("feature_fusion_for_segmentation", ["<D>", ["ndvi", "lbp", "nope", "pca_result", "bsi"]], {}),
    ("feature_fusion_for_segmentation", ["<D>"], {"fusion_method": "concatenate"}),
    ("feature_fusion_for_segmentation", ["<D>", ["constant", "evi"], "concatenate"], {}),
    ("feature_fusion_for_segmentation", ["<D>", ["nope", "pca_result"]], {}),
    ("feature_fusion_for_segmentation", ["<D>"], {"fusion_method": "mean"}),
    ("hierarchical_feature_fusion", ["<D>"], {}),
    ("semantic_merge_water_classes", ["<seg>"], {}),
    ("prepare_features_for_segmentation", ["<D>"], {}),
    ("prepare_features_for_segmentation", ["<D>", ["ndwi", "pca_result_1", "pca_result_9", "pca_result_x", "nope", "glcm_features_0", "bsi"]], {}),
    ("prepare_features_for_segmentation", ["<D>", ["nope", "pca_result_7"]], {}),
]
GPU_FUNCTIONS = ("prepare_features_for_segmentation",)   # goes through the mirror's robust_normalize


def load(path):
    """(input dictionary, label map, manifest, {out<i>/<path>: array}) of the fixture."""
    z = np.load(path)
    manifest = json.loads(str(z["manifest"]))
    D = unflatten({k[3:]: z[k] for k in z.files if k.startswith("in/")})
    return D, z["in_seg"], manifest, z


def replay(mod, entry, D, seg):
    """Runs one manifest entry on `mod`: ('raises', [type name, text]) or ('result', kind, {path: array})."""
    a = [seg if x == "<seg>" else (D if x == "<D>" else x) for x in entry["args"]]
    try:
        res = getattr(mod, entry["fn"])(*a, **entry["kwargs"])
    except (ValueError, KeyError, TypeError) as e:
        return "raises", [type(e).__name__, str(e)], None
    return "result", type(res).__name__, flatten(res)


def check(i, entry, got, z):
    """Bit for bit: the exception's type and text, or the result's kind, member order, dtypes, shapes and bytes."""
    tag, kind, flat = got
    if "raises" in entry:
        assert tag == "raises" and kind == entry["raises"], (entry["fn"], kind, entry["raises"])
        return
    assert tag == "result", (entry["fn"], kind)
    assert kind == entry["kind"]
    assert [[k, str(v.dtype), list(v.shape)] for k, v in flat.items()] == entry["result"], entry["fn"]
    for k, v in flat.items():
        want = z[f"out{i}/{k}"]
        assert v.tobytes() == want.tobytes(), f"{entry['fn']} call {i}: member {k!r} differs in {int((v != want).sum())} elements"
