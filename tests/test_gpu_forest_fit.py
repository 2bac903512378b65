"""K16 on the GPU: RandomForestClassifier fitted by rsseg.forest_fit equals scikit-learn's own fit, whole fitted state,
floats bitwise: the reference's training problem, crop96's stack, tie-heavy data, capacity edges, a seeded sample of the
parameter space ($RSSEG_FUZZ_N for more), one larger case; the mirrors, joblib, refusals and the classification stage."""
import os
import subprocess
import sys

import numpy as np
import pytest
from sklearn.ensemble import RandomForestClassifier

from test_forest_fit_host import state_equal, tie_heavy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(X, y, ctx, **kw):
    from rsseg.forest_fit import fit
    want = RandomForestClassifier(**kw).fit(X, y)
    got = fit(RandomForestClassifier(**kw), X, y, ctx=ctx)
    return want, got


def check(X, y, ctx, **kw):
    want, got = both(X, y, ctx, **kw)
    state_equal(want, got)
    return want, got


def scene_samples(ctx, golden_dir):
    from rsseg import pipeline as P
    from rsseg.preprocess import preprocess_to_device
    scene = np.load(os.path.join(golden_dir, "scene_aa.npz"))
    planes = preprocess_to_device(ctx, [scene["dn"][i] for i in range(7)])
    stack, _ = P.feature_stack19(ctx, planes, 600, 600)
    host = P.stack19_to_host(stack, 600, 600)
    xy = scene["sample_coords"]
    return host, host[xy[:, 1], xy[:, 0]], scene["sample_labels"], scene


def test_reference_training_problem(ctx, golden_dir):
    from rsseg.forest import flatten_forest
    host, X, y, scene = scene_samples(ctx, golden_dir)
    want, got = check(X, y, ctx, n_estimators=100, random_state=42)
    # figures for the record (not assertions): class-map agreement and trees equal to the reference's committed model
    ctx.forest_load(flatten_forest(got))
    planes = [ctx.upload_f32(host[:, :, i].reshape(-1)) for i in range(19)]
    cm = ctx.forest_predict(planes).cpu().numpy().reshape(600, 600)
    ref = dict(np.load(os.path.join(golden_dir, "rf_samples_model_flat.npz")))
    mine = flatten_forest(got)
    same = 0
    for t in range(100):
        a, b = slice(ref["tree_off"][t], ref["tree_off"][t + 1]), slice(mine["tree_off"][t], mine["tree_off"][t + 1])
        same += int(all(np.array_equal(ref[k][a], mine[k][b]) for k in ("left", "right", "feature", "threshold", "value")))
    print(f"\n[K16] reference problem: class map agreement {float(np.mean(cm == scene['class_map'])):.6f}, "
          f"{same}/100 trees equal to rf_samples_model_flat.npz")


def test_crop96_stack19(ctx, golden_dir):
    z = np.load(os.path.join(golden_dir, "crop96.npz"))
    X = z["stack19"].reshape(-1, 19)                 # float64: fit casts to float32
    y = z["kmeans_stack19_k6"].reshape(-1) + 1
    check(X, y, ctx, n_estimators=100, random_state=42)


def test_tie_heavy(ctx):
    X, y = tie_heavy(3000, F=8, C=4, seed=11)
    check(X, y, ctx, n_estimators=20, random_state=0)
    check(X, y, ctx, n_estimators=5, random_state=3, max_features=None)


@pytest.mark.parametrize("F,C", [(1, 2), (64, 2), (5, 64), (64, 64)])
def test_capacity_edges(ctx, F, C):
    rs = np.random.RandomState(F * 100 + C)
    n = 2000
    X = (rs.randint(0, 50, (n, F)) / 49.0).astype(np.float32)
    y = (X[:, 0] * C * 0.9 + rs.randint(0, 3, n)).astype(int) % C
    y[:C] = np.arange(C)
    check(X, y, ctx, n_estimators=4, random_state=1)


def test_parameter_space_sample(ctx):
    rs = np.random.RandomState(2024)
    n_cases = int(os.environ.get("RSSEG_FUZZ_N", "12"))
    for _ in range(n_cases):
        n, F, C = int(rs.randint(20, 1500)), int(rs.randint(1, 24)), int(rs.randint(2, 7))
        X = rs.randint(0, int(rs.choice([3, 16, 256])), (n, F)).astype(np.float32) / 255.0
        y = (X.sum(1) * 7 + rs.randint(0, 2, n)).astype(int) % C
        kw = dict(n_estimators=int(rs.randint(1, 6)),
                  max_depth=[1, 2, 10, None][rs.randint(4)],
                  max_features=["sqrt", "log2", None, 1, 0.3][rs.randint(5)],
                  min_samples_leaf=[1, 3, 0.01][rs.randint(3)],
                  min_samples_split=[2, 7][rs.randint(2)],
                  bootstrap=bool(rs.randint(2)),
                  random_state=[0, 42, "rs7"][rs.randint(3)])
        if kw["random_state"] == "rs7":
            want = RandomForestClassifier(**{**kw, "random_state": np.random.RandomState(7)}).fit(X, y)
            from rsseg.forest_fit import fit
            got = fit(RandomForestClassifier(**{**kw, "random_state": np.random.RandomState(7)}), X, y, ctx=ctx)
            want.random_state = got.random_state = None    # the RandomState objects themselves differ by identity only
            state_equal(want, got)
        else:
            check(X, y, ctx, **kw)


def test_larger_case(ctx):
    rs = np.random.RandomState(5)
    n = 200_000
    X = rs.rand(n, 19).astype(np.float32)
    y = (X[:, 0] * 2 + X[:, 3] > 1.4).astype(int) + (X[:, 7] > 0.6).astype(int)
    flip = rs.rand(n) < 0.1
    y[flip] = rs.randint(0, 3, int(flip.sum()))
    check(X, y, ctx, n_estimators=8, random_state=42, n_jobs=-1)


def test_mirrors_predict_and_joblib(ctx, tmp_path):
    from modules import supervised_classifiers as S
    z = np.load(os.path.join(ROOT, "tests", "golden", "crop96.npz"))
    stack = z["stack19"]
    roi = np.zeros((96, 96), int)
    roi[::7, ::5] = (z["kmeans_stack19_k6"][::7, ::5] % 3) + 1
    X, y = S.prepare_training_samples(stack, roi, [1, 2, 3])
    path = str(tmp_path / "rf.pkl")
    model = S.train_random_forest_from_samples(X, y, save_path=path)
    want = RandomForestClassifier(n_estimators=100, max_depth=None, random_state=42).fit(X, y)
    state_equal(want, model)
    assert np.array_equal(S.predict_image(model, stack), want.predict(stack.reshape(-1, 19)).reshape(96, 96))
    code = ("import joblib, numpy as np, sys; m = joblib.load(sys.argv[1]); from sklearn.ensemble import RandomForestClassifier; "
            "assert type(m) is RandomForestClassifier; print(int(m.predict(np.zeros((1, 19), np.float32))[0]))")
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH",)}
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip()) == int(want.predict(np.zeros((1, 19), np.float32))[0])


def test_refusals_and_fallback(ctx):
    from modules.features import extract as E
    from rsseg.forest_fit import fit
    from rsseg.runtime import RssegUnsupported
    X, y = tie_heavy(300)
    Xn = X.copy()
    Xn[5, 0] = np.nan
    with pytest.raises(RssegUnsupported, match="NaN"):
        fit(RandomForestClassifier(), Xn, y, ctx=ctx)
    with pytest.raises(RssegUnsupported, match="criterion"):
        fit(RandomForestClassifier(criterion="entropy"), X, y, ctx=ctx)
    Xi = X.copy()
    Xi[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        fit(RandomForestClassifier(), Xi, y, ctx=ctx)
    # a matrix K16 cannot take (65 features) is fitted by scikit-learn on the host, with the same result
    rs = np.random.RandomState(0)
    Xw = rs.rand(200, 65).astype(np.float32)
    yw = (Xw[:, 0] > 0.5).astype(int) + 1
    clf = E.train_random_forest_classifier(Xw, yw, [f"f{i}" for i in range(65)], n_estimators=5)
    from sklearn.model_selection import train_test_split
    Xt, _, yt, _ = train_test_split(Xw, yw, test_size=0.3, random_state=42, stratify=yw)
    state_equal(RandomForestClassifier(n_estimators=5, random_state=42, n_jobs=-1).fit(Xt, yt), clf)


def test_classification_stage_caches_the_gpu_fit(ctx, tmp_path, golden_dir):
    import joblib
    from modules.features import extract as E
    from rsseg import stages
    from rsseg.tiff import write_tiff
    from sklearn.model_selection import train_test_split
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    fd, hier = stages.run_feature_extraction_stage(list(crop["bands"]))
    paths = stages.save_feature_outputs(str(tmp_path), fd, hier, 96, 96)
    roi = np.zeros((96, 96), np.uint8)
    roi[4:60, 4:60] = (crop["kmeans_stack19_k6"][4:60, 4:60] % 3 + 1).astype(np.uint8)
    write_tiff(str(tmp_path / "roi.tif"), roi)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        stages.run_classification_stage(paths["pkl"], "random_forest", str(tmp_path / "rf"), labeled_roi_file=str(tmp_path / "roi.tif"),
                                        ctx=ctx)
        _, calls = ctx.prof_get("forest_fit")
    finally:
        ctx.prof_enable(False)
    assert calls >= 1
    model = joblib.load(tmp_path / "rf" / stages.RF_MODEL_FILE)
    X, y = E.prepare_training_samples(hier["all"], str(tmp_path / "roi.tif"))
    Xt, _, yt, _ = train_test_split(X, y, test_size=0.3, random_state=42, stratify=y)
    state_equal(RandomForestClassifier(n_estimators=100, random_state=42, n_jobs=-1).fit(Xt, yt), model)
