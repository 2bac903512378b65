"""K30 on the GPU: rsseg_mlp_classify equals the restatement (tests/mlp_ref.py) as values (-0 equals +0, the NaN positions
coincide) in labels, margin, confidence and every probability plane over the feature counts, hidden widths, depths, class
counts, activations, alignments, pixel counts and the activations' and the softmax's range; the model object against
scikit-learn; the stage and the command; the error codes."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import mlp_cases as MC
import mlp_ref as R

pytestmark = pytest.mark.gpu

# (F, hidden, k, activation): F in {1, 3, 4, 5, 19, 64}; widths {1, 3, 4, 5, 15, 16, 17, 33, 100, 128} (the seams of the 4-wide k
# step and of the 16-wide tile); one, two and three hidden layers; k in {2, 3, 8, 9, 16, 17, 32}; the four activations; models
# small enough for a 256-pixel tile and large enough for the 128-, 64- and 32-pixel ones (test_the_sweep_takes_every_tile)
SWEEP = [(1, (15,), 2, "relu"), (3, (1,), 3, "identity"), (4, (3,), 8, "relu"), (5, (4, 15), 9, "tanh"), (19, (16,), 16, "logistic"),
         (19, (17, 33), 17, "relu"), (64, (128, 128), 32, "relu"), (19, (100,), 8, "relu"), (19, (100, 100), 8, "relu"),
         (19, (64, 64, 64), 16, "tanh"), (5, (33, 4, 5), 3, "logistic"), (3, (15,), 2, "tanh"), (4, (128,), 3, "identity")]
N_SWEEP = 577     # two whole 256-pixel tiles and a part of a third; an odd last pixel
N_REVERSED = 64   # pixels on which the reversed chains are restated (every pixel for a model of fewer than 2000 weights)
# twice the largest |restated probability - MLPClassifier.predict_proba| measured on the host over mlp_cases.FITTED (8.05e-07,
# tests/test_mlp_host.py): the GPU equals the restatement, the factor covers other BLAS builds
PROBA_TOL = 2 * 8.05e-7


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def sweep_case(F, hidden, k, activation, n=N_SWEEP):
    model = MC.random_model(F, hidden, k, activation, 1000 * F + 10 * k + len(hidden) + sum(hidden))
    X = MC.pixels(n, F, 7 * F + k)
    ref = R.classify(X, model)
    if n >= 64 and np.unique(ref["labels"][~ref["bad"]]).size < 2:
        # a narrow network whose logits hardly move with the pixel: one class wins everywhere.  The output biases are moved so
        # that every logit has mean 0 over the pixels, which lets the classes compete
        model["biases"][-1] = (model["biases"][-1] - ref["sums"][-1][~ref["bad"]].astype(np.float64).mean(axis=0)).astype(np.float32)
        ref = R.classify(X, model)
    return dict(model=model, X=X, ref=ref)


def _planes(ctx, X, shift=0):
    """Flat device planes of the columns of X; shift: every plane starts `shift` elements off its allocation (which is
    256-byte aligned), so one element off 16-byte alignment for shift = 1."""
    torch = _torch()
    out = []
    for f in range(X.shape[1]):
        t = torch.empty(X.shape[0] + shift, dtype=torch.float32, device=ctx.device)
        t[shift:] = torch.from_numpy(np.ascontiguousarray(X[:, f])).to(ctx.device)
        out.append(t[shift:])
    return out


def _same(got, want):
    """Equal as values: -0 equals +0, NaN where and only where the other has one."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))


def _check(ctx, c, shift=0, margin=True, conf=True, proba=True):
    ref = c["ref"]
    lab, mg, cf, pr = ctx.mlp_classify(_planes(ctx, c["X"], shift), want_margin=margin, want_conf=conf, want_proba=proba, **MC.model_args(c["model"]))
    assert np.array_equal(lab.cpu().numpy(), ref["labels"])
    assert ((mg is None), (cf is None), (pr is None)) == (not margin, not conf, not proba)
    if margin:
        assert _same(mg.cpu().numpy(), ref["margin"])
    if conf:
        assert _same(cf.cpu().numpy(), ref["conf"])
    if proba:
        assert _same(pr.cpu().numpy(), ref["proba"])
    return ref


@pytest.mark.parametrize("F,hidden,k,activation", SWEEP)
def test_kernel_equals_the_restatement(ctx, F, hidden, k, activation):
    c = sweep_case(F, hidden, k, activation)
    ref = _check(ctx, c)
    _check(ctx, c, shift=1, margin=False, conf=False, proba=False)      # planes one element off 16-byte alignment, labels alone
    # the case is worth its name.  Chains summed in the other order give other bits: in a hidden layer wherever one has a chain
    # of two or more terms (F >= 2, or a second hidden layer), else (F = 1, one hidden layer) in the output layer's sums
    m, X = c["model"], c["X"]
    nr = X.shape[0] if sum(w.size for w in m["weights"]) < 2000 else N_REVERSED
    rev = R.classify(X[:nr], m, reverse=True)
    layers = range(len(hidden)) if (F >= 2 or len(hidden) >= 2) else [len(hidden)]
    assert any(not np.array_equal(rev["sums"][l].view(np.uint32), ref["sums"][l][:nr].view(np.uint32)) for l in layers)
    if activation == "relu":      # units of both kinds, dead and alive
        a = np.concatenate([s[~ref["bad"]].reshape(-1) for s in ref["sums"][:-1]])
        assert bool((a > 0).any()) and bool((a <= 0).any())
    bad = ref["bad"]
    assert np.array_equal(bad, np.isinf(X).any(axis=1)) and int(bad.sum()) == 2      # the refused pixels are exactly the infinite ones
    assert np.all(ref["labels"][bad] == 0) and np.all(np.isnan(ref["margin"][bad])) and np.all(np.isnan(ref["conf"][bad])) and np.all(np.isnan(ref["proba"][:, bad]))
    assert np.all(ref["labels"][~bad] != 0) and np.all(np.isfinite(ref["margin"][~bad])) and np.all(np.isfinite(ref["proba"][:, ~bad]))
    assert bool(np.isnan(X[~bad]).any())
    W = np.concatenate([w.reshape(-1) for w in m["weights"]])
    assert bool((W > 0).any()) and bool((W < 0).any()) and (W.size < 8 or bool((W == 0).any())) and bool((m["scale"] < 0).any())
    assert np.all(np.diff(m["class_values"].astype(int)) < 0) and not np.array_equal(np.sort(m["class_values"]), np.arange(1, k + 1))
    assert np.unique(ref["labels"][~bad]).size >= 2


def test_the_sweep_takes_every_tile(ctx):
    tiles = set()
    for F, hidden, k, _ in SWEEP:
        fits, tile = ctx.mlp_plan([F, *hidden, 1 if k == 2 else k], k)
        assert fits and tile in (256, 128, 64, 32, 16)
        tiles.add(tile)
    assert {256, 128, 64, 32} <= tiles
    assert ctx.mlp_plan([64, 128, 128, 128, 32], 32) == (False, 0)


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True)])
def test_each_optional_output_alone(ctx, want):
    _check(ctx, sweep_case(19, (17, 33), 17, "relu"), shift=1, margin=want[0], conf=want[1], proba=want[2])


@pytest.mark.parametrize("F,hidden,k,activation", [(19, (100,), 8, "relu"), (19, (64, 64, 64), 16, "tanh"), (19, (100, 100), 8, "relu")])      # tiles of 256, 128, 64
def test_pixel_counts(ctx, F, hidden, k, activation):
    _, tile = ctx.mlp_plan([F, *hidden, k], k)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1025, 2 * tile + 1):
        c = sweep_case(F, hidden, k, activation, n)
        _check(ctx, c)
        _check(ctx, c, shift=1, margin=False, conf=False, proba=False)


def test_outputs_at_any_element_alignment(ctx):
    """Output planes that start one element off their vector alignment: nothing outside [0, n) of any of them is written."""
    torch = _torch()
    n = 1023
    c = sweep_case(4, (3,), 8, "relu", n)
    m, ref, k = c["model"], c["ref"], 8
    lab = torch.full((n + 9,), 77, dtype=torch.uint8, device=ctx.device)
    mg = torch.full((n + 9,), -5.0, dtype=torch.float32, device=ctx.device)
    cf = torch.full((n + 9,), -6.0, dtype=torch.float32, device=ctx.device)
    pr = torch.full((k * n + 9,), -7.0, dtype=torch.float32, device=ctx.device)
    assert _raw(ctx, dict(planes=_planes(ctx, c["X"]), n=n, labels=lab[1:], margin=mg[3:], conf=cf[1:], proba=pr[5:], **_model_kw(m))) == 0
    ctx.sync()
    lab, mg, cf, pr = lab.cpu().numpy(), mg.cpu().numpy(), cf.cpu().numpy(), pr.cpu().numpy()
    assert np.array_equal(lab[1:n + 1], ref["labels"]) and lab[0] == 77 and np.all(lab[n + 1:] == 77)
    assert _same(mg[3:n + 3], ref["margin"]) and np.all(mg[:3] == -5.0) and np.all(mg[n + 3:] == -5.0)
    assert _same(cf[1:n + 1], ref["conf"]) and cf[0] == -6.0 and np.all(cf[n + 1:] == -6.0)
    assert _same(pr[5:k * n + 5].reshape(k, n), ref["proba"]) and np.all(pr[:5] == -7.0) and np.all(pr[k * n + 5:] == -7.0)


@pytest.mark.parametrize("activation", ["logistic", "tanh"])
def test_the_activation_range(ctx, activation):
    """Arguments of the activation from 0 through 2^-13 (where tanh changes form) to beyond 708 (where svm_exp gives +0), of
    both signs: one feature, hidden units that take it times 1, -1 and 0.5."""
    m = MC.random_model(1, (3,), 3, activation, 61)
    m.update(offset=np.zeros(1, np.float32), scale=np.ones(1, np.float32))
    m["weights"][0] = np.array([[1.0, -1.0, 0.5]], np.float32)
    m["biases"][0] = np.zeros(3, np.float32)
    edge = np.float32(2.0 ** -13)
    mag = np.concatenate([[0.0, edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1)), 354.0, 354.5, 708.0, 709.0, 1416.0, 1e4, 3e38],
                          np.geomspace(1e-8, 2e3, 600)]).astype(np.float32)
    X = np.concatenate([mag, -mag]).reshape(-1, 1)
    c = dict(model=m, X=X, ref=R.classify(X, m))
    ref = _check(ctx, c)
    a = np.abs(ref["sums"][0].astype(np.float64))
    assert bool((a == 0).any()) and bool(((a > 0) & (a < 2.0 ** -13)).any()) and bool((a == 2.0 ** -13).any()) and bool((a > 708).any()) and bool((a > 1416).any())
    h = R.activation(ref["sums"][0], activation)
    assert np.all(np.isfinite(h)) and float(h.max()) == 1.0 and float(h.min()) == (0.0 if activation == "logistic" else -1.0)
    if activation == "tanh":
        small = a[:, 0] < 2.0 ** -13
        big = a[:, 0] > 0.01      # just above 2^-13 the float32 nearest tanh(a) is still a: 1 - a^2 / 3 rounds to 1
        assert np.array_equal(h[small, 0], ref["sums"][0][small, 0]) and np.all(h[big, 0] != ref["sums"][0][big, 0])


def test_logits_far_apart_and_overflowed(ctx):
    """An identity network whose logits grow with the pixel's magnitude: differences beyond 708 (a probability of exactly +0),
    then logits that overflow to +-inf and NaN (inf - inf, 0 * inf), whose labels follow the winner rule: the lowest j with the
    largest logit, a NaN never the winner unless all are."""
    F, k = 3, 5
    m = MC.random_model(F, (4,), k, "identity", 71)
    m.update(offset=np.zeros(F, np.float32), scale=np.ones(F, np.float32))
    m["weights"][0] *= np.float32(8)      # hidden sums of a few times the pixel's magnitude: the largest pixels overflow
    m["weights"][1][:, 2] = 0.0      # one logit is its bias, until a hidden unit is infinite: 0 * inf
    rng = np.random.default_rng(72)
    n = 640
    X = (rng.standard_normal((n, F)) * np.repeat([1.0, 1e2, 1e4, 1e19, 1e30, 1e37, 1e38, 3e38], n // 8)[:, None]).clip(-3e38, 3e38).astype(np.float32)      # finite pixels
    X[-40:, 1] = 0.0
    c = dict(model=m, X=X, ref=R.classify(X, m))
    ref = _check(ctx, c)
    assert not ref["bad"].any()
    o, p = ref["o"], ref["proba"]
    assert bool((p == 0).any()) and bool(((p > 0) & (p < 1e-30)).any()) and bool((ref["conf"] == 1.0).any())
    assert bool(np.isposinf(o).any()) and bool(np.isneginf(o).any()) and bool(np.isnan(o).any()) and bool(np.isfinite(o).all(axis=1).any())
    some_nan = np.isnan(o).any(axis=1) & ~np.isnan(o).all(axis=1)
    assert bool(some_nan.any()) and not bool(np.isnan(o[some_nan, ref["win"][some_nan]]).any())
    rank = np.where(np.isnan(o), -np.inf, np.maximum(o.astype(np.float64), -1e300))      # a NaN below everything, -inf included
    assert np.array_equal(ref["win"][some_nan], np.argmax(rank[some_nan], axis=1))
    ties = np.isposinf(o).sum(axis=1) >= 2      # two logits at +inf: the lower index wins
    assert bool(ties.any()) and np.array_equal(ref["win"][ties], np.argmax(np.isposinf(o[ties]), axis=1))
    assert np.array_equal(ref["labels"], m["class_values"][ref["win"]]) and np.all(np.isnan(ref["conf"][np.isposinf(o).any(axis=1)]))


def test_all_nan_logits_take_the_first_class(ctx):
    m = MC.random_model(2, (4,), 3, "identity", 73)
    m.update(offset=np.zeros(2, np.float32), scale=np.ones(2, np.float32))
    m["weights"][0] = np.array([[1, -1, 1, -1], [1, 1, -1, -1]], np.float32)
    m["weights"][1] = np.ones((4, 3), np.float32)
    X = np.array([[3e38, 3e38], [1.0, 2.0], [-3e38, 3e38]], np.float32)
    c = dict(model=m, X=X, ref=R.classify(X, m))
    ref = _check(ctx, c)
    assert np.isnan(ref["o"][0]).all() and ref["win"][0] == 0 and ref["labels"][0] == m["class_values"][0] and np.isnan(ref["margin"][0])


def _clf(k, F, hidden, activation):
    from rsseg.mlp import NeuralNetClassifier
    mlp, offset, scale, Xte = MC.fitted(k, F, hidden, activation)
    return mlp, NeuralNetClassifier.from_sklearn(mlp, offset, scale), (Xte - offset) * scale, Xte


@pytest.mark.parametrize("k,F,hidden,activation", MC.FITTED)
def test_fitted_model_reproduces_scikit_learn(ctx, k, F, hidden, activation):
    """Labels equal MLPClassifier.predict wherever the restated margin exceeds 1e-4 max(1, |o_win|); at most 0.1 % of the
    pixels are excluded.  predict_proba within PROBA_TOL of scikit-learn's."""
    mlp, clf, Xs, Xte = _clf(k, F, hidden, activation)
    got = clf.predict(Xte, ctx=ctx)
    ref = R.classify(Xte, MC.model_of(clf))
    o_win = ref["o"][np.arange(Xte.shape[0]), ref["win"]]
    sure = ref["margin"] > 1e-4 * np.maximum(1.0, np.abs(o_win))
    assert int((~sure).sum()) <= 0.001 * sure.size
    assert np.array_equal(got[sure], mlp.predict(Xs)[sure])
    proba = clf.predict_proba(Xte, ctx=ctx)
    assert proba.shape == (Xte.shape[0], k) and proba.dtype == np.float32 and _same(proba, ref["proba"].T)
    worst = float(np.abs(proba.astype(np.float64) - mlp.predict_proba(Xs)).max())
    print(f"k={k} F={F} hidden={hidden} {activation}: worst probability difference from scikit-learn {worst:.3g}")
    assert worst <= PROBA_TOL


def test_predict_image_with_a_mask(ctx):
    mlp, clf, _, _ = _clf(3, 8, (32,), "relu")
    rng = np.random.default_rng(91)
    h, w, k = 67, 131, 3          # more than two compaction tiles
    feats = (1.5 * rng.standard_normal((h, w, 8))).astype(np.float32)
    mask = rng.random((h, w)) < 0.6
    mask[:9] = False
    got, mg, cf, pr = clf.predict_image(feats, mask=mask, want_margin=True, want_conf=True, want_proba=True, ctx=ctx)
    assert got.shape == (h, w) and got.dtype == clf.classes_.dtype and mg.dtype == cf.dtype == pr.dtype == np.float32
    assert mg.shape == cf.shape == (h, w) and pr.shape == (k, h, w)
    want = np.zeros((h, w), np.int64)
    want[mask] = clf.predict(feats[mask], ctx=ctx)      # the host-compacted pixels
    assert np.array_equal(got, want) and set(np.unique(got[mask])) <= set(clf.classes_.tolist())
    ref = R.classify(feats[mask], MC.model_of(clf))
    assert np.array_equal(got[mask], clf._to_classes(ref["labels"])) and np.all(got[~mask] == 0)
    assert _same(mg[mask], ref["margin"]) and np.all(np.isnan(mg[~mask]))
    assert _same(cf[mask], ref["conf"]) and np.all(np.isnan(cf[~mask]))
    assert _same(pr[:, mask], ref["proba"]) and np.all(np.isnan(pr[:, ~mask]))
    plain, conf = clf.predict_image([feats[:, :, i] for i in range(8)], want_conf=True, ctx=ctx)      # unmasked, from a list of planes
    assert np.array_equal(plain[mask], got[mask]) and _same(conf[mask], cf[mask])
    assert np.array_equal(plain.reshape(-1), clf.predict(feats.reshape(-1, 8), ctx=ctx))
    assert np.array_equal(clf.predict_image(feats, ctx=ctx), plain)


def test_stage_and_command(ctx, golden_dir, tmp_path):
    """python -m rsseg.mlp on the directory of an earlier stages run: the five files, equal to the model object called
    directly; every earlier file byte-identical; --model reproduces the map.  run_mlp_stage with a valid mask."""
    from rsseg import mlp, stages
    from rsseg.mlp import NeuralNetClassifier
    from rsseg.tiff import read_tiff, write_tiff
    crop = np.load(os.path.join(golden_dir, "crop96.npz"))
    bands = np.ascontiguousarray(crop["bands"])
    image, out = str(tmp_path / "in.tif"), tmp_path / "run"
    write_tiff(image, bands, transform=(30.0, 0.0, 440000.0, 0.0, -30.0, 3300000.0), epsg=32649)
    roi = np.zeros((96, 96), np.uint8)
    roi[4:60:2, 4:60:2] = (crop["kmeans_stack19_k6"][4:60:2, 4:60:2] % 3 + 1).astype(np.uint8) * 4
    write_tiff(str(tmp_path / "roi.tif"), roi)
    assert stages.main([image, str(out), "--classify", "rule_based"]) == 0

    def snapshot():
        return {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}

    before = snapshot()
    assert mlp.main([str(out), "--roi", str(tmp_path / "roi.tif"), "--hidden", "24,12", "--max-iter", "60", "--rule-image"]) == 0
    after = snapshot()
    new = {os.path.join("segmentation_results", f) for f in ("classification_mlp.npy", "mlp_classification_map.tif", "mlp_model.npz", "mlp_margin.npy",
                                                             "mlp_confidence.npy")}
    assert set(after) - set(before) == new
    assert all(after[f] == before[f] for f in before)
    sdir = out / "segmentation_results"
    allf = np.load(out / "feature_outputs" / "all_hierarchical_features.npy")
    clf = NeuralNetClassifier(hidden_layer_sizes=(24, 12), max_iter=60).fit_image(allf, roi)
    want, mg, cf = clf.predict_image(allf, want_margin=True, want_conf=True, ctx=ctx)
    got = np.load(sdir / "classification_mlp.npy")
    assert got.dtype == np.uint8 and np.array_equal(got, want) and set(np.unique(got)) <= {4, 8, 12}
    assert np.array_equal(read_tiff(str(sdir / "mlp_classification_map.tif"))[0], want)
    assert _same(np.load(sdir / "mlp_margin.npy"), mg) and _same(np.load(sdir / "mlp_confidence.npy"), cf)
    a, b = clf.params(), NeuralNetClassifier.load(str(sdir / "mlp_model.npz")).params()
    assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)
    assert float((got[roi != 0] == roi[roi != 0]).mean()) > 0.5
    # --model: the saved model, applied to a directory that has no MLP files yet
    model = str(tmp_path / "kept_model.npz")
    shutil.copy(sdir / "mlp_model.npz", model)
    for f in new:
        os.remove(out / f)
    assert mlp.main([str(out), "--model", model]) == 0
    assert np.array_equal(np.load(sdir / "classification_mlp.npy"), want) and not os.path.exists(sdir / "mlp_margin.npy")
    assert all(np.asarray(a[key]).tobytes() == np.asarray(v).tobytes() for key, v in NeuralNetClassifier.load(str(sdir / "mlp_model.npz")).params().items())
    # the stage function, tanh, under a valid mask
    valid = np.ones((96, 96), np.uint8)
    valid[:, 70:] = 0
    lin = stages.run_mlp_stage(str(out / "feature_outputs" / "all_features_and_metadata.pkl"), str(tmp_path / "lin"),
                               labeled_roi_file=str(tmp_path / "roi.tif"), hidden_layer_sizes=(10,), activation="tanh", max_iter=40, valid_mask=valid, ctx=ctx)
    want_lin = NeuralNetClassifier(hidden_layer_sizes=(10,), activation="tanh", max_iter=40).fit_image(allf, roi).predict_image(allf, mask=valid, ctx=ctx)
    assert np.array_equal(lin, want_lin) and np.all(lin[:, 70:] == 0) and np.all(lin[:, :70] != 0)
    assert sorted(os.listdir(tmp_path / "lin")) == ["classification_mlp.npy", "mlp_classification_map.tif", "mlp_model.npz"]


def _model_kw(m):
    a = MC.model_args(m)
    return dict(F=int(m["widths"][0]), n_layers=len(m["weights"]), widths=m["widths"], weights=a["weights"], biases=a["biases"], offset=m["offset"],
                scale=m["scale"], activation=("relu", "identity", "logistic", "tanh").index(m["activation"]), k=len(m["class_values"]),
                cv=m["class_values"])


def _raw(ctx, a):
    fp = C.POINTER(C.c_float)
    f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)   # noqa: E731
    keep = {key: f32(a[key]) for key in ("weights", "biases", "offset", "scale")}
    widths = None if a["widths"] is None else np.ascontiguousarray(a["widths"], np.int32)
    cv = None if a["cv"] is None else np.ascontiguousarray(a["cv"], np.uint8)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    d = lambda key: None if keep[key] is None else keep[key].ctypes.data_as(fp)   # noqa: E731
    return ctx.lib.rsseg_mlp_classify(ctx.h, ctx._pp(a["planes"]), a["F"], a["n"], a["n_layers"],
                                      None if widths is None else widths.ctypes.data_as(C.POINTER(C.c_int)), d("weights"), d("biases"), d("offset"),
                                      d("scale"), a["activation"], a["k"], None if cv is None else cv.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      ptr(a["labels"]), ptr(a.get("margin")), ptr(a.get("conf")), ptr(a.get("proba")))


def test_error_codes(ctx):
    from rsseg.runtime import RssegUnsupported
    torch = _torch()
    F, k, n = 3, 3, 10
    m = MC.random_model(F, (5, 4), k, "relu", 5)
    two = MC.random_model(F, (5,), 2, "tanh", 6)
    pl = _planes(ctx, np.zeros((n, F), np.float32))
    lab = torch.full((n,), 9, dtype=torch.uint8, device=ctx.device)
    odd = torch.zeros(4 * n + 8, dtype=torch.uint8, device=ctx.device)[1:4 * n + 1].view(torch.uint8)      # a byte off float alignment
    ok = dict(planes=pl, n=n, labels=lab, **_model_kw(m))

    def call(**kw):
        rc = _raw(ctx, {**ok, **kw})
        return rc, ctx.lib.rsseg_last_error(ctx.h).decode()

    assert call()[0] == 0 and call(**_model_kw(two))[0] == 0
    INVALID, UNSUPPORTED = -1, -5
    at = lambda a, i, v: np.where(np.arange(a.size).reshape(a.shape) == i, v, a).astype(np.float32)   # noqa: E731
    W, B = ok["weights"], ok["biases"]
    for kw, code, word in (
            (dict(planes=[pl[0], None, pl[2]]), INVALID, "d_planes[1] is null"),
            (dict(planes=[pl[0], odd, pl[2]]), INVALID, "d_planes[1] is not aligned"),
            (dict(F=0), INVALID, "d_planes"),
            (dict(F=65), UNSUPPORTED, "F=65"),
            (dict(F=2), INVALID, "widths[0]=3"),
            (dict(n_layers=1), UNSUPPORTED, "n_layers=1"),
            (dict(n_layers=5), UNSUPPORTED, "n_layers=5"),
            (dict(k=1), INVALID, "k=1"),
            (dict(k=33), UNSUPPORTED, "k=33"),
            (dict(k=4), INVALID, "widths[3]=3 output units"),
            (dict(k=2), INVALID, "output units"),
            (dict(activation=4), UNSUPPORTED, "activation=4"),
            (dict(activation=-1), UNSUPPORTED, "activation=-1"),
            (dict(n=-1), INVALID, "n=-1"),
            (dict(widths=None), INVALID, "model"),
            (dict(weights=None), INVALID, "model"),
            (dict(biases=None), INVALID, "model"),
            (dict(offset=None), INVALID, "model"),
            (dict(scale=None), INVALID, "model"),
            (dict(cv=None), INVALID, "model"),
            (dict(widths=[3, 0, 4, 3]), INVALID, "widths[1]=0"),
            (dict(widths=[3, 129, 4, 3]), UNSUPPORTED, "widths[1]=129"),
            (dict(offset=at(m["offset"], 1, np.nan)), INVALID, "offset[1]"),
            (dict(scale=at(m["scale"], 2, np.inf)), INVALID, "scale[2]"),
            (dict(scale=at(m["scale"], 0, 0.0)), INVALID, "scale[0] is 0"),
            (dict(weights=at(W, 17, np.nan)), INVALID, "weights[17]"),
            (dict(biases=at(B, 6, -np.inf)), INVALID, "biases[6]"),
            (dict(cv=np.array([3, 0, 4], np.uint8)), INVALID, "class_values[1] is 0"),
            (dict(cv=np.array([3, 4, 3], np.uint8)), INVALID, "class_values[2]=3 occurs twice"),
            (dict(labels=None), INVALID, "d_labels"),
            (dict(margin=odd), INVALID, "d_margin"),
            (dict(conf=odd), INVALID, "d_conf"),
            (dict(proba=odd), INVALID, "d_proba")):
        rc, msg = call(**kw)
        assert rc == code and word in msg and msg.startswith("mlp_classify: "), (list(kw), rc, msg)
    # a model within every single limit that does not fit LDS
    big = MC.random_model(64, (128, 128, 128), 32, "relu", 7)
    rc, msg = call(planes=_planes(ctx, np.zeros((n, 64), np.float32)), **_model_kw(big))
    assert rc == UNSUPPORTED and "LDS" in msg
    # n == 0 touches nothing, whatever the planes
    ctx.sync()
    lab.fill_(9)
    assert call(n=0, planes=[None] * F, labels=None)[0] == 0
    ctx.sync()
    assert bool((lab == 9).all().item())
    # the Python side
    args = MC.model_args(m)
    with pytest.raises(ValueError, match="class_values"):
        ctx.mlp_classify(pl, **{**args, "class_values": [1, 2, 256]})
    with pytest.raises(ValueError, match="is 0"):
        ctx.mlp_classify(pl, **{**args, "class_values": [1, 0, 2]})
    with pytest.raises(ValueError, match="shapes"):
        ctx.mlp_classify(pl, **{**args, "weights": args["weights"][:-1]})
    with pytest.raises(ValueError, match="shapes"):
        ctx.mlp_classify(pl[:2], **args)
    with pytest.raises(ValueError, match="activation"):
        ctx.mlp_classify(pl, **{**args, "activation": "softplus"})
    with pytest.raises(ValueError, match="float32"):
        ctx.mlp_classify([pl[0], pl[1], pl[2].double()], **args)
    with pytest.raises(RssegUnsupported):
        ctx.mlp_classify(_planes(ctx, np.zeros((4, 64), np.float32)), **MC.model_args(big))
    out = ctx.mlp_classify(_planes(ctx, np.zeros((0, F), np.float32)), want_margin=True, want_conf=True, want_proba=True, **args)
    assert out[0].numel() == out[1].numel() == out[2].numel() == 0 and tuple(out[3].shape) == (k, 0)


def test_profiler_name(ctx):
    c = sweep_case(3, (1,), 3, "identity", 3)
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        _check(ctx, c)
        _, calls = ctx.prof_get("mlp_classify")
    finally:
        ctx.prof_enable(False)
    assert calls == 1
