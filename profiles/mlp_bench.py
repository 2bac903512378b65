"""K30, the neural-network pass (Context.mlp_classify), timed at the size a user would run it: 19 float32 feature planes,
k = 8 classes, --size (16384) squared pixels, relu networks with hidden layers (100,) and (100, 100) fitted by scikit-learn's
MLPClassifier on seeded blobs (a few epochs: the time of a pass does not depend on the weights).

Per network and per form (labels only; labels + margin + confidence): device events around the call (model upload included), one
warm-up and then --reps calls: minimum and median; Mpixel/s; and against four yardsticks
  copy      a device-to-device copy of the bytes the pass reads (19 planes), timed the same way
  peak      the 157.3 TFLOP/s float32 matrix peak under 2 (sum of in x out) + 2 F operations per pixel (an fma as two)
  gauss_ml  K22's maximum-likelihood pass (Context.gauss_classify, labels only) on the same planes
  cpu       MLPClassifier.predict of the same network on a --cpu-size (4096) squared raster on the host, with the threads the
            process is given (OMP_NUM_THREADS), extrapolated to the timed size
--valu-lib PATH: the same calls in a child process that loads another build of the library, one whose layers run on the
vector ALUs (docs/experiments/k30_mlp_valu_experiment.diff.txt), for the A/B figure; --lib PATH / --child are that child.
One JSON object on stdout (and in --out).
Usage: python profiles/mlp_bench.py [--size 16384] [--reps 3] [--cpu-size 4096] [--no-cpu] [--valu-lib PATH] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
F, K = 19, 8
NETWORKS = {"h100": (100,), "h100_100": (100, 100)}
FORMS = {"labels": (False, False), "labels_margin_conf": (True, True)}


def training_set(n_per_class=200, seed=30):
    """Correlated Gaussian blobs that overlap, rounded to float32: (X, y) with classes 1..K."""
    rng = np.random.default_rng(seed)
    means = 0.8 * rng.standard_normal((K, F))
    X = np.concatenate([means[j] + rng.standard_normal((n_per_class, F)) @ (rng.standard_normal((F, F)) / np.sqrt(F) + 0.6 * np.eye(F)).T
                        for j in range(K)]).astype(np.float32)
    return X, np.repeat(np.arange(1, K + 1), n_per_class)


def fitted(hidden):
    """(sklearn MLPClassifier, rsseg NeuralNetClassifier of it) on the standardised training set."""
    from sklearn.neural_network import MLPClassifier
    from rsseg.mlp import NeuralNetClassifier
    X, y = training_set()
    offset = X.mean(axis=0, dtype=np.float32)
    scale = (np.float32(1) / X.std(axis=0, dtype=np.float32)).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mlp = MLPClassifier(hidden_layer_sizes=hidden, max_iter=30, random_state=0).fit((X - offset) * scale, y)
    return mlp, NeuralNetClassifier.from_sklearn(mlp, offset, scale)


def flop_per_pixel(clf):
    w = clf.widths_.astype(np.int64)
    return int(2 * (w[:-1] * w[1:]).sum() + 2 * F)


def event_ms(torch, stream, fn, reps):
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), runs=[float(x) for x in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-size", type=int, default=4096)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--valu-lib", default="")
    ap.add_argument("--lib", default="", help="load this build of the library (the A/B child)")
    ap.add_argument("--child", action="store_true", help="the kernel's figures alone")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from rsseg import _lib
    if a.lib:
        _lib.load(a.lib)
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    n = a.size * a.size
    g = torch.Generator(device=ctx.device)
    g.manual_seed(23)
    planes = [2.0 * torch.randn(n, generator=g, device=ctx.device, dtype=torch.float32) for _ in range(F)]
    res = dict(device=torch.cuda.get_device_name(0), planes=F, dtype="float32", k=K, size=a.size, pixels=n, reps=a.reps, library=a.lib or "this build",
               f32_matrix_peak_tflop_per_s=F32_MATRIX_PEAK / 1e12, bytes_read=4 * F * n, networks={})
    if not a.child:
        src = torch.cat([p[: n // 8] for p in planes])      # an eighth of every plane: the copy is timed on 19 n / 8 floats, 8 times
        dst = torch.empty_like(src)
        ms = event_ms(torch, ctx.torch_stream, lambda: [dst.copy_(src) for _ in range(8)], a.reps)
        res["copy_of_bytes_read"] = dict(call_ms=ms, gb_per_s_read=4 * F * n / (ms["min"] * 1e-3) / 1e9,
                                         note="8 device-to-device copies of 19 n / 8 floats each, back to back")
        del src, dst
        from rsseg.gaussian import GaussianClassifier
        gc = GaussianClassifier("ml").fit(*training_set())
        ms = event_ms(torch, ctx.torch_stream,
                      lambda: ctx.gauss_classify(planes, gc.mean_, gc.whiten_, gc.offset_, gc.class_values_, gc.max_dist2_), a.reps)
        res["gauss_ml_labels"] = dict(call_ms=ms)
    models = {}
    for name, hidden in NETWORKS.items():
        mlp, clf = fitted(hidden)
        models[name] = (mlp, clf)
        fits, tile = ctx.mlp_plan(clf.widths_, K)
        entry = dict(hidden=list(hidden), widths=clf.widths_.tolist(), tile_pixels=tile, flop_per_pixel=flop_per_pixel(clf), forms={})
        for form, (wm, wc) in FORMS.items():
            ms = event_ms(torch, ctx.torch_stream, lambda: clf._classify(ctx, planes, want_margin=wm, want_conf=wc), a.reps)
            t = ms["min"] * 1e-3
            f = dict(call_ms=ms, mpixel_per_s=n / t / 1e6, tflop_per_s=entry["flop_per_pixel"] * n / t / 1e12,
                     share_of_f32_matrix_peak=entry["flop_per_pixel"] * n / t / F32_MATRIX_PEAK, gb_per_s_read=4 * F * n / t / 1e9)
            if not a.child:
                f["times_the_copy"] = ms["min"] / res["copy_of_bytes_read"]["call_ms"]["min"]
                f["times_gauss_ml"] = ms["min"] / res["gauss_ml_labels"]["call_ms"]["min"]
            entry["forms"][form] = f
        res["networks"][name] = entry
        print(json.dumps({name: entry}), file=sys.stderr, flush=True)
    del planes
    ctx.close()
    if not a.child and not a.no_cpu:
        rng = np.random.default_rng(29)
        m = a.cpu_size * a.cpu_size
        Xp = (2.0 * rng.standard_normal((m, F), dtype=np.float32))
        for name, (mlp, clf) in models.items():
            Xs = (Xp - clf.offset_) * clf.scale_
            mlp.predict(Xs[:65536])      # warm-up
            t = time.perf_counter()
            mlp.predict(Xs)
            s = time.perf_counter() - t
            gpu = res["networks"][name]["forms"]["labels"]["call_ms"]["min"] * 1e-3
            res["networks"][name]["cpu_mlp_predict"] = dict(pixels=m, threads=os.environ.get("OMP_NUM_THREADS", "unset"), seconds=s,
                                                            mpixel_per_s=m / s / 1e6, extrapolated_seconds_at_size=s * n / m,
                                                            gpu_speedup=(s * n / m) / gpu)
    if a.valu_lib and not a.child:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", a.valu_lib, "--size", str(a.size), "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"the A/B child failed ({p.returncode}):\n{p.stderr[-2000:]}")
        child = json.loads(p.stdout.strip().splitlines()[-1])
        res["valu_variant"] = dict(library=os.path.basename(a.valu_lib), networks=child["networks"],
                                   mfma_over_valu={nm: {form: child["networks"][nm]["forms"][form]["call_ms"]["min"] / res["networks"][nm]["forms"][form]["call_ms"]["min"]
                                                        for form in FORMS} for nm in NETWORKS})
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
