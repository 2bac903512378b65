"""K28, the support vector machine sweep (Context.svm_classify), timed on 19 float32 feature planes and k = 8 classes.

Models: sklearn.svm.SVC fitted through rsseg.svm.SVMClassifier on seeded overlapping blobs, the training size chosen so that
the RBF models come out near 500 and near 2000 support vectors; polynomial (degree 3, coef0 1) and linear on the larger set.
The cost of a pixel is S x F, so one size does not fit every model inside a run's time limit: per model the
largest of --sizes (16384, 8192, 4096, 2048, squared) whose call, extrapolated from a 1024 x 1024 probe, stays under
--call-budget seconds is timed, and the size used is recorded with the probe it was chosen from.
Per model: device events around the call (model upload included), one warm-up and --reps calls: minimum and median; Mpixel/s;
the share of the 78.6 TFLOP/s float64 vector peak under the operation count below.
Operations per pixel and support vector, an fma as two (counted from csrc/k28_svm.hip):
  rbf     F subtractions + F fma + gamma * q + [t * LOG2E, rint, 2 fma, 13 fma, p * 2^n] + (k - 1) fma = 3 F + 34 + 2 (k - 1)
  poly    F fma + fma(gamma, t, coef0) + (degree - 1) products + (k - 1) fma                           = 2 F + 2 + (degree - 1) + 2 (k - 1)
and per pixel 2 F for the scaling; linear has no support-vector loop: per pixel P (2 F + 1) + 2 F, P = k (k - 1) / 2.
For scale: SVC.predict of the same RBF models on a --cpu-size (512) squared crop on the host, extrapolated to the timed size.
One JSON object on stdout (and in --out).
Usage: python profiles/svm_bench.py [--sizes 16384,8192,4096,2048] [--call-budget 10] [--reps 3] [--cpu-size 512] [--out FILE] [--no-cpu] [--models rbf_s500,...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

F64_PEAK = 78.6e12
F, K = 19, 8
PROBE = 1024
# name -> (kernel, training samples per class)
MODELS = {"rbf_s500": ("rbf", 75), "rbf_s2000": ("rbf", 375), "poly3": ("poly", 375), "linear": ("linear", 375)}


def training_set(n_per_class, seed=28):
    """Correlated Gaussian blobs that overlap (means 0.6 spreads apart), rounded to float32: (X, y) with classes 1..K."""
    rng = np.random.default_rng(seed)
    means = 0.6 * rng.standard_normal((K, F))
    X = np.concatenate([means[j] + rng.standard_normal((n_per_class, F)) @ (rng.standard_normal((F, F)) / np.sqrt(F) + 0.6 * np.eye(F)).T
                        for j in range(K)]).astype(np.float32)
    return X, np.repeat(np.arange(1, K + 1), n_per_class)


def model(name):
    from rsseg.svm import SVMClassifier
    kernel, n_per_class = MODELS[name]
    X, y = training_set(n_per_class)
    return SVMClassifier(kernel, degree=3, coef0=1.0 if kernel == "poly" else 0.0).fit(X, y)


def flop_per_pixel(clf):
    S, k = clf.support_vectors_.shape[0], clf.classes_.size
    if clf.kernel == "linear":
        return k * (k - 1) // 2 * (2 * F + 1) + 2 * F
    per_sv = 3 * F + 34 + 2 * (k - 1) if clf.kernel == "rbf" else 2 * F + 2 + (clf.degree - 1) + 2 * (k - 1)
    return S * per_sv + 2 * F


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


def cpu_predict(clf, n_per_class, size):
    """sklearn's SVC.predict (the same model, trained again) on size x size standardised pixels: seconds."""
    from sklearn.svm import SVC
    X, y = training_set(n_per_class)
    svc = SVC(kernel=clf.kernel).fit((X.astype(np.float64) - clf.offset_) * clf.scale_, y)
    assert svc.support_vectors_.shape == clf.support_vectors_.shape
    rng = np.random.default_rng(29)
    Xp = 2.0 * rng.standard_normal((size * size, F))
    svc.predict(Xp[:4096])   # warm-up
    t = time.perf_counter()
    svc.predict(Xp)
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: sorted((int(v) for v in s.split(",")), reverse=True), default=[16384, 8192, 4096, 2048])
    ap.add_argument("--call-budget", type=float, default=10.0, help="seconds one timed call may take")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-size", type=int, default=512)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--models", type=lambda s: s.split(","), default=list(MODELS), help="a subset of " + ",".join(MODELS))
    a = ap.parse_args()
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(23)
    n_max = max(a.sizes) ** 2
    planes = [2.0 * torch.randn(n_max, generator=g, device=ctx.device, dtype=torch.float32) for _ in range(F)]
    res = dict(device=torch.cuda.get_device_name(0), planes=F, dtype="float32", k=K, reps=a.reps, f64_peak_tflop_per_s=F64_PEAK / 1e12,
               sizes_offered=a.sizes, call_budget_s=a.call_budget, models={})
    for name in a.models:
        clf = model(name)
        call = lambda n: clf._classify(ctx, [p[:n] for p in planes], False)   # noqa: E731
        probe = event_ms(torch, ctx.torch_stream, lambda: call(PROBE * PROBE), 2)["min"]
        fit = [s for s in a.sizes if probe * 1e-3 * (s / PROBE) ** 2 <= a.call_budget]
        size = fit[0] if fit else min(a.sizes)
        n = size * size
        ms = event_ms(torch, ctx.torch_stream, lambda: call(n), a.reps)
        flop = flop_per_pixel(clf) * n
        entry = dict(kernel=clf.kernel, support_vectors=int(clf.support_vectors_.shape[0]), n_support=clf.n_support_.tolist(), gamma=clf.gamma_,
                     probe_1024_ms=probe, size=size, pixels=n,
                     size_note=("the largest offered size" if size == max(a.sizes) else
                                f"{max(a.sizes)} squared would take about {probe * 1e-3 * (max(a.sizes) / PROBE) ** 2:.0f} s a call, over the budget"),
                     call_ms=ms, mpixel_per_s=n / (ms["min"] * 1e-3) / 1e6, flop_per_pixel=flop_per_pixel(clf), flop_total=flop,
                     tflop_per_s=flop / (ms["min"] * 1e-3) / 1e12, share_of_f64_peak=flop / (ms["min"] * 1e-3) / F64_PEAK)
        if not a.no_cpu and clf.kernel == "rbf":
            s = cpu_predict(clf, MODELS[name][1], a.cpu_size)
            entry["cpu_svc_predict"] = dict(pixels=a.cpu_size ** 2, seconds=s, mpixel_per_s=a.cpu_size ** 2 / s / 1e6,
                                            extrapolated_seconds_at_size=s * n / a.cpu_size ** 2, gpu_speedup=(s * n / a.cpu_size ** 2) / (ms["min"] * 1e-3))
        res["models"][name] = entry
        print(json.dumps({name: entry}), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
