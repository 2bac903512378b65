"""K22, the Gaussian maximum-likelihood / Mahalanobis / minimum-distance sweep (Context.gauss_classify), timed at the size a
user would run it: 19 float32 feature planes, k = 8 classes, --size (16384) squared pixels.

Per method ('ml', 'mahalanobis', 'mindist': models fitted by rsseg.gaussian.GaussianClassifier on seeded blobs) and per form
(labels only; + dist2; + dist2 + margin):
  in this process   device events around the call, one warm-up and then --reps calls: minimum and median;
  in a child process of its own under `rocprofv3 --kernel-trace --stats` (one child per method): the kernel's time.
Also in this process: a device-to-device copy of one plane (the bandwidth the byte counts are held against), and
scikit-learn's QuadraticDiscriminantAnalysis.predict with 16 threads on a --cpu-size (4096) squared crop, the CPU figure.

Counted from the code, per pixel and class: F subtractions, F (F + 1) / 2 + F fused multiply-adds and one addition, i.e.
F (F + 1) / 2 + 2 F + 1 float64 instructions (229 at F = 19) or F (F + 1) + 3 F + 1 floating-point operations with an fma as
two (438 at F = 19); bytes per pixel: 4 F + 1 for labels only, + 4 for each float32 output plane.  Each kernel figure is given
as float64 FLOP/s against the 78.6 TFLOP/s vector peak and as bytes/s against the measured copy; the larger of
(operations / peak) and (bytes / copy rate) is the least time the hardware could take, and `binds` names which of the two it
is.  The planes are random (a kernel with no data-dependent branch, but the clock a chip holds depends on the data).
One JSON object on stdout (and in --out).
Usage: python profiles/gauss_bench.py [--size 16384] [--cpu-size 4096] [--reps 7] [--out FILE] [--no-trace] [--no-cpu]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

F64_PEAK = 78.6e12
F, K = 19, 8
METHODS = ("ml", "mahalanobis", "mindist")
FORMS = (("labels", False, False, 0), ("labels_dist2", True, False, 1), ("labels_dist2_margin", True, True, 3))   # name, dist2, margin, MODE


def training_set(seed=22, n_per_class=4000):
    """Correlated Gaussian blobs rounded to float32: (X, y) with classes 1..K."""
    rng = np.random.default_rng(seed)
    means = 1.5 * rng.standard_normal((K, F))
    X = np.concatenate([means[j] + rng.standard_normal((n_per_class, F)) @ (rng.standard_normal((F, F)) / np.sqrt(F) + 0.6 * np.eye(F)).T
                        for j in range(K)]).astype(np.float32)
    return X, np.repeat(np.arange(1, K + 1), n_per_class)


def models():
    from rsseg.gaussian import GaussianClassifier
    X, y = training_set()
    return {m: GaussianClassifier(m).fit(X, y) for m in METHODS}


def planes_of(torch, device, n, seed=23):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return [2.0 * torch.randn(n, generator=g, device=device, dtype=torch.float32) for _ in range(F)]


def counts(n):
    instr = F * (F + 1) // 2 + 2 * F + 1
    flop = F * (F + 1) + 3 * F + 1
    return dict(f64_instructions_per_pixel_class=instr, flop_per_pixel_class=flop, flop_total=flop * K * n,
                bytes_per_pixel={name: 4 * F + 1 + 4 * (int(d) + int(m)) for name, d, m, _ in FORMS})


def rate(c, name, n, ms, copy_bps):
    s = ms * 1e-3
    bpp = c["bytes_per_pixel"][name]
    t_flop, t_bytes = c["flop_total"] / F64_PEAK, bpp * n / copy_bps
    return dict(tflop_per_s=c["flop_total"] / s / 1e12, share_of_f64_peak=c["flop_total"] / s / F64_PEAK, tb_per_s=bpp * n / s / 1e12,
                share_of_copy_rate=bpp * n / s / copy_bps, least_ms_arithmetic=t_flop * 1e3, least_ms_bytes=t_bytes * 1e3,
                binds="float64 arithmetic" if t_flop >= t_bytes else "memory traffic", share_of_bound=max(t_flop, t_bytes) / s)


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


def call(ctx, planes, clf, d, m):
    return ctx.gauss_classify(planes, clf.mean_, clf.whiten_, clf.offset_, clf.class_values_, clf.max_dist2_, want_dist2=d, want_margin=m)


def worker(method, size, reps):
    """The traced child: --reps calls of each form of one method."""
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    planes = planes_of(torch, ctx.device, size * size)
    clf = models()[method]
    for _, d, m, _ in FORMS:
        for _ in range(reps):
            call(ctx, planes, clf, d, m)
    ctx.sync()
    ctx.close()


def traced(method, size, reps, c, copy_bps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "k22", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--worker", method, "--size", str(size), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"traced run failed ({p.returncode}): {p.stderr[-2000:]}")
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        rows = [r for f in files for r in csv.DictReader(open(f))]
    out = {}
    for name, _, _, mode in FORMS:
        sel = [r for r in rows if "gauss_classify" in r["Name"] and int(r["Name"].split("<")[1].split(">")[0].split(",")[-1]) == mode]
        assert len(sel) == 1, [r["Name"] for r in rows]
        r = sel[0]
        k = dict(kernel=r["Name"].split("(")[0].replace("void ", ""), calls=int(r["Calls"]), mean_ms=float(r["AverageNs"]) / 1e6,
                 min_ms=float(r["MinNs"]) / 1e6, max_ms=float(r["MaxNs"]) / 1e6, stddev_ms=float(r["StdDev"]) / 1e6)
        k.update(rate(c, name, size * size, k["mean_ms"], copy_bps))
        out[name] = k
    return out


def cpu_qda(size):
    """QuadraticDiscriminantAnalysis.predict on size x size pixels with 16 threads: seconds, pixels per second."""
    from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis
    X, y = training_set()
    q = QuadraticDiscriminantAnalysis().fit(X.astype(np.float64), y)
    rng = np.random.default_rng(24)
    Xp = (2.0 * rng.standard_normal((size * size, F), dtype=np.float32))

    q.predict(Xp[:65536])   # warm-up

    def run():
        t = time.perf_counter()
        q.predict(Xp)
        return time.perf_counter() - t

    try:
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=16):
            s = run()
        threads = 16
    except ImportError:
        s = run()
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    return dict(pixels=size * size, threads=threads, seconds=s, mpixel_per_s=size * size / s / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--cpu-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.size, a.reps)
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    n = a.size * a.size
    c = counts(n)
    ctx = Context(0, use_dist=False)
    planes = planes_of(torch, ctx.device, n)
    dst = torch.empty_like(planes[0])
    cp = event_ms(torch, ctx.torch_stream, lambda: dst.copy_(planes[0]), a.reps)
    copy_bps = 2 * 4 * n / (cp["min"] * 1e-3)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, pixels=n, planes=F, dtype="float32", k=K, reps=a.reps,
               f64_peak_tflop_per_s=F64_PEAK / 1e12, counted=c,
               device_copy=dict(bytes=2 * 4 * n, ms=cp, tb_per_s=copy_bps / 1e12), methods={})
    del dst
    fitted = models()
    for method in METHODS:
        forms = {}
        for name, d, m, _ in FORMS:
            ms = event_ms(torch, ctx.torch_stream, lambda: call(ctx, planes, fitted[method], d, m), a.reps)
            forms[name] = dict(call_ms=ms, at_min_call_time=rate(c, name, n, ms["min"], copy_bps))
        res["methods"][method] = dict(calls=forms)
        print(json.dumps({method: forms}), file=sys.stderr, flush=True)
    ctx.close()
    del ctx, planes
    torch.cuda.empty_cache()
    if not a.no_trace:
        for method in METHODS:
            res["methods"][method]["kernels"] = traced(method, a.size, a.reps, c, copy_bps)
            print(json.dumps({method: res["methods"][method]["kernels"]}), file=sys.stderr, flush=True)
        k = res["methods"]["ml"]["kernels"]
        lab, both = k["labels"], k["labels_dist2_margin"]
        res["which_limit_binds"] = dict(
            limit=lab["binds"], kernel_ms=lab["mean_ms"], least_ms_arithmetic=lab["least_ms_arithmetic"], least_ms_bytes=lab["least_ms_bytes"],
            time_with_both_outputs_over_labels_only=both["mean_ms"] / lab["mean_ms"],
            bytes_with_both_outputs_over_labels_only=c["bytes_per_pixel"]["labels_dist2_margin"] / c["bytes_per_pixel"]["labels"],
            mindist_over_ml=res["methods"]["mindist"]["kernels"]["labels"]["mean_ms"] / lab["mean_ms"],
            reading="the kernel takes kernel_ms; the arithmetic alone needs least_ms_arithmetic at the vector peak and the bytes alone "
                    "least_ms_bytes at the measured copy rate; the two output planes add the bytes ratio but only the time ratio; "
                    "'mindist' runs the same instructions on an identity W (mindist_over_ml)")
    if not a.no_cpu:
        res["cpu_qda_predict"] = cpu_qda(a.cpu_size)
        gpu_s = res["methods"]["ml"]["calls"]["labels"]["call_ms"]["min"] * 1e-3
        res["cpu_qda_predict"]["gpu_ml_mpixel_per_s"] = n / gpu_s / 1e6
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
