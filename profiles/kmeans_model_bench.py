"""K18, the sweep of a fitted KMeans model (Context.kmeans_predict), timed on the planes a user would run it on:
  c3    the 15 float32 planes of config 3 (7 indices, 3 PCA components, 5 GLCM textures; k = 8) at --size3 (16384) squared
  s19   the 19-plane stack (feature_stack19) as float64 (k = 7) at --size19 (8192) squared
The model of each workload comes from one kmeans_fit_predict on the same planes.

Per workload, in this process: the three forms of the sweep (labels only; labels + distance plane; labels + distance +
summary) with device events around the call, one warm-up call and then --reps calls each: minimum and median.
Then, in a child process of its own under `rocprofv3 --kernel-trace --stats`: --reps fits (max_iter=2, so that every fit ends
with the final E-step kernel, km_lloyd<..., false>) and --reps calls of each form, and from the kernel statistics the time of
the sweep's kernels beside that final E-step kernel, the kernel the labels-only form moves the same bytes as.
Every kernel figure is also given as bytes per pixel over kernel time and as a share of the 8 TB/s HBM peak, which bounds it:
F * sizeof(T) + 4 bytes per pixel for labels only, + sizeof(T) with the distance plane (computed here from the shapes).
One JSON object on stdout (and in --out).
Usage: python profiles/kmeans_model_bench.py [--size3 16384] [--size19 8192] [--reps 7] [--out FILE] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12
FORMS = (("labels", False, False), ("labels_distance", True, False), ("labels_distance_summary", True, True))


def planes_of(ctx, torch, which, size):
    """-> (planes, k, dtype name)"""
    import bench
    from rsseg import pipeline as P
    bands = bench.synth_rows(torch, ctx.device, size, 0, size)
    if which == "c3":
        _, _, planes = P.config3(ctx, bands, size, size, 8, 7, 1, 3, size * size)
        return list(planes), 8, "float32"
    planes, _ = P.feature_stack19(ctx, bands, size, size, n_global=size * size)
    return [p.double() for p in planes], 7, "float64"


def bytes_per_pixel(F, itemsize):
    return {"labels": F * itemsize + 4, "labels_distance": F * itemsize + 4 + itemsize, "labels_distance_summary": F * itemsize + 4 + itemsize}


def rate(bpp, n, ms):
    bps = bpp * n / (ms * 1e-3)
    return dict(bytes_per_pixel=bpp, tb_per_s=bps / 1e12, share_of_hbm_peak=bps / HBM_PEAK)


def fit_model(ctx, planes, k):
    _, meta = ctx.kmeans_fit_predict(planes, k, max_iter=2)
    return meta["centers"], meta["scale"], meta["min"]


def timed(ctx, torch, which, size, reps):
    planes, k, dt = planes_of(ctx, torch, which, size)
    n, F, item = planes[0].numel(), len(planes), planes[0].element_size()
    model = fit_model(ctx, planes, k)
    bpp = bytes_per_pixel(F, item)
    out = dict(planes=F, dtype=dt, k=k, pixels=n, forms={})
    for name, want_d, want_s in FORMS:
        ms = []
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(ctx.torch_stream):
                a.record()
                ctx.kmeans_predict(planes, *model, want_distance=want_d, want_summary=want_s)
                b.record()
            b.synchronize()
            if r:
                ms.append(a.elapsed_time(b))
        out["forms"][name] = dict(call_ms=dict(min=float(np.min(ms)), median=float(np.median(ms)), runs=[float(x) for x in ms]),
                                  **{"at_min_call_time": rate(bpp[name], n, float(np.min(ms)))})
    return out


def worker(which, size, reps):
    """The traced child: fits and sweeps, nothing printed but the shapes."""
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    planes, k, dt = planes_of(ctx, torch, which, size)
    for _ in range(reps):
        model = fit_model(ctx, planes, k)
    for name, want_d, want_s in FORMS:
        for _ in range(reps):
            ctx.kmeans_predict(planes, *model, want_distance=want_d, want_summary=want_s)
    ctx.sync()
    print(json.dumps(dict(planes=len(planes), itemsize=planes[0].element_size(), pixels=planes[0].numel())))
    ctx.close()


def traced(which, size, reps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "k18", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--worker", which, "--size", str(size), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError(f"traced run failed ({p.returncode}): {p.stderr[-2000:]}")
        shape = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        rows = [r for f in files for r in csv.DictReader(open(f))]
    F, item, n = shape["planes"], shape["itemsize"], shape["pixels"]
    bpp = bytes_per_pixel(F, item)

    def pick(pred):
        sel = [r for r in rows if pred(r["Name"])]
        assert len(sel) == 1, [r["Name"] for r in sel]
        r = sel[0]
        return dict(kernel=r["Name"].split("(")[0].replace("void ", ""), calls=int(r["Calls"]), mean_ms=float(r["AverageNs"]) / 1e6,
                    min_ms=float(r["MinNs"]) / 1e6, max_ms=float(r["MaxNs"]) / 1e6, stddev_ms=float(r["StdDev"]) / 1e6)

    def mode_of(name):      # km_apply<T, KMAX, FR, MODE> / km_apply_blk<T, KMAX, MODE>: the last template argument
        return int(name.split("<")[1].split(">")[0].split(",")[-1])

    base = pick(lambda s: "km_lloyd" in s and "false>" in s)
    base.update(rate(bpp["labels"], n, base["mean_ms"]))
    base["spread_of_mean"] = (base["max_ms"] - base["min_ms"]) / base["mean_ms"]
    out = dict(final_e_step=base, forms={})
    for name, mode in (("labels", 0), ("labels_distance", 1), ("labels_distance_summary", 3)):
        k = pick(lambda s: "km_apply" in s and mode_of(s) == mode)
        k.update(rate(bpp[name], n, k["mean_ms"]))
        k["over_final_e_step"] = k["mean_ms"] / base["mean_ms"]
        out["forms"][name] = k
    lab, dist = out["forms"]["labels"], out["forms"]["labels_distance"]
    out["labels_within_baseline_spread"] = bool(lab["mean_ms"] <= base["max_ms"])
    out["distance_over_labels"] = dict(time_ratio=dist["mean_ms"] / lab["mean_ms"], byte_ratio=bpp["labels_distance"] / bpp["labels"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size3", type=int, default=16384)
    ap.add_argument("--size19", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--worker", default="")
    ap.add_argument("--size", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.size, a.reps)
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    res = dict(device=torch.cuda.get_device_name(0), hbm_peak_tb_per_s=HBM_PEAK / 1e12, reps=a.reps,
               note="every form is bounded by HBM: bytes per pixel = F * sizeof(T) + 4 (labels), + sizeof(T) with the distance plane", workloads={})
    for which, size in (("c3", a.size3), ("s19", a.size19)):
        ctx = Context(0, use_dist=False)
        w = timed(ctx, torch, which, size, a.reps)
        ctx.close()
        del ctx
        torch.cuda.empty_cache()
        w["size"] = size
        if not a.no_trace:
            w["kernels"] = traced(which, size, a.reps)
        res["workloads"][which] = w
        print(json.dumps({which: w}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
