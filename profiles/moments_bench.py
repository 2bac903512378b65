"""K24, the keyed Gram pass (Context.class_moments), timed at the sizes a user would run it (--size, 16384 squared pixels):

  dense19   19 float32 planes, 8 labels, every pixel counted
  kmeans15  15 float32 planes under a blocky 7-cluster map (runs of 64 pixels), label 0 ignored
  u8_7      7 uint8 planes, 8 labels
  roi       19 float32 planes, a 0.1 % ROI (runs of 1024 labelled pixels in every thousandth run), label 0 ignored
  f64k64    64 float32 planes, 64 classes drawn at random per pixel (Path B at its worst: a tile of 256 pixels holds 64 runs of
            four), --wide-size (4096) squared pixels
  f64k64b   the same planes under a blocky 64-cluster map (runs of 64 pixels: what a class map looks like)

Per case, in this process: device events around the call, one warm-up and then --reps calls (minimum and median), and the
library's own kernel timer ("class_moments": the launch without the readback).  Held against
  a device-to-device copy of as many bytes as the case reads (labels, mask and, for the tiles that hold a counted pixel, the
  planes): ratio = call time / copy time, the unit of the README's tables;
  k3_gram (the unkeyed Gram of rsseg_pca_fit_transform_f32, profiler name "gram") on 7 float32 planes of the same raster:
  time per pair-term, a pair-term being one column of one counted pixel (1 + F + F (F + 1) / 2 per pixel here, 7 + 28 there);
  np.cov per class on --cpu-size (4096) squared pixels with 16 threads: the host fit this pass replaces;
  the extrema pass (rsseg.signatures.plane_extrema), timed on its own.
--pmc DIR: instead, one `rocprofv3 --pmc` run of its own (no tracing alongside) over a child that makes --reps dense19 calls;
the counters of the class_moments kernel go to DIR/moments_pmc.json.
One JSON object on stdout (and in --out).
Usage: python profiles/moments_bench.py [--size 16384] [--wide-size 4096] [--cpu-size 4096] [--reps 7] [--out FILE] [--no-cpu]
       python profiles/moments_bench.py --pmc DIR [--size 16384] [--reps 3]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CASES = ("dense19", "kmeans15", "u8_7", "roi", "f64k64", "f64k64b")
PMC = ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_BUSY_CYCLES")


def make_case(torch, device, name, n, seed=24):
    """(planes, labels, n_classes, plane_exp, Q, ignore, counted pixels, bytes read)"""
    from rsseg.signatures import q_for
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    idx = torch.arange(n, device=device, dtype=torch.int64)
    F = {"dense19": 19, "kmeans15": 15, "u8_7": 7, "roi": 19, "f64k64": 64, "f64k64b": 64}[name]
    if name == "u8_7":
        planes = [torch.randint(0, 256, (n,), generator=g, device=device, dtype=torch.uint8) for _ in range(F)]
        pe, Q = None, 0
    else:
        planes = [torch.rand(n, generator=g, device=device, dtype=torch.float32) * 2.0 - 1.0 for _ in range(F)]
        pe, Q = [0] * F, q_for(n)
    if name in ("dense19", "u8_7"):
        labels, k, ignore = torch.randint(0, 8, (n,), generator=g, device=device, dtype=torch.uint8), 8, -1
    elif name == "kmeans15":
        labels, k, ignore = ((((idx >> 6) * 2654435761) >> 13) % 7 + 1).to(torch.uint8), 8, 0
    elif name == "roi":
        labels, k, ignore = torch.where((idx >> 10) % 1000 == 0, ((idx >> 10) // 1000) % 8 + 1, 0).to(torch.uint8), 9, 0
    elif name == "f64k64b":
        labels, k, ignore = ((((idx >> 6) * 2654435761) >> 13) % 64).to(torch.uint8), 64, -1
    else:
        labels, k, ignore = torch.randint(0, 64, (n,), generator=g, device=device, dtype=torch.uint8), 64, -1
    counted = int((labels != ignore).sum().item()) if ignore >= 0 else n
    elem = 1 if name == "u8_7" else 4
    plane_bytes = elem * F * (n if name != "roi" else counted)   # a tile without a counted pixel reads no plane
    return planes, labels, k, pe, Q, ignore, counted, n + plane_bytes


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


def copy_ms(torch, ctx, nbytes, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device).zero_()
    dst = torch.empty_like(src)
    return event_ms(torch, ctx.torch_stream, lambda: dst.copy_(src), reps)


def prof_ms(ctx, name, fn, reps):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for _ in range(reps):
            fn()
        ms, calls = ctx.prof_get(name)
    finally:
        ctx.prof_enable(False)
    return ms / max(calls, 1)


def cpu_cov(size, F=19, k=8):
    """np.cov of every class on size x size pixels of F float32 planes, gathered the way GaussianClassifier.fit does."""
    rng = np.random.default_rng(25)
    n = size * size
    X = rng.random((n, F), dtype=np.float32)
    y = rng.integers(0, k, n)

    def run():
        t = time.perf_counter()
        for c in range(k):
            np.cov(X[y == c].astype(np.float64), rowvar=False)
        return time.perf_counter() - t

    try:
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=16):
            s = run()
        threads = 16
    except ImportError:
        s = run()
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
    return dict(pixels=n, planes=F, classes=k, threads=threads, seconds=s, mpixel_per_s=n / s / 1e6)


def worker(name, size, reps):
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    planes, labels, k, pe, Q, ignore, _, _ = make_case(torch, ctx.device, name, size * size)
    for _ in range(reps):
        ctx.class_moments(planes, labels, k, pe, Q, ignore=ignore)
    ctx.sync()
    ctx.close()


def pmc(outdir, size, reps):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--pmc", *PMC, "-d", os.path.join(outdir, "pmc"), "-o", "m", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--worker", "dense19", "--size", str(size), "--reps", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"counter run failed ({p.returncode}): {p.stderr[-2000:]}")
    tot, launches = {}, 0
    for f in glob.glob(os.path.join(outdir, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "class_moments<" in r["Kernel_Name"]:
                tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                launches += r["Counter_Name"] == PMC[0]
    w = max(tot.get("SQ_WAVES", 0.0), 1.0)
    res = dict(case="dense19", size=size, launches=launches, counters=tot, valu_insts_per_wave=tot.get("SQ_INSTS_VALU", 0) / w,
               lds_insts_per_wave=tot.get("SQ_INSTS_LDS", 0) / w,
               valu_active_per_wave_cycle=tot.get("SQ_ACTIVE_INST_VALU", 0) / max(tot.get("SQ_WAVE_CYCLES", 1), 1),   # both in quad-cycles
               wait_inst_any_per_wave_cycle=tot.get("SQ_WAIT_INST_ANY", 0) / max(tot.get("SQ_WAVE_CYCLES", 1), 1))
    # VALU busy of a launch that took `ms`: 4 * SQ_ACTIVE_INST_VALU / launches / (ms * 1e-3 * 2.4 GHz * 1024 SIMDs)
    with open(os.path.join(outdir, "moments_pmc.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--wide-size", type=int, default=4096)
    ap.add_argument("--cpu-size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--worker", default="")
    ap.add_argument("--pmc", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.size, a.reps)
    if a.pmc:
        return pmc(a.pmc, a.size, a.reps)
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    from rsseg.signatures import n_columns, plane_extrema
    ctx = Context(0, use_dist=False)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, wide_size=a.wide_size, reps=a.reps, cases={})
    for name in a.cases.split(","):
        size = a.wide_size if name.startswith("f64k64") else a.size
        n = size * size
        planes, labels, k, pe, Q, ignore, counted, nbytes = make_case(torch, ctx.device, name, n)
        F = len(planes)
        call = lambda: ctx.class_moments(planes, labels, k, pe, Q, ignore=ignore)   # noqa: E731
        ms = event_ms(torch, ctx.torch_stream, call, a.reps)
        kernel = prof_ms(ctx, "class_moments", call, a.reps)
        cp = copy_ms(torch, ctx, nbytes, a.reps)
        terms = counted * n_columns(F)
        c = dict(size=size, pixels=n, planes=F, classes=k, path=ctx.class_moments_plan(F, k)[0], tile=ctx.class_moments_plan(F, k)[1], Q=Q,
                 counted_pixels=counted, bytes_read=nbytes, call_ms=ms, kernel_ms=kernel, copy_of_bytes_read_ms=cp,
                 ratio_to_copy=ms["min"] / cp["min"], pair_terms=terms, ps_per_pair_term=kernel * 1e9 / max(terms, 1))
        if name == "dense19":
            ext = event_ms(torch, ctx.torch_stream, lambda: plane_extrema(ctx, planes), 5)
            c["extrema_pass_ms"] = ext
            seven = planes[:7]
            gram = prof_ms(ctx, "gram", lambda: ctx.pca_fit_transform(seven, None, None, 3), 5)
            c["k3_gram_7_planes"] = dict(kernel_ms=gram, pair_terms=n * 35, ps_per_pair_term=gram * 1e9 / (n * 35))
        res["cases"][name] = c
        print(json.dumps({name: c}), file=sys.stderr, flush=True)
        del planes, labels
        torch.cuda.empty_cache()
    ctx.close()
    if not a.no_cpu:
        res["cpu_np_cov_per_class"] = cpu_cov(a.cpu_size)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
