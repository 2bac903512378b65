"""K26, the fused ISODATA sweep (Context.isodata_sweep), timed at the size a user would run it (--size, 16384 squared pixels):

  f15k8     15 float32 planes, 8 centres
  f19k32    19 float32 planes, 32 centres
  u8_7k8    7 uint8 planes, 8 centres
  f15k8_labels   the labels-only form of f15k8 (IsodataModel.predict)

Per case, in this process: device events around the call, one warm-up and then --reps calls (minimum, median and the spread
(max - min) / min), and the library's own kernel timer ("isodata_sweep": the launch without the readback).  Held against
  (a) a device-to-device copy of as many bytes as the case reads (the planes and the label plane): ratio_to_copy;
  (b) the route there was before this kernel: Context.kmeans_predict with its summary (K18: labels and counts from float32
      distances) followed by Context.class_moments on those labels over the same planes (K24: the full triangle); uint8 planes
      are widened first (Context.widen_u8), since K18 takes none: ratio_to_composed = composed / sweep.
--pmc DIR: instead, one `rocprofv3 --pmc` run of its own (no tracing alongside) over a child that makes --reps calls of
--pmc-case; the counters of the isodata_sweep kernel go to DIR/isodata_pmc.json.
One JSON object on stdout (and in --out).
Usage: python profiles/isodata_bench.py [--size 16384] [--reps 7] [--out FILE]
       python profiles/isodata_bench.py --pmc DIR [--pmc-case f19k32] [--size 16384] [--reps 3]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CASES = {"f15k8": (15, 8, False, True), "f19k32": (19, 32, False, True), "u8_7k8": (7, 8, True, True), "f15k8_labels": (15, 8, False, False)}
PMC = ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_BUSY_CYCLES")


def make_case(torch, device, name, n, seed=26):
    """(planes, labels, centers, weight, plane_exp, Q, want_table, bytes read)"""
    from rsseg.signatures import q_for
    F, k, u8, want_table = CASES[name]
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    if u8:
        planes = [torch.randint(0, 256, (n,), generator=g, device=device, dtype=torch.uint8) for _ in range(F)]
        pe, Q, weight = None, 0, np.full(F, float(np.float32(1.0 / 255.0)))
        centers = rng.uniform(0.1, 0.9, (k, F))
    else:
        planes = [torch.rand(n, generator=g, device=device, dtype=torch.float32) * 2.0 - 1.0 for _ in range(F)]
        pe, Q, weight = [0] * F, q_for(n), np.full(F, 0.5)
        centers = rng.uniform(-0.4, 0.4, (k, F))
    centers = centers.astype(np.float32).astype(np.float64)   # K18 takes a model that float32 holds
    labels = torch.full((n,), 255, device=device, dtype=torch.uint8)
    return planes, labels, centers, weight, pe, Q, want_table, n + (1 if u8 else 4) * F * n


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
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), spread=float((np.max(ms) - np.min(ms)) / np.min(ms)),
                runs=[float(x) for x in ms])


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


def composed(torch, ctx, planes, centers, weight, pe, Q, u8):
    """K18 then K24: what gave labels, counts and moments before the fused sweep.  The k-means model that assigns in the same
    space: MinMaxScaler scale_ = weight (times 255 / 255 for bytes), min_ = 0."""
    k = centers.shape[0]

    def run():
        fl = [ctx.widen_u8(p) for p in planes] if u8 else planes
        labels, _, summary = ctx.kmeans_predict(fl, centers, weight, np.zeros(len(planes)), want_summary=True)
        ctx.class_moments(planes, labels, k, pe, Q)
        return summary
    return run


def worker(name, size, reps):
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    planes, labels, centers, weight, pe, Q, want_table, _ = make_case(torch, ctx.device, name, size * size)
    for _ in range(reps):
        ctx.isodata_sweep(planes, labels, centers, weight, pe, Q, want_table=want_table)
    ctx.sync()
    ctx.close()


def pmc(outdir, name, size, reps):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--pmc", *PMC, "-d", os.path.join(outdir, "pmc"), "-o", "m", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--worker", name, "--size", str(size), "--reps", str(reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"counter run failed ({p.returncode}): {p.stderr[-2000:]}")
    tot, launches = {}, 0
    for f in glob.glob(os.path.join(outdir, "pmc", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "isodata_sweep<" in r["Kernel_Name"]:
                tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                launches += r["Counter_Name"] == PMC[0]
    w = max(tot.get("SQ_WAVES", 0.0), 1.0)
    res = dict(case=name, size=size, launches=launches, counters=tot, valu_insts_per_wave=tot.get("SQ_INSTS_VALU", 0) / w,
               lds_insts_per_wave=tot.get("SQ_INSTS_LDS", 0) / w,
               valu_active_per_wave_cycle=tot.get("SQ_ACTIVE_INST_VALU", 0) / max(tot.get("SQ_WAVE_CYCLES", 1), 1),   # both in quad-cycles
               wait_inst_any_per_wave_cycle=tot.get("SQ_WAIT_INST_ANY", 0) / max(tot.get("SQ_WAVE_CYCLES", 1), 1))
    with open(os.path.join(outdir, "isodata_pmc.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--worker", default="")
    ap.add_argument("--pmc", default="")
    ap.add_argument("--pmc-case", default="f19k32")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.size, a.reps)
    if a.pmc:
        return pmc(a.pmc, a.pmc_case, a.size, a.reps)
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    n = a.size * a.size
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, pixels=n, reps=a.reps, cases={})
    for name in a.cases.split(","):
        F, k, u8, want_table = CASES[name]
        planes, labels, centers, weight, pe, Q, _, nbytes = make_case(torch, ctx.device, name, n)
        call = lambda: ctx.isodata_sweep(planes, labels, centers, weight, pe, Q, want_table=want_table)   # noqa: E731
        ms = event_ms(torch, ctx.torch_stream, call, a.reps)
        kernel = prof_ms(ctx, "isodata_sweep", call, a.reps)
        cp = copy_ms(torch, ctx, nbytes, a.reps)
        c = dict(planes=F, centres=k, dtype="uint8" if u8 else "float32", table=want_table, path=ctx.isodata_plan(F, k, u8)[0],
                 tile=ctx.isodata_plan(F, k, u8)[1], Q=Q, bytes_read=nbytes, call_ms=ms, kernel_ms=kernel, copy_of_bytes_read_ms=cp,
                 ratio_to_copy=ms["min"] / cp["min"], ns_per_pixel=kernel * 1e6 / n,
                 float64_ops_per_pixel=3 * k * F)
        if want_table:
            comp = composed(torch, ctx, planes, centers, weight, pe, Q, u8)
            summary = comp()
            table, _, _ = call()
            # the two routes count alike wherever the float32 distances of K18 rank the centres as the float64 ones do
            c["pixels_counted_differently_by_k18"] = int(np.abs(summary["counts"] - table[:, 0].cpu().numpy()).sum() // 2)
            cm = event_ms(torch, ctx.torch_stream, comp, a.reps)
            c["composed_k18_k24_ms"] = cm
            c["ratio_to_composed"] = cm["min"] / ms["min"]
        res["cases"][name] = c
        print(json.dumps({name: c}), file=sys.stderr, flush=True)
        del planes, labels
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
