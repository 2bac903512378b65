"""K25, the object-table pass (Context.segment_features), timed at the size a user would run it (--size, 16384 squared pixels)
under a SLIC map of step 16 (Context.slic_u8 on seven blocky uint8 planes, --slic-iterations assignment iterations):

  u8_7      7 uint8 planes
  f32_15    15 float32 planes, uniform in [-1, 1)
  each with and without the geometry columns, and
  overflow  one segment per pixel on --overflow-size (1024) squared pixels, 7 uint8 planes: every tile meets 1024 labels for the
            64 rows of its LDS table, so nearly every run is committed straight to the global table

Per case, in this process: device events around the call, one warm-up and then --reps calls (minimum and median), and the
library's own kernel timer ("segment_features": the table's initialisation and the pass, without the readback).  Held against
  Context.segment_sums on the same segment map and planes (rsseg_segment_sums, unchanged since K23: one column per plane where
  this pass fills four, and no geometry beyond the centroid), profiler name "segment_sums";
  a device-to-device copy of as many bytes as the case reads (the label plane and the planes): ratio = call time / copy time.
--pmc DIR [--pmc-case f32_15 | overflow]: instead, one `rocprofv3 --pmc` run of its own (no tracing alongside) over a child that
makes --reps calls of that case; the counters of the k25_features kernel go to DIR/object_features_pmc_<case>.json.
One JSON object on stdout (and in --out).
Usage: python profiles/object_features_bench.py [--size 16384] [--overflow-size 1024] [--reps 7] [--out FILE]
       python profiles/object_features_bench.py --pmc DIR [--pmc-case f32_15] [--size 16384] [--reps 3]"""
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

STEP = 16
PMC = ("SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "SQ_BUSY_CYCLES")


def blocky_u8(torch, g, device, size, cell):
    """a uint8 plane of cell x cell blocks of one grey level, a tenth of the pixels redrawn: regions, edges and speckle"""
    c = -(-size // cell)
    coarse = torch.randint(0, 6, (c, c), generator=g, device=device, dtype=torch.uint8) * 50
    p = coarse.repeat_interleave(cell, 0).repeat_interleave(cell, 1)[:size, :size].contiguous()
    flip = torch.rand((size, size), generator=g, device=device) < 0.1
    p[flip] = torch.randint(0, 256, (int(flip.sum().item()),), generator=g, device=device, dtype=torch.uint8)
    return p.reshape(-1)


def make_scene(torch, ctx, size, slic_iterations, seed=25):
    """(segment plane int32, n_segments, 7 uint8 planes, 15 float32 planes)"""
    g = torch.Generator(device=ctx.device)
    g.manual_seed(seed)
    u8 = [blocky_u8(torch, g, ctx.device, size, 24 + 8 * (i % 3)) for i in range(7)]
    seg, ns, _, _ = ctx.slic_u8(u8, size, size, STEP, (10.0 / STEP) ** 2, slic_iterations, STEP * STEP // 4)
    f32 = [torch.rand(size * size, generator=g, device=ctx.device, dtype=torch.float32) * 2.0 - 1.0 for _ in range(15)]
    return seg, ns, u8, f32


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


def time_case(torch, ctx, seg, size, ns, planes, reps, with_sums=True):
    elem = planes[0].element_size()
    nbytes = size * size * (4 + elem * len(planes))
    out = dict(size=size, pixels=size * size, n_segments=ns, planes=len(planes), dtype="uint8" if elem == 1 else "float32", bytes_read=nbytes,
               table_columns=11 + 4 * len(planes))
    for geo in (True, False):
        call = lambda: ctx.segment_features(seg, size, size, ns, planes, geometry=geo)   # noqa: E731
        ms = event_ms(torch, ctx.torch_stream, call, reps)
        out["geometry" if geo else "no_geometry"] = dict(call_ms=ms, kernel_ms=prof_ms(ctx, "segment_features", call, reps))
    cp = copy_ms(torch, ctx, nbytes, reps)
    out["copy_of_bytes_read_ms"] = cp
    out["ratio_to_copy"] = {k: out[k]["call_ms"]["min"] / cp["min"] for k in ("geometry", "no_geometry")}
    if with_sums:
        sums = lambda: ctx.segment_sums(seg, size, size, ns, planes)   # noqa: E731
        sm = event_ms(torch, ctx.torch_stream, sums, reps)
        out["segment_sums"] = dict(call_ms=sm, kernel_ms=prof_ms(ctx, "segment_sums", sums, reps))
        out["ratio_to_segment_sums"] = {k: out[k]["call_ms"]["min"] / sm["min"] for k in ("geometry", "no_geometry")}
    return out


def make_overflow(torch, ctx, size, seed=26):
    """(one segment per pixel in random order, 7 uint8 planes)"""
    g = torch.Generator(device=ctx.device)
    g.manual_seed(seed)
    n = size * size
    own = (torch.randperm(n, generator=g, device=ctx.device) + 1).to(torch.int32)
    return own, [torch.randint(0, 256, (n,), generator=g, device=ctx.device, dtype=torch.uint8) for _ in range(7)]


def worker(case, size, reps, slic_iterations):
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    if case == "overflow":
        seg, planes = make_overflow(torch, ctx, size)
        ns = size * size
    else:
        seg, ns, _, planes = make_scene(torch, ctx, size, slic_iterations)
    for _ in range(reps):
        ctx.segment_features(seg, size, size, ns, planes)
    ctx.sync()
    ctx.close()


def pmc(outdir, case, size, reps, slic_iterations, counters=PMC):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--pmc", *counters, "-d", os.path.join(outdir, "pmc_" + case), "-o", "o", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--worker", case, "--size", str(size), "--reps", str(reps), "--slic-iterations", str(slic_iterations)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"counter run failed ({p.returncode}): {p.stderr[-2000:]}")
    tot, launches = {}, 0
    for f in glob.glob(os.path.join(outdir, "pmc_" + case, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k25_features" in r["Kernel_Name"]:
                tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                launches += r["Counter_Name"] == counters[0]
    w = max(tot.get("SQ_WAVES", 0.0), 1.0)
    cyc = max(tot.get("SQ_WAVE_CYCLES", 1.0), 1.0)
    res = dict(case=case, size=size, launches=launches, counters=tot, valu_insts_per_wave=tot.get("SQ_INSTS_VALU", 0) / w,
               lds_insts_per_wave=tot.get("SQ_INSTS_LDS", 0) / w, valu_active_per_wave_cycle=tot.get("SQ_ACTIVE_INST_VALU", 0) / cyc,
               wait_inst_any_per_wave_cycle=tot.get("SQ_WAIT_INST_ANY", 0) / cyc)
    with open(os.path.join(outdir, f"object_features_pmc_{case}.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--overflow-size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slic-iterations", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--pmc", default="")
    ap.add_argument("--pmc-case", default="f32_15", choices=["f32_15", "overflow"])
    ap.add_argument("--pmc-counters", default=",".join(PMC), help="the counters of the run (one pass: keep them few)")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.size, a.reps, a.slic_iterations)
    if a.pmc:
        return pmc(a.pmc, a.pmc_case, a.overflow_size if a.pmc_case == "overflow" else a.size, a.reps, a.slic_iterations,
                   tuple(a.pmc_counters.split(",")))
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    tw, th, slots = ctx.segment_features_plan(15)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, step=STEP, reps=a.reps, tile=[tw, th], lds_slots=slots, cases={})
    seg, ns, u8, f32 = make_scene(torch, ctx, a.size, a.slic_iterations)
    area = torch.bincount(seg.to(torch.int64))[1:]
    res["segments"] = dict(n=ns, area_min=int(area.min()), area_median=float(area.float().median()), area_max=int(area.max()),
                           slic_iterations=a.slic_iterations)
    for name, planes in (("u8_7", u8), ("f32_15", f32)):
        res["cases"][name] = time_case(torch, ctx, seg, a.size, ns, planes, a.reps)
        print(json.dumps({name: res["cases"][name]}), file=sys.stderr, flush=True)
    del seg, f32, u8
    torch.cuda.empty_cache()
    own, planes = make_overflow(torch, ctx, a.overflow_size)
    res["cases"]["overflow"] = time_case(torch, ctx, own, a.overflow_size, a.overflow_size * a.overflow_size, planes, a.reps)
    print(json.dumps({"overflow": res["cases"]["overflow"]}), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
