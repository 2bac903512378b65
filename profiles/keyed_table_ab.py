#!/usr/bin/env python3
"""The keyed-table kernels (csrc/k23_slic.hip segment sums, k24_moments.hip, k25_objects.hip, k26_isodata.hip,
k27_adjacency.hip), two builds of the library against each other, in the manner of profiles/forest_shared_steps_ab.py: the
same inputs for both, each build in a process of its own, the builds alternating for several rounds, HIP-event time per
launch from the context's profiler, every output hashed so that the builds are also compared bit for bit.

One case per kernel instantiation that a device helper of an earlier build of csrc/keyed_table.h changed (profiler family in
brackets; DESIGN.md section 5 says which helpers those were and why the committed kernels have the steps written out and
the parent's instructions).  The builders are those of moments_bench.py, isodata_bench.py and object_features_bench.py; the
adjacency and segment-sum cases run on the scene and the overflow raster of object_features_bench.py:
  mo-*    [class_moments]   float32 / uint8 planes x uint8 / int32 labels; F = 19 and 7 with 8 classes on Path A (the table in
                            LDS), F = 64 with 64 classes on Path B, --size squared pixels (Path B: --wide-size)
  iso-*   [isodata_sweep]   with a table: F = 7, 15, 19, 32 and 64 (the five register widths) on Path A, F = 19 / k = 32 among
                            them, and F = 64 / k = 64 on Path B, both plane types
  obj-*   [segment_features] the SLIC scene of object_features_bench.py (--scene-size), 7 uint8 / 15 float32 planes, with and
                            without geometry; obj-overflow: one segment per pixel, the LDS table always full
  adj-*   [segment_adjacency] the same scene with 7 planes; adj-overflow: one segment per pixel
  sums-*  [segment_sums]    the same scene, 7 uint8 / 15 float32 planes
  compact-plan [compact_plan] rsseg_compact_plan of a 70 % mask over --size squared pixels (k19_scan, behind wave_incl_scan)

  driver:  python profiles/keyed_table_ab.py --parent <parent librsseg_hip.so> [--new <librsseg_hip.so>] [--rounds 3]
                                             [--resources table.json] > session.json
  worker:  python profiles/keyed_table_ab.py --lib <librsseg_hip.so>
  merge:   python profiles/keyed_table_ab.py --merge name=session.json [name=session.json ...]

A case passes if the median of the new build is no slower than the SLOWEST run of the parent in the same session (the
parent's spread on the day is the margin)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "rs-image-segmentation_amd", "librsseg_hip.so")
LAUNCHES = 5


def worker(a):
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT]
    import numpy as np
    import torch
    from rsseg import _lib as L
    L.LIB_PATH = os.path.abspath(a.lib)
    from rsseg.runtime import Context
    import isodata_bench as IB
    import moments_bench as MB
    import object_features_bench as OB
    ctx = Context(0, use_dist=False)
    res = {}

    def timed(name, fam, call):
        outs = call()                       # warm-up: code object, LDS attribute, allocator
        runs = []
        for _ in range(2):
            del outs
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(LAUNCHES):
                outs = call()
            ctx.sync()
            ms, cnt = ctx.prof_get(fam)
            assert cnt == LAUNCHES, (name, fam, cnt)
            runs.append(round(ms / cnt, 4))
            ctx.prof_enable(False)
        sha = [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()[:16] for o in outs]
        res[name] = {"family": fam, "ms_per_launch": runs, "sha256_16": sha}

    # ---- K24
    for name, bench_case, size in (("mo-f19k8", "dense19", a.size), ("mo-u8f7k8", "u8_7", a.size), ("mo-f64k64-B", "f64k64", a.wide_size)):
        planes, labels, k, pe, Q, ignore, _, _ = MB.make_case(torch, ctx.device, bench_case, size * size)
        if name == "mo-u8f7k8":             # Path B of the uint8 kernels takes 64 planes and 64 classes
            wide = planes + [planes[i % 7].flip(0) for i in range(57)]
            wl = (labels.to(torch.int32) * 8 + torch.roll(labels, 1).to(torch.int32)).to(torch.uint8)
        for lt in (torch.uint8, torch.int32):
            lab = labels.to(lt)
            timed(f"{name}-{'u8' if lt == torch.uint8 else 'i32'}lab", "class_moments",
                  lambda: [ctx.class_moments(planes, lab, k, pe, Q, ignore=ignore)[0]])
            if name == "mo-u8f7k8":
                n2 = a.wide_size * a.wide_size
                wp, wlab = [p[:n2] for p in wide], wl[:n2].to(lt)
                assert ctx.class_moments_plan(64, 64, True)[0] == 1
                timed(f"mo-u8f64k64-B-{'u8' if lt == torch.uint8 else 'i32'}lab", "class_moments", lambda: [ctx.class_moments(wp, wlab, 64, None, 0)[0]])
                del wp, wlab
        del planes, labels, lab
        torch.cuda.empty_cache()
    # ---- K26: every register width with a table, Path B at F = 64 / k = 64
    IB.CASES.update({"f7k8": (7, 8, False, True), "f32k8": (32, 8, False, True), "f64k16": (64, 16, False, True), "f64k64": (64, 64, False, True),
                     "u8_15k8": (15, 8, True, True), "u8_19k32": (19, 32, True, True), "u8_32k8": (32, 8, True, True), "u8_64k16": (64, 16, True, True),
                     "u8_64k64": (64, 64, True, True)})
    for bench_case in ("f7k8", "f15k8", "f19k32", "f32k8", "f64k16", "f64k64", "u8_7k8", "u8_15k8", "u8_19k32", "u8_32k8", "u8_64k16", "u8_64k64"):
        F, k, u8, _ = IB.CASES[bench_case]
        size = a.wide_size if F == 64 else a.size
        planes, labels, centers, weight, pe, Q, _, _ = IB.make_case(torch, ctx.device, bench_case, size * size)
        assert ctx.isodata_plan(F, k, u8)[0] == (1 if k == 64 else 0)

        def sweep():
            labels.fill_(255)
            table, changed, left = ctx.isodata_sweep(planes, labels, centers, weight, pe, Q)
            return [table, labels, torch.tensor([changed, left])]
        timed("iso-" + bench_case + ("-B" if k == 64 else ""), "isodata_sweep", sweep)
        del planes, labels
        torch.cuda.empty_cache()
    # ---- K25, K27, K23's segment sums: the SLIC scene, and one segment per pixel
    S = a.scene_size
    seg, ns, u8p, f32p = OB.make_scene(torch, ctx, S, a.slic_iterations)
    for tag, planes in (("u8p7", u8p), ("f32p15", f32p)):
        timed(f"obj-{tag}-geo", "segment_features", lambda: [ctx.segment_features(seg, S, S, ns, planes)])
        timed(f"obj-{tag}", "segment_features", lambda: [ctx.segment_features(seg, S, S, ns, planes, geometry=False)])
        timed(f"sums-{tag}", "segment_sums", lambda: [ctx.segment_sums(seg, S, S, ns, planes)])
    timed("adj-u8p7", "segment_adjacency", lambda: [ctx.segment_adjacency(seg, S, S, ns, u8p)])
    del seg, u8p, f32p
    V = a.overflow_size
    own, planes = OB.make_overflow(torch, ctx, V)
    timed("obj-overflow", "segment_features", lambda: [ctx.segment_features(own, V, V, V * V, planes)])
    timed("adj-overflow", "segment_adjacency", lambda: [ctx.segment_adjacency(own, V, V, V * V, planes)])
    # ---- K19: the tile scan behind wave_incl_scan (k19_scan is the one kernel of k19_compact.hip that is not identical)
    g = torch.Generator(device=ctx.device)
    g.manual_seed(19)
    valid = (torch.rand(a.size * a.size, generator=g, device=ctx.device) < 0.7).to(torch.uint8)
    timed("compact-plan", "compact_plan", lambda: [ctx.compact_plan(valid).tile_off])
    print(json.dumps({"lib": a.lib, "cases": res, "scene_segments": int(ns)}))
    ctx.close()


def driver(args):
    out = {"note": f"ms per launch; --size {args.size}, --wide-size {args.wide_size}, --scene-size {args.scene_size}, --overflow-size "
                   f"{args.overflow_size}; per process two timings of {LAUNCHES} launches after one warm-up launch; parent and new build "
                   "alternate, one process each, one after another",
           "rounds": args.rounds, "cases": {}}
    me = [sys.executable, os.path.abspath(__file__)]
    for _ in range(args.rounds):
        for build, lib in (("parent", args.parent), ("new", args.new)):
            p = subprocess.run(me + ["--lib", lib, "--size", str(args.size), "--wide-size", str(args.wide_size), "--scene-size", str(args.scene_size),
                                     "--overflow-size", str(args.overflow_size), "--slic-iterations", str(args.slic_iterations)],
                               capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:       # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{build} process exited with {p.returncode}")
            got = json.loads(p.stdout.strip().splitlines()[-1])
            for name, r in got["cases"].items():
                c = out["cases"].setdefault(name, {"family": r["family"], "parent": [], "new": [], "sha": {"parent": set(), "new": set()}})
                c[build].extend(r["ms_per_launch"])
                c["sha"][build].add(tuple(r["sha256_16"]))
            sys.stderr.write(f"[keyed_table_ab] {build}: " + ", ".join(f"{k} {v['ms_per_launch']}" for k, v in got["cases"].items()) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for name, c in out["cases"].items():
        sha = c.pop("sha")
        c["bit_identical"] = len(sha["parent"] | sha["new"]) == 1
        c["sha256_16"] = sorted(sha["parent"] | sha["new"])
        c["parent_min_max"] = [min(c["parent"]), max(c["parent"])]
        c["new_median"] = med(c["new"])
        c["parent_median"] = med(c["parent"])
        c["passes"] = c["new_median"] <= max(c["parent"])
    out["all_pass"] = all(c["passes"] and c["bit_identical"] for c in out["cases"].values())
    if args.resources:
        out["code_objects_parent_new"] = json.load(open(args.resources))
    print(json.dumps(out, indent=1))


def merge(parts):
    out = {}
    for part in parts:
        name, path = part.split("=", 1)
        out[name] = json.load(open(path))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--parent")
    ap.add_argument("--new", default=NEW_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--wide-size", type=int, default=4096)
    ap.add_argument("--scene-size", type=int, default=8192)
    ap.add_argument("--overflow-size", type=int, default=2048)
    ap.add_argument("--slic-iterations", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--resources")
    ap.add_argument("--merge", nargs="+", metavar="NAME=FILE")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge)
    elif a.lib:
        worker(a)
    elif a.parent:
        driver(a)
    else:
        ap.error("--lib (worker) or --parent (driver)")
