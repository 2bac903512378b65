#!/usr/bin/env python3
"""The LDS stencils of csrc/k5_window.hip (k6_box, k6_std, k7_morph, k8_filter) at 16384^2, two builds of the library against
each other, in the manner of profiles/glcm_finish_ab.py: the same synthetic planes for both, each build in a process of its
own, the builds alternating for several rounds, HIP-event time per launch from the context's profiler, every output plane
hashed so that the builds are also compared bit for bit.

  driver:  python profiles/window_shared_steps_ab.py --parent <parent librsseg_hip.so> [--new <librsseg_hip.so>] [--rounds 3]
                                                     [--resources table.json] > window_shared_steps_ab.json
  worker:  python profiles/window_shared_steps_ab.py --lib <librsseg_hip.so>     (one JSON line: per case ms per launch, hashes)

A case passes if the median of the new build is no slower than the SLOWEST run of the parent in the same session (the
parent's spread on the day is the margin).  --resources names the per-kernel table of profiles/code_object_diff.py (registers,
LDS, scratch, waves per SIMD and whether the instruction sequences are equal; no GPU needed), recorded beside the times."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "rs-image-segmentation_amd", "librsseg_hip.so")
LAUNCHES = 5


def worker(lib_path, size):
    sys.path[:0] = [os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT]
    import torch

    import bench
    from rsseg import _lib as L
    L.LIB_PATH = os.path.abspath(lib_path)
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    H = W = size
    bands = bench.synth_rows(torch, ctx.device, W, 0, H, want=range(7))
    q = bands[3].to(torch.uint8)
    f = [b / 255.0 for b in bands]          # not integer-valued: the float64 sums have low bits to lose
    del bands
    x = f[3]
    # (kernel, [profiler families], call returning the output planes)
    cases = [
        ("k6_box<7,false> x 7 planes", ["ctxmean"], lambda: ctx.box_mean_multi(f, H, W, 7, L.BORDER_REFLECT)),
        ("k6_box<9,true>", ["box"], lambda: [ctx.box_mean(x, H, W, 9, L.BORDER_REFLECT101, True)]),
        ("k6_std<5,false>", ["box"], lambda: [ctx.local_std(x, H, W, 5)]),
        ("k6_std<7,true>", ["box"], lambda: [ctx.local_var(x, H, W, 7)]),
        ("k7_morph<5,2>", ["morph"], lambda: [ctx.morph(q, H, W, 5, L.MORPH_GRADIENT)]),
        ("k7_morph<7,0>", ["morph"], lambda: [ctx.morph(q, H, W, 7, L.MORPH_ERODE)]),
        ("k8_filter<0,PASS>", ["filt_max", "filt_write"], lambda: [ctx.sobel_mag(q, H, W)]),
        ("k8_filter<1,PASS>", ["filt_max", "filt_write"], lambda: [ctx.laplacian_norm(q, H, W)]),
    ]
    res = {}
    for name, fams, call in cases:
        outs = call()                       # warm-up: code object
        runs = {fam: [] for fam in fams}
        for _ in range(2):
            del outs
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(LAUNCHES):
                outs = call()
            for fam in fams:
                ms, cnt = ctx.prof_get(fam)
                assert cnt == LAUNCHES, (name, fam, cnt)
                runs[fam].append(round(ms / cnt, 4))
            ctx.prof_enable(False)
        sha = [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()[:16] for o in outs]
        del outs
        for fam in fams:
            key = name if len(fams) == 1 else name.replace("PASS", "0" if fam == "filt_max" else "1")
            res[key] = {"family": fam, "ms_per_launch": runs[fam], "sha256_16": sha}
    print(json.dumps({"lib": lib_path, "cases": res}))
    ctx.close()


def driver(args):
    out = {"note": f"ms per launch on a {args.size}x{args.size} plane (one plane unless the case says otherwise): per process two timings of "
                   f"{LAUNCHES} launches after one warm-up launch; parent and new build alternate, one process each, one after another",
           "rounds": args.rounds, "cases": {}}
    for _ in range(args.rounds):
        for build, lib in (("parent", args.parent), ("new", args.new)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--size", str(args.size)], capture_output=True, text=True,
                               timeout=args.timeout)
            if p.returncode != 0:       # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{build} worker exited with {p.returncode}")
            for name, r in json.loads(p.stdout.strip().splitlines()[-1])["cases"].items():
                c = out["cases"].setdefault(name, {"family": r["family"], "parent": [], "new": [], "sha": {"parent": set(), "new": set()}})
                c[build].extend(r["ms_per_launch"])
                c["sha"][build].add(tuple(r["sha256_16"]))
    med = lambda v: sorted(v)[len(v) // 2]
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--parent")
    ap.add_argument("--new", default=NEW_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--resources")
    a = ap.parse_args()
    if a.lib:
        worker(a.lib, a.size)
    elif a.parent:
        driver(a)
    else:
        ap.error("--lib (worker) or --parent (driver)")
