#!/usr/bin/env python3
"""Texture kernel of the dense case (k4_glcm_quad: window 7, step 1, 32 levels) at 16384^2, two builds of the library against
each other (--dense pair: k4_glcm_pair on the same case; --step 7: k4_glcm_thread<7,3>, the same window at step 7): the same quantised plane and the same HIP-event timers as profiles/r04_glcm_ab.py, each build in a process of
its own, alternating, several rounds; the five maps of every run are hashed, so the builds are also compared bit for bit.

  driver:  python profiles/glcm_finish_ab.py --parent <parent librsseg_hip.so> [--new <librsseg_hip.so>] [--rounds 3]
                                             [--dense {quad,pair}] [--step 7] > out.json
  worker:  python profiles/glcm_finish_ab.py --lib <librsseg_hip.so>            (one JSON line: ms per launch, map hashes)

The gain counts if the slowest run of the new build is faster than the fastest run of the parent ("separated").  The
compiler's resource remarks of the new build's kernel (hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed) are
recorded beside the times when --remarks FILE names the compiler's output."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "rs-image-segmentation_amd", "librsseg_hip.so")
LAUNCHES = 5


def kernel_of(args):
    """(name, mangled prefix) of the kernel the dispatch picks for window 7, 32 levels at this step"""
    if args.step != 1:
        return "k4_glcm_thread<7,3>", "_Z14k4_glcm_threadILi7ELi3EE"
    return ("k4_glcm_pair", "_Z12k4_glcm_pair") if args.dense == "pair" else ("k4_glcm_quad", "_Z12k4_glcm_quad")


def worker(lib_path, size, dense, step):
    sys.path[:0] = [os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT]
    import torch

    import bench
    from rsseg import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    H = W = size
    nir = bench.synth_rows(torch, ctx.device, W, 0, H, want=[3])[0]
    q = (nir / 255.0 * 31).to(torch.uint8)
    os.environ["RSSEG_GLCM_DENSE"] = dense
    ctx.glcm(q, H, W, 32, 7, step)       # warm-up: code object, tables
    runs = []
    for _ in range(2):
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(LAUNCHES):
            maps, _ = ctx.glcm(q, H, W, 32, 7, step)
        ms, cnt = ctx.prof_get("glcm")
        ctx.prof_enable(False)
        runs.append(round(ms / cnt, 3))
    sha = [hashlib.sha256(m.cpu().numpy().tobytes()).hexdigest()[:16] for m in maps]
    print(json.dumps({"lib": lib_path, "ms_per_launch": runs, "maps_sha256_16": sha}))
    ctx.close()


def remarks(path, mangled):
    text = open(path).read()
    m = re.search(r"Function Name: " + re.escape(mangled) + r"\w*(.*?)(?:Function Name:|\Z)", text, re.S)
    if not m:
        return None
    out = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                     ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)")):
        v = re.search(pat, m.group(1))
        out[key] = int(v.group(1)) if v else None
    return out


def driver(args):
    name, mangled = kernel_of(args)
    out = {"note": f"ms per launch of {name} on a {args.size}x{args.size} plane (32 levels); per process two timings of {LAUNCHES} "
                   "launches after one warm-up launch; parent and new build alternate, one process each",
           "parent": [], "new": [], "rounds": args.rounds}
    sha = {}
    for _ in range(args.rounds):
        for build, lib in (("parent", args.parent), ("new", args.new)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--size", str(args.size), "--dense", args.dense,
                                "--step", str(args.step)], capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:       # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{build} worker exited with {p.returncode}")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            out[build].extend(r["ms_per_launch"])
            sha.setdefault(build, set()).add(tuple(r["maps_sha256_16"]))
    out["bit_identical"] = len(sha["parent"] | sha["new"]) == 1
    out["parent_min_max"] = [min(out["parent"]), max(out["parent"])]
    out["new_min_max"] = [min(out["new"]), max(out["new"])]
    out["separated"] = max(out["new"]) < min(out["parent"])
    med = lambda v: sorted(v)[len(v) // 2]
    out["median_gain_ms"] = round(med(out["parent"]) - med(out["new"]), 3)
    if args.remarks:
        out[name + "_resources_new_build"] = remarks(args.remarks, mangled)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--parent")
    ap.add_argument("--new", default=NEW_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--remarks")
    ap.add_argument("--dense", choices=("quad", "pair"), default="quad")
    ap.add_argument("--step", type=int, choices=(1, 7), default=1)
    a = ap.parse_args()
    if a.lib:
        worker(a.lib, a.size, a.dense, a.step)
    elif a.parent:
        driver(a)
    else:
        ap.error("--lib (worker) or --parent (driver)")
