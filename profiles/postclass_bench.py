"""K20 (class-map clean-up) measured at --size (16384) squared, one process, device events, --reps timed launches after two
warm-up launches, medians.

Majority filter: k in {3, 5, 7, 15} on maps of 8, 20 and 65 labels (blocks of one label with 5 % of the pixels redrawn, every
value voting, the group mask given so that the launch alone is timed; the histogram that finds the mask is timed by itself).
Yardsticks of the same run: a device-to-device copy of the uint8 plane (the traffic floor: one byte in, one out) and k7_morph's
dilate of the same k where it exists (the same tile walk with a cheaper operator).
Sieve: the 8-label map, noisy (5 % redrawn) and smooth (none), min_area 16, against today's way on this library:
remove_small_components once per label on masks made on the host and merged there.  Both are timed as wall time from a host
map to a host map, and their GPU parts by events.
CPU: scipy.ndimage.label + bincount per class at --cpu-size (4096) squared, once, for scale.
The registers / LDS / scratch of every k20 kernel are copied from profiles/postclass_code_objects.json
(profiles/code_object_diff.py) when that file is there.  Nothing is gated on these figures.
Usage: python profiles/postclass_bench.py [--size 16384] [--reps 7] [--cpu-size 4096] [--out profiles/postclass_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def class_map(torch, device, size, n_labels, noise, seed):
    """blocks of 64 x 64 pixels of one label in 0 .. n_labels - 1, `noise` of the pixels redrawn"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    c = (size + 63) // 64
    coarse = torch.randint(0, n_labels, (c, c), device=device, generator=g, dtype=torch.uint8)
    q = coarse.repeat_interleave(64, 0).repeat_interleave(64, 1)[:size, :size].contiguous()
    if noise:
        flip = torch.rand((size, size), device=device, generator=g) < noise
        q[flip] = torch.randint(0, n_labels, (int(flip.sum()),), device=device, generator=g, dtype=torch.uint8)
    return q.reshape(-1)


def timed(torch, stream, fn, reps, warm=2):
    ms = []
    for r in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            fn()
            b.record()
        b.synchronize()
        if r >= warm:
            ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-size", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from rsseg import _lib as L
    from rsseg import postclass as PC
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    size, n = a.size, a.size * a.size
    st = ctx.torch_stream
    res = dict(device=torch.cuda.get_device_name(0), size=size, pixels=n, reps=a.reps,
               note="majority: ignore = fill = -1 (every value votes), group mask given; times are device events around the library call "
                    "(launch, the 16-byte counter reset and read-back); ratios are medians over medians of this run")
    out = torch.empty(n, dtype=torch.uint8, device=ctx.device)
    maps = {8: class_map(torch, ctx.device, size, 8, 0.05, 1)}
    copy = timed(torch, st, lambda: out.copy_(maps[8]), a.reps)
    copy["tb_per_s"] = 2 * n / (copy["median_ms"] * 1e-3) / 1e12
    res["copy_u8"] = copy
    dil = {}
    for k in (3, 5, 7):
        dil[k] = timed(torch, st, lambda: ctx.morph(maps[8], size, size, k, L.MORPH_DILATE), a.reps)
    res["k7_morph_dilate"] = {str(k): v for k, v in dil.items()}
    res["hist_u8"] = timed(torch, st, lambda: ctx.hist_u8(maps[8]), a.reps)
    res["majority"] = {}
    for nl in (8, 20, 65):
        if nl not in maps:
            maps[nl] = class_map(torch, ctx.device, size, nl, 0.05, nl)
        q = maps[nl]
        gm = PC._group_mask(ctx.hist_u8(q))
        row = {"groups": bin(gm).count("1")}
        for k in (3, 5, 7, 15):
            nc = []

            def go():
                nc.append(ctx.majority_u8(q, size, size, k, group_mask=gm, out=out)[1])
            t = timed(torch, st, go, a.reps)
            t["n_changed"] = int(nc[-1])
            t["over_copy"] = t["median_ms"] / copy["median_ms"]
            if k in dil:
                t["over_dilate"] = t["median_ms"] / dil[k]["median_ms"]
            row[str(k)] = t
            print(json.dumps({f"majority labels={nl} k={k}": t}), file=sys.stderr, flush=True)
        res["majority"][str(nl)] = row
        if nl != 8:
            del maps[nl]
    # ---- sieve ----
    res["sieve"] = {}
    min_area = 16
    for name, noise in (("noisy", 0.05), ("smooth", 0.0)):
        q = maps[8] if noise else class_map(torch, ctx.device, size, 8, 0.0, 2)
        host = q.cpu().numpy()
        entry = {"min_area": min_area, "labels": 8}
        entry["one_pass_gpu"] = timed(torch, st, lambda: ctx.sieve_u8(q, size, size, min_area, 8, -1, 255), max(3, a.reps // 2), warm=1)
        t = time.perf_counter()
        got, removed = ctx.sieve_u8(ctx.to_device(host), size, size, min_area, 8, -1, 255)
        got = got.cpu().numpy()
        entry["one_pass_wall_ms"] = (time.perf_counter() - t) * 1e3
        entry["n_removed"] = int(removed)
        # today's way: one binary mask per label made on the host, remove_small_components, merged on the host
        gpu_ms = 0.0
        t = time.perf_counter()
        merged = host.copy()
        for lab in range(8):
            mask = (host == lab).astype(np.uint8)
            d = ctx.to_device(mask)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record()
                kept = ctx.remove_small_components(d, size, size, min_area)
                e1.record()
            e1.synchronize()
            gpu_ms += e0.elapsed_time(e1)
            merged[(mask != 0) & (kept.cpu().numpy() == 0)] = 255
        entry["per_label_wall_ms"] = (time.perf_counter() - t) * 1e3
        entry["per_label_gpu_ms"] = gpu_ms
        entry["equal"] = bool(np.array_equal(merged, got))
        entry["per_label_over_one_pass_gpu"] = gpu_ms / entry["one_pass_gpu"]["median_ms"]
        entry["per_label_over_one_pass_wall"] = entry["per_label_wall_ms"] / entry["one_pass_wall_ms"]
        res["sieve"][name] = entry
        print(json.dumps({f"sieve {name}": entry}), file=sys.stderr, flush=True)
        del host, merged, got
    # ---- CPU, for scale ----
    from scipy import ndimage
    cs = a.cpu_size
    small = class_map(torch, ctx.device, cs, 8, 0.05, 3).cpu().numpy().reshape(cs, cs)
    t = time.perf_counter()
    cpu = small.copy()
    for lab in range(8):
        comp, m = ndimage.label(small == lab, structure=np.ones((3, 3), int))
        area = np.bincount(comp.ravel(), minlength=m + 1)
        cpu[(area[comp] < min_area) & (comp > 0)] = 255
    cpu_ms = (time.perf_counter() - t) * 1e3
    g, _ = ctx.sieve_u8(ctx.to_device(small.reshape(-1)), cs, cs, min_area, 8, -1, 255)
    res["cpu_scipy_sieve"] = dict(size=cs, wall_ms=cpu_ms, equal=bool(np.array_equal(g.cpu().numpy().reshape(cs, cs), cpu)))
    p = os.path.join(ROOT, "profiles", "postclass_code_objects.json")
    if os.path.exists(p):
        res["code_objects"] = {r["kernel"]: dict(vgprs=r["vgprs"][1], sgprs=r["sgprs"][1], lds=r["lds"][1], scratch=r["scratch"][1],
                                                 waves_per_simd=r["waves_per_simd"][1])
                               for r in json.load(open(p)) if r["file"] == "k20_postclass.hip"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
