"""K23 timed at the size a user would run it: --size (16384) squared pixels, P = 7 and 15 uint8 planes, grid step S = 8, 16, 32.

Per (P, S), in this process, from the library's own device events (Context.prof_get; one warm-up call, then --reps calls of
Context.slic_u8 with max_iter = --iters, compactness 10, min_area = S * S // 4):
  slic_init      the grid labels and their sums (once per call);
  slic_assign    ONE assign-and-accumulate iteration: centres from the sums, the zeroing of the sums, the assignment kernel;
  slic_enforce   components, marking, all growth rounds of a call;
  slic_relabel   first pixels, flags, the tile scan, numbering, the final plane;
and around whole calls (torch events): segment_sums of the P planes, segment_majority_u8 of a 9-class map, segment_paint of the
uint8 table.  Two yardsticks in the same process:
  copy           a device-to-device copy moving as many bytes as one iteration must (P n read + 4 n label bytes written and
                 4 n read: a buffer of (P + 8) n / 2 bytes copied once reads and writes that total);
  kmeans_sweep   one Context.kmeans_predict with k = 9 centres over F = P float32 planes of the same raster: the same nine
                 distances per pixel, in the library's fastest form.
No ratio is fixed in advance: both are recorded beside every time.  The planes are smooth fields plus noise (upsampled coarse
noise), so that superpixels have something to follow and some pieces need regrowing.
--worker P S: one warm-up and --reps calls and nothing else, for a counter run of its own (profiles/slic_pmc.sh).
One JSON object on stdout (and in --out).
Usage: python profiles/slic_bench.py [--size 16384] [--reps 5] [--iters 3] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PLANES = (7, 15)
STEPS = (8, 16, 32)
K = 9
FAMILIES = ("slic_init", "slic_assign", "slic_enforce", "slic_relabel")


def planes_of(torch, device, size, P, seed=23):
    """P flat uint8 planes: a coarse random field upsampled 32 x (bilinear) plus a little noise"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = []
    for _ in range(P):
        coarse = torch.rand(1, 1, size // 32 + 2, size // 32 + 2, generator=g, device=device)
        f = torch.nn.functional.interpolate(coarse, scale_factor=32, mode="bilinear", align_corners=False)[0, 0, :size, :size]
        f = f * 220.0 + torch.rand(size, size, generator=g, device=device) * 35.0
        out.append(f.clamp_(0, 255).to(torch.uint8).reshape(-1).contiguous())
        del f, coarse
    return out


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


def slic_call(ctx, planes, size, S, iters):
    return ctx.slic_u8(planes, size, size, S, (10.0 * 10.0) / (S * S), iters, S * S // 4)


def worker(size, P, S, reps, iters):
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    planes = planes_of(torch, ctx.device, size, P)
    for _ in range(reps + 1):
        slic_call(ctx, planes, size, S, iters)
    ctx.sync()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", nargs=2, type=int, metavar=("P", "S"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.size, a.worker[0], a.worker[1], a.reps, a.iters)
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    size, n = a.size, a.size * a.size
    ctx = Context(0, use_dist=False)
    res = dict(device=torch.cuda.get_device_name(0), size=size, pixels=n, reps=a.reps, max_iter=a.iters, compactness=10.0, tile=list(ctx.slic_tile()),
               cases=[])
    rs = np.random.RandomState(5)
    for P in PLANES:
        planes = planes_of(torch, ctx.device, size, P)
        # yardstick 1: the bytes of one iteration as a copy
        half = (P + 8) * n // 2
        src, dst = torch.empty(half, dtype=torch.uint8, device=ctx.device), torch.empty(half, dtype=torch.uint8, device=ctx.device)
        src.zero_()
        cp = event_ms(torch, ctx.torch_stream, lambda: dst.copy_(src), a.reps)
        del src, dst
        # yardstick 2: the k-means sweep over the same planes as float32
        fl = [p.to(torch.float32) for p in planes]
        centers = (rs.rand(K, P) * 255.0).astype(np.float32).astype(np.float64)   # a model fitted on float32 planes
        km = event_ms(torch, ctx.torch_stream, lambda: ctx.kmeans_predict(fl, centers, np.ones(P), np.zeros(P)), a.reps)
        del fl
        torch.cuda.empty_cache()
        yard = dict(copy=dict(bytes_moved=2 * half, ms=cp, tb_per_s=2 * half / (cp["min"] * 1e-3) / 1e12), kmeans_sweep=dict(k=K, F=P, ms=km))
        print(json.dumps({"P": P, "yardsticks": yard}), file=sys.stderr, flush=True)
        for S in STEPS:
            labels, ns, ni, nr = slic_call(ctx, planes, size, S, a.iters)     # warm-up
            ctx.prof_enable(True)
            ctx.prof_reset()
            whole = event_ms(torch, ctx.torch_stream, lambda: slic_call(ctx, planes, size, S, a.iters), a.reps - 1)
            fam = {}
            for name in FAMILIES + ("compact_plan",):
                ms, cnt = ctx.prof_get(name)
                fam[name] = dict(ms_total=ms, scopes=cnt, ms_per_scope=ms / max(cnt, 1), ms_per_call=ms / a.reps)
            ctx.prof_enable(False)
            it = fam["slic_assign"]["ms_per_scope"]
            cm = torch.randint(0, K, (n,), device=ctx.device, dtype=torch.uint8)
            sums = event_ms(torch, ctx.torch_stream, lambda: ctx.segment_sums(labels, size, size, ns, planes), a.reps)
            maj = event_ms(torch, ctx.torch_stream, lambda: ctx.segment_majority_u8(labels, ns, cm, ignore=-1, fill=0), a.reps)
            table = ctx.segment_majority_u8(labels, ns, cm, ignore=-1, fill=0)
            pnt = event_ms(torch, ctx.torch_stream, lambda: ctx.segment_paint(labels, ns, table), a.reps)
            case = dict(P=P, S=S, n_segments=int(ns), n_iter=int(ni), n_regrown=int(nr), call_ms=whole, families=fam,
                        iteration_ms=it, iteration_over_copy=it / cp["min"], iteration_over_kmeans_sweep=it / km["min"],
                        enforce_ms_per_call=fam["slic_enforce"]["ms_per_call"],
                        relabel_ms_per_call=fam["slic_relabel"]["ms_per_call"] + fam["compact_plan"]["ms_per_call"],
                        reductions=dict(segment_sums=sums, segment_majority=maj, segment_paint=pnt), yardsticks=yard)
            res["cases"].append(case)
            print(json.dumps({k: case[k] for k in ("P", "S", "n_segments", "n_iter", "n_regrown", "iteration_ms", "iteration_over_copy",
                                                   "iteration_over_kmeans_sweep", "enforce_ms_per_call", "relabel_ms_per_call")}),
                  file=sys.stderr, flush=True)
            del labels, cm, table
        del planes
        torch.cuda.empty_cache()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
