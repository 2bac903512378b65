"""K19 (order-preserving compaction) measured on the planes a masked classification moves: the 15 float32 planes of config 3
at --size (16384) squared, with 0 % (everything valid), 30 % (a nodata collar) and 50 % (random pixels) masked.

Per mask, in this process and alternating round by round (--reps rounds after one warm-up round):
  copy      a plain device-to-device copy of the same 15 input planes (torch's copy_, one per plane)
  compact   rsseg_compact_planes of the 15 planes, one launch
  expand    rsseg_expand_plane of the 15 compacted planes, one launch each
  plan      rsseg_compact_plan (count + scan + the read-back of the valid count)
each with device events around it; minimum and median, the bytes each moves by its algorithm, and the fraction of the copy's
bandwidth it reaches (its bytes over its time, over the copy's bytes over the copy's time).
With --variant-lib PATH (the library linked with csrc/k19_compact.hip compiled -DK19_STAGED_STORE=0 -DK19_STAGED_FETCH=1: the
survivors stored element by element straight to global memory, and expansion staging the compacted run through LDS: the two
alternatives to what is built) the same compact and expand calls are also made through that library, in the same rounds.
Then, for the 30 % case, the masked KMeans fit (rsseg.masked.kmeans_fit_predict_masked, k = 8) against the unmasked fit of the
same raster.  Nothing is gated on these figures.  One JSON object on stdout (and in --out).
Usage: python profiles/compact_bench.py [--size 16384] [--reps 5] [--variant-lib PATH] [--out profiles/compact_bench.json] [--no-fit]"""
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


def masks(torch, device, size):
    n = size * size
    b = int(round(size * (1 - 0.7 ** 0.5) / 2))
    collar = torch.zeros((size, size), dtype=torch.uint8, device=device)
    collar[b:size - b, b:size - b] = 1
    g = torch.Generator(device=device)
    g.manual_seed(1)
    rnd = (torch.rand(n, device=device, generator=g) < 0.5).to(torch.uint8)
    return {"0%": torch.ones(n, dtype=torch.uint8, device=device), "30% collar": collar.reshape(-1).contiguous(), "50% random": rnd}


class Direct:
    """The compaction entry points of another build of the library, on a context of its own over the same stream."""

    def __init__(self, path, device, stream):
        from rsseg import _lib as L
        self.lib = C.CDLL(path)
        for name in ("rsseg_ctx_create", "rsseg_ctx_destroy", "rsseg_last_error", "rsseg_compact_planes", "rsseg_expand_plane"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        self.h = C.c_void_p()
        assert self.lib.rsseg_ctx_create(device, C.c_void_p(stream), C.byref(self.h)) == 0


def timed(torch, stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms, nbytes, copy=None):
    out = dict(min_ms=float(np.min(ms)), median_ms=float(np.median(ms)), runs_ms=[float(x) for x in ms], bytes=int(nbytes),
               tb_per_s_at_median=nbytes / (float(np.median(ms)) * 1e-3) / 1e12)
    if copy is not None:
        out["fraction_of_copy_bandwidth"] = out["tb_per_s_at_median"] / copy["tb_per_s_at_median"]
        out["time_over_copy"] = out["median_ms"] / copy["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variant-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    from rsseg import pipeline as P
    from rsseg.masked import kmeans_fit_predict_masked
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    size, n = a.size, a.size * a.size
    bands = bench.synth_rows(torch, ctx.device, size, 0, size)
    _, _, planes = P.config3(ctx, bands, size, size, 8, 7, 1, 3, n)
    planes = list(planes)
    del bands
    F, eb = len(planes), planes[0].element_size()
    lib, h = ctx.lib, ctx.h
    direct = Direct(a.variant_lib, 0, ctx.torch_stream.cuda_stream or 1) if a.variant_lib else None   # 1: the legacy default stream, as Context
    res = dict(device=torch.cuda.get_device_name(0), size=size, pixels=n, planes=F, dtype="float32", reps=a.reps,
               tile=lib.rsseg_compact_tile(), scan_span=lib.rsseg_compact_scan_span(),
               note="fraction_of_copy_bandwidth = (algorithmic bytes / median time) of the step over the same of the plain copy, same process, "
                    "alternating rounds; bytes: copy 2 * P * n * 4; compact n (mask) + P * (n + n_valid) * 4; expand P * (n (mask) + (n_valid + n) * 4)",
               masks={})
    copy_dst = [torch.empty_like(p) for p in planes]
    comp = [torch.empty_like(p) for p in planes]
    back = torch.empty_like(planes[0])
    fill = np.float32(np.nan).tobytes()
    pp_in, pp_out = ctx._pp(planes), ctx._pp(comp)
    for name, mask in masks(torch, ctx.device, size).items():
        plan_ms = []
        for r in range(a.reps + 1):
            t = time.perf_counter()
            plan = ctx.compact_plan(mask)
            if r:
                plan_ms.append((time.perf_counter() - t) * 1e3)
        nv = plan.n_valid
        mp, op = C.c_void_p(mask.data_ptr()), C.c_void_p(plan.tile_off.data_ptr())

        def do_copy():
            for d, s in zip(copy_dst, planes):
                d.copy_(s)

        def do_compact(L=lib, H=h):
            assert L.rsseg_compact_planes(H, mp, op, n, pp_in, F, eb, pp_out) == 0

        def do_expand(L=lib, H=h):
            for c in comp:
                assert L.rsseg_expand_plane(H, mp, op, n, C.c_void_p(c.data_ptr()), eb, fill, C.c_void_p(back.data_ptr())) == 0

        steps = [("copy", do_copy), ("compact", do_compact), ("expand", do_expand)]
        if direct:
            steps += [("compact_direct_store", lambda: do_compact(direct.lib, direct.h)), ("expand_staged_fetch", lambda: do_expand(direct.lib, direct.h))]
        ms = {k: [] for k, _ in steps}
        for r in range(a.reps + 1):
            for k, fn in steps:
                v = timed(torch, ctx.torch_stream, fn)
                if r:
                    ms[k].append(v)
        nbytes = {"copy": 2 * F * n * eb, "compact": n + F * (n + nv) * eb, "expand": F * (n + (n + nv) * eb)}
        nbytes["compact_direct_store"], nbytes["expand_staged_fetch"] = nbytes["compact"], nbytes["expand"]
        copy = stats(ms["copy"], nbytes["copy"])
        entry = dict(n_valid=nv, masked_share=1 - nv / n, plan_wall_ms=dict(min=float(np.min(plan_ms)), median=float(np.median(plan_ms))), copy=copy)
        for k, _ in steps[1:]:
            entry[k] = stats(ms[k], nbytes[k], copy)
        if name == "0%":
            entry["compact_equals_copy"] = bool(all(torch.equal(c.view(torch.int32), p.view(torch.int32)) for c, p in zip(comp, planes)))
        res["masks"][name] = entry
        print(json.dumps({name: entry}), file=sys.stderr, flush=True)
        if name == "30% collar" and not a.no_fit:
            del plan
            fit = {}
            for which in ("unmasked", "masked", "unmasked", "masked"):
                t = time.perf_counter()
                if which == "masked":
                    _, meta = kmeans_fit_predict_masked(planes, mask, 8, ctx=ctx)
                else:
                    _, meta = ctx.kmeans_fit_predict(planes, 8)
                ctx.sync()
                fit.setdefault(which, []).append(dict(wall_ms=(time.perf_counter() - t) * 1e3, n_iter=int(meta["n_iter"]),
                                                      ms_init=meta["ms_init"], ms_lloyd=meta["ms_lloyd"]))
            fit["masked_over_unmasked_wall"] = min(f["wall_ms"] for f in fit["masked"]) / min(f["wall_ms"] for f in fit["unmasked"])
            fit["note"] = ("the two fits are different problems (the unmasked one clusters the collar as a block of zeros): iteration counts differ; "
                           "the masked wall time includes plan, compaction of the 15 planes and expansion of the labels")
            res["kmeans_fit_30%_collar_k8"] = fit
            print(json.dumps(fit), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
