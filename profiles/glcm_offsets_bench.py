"""Texture windows with (distance, angle) entries on one 16384^2 uint8 plane: device-event times of the GLCM launch
alone (the quantised plane resident, no upsample), warm-up then several reps, one JSON object on stdout.
  a  21 / 21, distances [1, 2, 3] x the four default angles (10 distinct offsets), 32 levels
  b  7 / 1, the same entries, 32 levels
  c  21 / 21, the default entries, 256 levels
  d  7 / 1 and 21 / 21, the default entries, 32 levels (the kernels of rsseg_glcm_u8)
Usage: python profiles/glcm_offsets_bench.py [--size 16384] [--reps 5] [--warmup 2] [--cases a,b,c,d7,d21]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))

import torch  # noqa: E402

from rsseg.runtime import Context  # noqa: E402

ANGLES = [0, math.pi / 4, math.pi / 2, 3 * math.pi / 4]   # the entries of case a / b: distances [1, 2, 3] x ANGLES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c,d7,d21")
    args = ap.parse_args()
    ctx = Context(0, use_dist=False)
    n = args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randint(0, 256, (n, n), device="cuda", dtype=torch.int32, generator=g)
    ramp = (torch.arange(n, device="cuda", dtype=torch.int32)[:, None] + torch.arange(n, device="cuda", dtype=torch.int32)[None, :]) // 9
    planes = {}
    for levels in (32, 256):
        # half noise, half smooth ramp: runs of equal cells as well as spread histograms
        q = torch.where(base < 128, base % levels, ramp % levels).to(torch.uint8).contiguous().reshape(-1)
        planes[levels] = q
    # glcm_offset_plan([1, 2, 3], ANGLES), written out so that the default cases also run on a tree without it
    multi = [(0, 1), (1, 1), (1, 0), (1, -1), (0, 2), (1, 1), (2, 0), (1, -1), (0, 3), (2, 2), (3, 0), (2, -2)]
    cases = {"a": (32, 21, 21, multi), "b": (32, 7, 1, multi), "c": (256, 21, 21, None),
             "d7": (32, 7, 1, None), "d21": (32, 21, 21, None)}
    out = dict(size=n, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0), cases={})
    for name in args.cases.split(","):
        levels, win, step, offs = cases[name]
        q = planes[levels]
        # the default entries go through the call without `offsets` (the same call on a tree without the keyword)
        kw = {} if offs is None else dict(offsets=offs)
        for _ in range(args.warmup):
            ctx.glcm(q, n, n, levels, win, step, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res, _ = ctx.glcm(q, n, n, levels, win, step, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            del res
        out["cases"][name] = dict(levels=levels, win=win, step=step, entries=None if offs is None else len(offs),
                                  ms_median=sorted(ms)[len(ms) // 2], ms_min=min(ms), ms_max=max(ms))
        print(name, out["cases"][name], file=sys.stderr, flush=True)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
