"""Stage 1 on the GPU (K15, rsseg_preprocess_u8): device-event times of the range pass and the stretch pass at 16384^2 x 7 for
uint8, uint16 and float32 DN, their bytes per pixel and the achieved HBM rate, one JSON object on stdout.  Then the time of
the whole --raw chain on the device (stage 1, then config 3 on its uint8 planes) against config 3 alone on the same planes
computed beforehand.
Usage: python profiles/preprocess_bench.py [--size 16384] [--reps 5] [--warmup 2] [--chain-reps 3] [--no-chain]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))

import torch  # noqa: E402

from rsseg import pipeline as P  # noqa: E402
from rsseg.preprocess import BIAS, GAIN  # noqa: E402
from rsseg.runtime import Context  # noqa: E402

# per-pixel bytes of each pass: read the DN once per pass, write one byte in the stretch
PASS_BYTES = {"uint8": (1, 2), "uint16": (2, 3), "float32": (4, 5)}


def dn_bands(n, dtype, seed):
    """seven smooth fields with noise, in the DN dtype (a TM-like value range for the integer types)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.linspace(0, 6.0, n, device="cuda").view(-1, 1)
    x = torch.linspace(0, 6.0, n, device="cuda").view(1, -1)
    out = []
    for i in range(7):
        f = torch.sin(x * (1 + i * 0.3) + y * 0.7) * torch.cos(y * (1.3 - i * 0.1) - x * 0.2)
        f = (f + 1.0) * 0.5 * (200 - 10 * i) + 20 + torch.rand(n, n, device="cuda", generator=g) * 12
        if dtype == torch.uint16:
            f = f * 50
        out.append(f.to(dtype).reshape(-1).contiguous() if dtype != torch.float32 else f.reshape(-1).contiguous())
        del f
    return out


def passes(ctx, bands, reps, warmup):
    for _ in range(warmup):
        ctx.preprocess_u8(bands, GAIN, BIAS)
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.host_syncs(reset=True)
    for _ in range(reps):
        ctx.preprocess_u8(bands, GAIN, BIAS)
    syncs = ctx.host_syncs()
    torch.cuda.synchronize()
    r = {}
    for name in ("pre_range", "pre_stretch"):
        ms, cnt = ctx.prof_get(name)
        r[name + "_ms"] = ms / cnt if cnt else None
    ctx.prof_enable(False)
    r["host_syncs_per_call"] = syncs / reps
    return r


def chain(ctx, dn, n, reps):
    """median wall ms (synchronised) of config 3 on stage 1's planes computed beforehand, and of stage 1 + config 3 on the
    same DN: the same KMeans input, so the difference is what stage 1 adds"""
    pre = ctx.preprocess_u8(dn, GAIN, BIAS)
    torch.cuda.synchronize()

    def c3(planes):
        lab, meta, _ = P.config3(ctx, planes, n, n, 8, 7, 1, 3)
        torch.cuda.synchronize()
        return meta

    out = {}
    for key, fn in (("stages23_ms", lambda: c3(pre)), ("raw_chain_ms", lambda: c3(ctx.preprocess_u8(dn, GAIN, BIAS)))):
        fn()
        ts, meta = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            meta = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[key] = sorted(ts)[len(ts) // 2]
        out[key.replace("_ms", "_kmeans_iter")] = int(meta["n_iter"]) if meta and "n_iter" in meta else None
    out["stage1_added_ms"] = out["raw_chain_ms"] - out["stages23_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chain-reps", type=int, default=3)
    ap.add_argument("--no-chain", action="store_true", help="the two passes only (what profiles/preprocess_pmc.sh profiles)")
    a = ap.parse_args()
    n = a.size
    ctx = Context(0, use_dist=False)
    res = {"size": n, "bands": 7, "device": torch.cuda.get_device_name(0), "passes": {}}
    for name, dt in (("uint8", torch.uint8), ("uint16", torch.uint16), ("float32", torch.float32)):
        bands = dn_bands(n, dt, 1)
        r = passes(ctx, bands, a.reps, a.warmup)
        px = 7 * n * n
        br, bs = PASS_BYTES[name]
        r["range_B_per_px"], r["stretch_B_per_px"] = br, bs
        r["range_TBps"] = px * br / (r["pre_range_ms"] * 1e-3) / 1e12
        r["stretch_TBps"] = px * bs / (r["pre_stretch_ms"] * 1e-3) / 1e12
        r["both_ms"] = r["pre_range_ms"] + r["pre_stretch_ms"]
        res["passes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del bands
        torch.cuda.empty_cache()
    if not a.no_chain:
        dn = dn_bands(n, torch.uint8, 2)
        res["chain"] = chain(ctx, dn, n, a.chain_reps)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
