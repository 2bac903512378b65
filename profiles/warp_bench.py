"""K21 (polynomial warp) measured at --size (16384) squared, 7 bands, one process, device events.

Configurations: uint8 and float32 planes x nearest / bilinear / cubic x two plans (a 5 degree rotation about the centre,
and the same with second-order terms that bend the grid by about 13 pixels at the corners).  Every round times each
configuration once, in turn, so that drift hits all of them alike; --warm rounds are dropped, --reps rounds kept, and each
figure is given as min / median / max over the kept rounds.
Yardsticks of the same run: a device-to-device copy of the bytes the call writes (7 output planes; the traffic floor of the
output alone), in the same rounds; and scipy.ndimage.map_coordinates of one float32 band at --cpu-size (4096) squared
for orders 0 and 1, once, on the host.
Beside each time: output pixels per second, taps gathered per second (pixels x bands x 1 / 4 / 16) and the float64
operations per second the kernel's arithmetic needs (counted from the source: per pixel 29 for the coordinates and the
validity test, 6 / 6 / 68 for the state of a valid pixel, per valid pixel and band 0 / 11 / 41), so that the bound can be
named.  The registers / scratch of every instantiation are in profiles/warp_code_objects.json.  Nothing is gated on these figures.
Usage: python profiles/warp_bench.py [--size 16384] [--bands 7] [--reps 9] [--warm 2] [--cpu-size 4096] [--out profiles/warp_bench.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

TAPS = {"nearest": 1, "bilinear": 4, "cubic": 16}
F64_PIXEL = 29                                            # X, Y, 3 products, 2 x (5 mul + 5 add), 4 compares
F64_STATE = {"nearest": 6, "bilinear": 6, "cubic": 68}    # fx, fy, two floors, two sums or fractions; cubic: 6 distances, 4 weights of 6 and 4 of 8 operations
F64_BAND = {"nearest": 0, "bilinear": 11, "cubic": 41}    # per valid pixel and band: conversions aside


def plans(size):
    """coef, cx, cy of the two backward maps (output pixel -> source pixel), both about the centre"""
    c, s = math.cos(math.radians(5.0)), math.sin(math.radians(5.0))
    h = size / 2
    rot = np.array([h, c, -s, 0, 0, 0, h, s, c, 0, 0, 0], np.float64)
    bend = rot.copy()
    k = 13.0 / (h * h)
    bend[3:6] = [k, -0.5 * k, 0.25 * k]
    bend[9:12] = [-0.5 * k, 0.75 * k, k]
    return {"rotate5": rot, "order2": bend}


def stats(ms):
    return dict(min_ms=float(np.min(ms)), median_ms=float(np.median(ms)), max_ms=float(np.max(ms)), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--bands", type=int, default=7)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--cpu-size", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    size, n, nb = a.size, a.size * a.size, a.bands
    st = ctx.torch_stream
    g = torch.Generator(device=ctx.device)
    g.manual_seed(1)
    src = {"uint8": [torch.randint(0, 256, (n,), device=ctx.device, generator=g, dtype=torch.uint8) for _ in range(nb)]}
    src["float32"] = [p.to(torch.float32) for p in src["uint8"]]
    out = {k: [torch.empty(n, dtype=v[0].dtype, device=ctx.device) for _ in range(nb)] for k, v in src.items()}
    pl = plans(size)
    cfgs = [(dt, m, p) for dt in ("uint8", "float32") for m in ("nearest", "bilinear", "cubic") for p in pl]
    copies = {}
    for dt in src:
        nbytes = nb * n * src[dt][0].element_size()
        copies[dt] = (torch.empty(nbytes, dtype=torch.uint8, device=ctx.device), torch.empty(nbytes, dtype=torch.uint8, device=ctx.device))
    ms = {c: [] for c in cfgs}
    cms = {dt: [] for dt in src}
    nvalid = {}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for r in range(a.warm + a.reps):
        for dt in src:
            t = event_ms(lambda: copies[dt][1].copy_(copies[dt][0]))
            if r >= a.warm:
                cms[dt].append(t)
        for c in cfgs:
            dt, m, p = c
            res = []
            t = event_ms(lambda: res.append(ctx.warp_poly(src[dt], size, size, pl[p], size / 2, size / 2, size, size, method=m, out=out[dt])))
            nvalid[p] = res[0][2]
            if r >= a.warm:
                ms[c].append(t)
        print(f"round {r} done", file=sys.stderr, flush=True)

    res = dict(device=torch.cuda.get_device_name(0), size=size, bands=nb, pixels=n, warm=a.warm, reps=a.reps,
               note="device events around the library call (counter reset, launch, 8-byte read-back); rounds alternate over all "
                    "configurations; min / median / max over the kept rounds; the mask plane is written too")
    res["copy_of_output_bytes"] = {}
    for dt in src:
        s = stats(cms[dt])
        nbytes = copies[dt][0].numel()
        s["bytes"] = nbytes
        s["tb_per_s_read_plus_write"] = [2 * nbytes / (s[k] * 1e-3) / 1e12 for k in ("max_ms", "median_ms", "min_ms")]
        res["copy_of_output_bytes"][dt] = s
    res["warp"] = {}
    for c in cfgs:
        dt, m, p = c
        s = stats(ms[c])
        nv = nvalid[p]
        sec = {k: s[k] * 1e-3 for k in ("max_ms", "median_ms", "min_ms")}
        s["n_valid"] = int(nv)
        s["valid_share"] = nv / n
        s["gpixel_per_s"] = [n / v / 1e9 for v in sec.values()]
        s["gtaps_per_s"] = [nv * nb * TAPS[m] / v / 1e9 for v in sec.values()]
        flop = n * F64_PIXEL + nv * (F64_STATE[m] + nb * F64_BAND[m])
        s["f64_tflop_per_s"] = [flop / v / 1e12 for v in sec.values()]
        esz = src[dt][0].element_size()
        s["bytes_written"] = nb * n * esz + n
        s["unique_bytes_read_at_most"] = nb * n * esz
        s["over_copy"] = [s[k] / res["copy_of_output_bytes"][dt]["median_ms"] for k in ("min_ms", "median_ms", "max_ms")]
        res["warp"][f"{dt} {m} {p}"] = s
    # ---- the host, for scale ----
    from scipy import ndimage
    cs = a.cpu_size
    band = src["float32"][0][:cs * cs].cpu().numpy().reshape(cs, cs)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import warp_ref as R
    u, v = R.source_coords(plans(cs)["rotate5"], cs / 2, cs / 2, cs, cs)
    coords = np.stack([v - 0.5, u - 0.5])
    res["cpu_scipy_map_coordinates"] = {"size": cs, "bands": 1, "plan": "rotate5"}
    for order in (0, 1):
        t = time.perf_counter()
        ndimage.map_coordinates(band, coords, order=order, mode="nearest")
        res["cpu_scipy_map_coordinates"][f"order{order}_wall_ms"] = (time.perf_counter() - t) * 1e3
    for m in ("nearest", "bilinear"):
        tm = []
        for r in range(3):
            tm.append(event_ms(lambda: ctx.warp_poly([src["float32"][0][:cs * cs]], cs, cs, plans(cs)["rotate5"], cs / 2, cs / 2, cs, cs, method=m)))
        res["cpu_scipy_map_coordinates"][f"gpu_{m}_one_band_ms"] = stats(tm[1:])
    p = os.path.join(ROOT, "profiles", "warp_code_objects.json")
    if os.path.exists(p):
        res["code_objects"] = {r["kernel"]: dict(vgprs=r["vgprs"][1], sgprs=r["sgprs"][1], scratch=r["scratch"][1], waves_per_simd=r["waves_per_simd"][1])
                               for r in json.load(open(p)) if r["file"] == "k21_warp.hip"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
