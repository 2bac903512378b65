"""K17 timed: the default Gabor bank (4 scales x 6 orientations, kernel sizes 5, 5, 5, 15) on the re-normalised 8-bit NIR plane
of the synthetic raster, device-resident.  One JSON object on stdout (and in --out).

Per size, after a warm-up of every call, `reps` rounds alternate in one process:
  group0..group3   Context.filter_bank_norm of one scale group (6 kernels, one launch): the correlation kernel ("correlate") and
                   the in-place normalising pass ("correlate_norm") by the library's device events, and the host's time around
                   the call (it includes the read-back of the extrema between the two)
  write6           a plain device write (memset) of 6 float32 planes            -- 4 x this is the bare write of the 24 planes
  rmw6             an in-place read-modify-write (x *= 1) of 6 float32 planes   -- 4 x this is the normalising pass's traffic
Reported: median, minimum and maximum of each, the bank as the sum over the groups per round, and two yardsticks:
  memory  4 x (write6 + rmw6), medians of the same rounds
  VALU    pixels x vector instructions per pixel / (256 CUs x 4 SIMDs x 16 lanes per cycle x 2.4 GHz).  The instructions per
          pixel are those of the inner loop of the code object built from this tree (one tap row under a run of 4 pixels, 6
          kernels: 128 vector instructions at 5 x 5, 384 at 15 x 15, of which 120 / 360 are v_pk_mul_f32 / v_pk_add_f32 — counted
          in the ISA that hipcc -save-temps keeps: VALU_PER_TAP_ROW below, or --isa FILE to count afresh), times ksize / 4;
          staging and the epilogue are not in it.  A launch without a count gets no VALU bound.
--cpu-size N adds the time of the NumPy restatement (tests/gabor_ref.py: NOT OpenCV) of the bank on an N x N crop.
Usage: python profiles/gabor_bench.py [--sizes 4096,16384] [--reps 7] [--cpu-size 1024] [--isa FILE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench as B  # noqa: E402
from rsseg import pipeline as P  # noqa: E402
from rsseg.gabor import gabor_plan  # noqa: E402
from rsseg.runtime import Context  # noqa: E402

# Vector instructions of the inner loop body (one tap row under a run of 4 pixels), by (ksize, kernels of the launch), as built
# by ROCm 7.2.0 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0) with the flags of csrc/Makefile.  Counted by count_isa() below in
# the file that
#   hipcc <CXXFLAGS of csrc/Makefile> -save-temps=obj -c k17_correlate.hip -o DIR/k17.o
# leaves as DIR/k17_correlate-hip-amdgcn-amd-amdhsa-gfx950.s.  Another compiler or a changed kernel makes these stale: pass that
# file as --isa and the count is taken from it instead; the JSON records which of the two was used.
VALU_PER_TAP_ROW = {(5, 6): 128, (15, 6): 384}
VALU_COUNTED_WITH = "ROCm 7.2.0, HIP 7.2.26015, AMD clang 22.0.0git (roc-7.2.0)"


def count_isa(path):
    """{(ksize, kernels): vector instructions of the inner loop} from hipcc's -save-temps ISA of k17_correlate.hip: per
    k17_correlate<K, NF>, the basic block that holds the most v_pk_mul_f32 (the tap-row loop; a build that does not pack
    has them as v_mul_f32), and in it every instruction whose mnemonic starts with v_."""
    import re
    out, key, blocks = {}, None, []

    def close():
        if key is not None and blocks:
            best = max(blocks, key=lambda b: b[1])
            if best[1]:
                out[key] = best[0]

    for line in open(path):
        m = re.match(r"^_Z13k17_correlateILi(\d+)ELi(\d+)EEv\w*:", line)
        if m:
            close()
            key, blocks = (int(m.group(1)), int(m.group(2))), [[0, 0]]
            continue
        if key is None:
            continue
        if line.startswith(".LBB"):
            blocks.append([0, 0])
        elif line.startswith("\tv_"):
            blocks[-1][0] += 1
            if line.startswith(("\tv_pk_mul_f32", "\tv_mul_f32")):
                blocks[-1][1] += 1
        elif line.startswith("\ts_endpgm"):
            close()
            key = None
    return out
LANE_RATE = 256 * 4 * 16 * 2.4e9         # vector lanes issued per second at one instruction per 4 cycles and SIMD


def stats(v):
    v = np.asarray(v, float)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), runs=[round(float(x), 4) for x in v])


def event_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def group_call(ctx, q, H, W, taps):
    ctx.prof_reset()
    t0 = time.perf_counter()
    out = ctx.filter_bank_norm(q, H, W, taps)
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    k, nk = ctx.prof_get("correlate")
    n, nn = ctx.prof_get("correlate_norm")
    assert nk == 1 and nn == 1, (nk, nn)
    del out
    return k, n, host


def one_size(ctx, dev, size, reps, valu_table):
    H = W = size
    n = H * W
    nir = B.synth_rows(torch, dev, W, 0, H, want=[3])[0]
    q = ctx.quantize_u8(P.renormalize(ctx, nir), 255.0)
    del nir
    plan = gabor_plan()
    buf = torch.empty(6 * n, dtype=torch.float32, device=dev)
    buf.zero_()
    for _, taps in plan:   # warm-up: code objects, workspace, allocator
        group_call(ctx, q, H, W, taps)
    event_ms(buf.zero_)
    event_ms(lambda: buf.mul_(1.0))
    t = {f"group{g}_{part}": [] for g in range(len(plan)) for part in ("kernel", "norm", "host")}
    t.update(write6=[], rmw6=[], bank_device=[], bank_host=[])
    for _ in range(reps):
        dev_sum = host_sum = 0.0
        for g, (_, taps) in enumerate(plan):
            k, nm, host = group_call(ctx, q, H, W, taps)
            t[f"group{g}_kernel"].append(k)
            t[f"group{g}_norm"].append(nm)
            t[f"group{g}_host"].append(host)
            dev_sum += k + nm
            host_sum += host
        t["bank_device"].append(dev_sum)
        t["bank_host"].append(host_sum)
        t["write6"].append(event_ms(buf.zero_))
        t["rmw6"].append(event_ms(lambda: buf.mul_(1.0)))
    res = {k: stats(v) for k, v in t.items()}
    res["pixels"] = n
    res["groups"] = []
    for g, (ksize, taps) in enumerate(plan):
        row = valu_table.get((ksize, len(taps)))     # None: no count for this launch, no VALU bound claimed
        per_px = row * ksize / 4.0 if row else None
        valu_ms = n * per_px / LANE_RATE * 1e3 if row else None
        mem_ms = res["write6"]["median_ms"]
        k_ms = res[f"group{g}_kernel"]["median_ms"]
        res["groups"].append(dict(ksize=ksize, kernels=len(taps), valu_instructions_per_pixel=per_px, valu_bound_ms=valu_ms, write_bound_ms=mem_ms,
                                  kernel_median_ms=k_ms, kernel_over_valu_bound=k_ms / valu_ms if row else None, kernel_over_write_bound=k_ms / mem_ms,
                                  norm_median_ms=res[f"group{g}_norm"]["median_ms"], norm_over_rmw=res[f"group{g}_norm"]["median_ms"] / res["rmw6"]["median_ms"]))
    res["yardstick_memory_ms"] = 4 * (res["write6"]["median_ms"] + res["rmw6"]["median_ms"])
    res["yardstick_valu_ms"] = sum(g["valu_bound_ms"] for g in res["groups"]) if all(g["valu_bound_ms"] for g in res["groups"]) else None
    res["bank_mpx_s"] = n / res["bank_device"]["median_ms"] / 1e3
    del buf, q
    return res


def cpu_restatement(size):
    import gabor_ref as R
    from oracle import ref_np as O
    u8 = O.to_u8(O.robust_normalize(O.synthetic_raster(size, size)[3]))
    t0 = time.perf_counter()
    out = R.bank_ref(u8)
    return dict(size=size, what="tests/gabor_ref.py (NumPy restatement of the bank, one thread; not OpenCV)", planes=len(out), seconds=time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-size", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--isa", default="", help="hipcc -save-temps ISA of k17_correlate.hip: count the inner loops there")
    a = ap.parse_args()
    valu_table = count_isa(a.isa) if a.isa else VALU_PER_TAP_ROW
    dev = torch.device("cuda", 0)
    ctx = Context(0, use_dist=False)
    ctx.prof_enable(True)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, sizes={},
               valu_count=dict(source=f"counted in {os.path.basename(a.isa)}" if a.isa else f"recorded in the script ({VALU_COUNTED_WITH})",
                               per_tap_row={f"{k}x{k}x{f}": v for (k, f), v in sorted(valu_table.items())}))
    for size in [int(s) for s in a.sizes.split(",") if s]:
        res["sizes"][str(size)] = one_size(ctx, dev, size, a.reps, valu_table)
        torch.cuda.empty_cache()
        print(json.dumps({str(size): res["sizes"][str(size)]}), file=sys.stderr, flush=True)
    if a.cpu_size:
        res["cpu_restatement"] = cpu_restatement(a.cpu_size)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
