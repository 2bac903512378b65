"""Accuracy assessment (K14, rsseg_confusion_counts): device-event times of the two passes on an int32 KMeans-like map
(8 clusters) against an int16 truth raster (5 classes), one JSON object on stdout.
  dense   every pixel valid
  sparse  about 0.1 % of the pixels valid (the rest 0)
For each: the call with the range pass, the call with `known_range`, and the call split by rows over 2 thread-ranks (one
context each, an all-reduce hook between them).  Then the reference-equivalent host evaluation (NumPy masks + scikit-learn,
the steps of scripts/4_evaluate.py) at --host-size, timed on this machine's CPU.
Usage: python profiles/eval_bench.py [--size 16384] [--reps 5] [--warmup 2] [--host-size 4096]"""
import argparse
import json
import os
import sys
import threading
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rsseg import _lib as L  # noqa: E402
from rsseg.runtime import Context  # noqa: E402


def maps(n, density, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    truth = torch.randint(1, 6, (n * n,), device="cuda", dtype=torch.int16, generator=g)
    if density < 1:
        keep = torch.rand(n * n, device="cuda", generator=g) < density
        truth = torch.where(keep, truth, torch.zeros_like(truth))
    noise = torch.randint(0, 8, (n * n,), device="cuda", dtype=torch.int32, generator=g)
    pick = torch.rand(n * n, device="cuda", generator=g) < 0.7
    pred = torch.where(pick, (truth.to(torch.int32) + 2) % 8, noise).contiguous()
    return truth.contiguous(), pred


def timed(ctx, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    ctx.prof_reset()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    r = {}
    for name in ("eval_range", "eval_table"):
        ms, cnt = ctx.prof_get(name)
        r[name + "_ms"] = ms / cnt if cnt else None
    ctx.prof_enable(False)
    r["call_ms_median"] = sorted(wall)[len(wall) // 2]
    return r


class Pair:
    """two thread-ranks on one GPU: rank 0 sums / mins / maxes the two device buffers"""

    def __init__(self):
        self.bar = threading.Barrier(2, timeout=120)
        self.slots = [None, None]
        self.res = None

    def hook(self, rank):
        views = {L.F32: torch.float32, L.F64: torch.float64, L.I64: torch.int64}

        def fn(buf, offset, count, dtype, op):
            t = buf[offset:offset + count * (4 if dtype == L.F32 else 8)].view(views[dtype])
            torch.cuda.synchronize()
            self.slots[rank] = t
            self.bar.wait()
            if rank == 0:
                st = torch.stack(self.slots)
                self.res = st.sum(0) if op == L.SUM else (st.amin(0) if op == L.MIN else st.amax(0))
                torch.cuda.synchronize()
            self.bar.wait()
            t.copy_(self.res)
            torch.cuda.synchronize()
            self.bar.wait()
        return fn


def two_ranks(truth, pred, reps, warmup):
    pair, out, errs = Pair(), [None, None], []
    half = truth.numel() // 2

    def rank(r):
        try:
            c = Context(0, use_dist=False)
            c.install_comm_hook(r, 2, pair.hook(r))
            t, p = (truth[:half], pred[:half]) if r == 0 else (truth[half:], pred[half:])
            out[r] = timed(c, lambda: c.confusion_counts(t, p), reps, warmup)
            c.close()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            pair.bar.abort()
    th = [threading.Thread(target=rank, args=(r,)) for r in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errs:
        raise errs[0]
    return {"rank0": out[0], "rank1": out[1]}


def host_reference(n, seed):
    """The steps of scripts/4 on the host (NumPy masks, np.unique per cluster, scikit-learn), seconds."""
    from sklearn.metrics import accuracy_score, classification_report, cohen_kappa_score, confusion_matrix
    rng = np.random.default_rng(seed)
    truth = rng.integers(1, 6, (n, n)).astype(np.int16)
    pred = np.where(rng.random((n, n)) < 0.7, (truth.astype(np.int32) + 2) % 8, rng.integers(0, 8, (n, n))).astype(np.int32)
    t0 = time.perf_counter()
    valid = truth > 0
    y_true, y_pred = truth[valid], pred[valid]
    np.unique(y_true), np.unique(y_pred)
    mapping = {}
    for c in np.unique(y_pred):
        u, cnt = np.unique(y_true[y_pred == c], return_counts=True)
        mapping[c] = u[np.argmax(cnt)]
    mapped = np.copy(y_pred)
    for c, v in mapping.items():
        mapped[y_pred == c] = v
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        accuracy_score(y_true, mapped)
        cohen_kappa_score(y_true, mapped)
        confusion_matrix(y_true, mapped)
        classification_report(y_true, mapped, output_dict=True)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-size", type=int, default=4096)
    args = ap.parse_args()
    ctx = Context(0, use_dist=False)
    n = args.size
    out = dict(size=n, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               bytes_per_pass=n * n * 6, estimate_ms_both_passes=round(2 * n * n * 6 / 5.9e12 * 1e3, 3), cases={})
    for name, density in (("dense", 1.0), ("sparse", 0.001)):
        truth, pred = maps(n, density, 1 if name == "dense" else 2)
        tv, pv, tab = ctx.confusion_counts(truth, pred)
        v = truth > 0
        want = torch.bincount((truth[v].long() - 1) * 8 + pred[v].long(), minlength=40).reshape(5, 8).cpu().numpy()
        case = dict(n_valid=int(tab.sum()), table_ok=bool(np.array_equal(tab, want)) and tab.shape == (5, 8))
        case["range_pass"] = timed(ctx, lambda: ctx.confusion_counts(truth, pred), args.reps, args.warmup)
        case["known_range"] = timed(ctx, lambda: ctx.confusion_counts(truth, pred, known_range=(1, 5, 0, 7)), args.reps, args.warmup)
        case["two_thread_ranks"] = two_ranks(truth, pred, args.reps, args.warmup)
        for k in ("range_pass", "known_range"):
            c = case[k]
            ms = (c["eval_range_ms"] or 0) + c["eval_table_ms"]
            c["kernels_ms"] = ms
            c["TBps"] = round((2 if k == "range_pass" else 1) * n * n * 6 / (ms * 1e-3) / 1e12, 2)
        out["cases"][name] = case
        print(name, json.dumps(case), file=sys.stderr, flush=True)
        del truth, pred, v
        torch.cuda.empty_cache()
    if args.host_size:
        out["host_reference_s"] = {str(args.host_size): round(host_reference(args.host_size, 3), 3)}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
