"""K29, the fused EM sweep (Context.gmm_sweep), timed at the size a user would run it (--size, 16384 squared pixels):

  f15k8_full    15 float32 planes, 8 components, 'full'
  f19k8_full    19 float32 planes, 8 components, 'full'
  u8_7k8_full   7 uint8 planes, 8 components, 'full' (at most 2^26 pixels: --size is capped at 8192 for this case)
  f15k8_diag    15 float32 planes, 8 components, 'diag'
  f15k8_predict the form without a table of f15k8_full (labels, posterior and log-likelihood written)
  f15k8_full_overlap   f15k8_full with the means drawn from a cube of 0.36 instead of 1: the components overlap

The pixels are drawn around the components' means with the components' spread (sigma 0.12).  With the means spread over a unit
cube the components are separate and nearly every pixel carries ONE non-zero weight, the best case for the accumulation, whose
work follows the non-zero weights; the overlap case is the other side.  nonzero_weights_per_pixel is recorded from a crop.
Per case, in this process: device events around the call, one warm-up and then --reps calls (minimum, median and the spread (max - min) / min), and the library's own kernel timer ("gmm_sweep": the launch
without the readback).  Held against
  (a) a device-to-device copy of as many bytes as the case reads: ratio_to_copy;
  (b) the hard two-pass alternative on the same planes and model: Context.gauss_classify (K22 labels) followed by
      Context.class_moments on those labels (K24: the full triangle); uint8 planes are widened first for K22:
      ratio_to_hard_two_pass = two-pass / sweep.  k passes of K24 for soft weights would cost k times its share;
  (c) one scikit-learn EM iteration on a --sk-size squared crop with 16 threads (fit with max_iter 3 less fit with max_iter 1,
      halved), scaled to the case's pixel count: ratio_to_sklearn.
One JSON object on stdout (and in --out).
Usage: python profiles/gmm_bench.py [--size 16384] [--reps 7] [--sk-size 1024] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# planes, components, uint8, diag, table, half-width of the cube the means are drawn from
CASES = {"f15k8_full": (15, 8, False, False, True, 0.5), "f19k8_full": (19, 8, False, False, True, 0.5),
         "u8_7k8_full": (7, 8, True, False, True, 0.5), "f15k8_diag": (15, 8, False, True, True, 0.5),
         "f15k8_predict": (15, 8, False, False, False, 0.5), "f15k8_full_overlap": (15, 8, False, False, True, 0.18)}
SIGMA = 0.12


def make_case(torch, device, name, n, seed=29):
    """(planes, kernel model, weights, means, sigma in plane units, bytes read)"""
    from rsseg.gmm import q_for
    F, k, u8, diag, _, half = CASES[name]
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    means = rng.uniform(-half, half, (k, F))
    sigma = SIGMA
    if u8:
        means, sigma = np.rint(127.5 + 127.5 * means), 127.5 * SIGMA
    comp = torch.randint(0, k, (n,), generator=g, device=device)
    mt = torch.tensor(means, dtype=torch.float32, device=device)
    planes = []
    for f in range(F):
        p = mt[:, f][comp] + sigma * torch.randn(n, generator=g, device=device, dtype=torch.float32)
        planes.append(p.clamp_(0, 255).round_().to(torch.uint8) if u8 else p.clamp_(-1, 1))
    del comp
    W = np.stack([np.eye(F) / sigma] * k)
    i, f = np.tril_indices(F)
    weights = np.full(k, 1.0 / k)
    offset = np.full(k, 2.0 * F * np.log(sigma) - 2.0 * np.log(1.0 / k))
    model = dict(mean=means, whiten=np.ascontiguousarray(W[:, i, f]), offset=offset, plane_exp=None if u8 else [0] * F, Q=q_for(n), diag=diag)
    return planes, model, weights, means, sigma, (1 if u8 else 4) * F * n


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
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), spread=float((np.max(ms) - np.min(ms)) / np.min(ms)),
                runs=[float(x) for x in ms])


def copy_ms(torch, ctx, nbytes, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device).zero_()
    dst = torch.empty_like(src)
    return event_ms(torch, ctx.torch_stream, lambda: dst.copy_(src), reps)


def prof_ms(ctx, name, fn, reps):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for _ in range(reps):
            fn()
        ms, calls = ctx.prof_get(name)
    finally:
        ctx.prof_enable(False)
    return ms / max(calls, 1)


def sklearn_iteration_s(planes, k, diag, weights, means, sigma, crop):
    """Seconds of one EM iteration of GaussianMixture on the first crop^2 pixels, 16 threads."""
    from sklearn.mixture import GaussianMixture
    import warnings
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        threadpool_limits = None
    X = np.stack([p[:crop * crop].cpu().numpy().astype(np.float64) for p in planes], axis=1)
    F = X.shape[1]
    prec = np.full((k, F), 1.0 / sigma ** 2) if diag else np.stack([np.eye(F) / sigma ** 2] * k)

    def fit(iters):
        gm = GaussianMixture(k, covariance_type="diag" if diag else "full", tol=0.0, max_iter=iters, weights_init=weights, means_init=means,
                             precisions_init=prec)
        t = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm.fit(X)
        return time.perf_counter() - t

    def both():
        fit(1)
        return min((fit(3) - fit(1)) / 2.0 for _ in range(2))
    if threadpool_limits is None:
        return both(), None
    with threadpool_limits(limits=16):
        return both(), 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sk-size", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from rsseg.runtime import Context
    from rsseg.signatures import q_for as q24
    ctx = Context(0, use_dist=False)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, reps=a.reps, sklearn_crop=a.sk_size, cases={})
    for name in a.cases.split(","):
        F, k, u8, diag, want_table, _ = CASES[name]
        size = min(a.size, 8192) if u8 else a.size
        n = size * size
        planes, model, weights, means, sigma, nbytes = make_case(torch, ctx.device, name, n)
        outs = {} if want_table else dict(want_labels=True, want_posterior=True, want_loglik=True)
        call = lambda: ctx.gmm_sweep(planes, model, want_table=want_table, **outs)   # noqa: E731
        ms = event_ms(torch, ctx.torch_stream, call, a.reps)
        kernel = prof_ms(ctx, "gmm_sweep", call, a.reps)
        cp = copy_ms(torch, ctx, nbytes, a.reps)
        path, tile = ctx.gmm_plan(F, k, u8, diag)
        crop = [p[:1 << 20] for p in planes]
        pr = ctx.gmm_sweep(crop, dict(model, Q=20), want_table=False, want_proba=True)["proba"]
        c = dict(planes=F, components=k, dtype="uint8" if u8 else "float32", covariance="diag" if diag else "full", table=want_table, size=size,
                 pixels=n, path=path, tile=tile, Q=model["Q"], bytes_read=nbytes, call_ms=ms, kernel_ms=kernel, copy_of_bytes_read_ms=cp,
                 ratio_to_copy=ms["min"] / cp["min"], ns_per_pixel=kernel * 1e6 / n,
                 nonzero_weights_per_pixel=float((pr >= 2.0 ** -21).sum().item() / pr.shape[1]),
                 float64_fma_per_pixel_e_step=k * ((2 * F) if diag else (F * (F + 1) // 2 + F)))
        del pr, crop
        if want_table:
            fl = [ctx.widen_u8(p) for p in planes] if u8 else planes

            def two_pass():
                lab, _, _ = ctx.gauss_classify(fl, model["mean"], model["whiten"], model["offset"], np.arange(1, k + 1))
                return ctx.class_moments(planes, lab, k + 1, model["plane_exp"], 0 if u8 else q24(n))
            tp = event_ms(torch, ctx.torch_stream, two_pass, a.reps)
            k22 = prof_ms(ctx, "gauss_classify", two_pass, 3)
            k24 = prof_ms(ctx, "class_moments", two_pass, 3)
            c.update(hard_two_pass_k22_k24_ms=tp, k22_kernel_ms=k22, k24_kernel_ms=k24, ratio_to_hard_two_pass=tp["min"] / ms["min"],
                     k22_plus_k_times_k24_ms=k22 + k * k24, ratio_to_k22_plus_k_times_k24=(k22 + k * k24) / kernel)
            del fl
            sk, threads = sklearn_iteration_s(planes, k, diag, weights, means, sigma, a.sk_size)
            c.update(sklearn_iteration_s_on_crop=sk, sklearn_threads=threads, sklearn_iteration_ms_scaled=sk * 1e3 * n / (a.sk_size ** 2),
                     ratio_to_sklearn=sk * 1e3 * n / (a.sk_size ** 2) / ms["min"])
        res["cases"][name] = c
        print(json.dumps({name: c}), file=sys.stderr, flush=True)
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
