"""K11's outputs beyond the label, timed: one JSON object on stdout (and in --out).

Inference: the config-5 forest of bench.py (fit_c5_forest: 100 trees, depth 16, 8 classes) on the 19-plane stack of a
size x size synthetic scene.  Three calls alternate in one process, each timed by the library's device events (prof_scope,
names "forest" / "forest_proba"):
  labels        rsseg_forest_predict
  conf_labels   rsseg_forest_predict_proba with confidence and labels
  all           rsseg_forest_predict_proba with probabilities, confidence and labels
and, in the same rounds, a plain device write (memset) of as many bytes as each of the two probability calls writes.
Reported: median, minimum and maximum of each.  The yardstick of a probability call is the median of `labels` plus the
median of the plain write of its output bytes; the margin is the spread (max - min) `labels` shows in the same run.

Out-of-bag: rsseg.forest_fit.fit_oob minus fit on the data of profiles/forest_fit_bench.py (19 features, 3 classes, 100
trees), beside scikit-learn's fit(oob_score=True) minus fit() with --jobs threads; and the kernel alone ("forest_oob").
Recorded without a target.
Usage: python profiles/forest_proba_bench.py [--sizes 4096,16384] [--reps 7] [--oob-sizes 9216,300000] [--trees 100]
                                             [--jobs 16] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.ensemble import RandomForestClassifier  # noqa: E402

import bench as B  # noqa: E402
from forest_fit_bench import data  # noqa: E402
from rsseg import forest_fit as FF  # noqa: E402
from rsseg import pipeline as P  # noqa: E402
from rsseg.runtime import Context  # noqa: E402


def stats(v):
    v = np.asarray(v, float)
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), runs=[round(float(x), 4) for x in v])


def timed(ctx, name, call):
    ctx.prof_reset()
    out = call()
    torch.cuda.synchronize()
    ms, launches = ctx.prof_get(name)
    assert launches == 1, (name, launches)
    del out
    return ms


def plain_write(nbytes, buf):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    buf[:nbytes].zero_()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def inference(ctx, dev, flat, size, reps):
    n_classes = int(flat["value"].shape[1])
    H = W = size
    bands = B.synth_rows(torch, dev, W, 0, H)
    planes, _ = P.feature_stack19(ctx, bands, H, W)
    fp = P.stack19_forest_planes(ctx, planes)
    del bands
    n = H * W
    bytes_cl, bytes_all = n * 16, n * (16 + 8 * n_classes)
    buf = torch.empty(bytes_all, dtype=torch.uint8, device=dev)
    calls = {
        "labels": ("forest", lambda: ctx.forest_predict(fp)),
        "conf_labels": ("forest_proba", lambda: ctx.forest_predict_proba(fp, proba=False, confidence=True, labels=True)),
        "all": ("forest_proba", lambda: ctx.forest_predict_proba(fp, proba=True, confidence=True, labels=True)),
    }
    for name, call in calls.values():   # warm-up: code objects, LDS attribute, allocator
        timed(ctx, name, call)
    plain_write(bytes_all, buf)
    t = {k: [] for k in ("labels", "conf_labels", "all", "write_conf_labels", "write_all")}
    for _ in range(reps):
        for k, (name, call) in calls.items():
            t[k].append(timed(ctx, name, call))
        t["write_conf_labels"].append(plain_write(bytes_cl, buf))
        t["write_all"].append(plain_write(bytes_all, buf))
    res = {k: stats(v) for k, v in t.items()}
    spread = res["labels"]["max_ms"] - res["labels"]["min_ms"]
    res["labels"]["mpx_s"] = n / res["labels"]["median_ms"] / 1e3
    for k, w in (("conf_labels", "write_conf_labels"), ("all", "write_all")):
        yard = res["labels"]["median_ms"] + res[w]["median_ms"]
        res[k].update(mpx_s=n / res[k]["median_ms"] / 1e3, yardstick_ms=yard, margin_ms=spread,
                      over_yardstick_ms=res[k]["median_ms"] - yard, within_yardstick=bool(res[k]["median_ms"] <= yard + spread))
    res.update(pixels=n, n_classes=n_classes, output_bytes=dict(labels=n * 8, conf_labels=bytes_cl, all=bytes_all), labels_spread_ms=spread)
    return res


def oob_case(ctx, n, trees, jobs):
    X, y = data(n)
    kw = dict(n_estimators=trees, random_state=42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        FF.fit_oob(RandomForestClassifier(n_estimators=2, random_state=0, oob_score=True), X[:1000], y[:1000], ctx=ctx)   # warm-up
        t0 = time.perf_counter()
        FF.fit(RandomForestClassifier(**kw), X, y, ctx=ctx)
        t1 = time.perf_counter()
        ctx.prof_reset()
        got = FF.fit_oob(RandomForestClassifier(oob_score=True, **kw), X, y, ctx=ctx)
        t2 = time.perf_counter()
        kern_ms, _ = ctx.prof_get("forest_oob")
        RandomForestClassifier(n_jobs=jobs, **kw).fit(X, y)
        t3 = time.perf_counter()
        want = RandomForestClassifier(n_jobs=jobs, oob_score=True, **kw).fit(X, y)
        t4 = time.perf_counter()
    # with several jobs scikit-learn adds the trees' votes in the order the threads finish: equality is the tests' business (n_jobs=None)
    return dict(samples=n, fit_ms=(t1 - t0) * 1e3, fit_oob_ms=(t2 - t1) * 1e3, oob_extra_ms=(t2 - t1 - (t1 - t0)) * 1e3, oob_kernel_ms=kern_ms,
                nodes_per_tree_max=int(max(t.tree_.node_count for t in got.estimators_)),
                sklearn_fit_ms=(t3 - t2) * 1e3, sklearn_fit_oob_ms=(t4 - t3) * 1e3, sklearn_oob_extra_ms=(t4 - t3 - (t3 - t2)) * 1e3,
                oob_score=float(got.oob_score_), sklearn_oob_score=float(want.oob_score_),
                max_abs_diff_vs_sklearn_threads=float(np.abs(got.oob_decision_function_ - want.oob_decision_function_).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oob-sizes", default="9216,300000")
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = Context(0, use_dist=False)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, inference={}, out_of_bag={}, sklearn_jobs=a.jobs, trees=a.trees)
    if a.sizes:
        fm = B.fit_c5_forest(torch, None, dev, P, 0, 1, 16384)
        nn = np.diff(fm["flat"]["tree_off"])
        res["forest"] = dict(n_trees=len(nn), nodes_per_tree_max=int(nn.max()), n_classes=int(fm["flat"]["value"].shape[1]))
        ctx.forest_load(fm["flat"])
        ctx.prof_enable(True)
        for size in [int(s) for s in a.sizes.split(",")]:
            try:
                res["inference"][str(size)] = inference(ctx, dev, fm["flat"], size, a.reps)
            except (MemoryError, torch.OutOfMemoryError) as e:
                res["inference"][str(size)] = dict(skipped=f"out of memory: {e}"[:200])
            torch.cuda.empty_cache()
            print(json.dumps({str(size): res["inference"][str(size)]}), file=sys.stderr, flush=True)
    ctx.prof_enable(True)
    for n in [int(s) for s in a.oob_sizes.split(",") if s]:
        res["out_of_bag"][str(n)] = oob_case(ctx, n, a.trees, a.jobs)
        print(json.dumps({str(n): res["out_of_bag"][str(n)]}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
