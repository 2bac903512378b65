"""Random-forest training (K16, rsseg.forest_fit.fit) against scikit-learn's RandomForestClassifier.fit on the same machine,
one JSON object on stdout (and in --out).  Data: seeded float32 features whose labels follow thresholds on a few features,
with about 10 % of the labels redrawn at random (so the trees are deep), 3 classes; 33 samples is the reference's own
training problem size.  For each size: the whole `fit` call, split into host preparation (validation, seeds, bootstrap
counts), upload, kernels (device events of "forest_fit") and copy-out plus assembly; nodes and depth per tree; scikit-learn
with n_jobs=--jobs on the first --sk-trees trees (scaled to all trees when fewer) and whether those trees are equal.
Usage: python profiles/forest_fit_bench.py [--sizes 33,9216,300000] [--trees 100] [--sk-trees 0 (= all)] [--jobs 16]
                                           [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn.ensemble import RandomForestClassifier  # noqa: E402

from rsseg import forest_fit as FF  # noqa: E402
from rsseg.runtime import Context  # noqa: E402


def data(n, F=19, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, F).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 3] > 0.8).astype(np.int64) + (X[:, 7] * X[:, 11] > 0.3).astype(np.int64)
    flip = rs.rand(n) < 0.1
    y[flip] = rs.randint(0, 3, int(flip.sum()))
    return X, y


def phases(ctx, X, y, T):
    """fit() step by step, timed (the same calls fit makes)."""
    est = RandomForestClassifier(n_estimators=T, random_state=42)
    t0 = time.perf_counter()
    Xf, y_enc, classes, rp = FF.prepare(est, X, y)
    n, F = Xf.shape
    seeds = FF.tree_seeds(est.random_state, T)
    counts = np.stack([FF.bootstrap_counts(int(s), n) for s in seeds])
    caps = 2 * (counts > 0).sum(axis=1) - 1
    xs = np.array([FF.splitter_seed(int(s)) for s in seeds], np.uint32)
    t1 = time.perf_counter()
    planes = [ctx.upload_f32(np.ascontiguousarray(Xf[:, f])) for f in range(F)]
    d_y = ctx.to_device(y_enc, np.int32)
    d_counts = ctx.to_device(counts.reshape(-1), np.int32)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    ctx.prof_reset()
    trees = ctx.forest_fit(planes, d_y, d_counts, xs, caps, rp["max_depth"], rp["min_samples_split"], rp["min_samples_leaf"],
                           rp["max_features"], len(classes))
    t3 = time.perf_counter()
    kern_ms, launches = ctx.prof_get("forest_fit")
    FF.assemble_forest(est, trees, seeds, n, F, classes, rp["max_features"])
    t4 = time.perf_counter()
    return est, dict(host_prep_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, kernels_ms=kern_ms,
                     copy_out_and_assembly_ms=(t3 - t2) * 1e3 - kern_ms + (t4 - t3) * 1e3, forest_fit_calls=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="33,9216,300000")
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--sk-trees", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = Context(0, use_dist=False)
    ctx.prof_enable(True)
    res = dict(trees=a.trees, features=19, classes=3, label_noise=0.1, sklearn_jobs=a.jobs, device=torch.cuda.get_device_name(0),
               cases={})
    from test_forest_fit_host import state_equal
    for n in [int(s) for s in a.sizes.split(",")]:
        X, y = data(n)
        FF.fit(RandomForestClassifier(n_estimators=2, random_state=0), X[: min(n, 1000)], y[: min(n, 1000)], ctx=ctx)   # warm-up
        t0 = time.perf_counter()
        got = FF.fit(RandomForestClassifier(n_estimators=a.trees, random_state=42), X, y, ctx=ctx)
        fit_ms = (time.perf_counter() - t0) * 1e3
        _, ph = phases(ctx, X, y, a.trees)
        nodes = np.array([t.tree_.node_count for t in got.estimators_])
        depth = np.array([t.tree_.max_depth for t in got.estimators_])
        sk_t = a.sk_trees or a.trees
        t0 = time.perf_counter()
        want = RandomForestClassifier(n_estimators=sk_t, random_state=42, n_jobs=a.jobs).fit(X, y)
        sk_ms = (time.perf_counter() - t0) * 1e3
        equal = True
        try:
            for i in range(sk_t):
                state_equal(want.estimators_[i], got.estimators_[i])
        except AssertionError:
            equal = False
        sk_scaled = sk_ms * a.trees / sk_t
        case = dict(samples=n, fit_ms=fit_ms, phases=ph, nodes_per_tree_mean=float(nodes.mean()), nodes_per_tree_max=int(nodes.max()),
                    depth_mean=float(depth.mean()), depth_max=int(depth.max()), sklearn_trees_timed=sk_t, sklearn_ms=sk_ms,
                    sklearn_ms_for_all_trees=sk_scaled, sklearn_scaled=sk_t != a.trees, timed_trees_equal=equal,
                    speedup_vs_sklearn=sk_scaled / fit_ms)
        res["cases"][str(n)] = case
        print(json.dumps({str(n): case}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
