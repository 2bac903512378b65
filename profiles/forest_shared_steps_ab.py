#!/usr/bin/env python3
"""The four entry points of the K11 forest walk (csrc/k11_forest*.hip), two builds of the library against each other, in the
manner of profiles/window_shared_steps_ab.py: the same inputs for both, each build in a process of its own, the builds
alternating for several rounds, HIP-event time per launch from the context's profiler, every output hashed so that the builds
are also compared bit for bit.

The forest is the config-5 forest of bench.py (fit_c5_forest: 100 trees, depth 16, 8 classes, 19 features), fitted once by
a first process and handed to the others as a file.  Cases (profiler family in brackets):
  labels        [forest]        rsseg_forest_predict on the 19-plane stack of a size x size scene (the config-5 call of bench.py)
  conf_labels   [forest_proba]  rsseg_forest_predict_proba with confidence and labels, same planes
  all           [forest_proba]  ... with probabilities, confidence and labels
  oob           [forest_oob]    rsseg_forest_oob on the first --oob-size^2 pixels, seeded counts in {0, 1, 2}
  perm          [forest_perm]   rsseg_forest_permutation_counts on the first --perm-samples pixels: 96 jobs (19 features x 5
                                seeded permutations + the unpermuted rows), seeded labels
That forest fits the LDS (at most 2763 nodes per tree): the five cases above time LDS-group kernels <8, 1024>.  The GENERAL
kernels are timed on two more forests, the same four entry points each (cases `gen300k-*`, `gen17-*`, `gen33-*`):
  gen300k       the out-of-bag case of profiles/forest_proba_bench.py: rsseg.forest_fit.fit of 100 trees on the 300 000
                samples of forest_fit_bench.data (19 features, 3 classes, trees up to ~58 000 nodes -> <4, 1024>), its own
                bootstrap counts, the same 300 000 samples; perm: 96 jobs
  gen17, gen33  the wide rows: the synthetic general forests `gen-nc32-th1024` (17 classes, 5 features -> <32, 1024>) and
                `gen-nc64-th512` (33 classes -> <64, 512>) of tests/forest_matrix_cases.py, six trees, over 2^22 seeded rows
                of integer-valued features; perm: 3 jobs

  driver:  python profiles/forest_shared_steps_ab.py --parent <parent librsseg_hip.so> [--new <librsseg_hip.so>] [--rounds 3]
                                                     [--resources table.json] > forest_shared_steps_ab.json
  worker:  python profiles/forest_shared_steps_ab.py --lib <librsseg_hip.so> --forest forest.npz
  merge:   python profiles/forest_shared_steps_ab.py --merge name=session.json [name=session.json ...]   (several drivers' outputs
           in one file, as profiles/forest_shared_steps_ab.json holds them)

A case passes if the median of the new build is no slower than the SLOWEST run of the parent in the same session (the
parent's spread on the day is the margin).  --resources names the per-kernel table of profiles/code_object_diff.py, recorded
beside the times."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_LIB = os.path.join(ROOT, "rs-image-segmentation_amd", "librsseg_hip.so")
LAUNCHES = 5


def _imports(lib_path):
    sys.path[:0] = [os.path.join(ROOT, "rs-image-segmentation_amd"), ROOT]
    import numpy as np
    import torch

    import bench
    from rsseg import _lib as L
    L.LIB_PATH = os.path.abspath(lib_path)
    from rsseg import pipeline as P
    from rsseg.runtime import Context
    return np, torch, bench, L, P, Context


def fit(lib_path, forest_path):
    np, torch, bench, L, P, Context = _imports(lib_path)
    fm = bench.fit_c5_forest(torch, None, torch.device("cuda", 0), P, 0, 1, 16384)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from forest_fit_bench import data
    from sklearn.ensemble import RandomForestClassifier
    from rsseg import forest_fit as FF
    from rsseg.forest import _flat_for_proba
    X, y = data(300000)
    ctx = Context(0, use_dist=False)
    model = FF.fit(RandomForestClassifier(n_estimators=100, random_state=42), X, y, ctx=ctx)
    ctx.close()
    big = {"g_" + k: v for k, v in _flat_for_proba(model).items()}
    big["g_counts"] = np.stack([FF.bootstrap_counts(int(t.random_state), len(y)) for t in model.estimators_]).astype(np.int32)
    np.savez(forest_path, **fm["flat"], **big)


def worker(lib_path, forest_path, size, oob_size, perm_samples):
    np, torch, bench, L, P, Context = _imports(lib_path)
    stored = dict(np.load(forest_path))
    flat = {k: v for k, v in stored.items() if not k.startswith("g_")}
    flat["n_features"] = int(flat["n_features"])
    ctx = Context(0, use_dist=False)
    dev = ctx.device
    H = W = size
    bands = bench.synth_rows(torch, dev, W, 0, H)
    planes, _ = P.feature_stack19(ctx, bands, H, W)
    fp = P.stack19_forest_planes(ctx, planes)
    del bands, planes
    ctx.forest_load(flat)
    n_trees, n_classes = len(flat["tree_off"]) - 1, int(flat["value"].shape[1])
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    n_oob = oob_size * oob_size
    fp_oob = [p[:n_oob] for p in fp]
    counts = torch.randint(0, 3, (n_trees * n_oob,), dtype=torch.int32, device=dev, generator=g)
    m = perm_samples
    fp_perm = [p[:m] for p in fp]
    y = torch.randint(-1, n_classes, (m,), dtype=torch.int32, device=dev, generator=g)
    src = torch.stack([torch.randperm(m, device=dev, generator=g).to(torch.int32) for _ in range(5)]).reshape(-1).contiguous()
    jobs = np.array([(-1, 0)] + [(f, r) for f in range(len(fp)) for r in range(5)], np.dtype(L.PERM_JOB))
    cases = [
        ("labels", "forest", lambda: [ctx.forest_predict(fp)]),
        ("conf_labels", "forest_proba", lambda: list(ctx.forest_predict_proba(fp, proba=False, confidence=True, labels=True))[1:]),
        ("all", "forest_proba", lambda: list(ctx.forest_predict_proba(fp, proba=True, confidence=True, labels=True))),
        ("oob", "forest_oob", lambda: list(ctx.forest_oob(fp_oob, counts))),
        ("perm", "forest_perm", lambda: [ctx.forest_permutation_counts(fp_perm, y, src, jobs)]),
    ]
    res = {}
    time_cases(ctx, np, cases, res)
    del fp, fp_oob, fp_perm, counts, src, y
    torch.cuda.empty_cache()
    # ---- the general kernels: the forest of the out-of-bag bench, then the two wide-row synthetic forests
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "tests")]
    from forest_fit_bench import data
    import forest_matrix_cases as T
    big = {k[2:]: v for k, v in stored.items() if k.startswith("g_")}
    big_counts = big.pop("counts")
    big["n_features"] = int(big["n_features"])
    forests = [("gen300k", big, data(300000)[0], big_counts, 5)]
    for tag, name in (("gen17", "gen-nc32-th1024"), ("gen33", "gen-nc64-th512")):
        c = T.build(name)
        rs = np.random.default_rng(3)
        forests.append((tag, c.flat, rs.integers(0, 16, (1 << 22, c.spec.F)).astype(np.float32), None, 1))
    for tag, fl, X, cnt, reps in forests:
        ctx.forest_load(fl)
        m, F = X.shape
        nt, nc = len(fl["tree_off"]) - 1, int(fl["value"].shape[1])
        pl = [ctx.to_device(np.ascontiguousarray(X[:, f])) for f in range(F)]
        cnt_d = ctx.to_device(cnt.reshape(-1)) if cnt is not None else torch.randint(0, 3, (nt * m,), dtype=torch.int32, device=dev, generator=g)
        yy = torch.randint(-1, nc, (m,), dtype=torch.int32, device=dev, generator=g)
        ss = torch.stack([torch.randperm(m, device=dev, generator=g).to(torch.int32) for _ in range(reps)]).reshape(-1).contiguous()
        jj = np.array([(-1, 0)] + [(f, r) for f in range(F) for r in range(reps)][:95], np.dtype(L.PERM_JOB))
        if reps == 1:
            jj = jj[:3]
        time_cases(ctx, np, [
            (tag + "-labels", "forest", lambda: [ctx.forest_predict(pl)]),
            (tag + "-all", "forest_proba", lambda: list(ctx.forest_predict_proba(pl, proba=True, confidence=True, labels=True))),
            (tag + "-oob", "forest_oob", lambda: list(ctx.forest_oob(pl, cnt_d))),
            (tag + "-perm", "forest_perm", lambda: [ctx.forest_permutation_counts(pl, yy, ss, jj)]),
        ], res)
        del pl, cnt_d, yy, ss
    nn = np.diff(flat["tree_off"])
    print(json.dumps({"lib": lib_path, "cases": res, "forest": dict(n_trees=n_trees, n_classes=n_classes, nodes_per_tree_max=int(nn.max()),
                                                                    gen300k_nodes_per_tree_max=int(np.diff(big["tree_off"]).max()))}))
    ctx.close()


def time_cases(ctx, np, cases, res):
    for name, fam, call in cases:
        outs = call()                       # warm-up: code object, LDS attribute, allocator
        runs = []
        for _ in range(2):
            del outs
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(LAUNCHES):
                outs = call()
            ctx.sync()
            ms, cnt = ctx.prof_get(fam)
            assert cnt == LAUNCHES, (name, fam, cnt)
            runs.append(round(ms / cnt, 4))
            ctx.prof_enable(False)
        sha = [hashlib.sha256((o if isinstance(o, np.ndarray) else o.cpu().numpy()).tobytes()).hexdigest()[:16] for o in outs]
        del outs
        res[name] = {"family": fam, "ms_per_launch": runs, "sha256_16": sha}


def driver(args):
    out = {"note": f"ms per launch: labels / conf_labels / all on {args.size}^2 pixels, oob on {args.oob_size}^2, perm on {args.perm_samples} samples "
                   f"x 96 jobs; per process two timings of {LAUNCHES} launches after one warm-up launch; parent and new build alternate, one "
                   "process each, one after another",
           "rounds": args.rounds, "cases": {}}
    me = [sys.executable, os.path.abspath(__file__)]

    def run(build, cmd):
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:       # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"{build} process exited with {p.returncode}")
        return p.stdout

    with tempfile.TemporaryDirectory() as tmp:
        forest = os.path.join(tmp, "forest.npz")
        run("fit", me + ["--lib", args.parent, "--fit", forest])
        for _ in range(args.rounds):
            for build, lib in (("parent", args.parent), ("new", args.new)):
                txt = run(build, me + ["--lib", lib, "--forest", forest, "--size", str(args.size), "--oob-size", str(args.oob_size),
                                       "--perm-samples", str(args.perm_samples)])
                got = json.loads(txt.strip().splitlines()[-1])
                out["forest"] = got["forest"]
                for name, r in got["cases"].items():
                    c = out["cases"].setdefault(name, {"family": r["family"], "parent": [], "new": [], "sha": {"parent": set(), "new": set()}})
                    c[build].extend(r["ms_per_launch"])
                    c["sha"][build].add(tuple(r["sha256_16"]))
                sys.stderr.write(f"[forest_shared_steps_ab] {build}: " + ", ".join(f"{k} {v['ms_per_launch']}" for k, v in got["cases"].items()) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for name, c in out["cases"].items():
        sha = c.pop("sha")
        c["bit_identical"] = len(sha["parent"] | sha["new"]) == 1
        c["sha256_16"] = sorted(sha["parent"] | sha["new"])
        c["parent_min_max"] = [min(c["parent"]), max(c["parent"])]
        c["new_median"] = med(c["new"])
        c["parent_median"] = med(c["parent"])
        c["passes"] = c["new_median"] <= max(c["parent"])
    out["all_pass"] = all(c["passes"] and c["bit_identical"] for c in out["cases"].values())
    if args.resources:
        out["code_objects_parent_new"] = json.load(open(args.resources))
    print(json.dumps(out, indent=1))


def merge(parts):
    out = {}
    for part in parts:
        name, path = part.split("=", 1)
        out[name] = json.load(open(path))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--fit", help="worker: fit the config-5 forest and write it to this file")
    ap.add_argument("--forest")
    ap.add_argument("--parent")
    ap.add_argument("--new", default=NEW_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--oob-size", type=int, default=4096)
    ap.add_argument("--perm-samples", type=int, default=200000)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--resources")
    ap.add_argument("--merge", nargs="+", metavar="NAME=FILE")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge)
    elif a.lib and a.fit:
        fit(a.lib, a.fit)
    elif a.lib:
        worker(a.lib, a.forest, a.size, a.oob_size, a.perm_samples)
    elif a.parent:
        driver(a)
    else:
        ap.error("--lib (worker) or --parent (driver)")
