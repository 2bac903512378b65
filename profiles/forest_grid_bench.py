"""The grid-searched forest training (rsseg.forest_grid.grid_search, one K16 call for every fold fit) against the same search
done two other ways on the same machine, and plain `fit` against another build of the library.  One JSON object on stdout (and
in --out).  Data: that of profiles/forest_fit_bench.py (19 seeded float32 features, 3 classes, 10 % label noise).

Search: the reference's default grid (n_estimators 100, max_depth 10 / 20 / None, random_state 42, cv=3: nine fold fits and a
refit), per problem size --runs times each, the three ways alternating within a round:
  (a) sklearn   GridSearchCV(RandomForestClassifier(), grid, cv=3, n_jobs=--jobs)
  (b) composed  the same search from ten separate rsseg.forest_fit.fit calls (nine on X[train], one refit) and nine K11 walks
  (c) batched   grid_search
Wall times around calls that end synchronised (every path ends with host arrays); the first round warms all three up (scikit-learn's
worker pool included) and is not kept.  `equal` says whether (b) and (c) reproduce (a)'s scores and best parameters.

Plain fit (--parent-lib FILE): child processes, alternating between FILE (the library built from the parent commit) and this
tree's library (the order within a round alternating as well), each timing rsseg.forest_fit.fit on --fit-sizes; the kernels behind rsseg_forest_fit read their parameters per
tree, and this shows whether that costs plain `fit` anything.
Usage: python profiles/forest_grid_bench.py [--sizes 33,3000,200000] [--runs 5] [--jobs 16] [--skip-sklearn-above N] [--sklearn-runs K]
           [--parent-lib FILE --fit-sizes 33,9216,300000 --fit-rounds 3 --fit-runs 2] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rs-image-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import numpy as np  # noqa: E402

GRID = {"n_estimators": [100], "max_depth": [10, 20, None], "random_state": [42]}


def data(n):
    from forest_fit_bench import data as d
    return d(n)


def spread(ms):
    ms = np.asarray(ms, float)
    return dict(runs_ms=[float(x) for x in ms], median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))


def composed(ctx, X, y):
    """The search from separate fits: per candidate and fold one forest_fit.fit on the training rows and one walk over the
    held-out rows, then the refit.  Returns (score table, best parameters)."""
    from sklearn.base import clone
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import ParameterGrid, check_cv
    from rsseg import forest_fit as FF
    from rsseg import forest_grid as G
    from rsseg.forest import _flat_for_proba
    cand = list(ParameterGrid(GRID))
    classes, y_enc = np.unique(y, return_inverse=True)
    folds = list(check_cv(3, y, classifier=True).split(X, y))
    scores = np.zeros((len(cand), len(folds)))
    for k, (tr, te) in enumerate(folds):
        planes = [ctx.upload_f32(np.ascontiguousarray(X[te, f])) for f in range(X.shape[1])]
        want = ctx.to_device(y_enc[te], np.int64)
        for c, p in enumerate(cand):
            est = FF.fit(RandomForestClassifier(**p), X[tr], y[tr], ctx=ctx)
            ctx.forest_load(_flat_for_proba(est))
            scores[c, k] = int((ctx.forest_predict(planes) == want).sum().item()) / len(te)
    res = G.format_results(cand, len(folds), scores)
    _, best, _ = G.best_of(res)
    FF.fit(clone(RandomForestClassifier(**best)), X, y, ctx=ctx)
    return scores, best


def search_case(ctx, n, runs, jobs, with_sklearn, sklearn_runs=0):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import GridSearchCV
    from rsseg import forest_grid as G
    X, y = data(n)
    times = {"sklearn": [], "composed": [], "batched": []}
    table = best = None
    equal = True
    for r in range(runs + 1):                      # round 0 warms every path up
        if with_sklearn and (r <= sklearn_runs if sklearn_runs else True) and (r or not sklearn_runs):
            t0 = time.perf_counter()
            sk = GridSearchCV(RandomForestClassifier(), GRID, cv=3, n_jobs=jobs).fit(X, y)
            t = time.perf_counter() - t0
            if r:
                times["sklearn"].append(t * 1e3)
            table = np.stack([sk.cv_results_[f"split{k}_test_score"] for k in range(3)], axis=1)
            best = sk.best_params_
        t0 = time.perf_counter()
        s_b, best_b = composed(ctx, X, y)
        t1 = time.perf_counter()
        got = G.grid_search(RandomForestClassifier(), GRID, X, y, cv=3, ctx=ctx)
        t2 = time.perf_counter()
        if r:
            times["composed"].append((t1 - t0) * 1e3)
            times["batched"].append((t2 - t1) * 1e3)
        s_c = np.stack([got.cv_results_[f"split{k}_test_score"] for k in range(3)], axis=1)
        equal = equal and s_b.tobytes() == s_c.tobytes() and best_b == got.best_params_
        if table is not None:
            equal = equal and table.tobytes() == s_c.tobytes() and best == got.best_params_
        print(f"[forest_grid_bench] n={n} round {r}: " + ", ".join(f"{k} {v[-1]:.0f} ms" for k, v in times.items() if v), file=sys.stderr, flush=True)
    case = dict(samples=n, rounds=runs, equal=bool(equal), compared_with_sklearn=bool(with_sklearn), sklearn_rounds=len(times["sklearn"]),
                **{k: spread(v) for k, v in times.items() if v})
    b, c = case["composed"], case["batched"]
    case["batched_over_composed_median"] = c["median_ms"] / b["median_ms"]
    case["batched_faster_beyond_spread"] = bool(c["max_ms"] < b["min_ms"])
    return case


def plain_fit_child(lib, sizes, runs):
    """Times forest_fit.fit with the library at `lib` (child process of plain_fit)."""
    from rsseg import _lib
    _lib.load(path=lib, missing_ok=("rsseg_forest_fit_jobs",))   # the parent's build lacks the entry point added since
    from sklearn.ensemble import RandomForestClassifier
    from rsseg import forest_fit as FF
    from rsseg.runtime import Context
    ctx = Context(0, use_dist=False)
    out = {}
    for n in sizes:
        X, y = data(n)
        FF.fit(RandomForestClassifier(n_estimators=100, random_state=42), X[: min(n, 2000)], y[: min(n, 2000)], ctx=ctx)   # warm-up
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            FF.fit(RandomForestClassifier(n_estimators=100, random_state=42), X, y, ctx=ctx)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[str(n)] = ts
    ctx.close()
    print("PLAIN_FIT " + json.dumps(out), flush=True)


def plain_fit(parent_lib, sizes, rounds, runs):
    from rsseg import _lib
    libs = {"parent": os.path.abspath(parent_lib), "new": _lib.LIB_PATH}
    got = {k: {str(n): [] for n in sizes} for k in libs}
    for r in range(rounds):
        for name in (("parent", "new") if r % 2 == 0 else ("new", "parent")):   # who goes first alternates too
            lib = libs[name]
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-lib", lib, "--fit-sizes", ",".join(map(str, sizes)),
                                "--fit-runs", str(runs)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(f"plain-fit child ({name}) ended with {p.returncode}: {p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PLAIN_FIT ")][-1]
            for n, ts in json.loads(line[len("PLAIN_FIT "):]).items():
                got[name][n] += ts
            print(f"[forest_grid_bench] plain fit round {r} {name}: {line}", file=sys.stderr, flush=True)
    res = {}
    for n in map(str, sizes):
        p, q = spread(got["parent"][n]), spread(got["new"][n])
        res[n] = dict(parent=p, new=q, new_within_parent_spread=bool(q["median_ms"] <= p["max_ms"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="33,3000,200000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--skip-sklearn-above", type=int, default=0, help="leave (a) out above this size (0: never)")
    ap.add_argument("--sklearn-runs", type=int, default=0, help="time (a) in the first K rounds only, without a warm-up (0: in every round)")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child-lib", default="")
    ap.add_argument("--fit-sizes", default="33,9216,300000")
    ap.add_argument("--fit-rounds", type=int, default=3)
    ap.add_argument("--fit-runs", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fit_sizes = [int(s) for s in a.fit_sizes.split(",") if s]
    if a.child_lib:
        return plain_fit_child(a.child_lib, fit_sizes, a.fit_runs)
    import torch
    from rsseg.runtime import Context
    res = dict(grid=GRID, cv=3, features=19, classes=3, label_noise=0.1, sklearn_jobs=a.jobs, device=torch.cuda.get_device_name(0), search={})
    sizes = [int(s) for s in a.sizes.split(",") if s]
    if sizes:
        ctx = Context(0, use_dist=False)
        for n in sizes:
            res["search"][str(n)] = search_case(ctx, n, a.runs, a.jobs, not (a.skip_sklearn_above and n > a.skip_sklearn_above), a.sklearn_runs)
            print(json.dumps({str(n): res["search"][str(n)]}), file=sys.stderr, flush=True)
        ctx.close()
    if a.parent_lib:
        res["plain_fit"] = plain_fit(a.parent_lib, fit_sizes, a.fit_rounds, a.fit_runs)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
