#!/usr/bin/env python3
"""The epsilon-SVR on the resident triangle (fsk_svr_train, fsk_svr_cv) on one GPU -> profiles/svr.json.

  (a) csvc     the UNCHANGED C-SVC solve against --parent-lib (a build of the commit before the SVR), in one process, in
               either seat, as tools/bench_svm_weighted.py does: ep300 (workgroup form) and dna32k (two-launch form);
  (b) svr      microseconds an iteration of fsk_svr_train at 2,000 (EP300), 4,096 (the last workgroup size; the first 4,096
               train rows of EP300_47848), 6,506 (EP300_47848) and 32,000 rows (synthetic DNA), beside fsk_svm_train at the
               same n. Targets: the label -1 / +1 plus a seeded normal of sigma 0.25. The solver is latency-bound and every
               kernel cell is read once for the two twins, so the two should be close; more than the C-SVC figure at 2n rows
               would mean the pairing does not work;
  (c) host     scikit-learn's SVR(kernel="precomputed", shrinking=False) on the host, getter included, at 2,000 and 6,506 rows;
  (d) cv       fsk_svr_cv with 5 folds x 3 C x 2 epsilon at 2,000 rows against its slowest problem alone and the 30 problems one
               after another (fsk_svr_train on the kernels of the folds' training sequences).

    tools/bench_svr.py [--parts csvc,svr,host,cv] [--parent-lib PATH] [--rounds 5] [--max-iter 20000] [--out profiles/svr.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_svm import golden, synthetic  # noqa: E402

NEW = ("fsk_svr_train", "fsk_svr_get_model", "fsk_svr_cv", "fsk_svr_cv_get")


def head(data, n):
    tok, off, y = data
    return tok[:off[n]], off[:n + 1], y[:n]


SIZES = {"ep300_2000": dict(data=lambda: golden("EP300"), g=10, m=6, combos=None),
         "ep47848_4096": dict(data=lambda: head(golden("EP300_47848"), 4096), g=10, m=6, combos=100),
         "ep47848_6506": dict(data=lambda: golden("EP300_47848"), g=10, m=6, combos=100),
         "dna_32000": dict(data=lambda: synthetic(32000), g=12, m=8, combos=None)}


def resident(case, tok, off, lib=None, wg_max=None):
    from fastsk_amd import _native
    e = _native.Engine(case["g"], case["m"], lib=lib)
    e.load_sequences(tok, off, len(off) - 1, 0)
    e.accumulate(np.arange(case.get("combos") or e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
    e.finalize()
    if wg_max is not None:
        e.set_tuning("svm_wg_max", wg_max)
    return e


def targets(y, seed=11):
    return y.astype(np.float64) + 0.25 * np.random.Generator(np.random.PCG64(seed)).standard_normal(len(y))


def brief(info):
    it = max(info["iterations"], 1)
    return dict(iterations=info["iterations"], converged=info["converged"], ms=round(info["ms"], 3), form=info["form"], n_sv=info["n_sv"],
                launches=info["launches"], us_per_iteration=round(1e3 * info["ms"] / it, 3))


def part_csvc(parent, rounds, max_iter):
    """(a): this library and the parent's in turns, the parent first and then second."""
    out = {}
    for name, case, wg_max in (("ep300", SIZES["ep300_2000"], None), ("dna32k", SIZES["dna_32000"], 0)):
        tok, off, y = case["data"]()
        for seat in ("first", "second"):
            old = resident(case, tok, off, parent, wg_max) if seat == "first" else None
            e = resident(case, tok, off, None, wg_max)
            if old is None:
                old = resident(case, tok, off, parent, wg_max)
            for x in (e, old):
                x.svm_train(y, 1.0, 1e-3, 50)
            mine, theirs, same = [], [], True
            for _ in range(rounds):
                if seat == "first":
                    theirs.append(brief(old.svm_train(y, 1.0, 1e-3, max_iter))["us_per_iteration"])
                mine.append(brief(e.svm_train(y, 1.0, 1e-3, max_iter))["us_per_iteration"])
                if seat == "second":
                    theirs.append(brief(old.svm_train(y, 1.0, 1e-3, max_iter))["us_per_iteration"])
                a, b = e.svm_model(), old.svm_model()
                same = same and np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2]["iterations"] == b[2]["iterations"] and a[2]["launches"] == b[2]["launches"]
            med = statistics.median(mine)
            out["%s_parent_%s" % (name, seat)] = dict(us_per_iteration=mine, parent_us_per_iteration=theirs, median=med,
                                                      parent_median=statistics.median(theirs), parent_lowest=min(theirs), parent_highest=max(theirs),
                                                      median_over_parents_median=round(med / statistics.median(theirs), 4),
                                                      median_within_the_parents_spread=bool(min(theirs) <= med <= max(theirs)),
                                                      model_equals_the_parents=bool(same), iterations=a[2]["iterations"])
            e.close()
            old.close()
    return out


def part_svr(max_iter, host):
    """(b) and (c)."""
    out = {}
    for name, case in SIZES.items():
        tok, off, y = case["data"]()
        n = len(y)
        z = targets(y)
        e = resident(case, tok, off)
        e.svr_train(z, 1.0, 0.1, 1e-3, 50)   # warm: code objects, buffers
        e.svm_train(y, 1.0, 1e-3, 50)
        r = dict(n_train=n, svr=brief(e.svr_train(z, 1.0, 0.1, 1e-3, max_iter)), csvc_same_n=brief(e.svm_train(y, 1.0, 1e-3, max_iter)))
        r["svr_over_csvc_same_n"] = round(r["svr"]["us_per_iteration"] / r["csvc_same_n"]["us_per_iteration"], 4)
        if host and n in (2000, 6506):
            from sklearn.svm import SVR
            t0 = time.perf_counter()
            K = e.get_train()
            t1 = time.perf_counter()
            m = SVR(kernel="precomputed", C=1.0, epsilon=0.1, tol=1e-3, shrinking=False, cache_size=4000).fit(K, z)
            t2 = time.perf_counter()
            info = e.svr_train(z, 1.0, 0.1, 1e-3, -1)
            r["to_convergence"] = brief(info)
            r["host"] = dict(getter_ms=round(1e3 * (t1 - t0), 3), svr_fit_ms=round(1e3 * (t2 - t1), 3), total_ms=round(1e3 * (t2 - t0), 3),
                             n_sv=int(len(m.support_)))
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        e.close()
    return out


def part_cv():
    """(d): 5 folds x 3 C x 2 epsilon at 2,000 rows."""
    import fastsk_amd
    case = SIZES["ep300_2000"]
    tok, off, y = case["data"]()
    n = len(y)
    z = targets(y)
    Cs, epsilons = [0.1, 1.0, 10.0], [0.05, 0.2]
    fold = fastsk_amd.kfold(n, 5, seed=0)
    e = resident(case, tok, off)
    e.svr_cv(z, fold, Cs, epsilons, 1e-3, 50)   # warm
    cv = e.svr_cv(z, fold, Cs, epsilons, 1e-3, -1)
    e.close()
    alone = []
    for f in range(5):
        rows = np.flatnonzero(fold != f)
        t = np.concatenate([tok[off[r]:off[r + 1]] for r in rows])
        o = np.concatenate(([0], np.cumsum(off[rows + 1] - off[rows]))).astype(np.int64)
        sub = resident(case, t, o)
        sub.svr_train(z[rows], 1.0, 0.1, 1e-3, 50)
        for C in Cs:
            for epsilon in epsilons:
                alone.append(brief(sub.svr_train(z[rows], C, epsilon, 1e-3, -1)))
        sub.close()
    its = [q["iterations"] for q in cv["problems"]]
    return dict(n_train=n, problems=len(its), cv_ms=round(cv["ms"], 3), form=cv["form"], launches=cv["launches"], iterations=its,
                slowest_problem_alone_ms=max(a["ms"] for a in alone), one_after_another_ms=round(sum(a["ms"] for a in alone), 3),
                iterations_alone=sorted(a["iterations"] for a in alone) == sorted(its), mse=cv["mse"].tolist(), r2=cv["r2"].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="csvc,svr,host,cv")
    ap.add_argument("--parent-lib", default=None, help="libfastsk_amd.so built from the commit before the SVR")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svr.json"))
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for both libraries: torch's, loaded first)
    from fastsk_amd import _native
    _native.library()
    parts = args.parts.split(",")
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)
    if "csvc" in parts:
        if not args.parent_lib:
            cur["csvc_against_parent"] = dict(not_run="no --parent-lib given")
        else:
            cur["csvc_against_parent"] = part_csvc(_native.Library(args.parent_lib, optional=NEW), args.rounds, args.max_iter)
        print(json.dumps(cur["csvc_against_parent"]), flush=True)
    if "svr" in parts:
        cur["svr_us_per_iteration"] = part_svr(args.max_iter, "host" in parts)
    if "cv" in parts:
        cur["cross_validate_svr"] = part_cv()
        print(json.dumps(cur["cross_validate_svr"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
