#!/usr/bin/env python3
"""The cross-validated SVM (fsk_svm_cv: folds x values of C in one batch) on one GPU -> profiles/svm_cv.json.

Workloads (--cases), each on 5 stratified folds (fastsk_amd.stratified_folds, seed 0):
  ep300     tests/golden/tokens_EP300.npz, 2000 train rows, g = 10, m = 6 exact, Cs = 10^(-2 ... 1 in half-decades), 35
            problems, the workgroup form;
  ep47848   tests/golden/tokens_EP300_47848.npz, its 6506 train rows, the first 100 of the 210 combos (BASELINE config 3),
            Cs = 0.1, 1, 10, the form the engine picks;
  dna32k    synthetic DNA 32,000 x 300 (tests/svm_cases.dna), g = 12, m = 8 exact, Cs = 0.1, 1, 10, the two-launch form,
            at most --max-iter steps a problem.
Per case: the batched wall time (host clock around a call that ends in a device synchronise; the second of two calls), the
problems' iteration counts, and
  sequential   the same problems one after another on the device: `per_C`, fsk_svm_cv called with one value of C at a time
               (5 problems side by side a call — the C ABI has no call for a single (fold, C), a fold array being what holds
               rows out), and `per_problem`, fsk_svm_train once a problem on an engine that holds the kernel of that fold's
               training rows alone (solve time only; the kernels' time is given beside it). per_problem runs where
               n <= --subset-max-n;
  host         scikit-learn's SVC(kernel="precomputed", shrinking=False) over the same folds and Cs on the matrix the getter
               copies out, getter time included, where n <= --host-max-n.
What does not run says so in the JSON. The prediction written down before the first measurement: while P <= 256 compute units
the batch costs about what its slowest problem costs alone (`slowest_problem_alone_ms`, from per_problem, beside it).

With --parent-lib none of that runs: the batched call alone, in turns with the same call on another build (versus_parent).

    tools/bench_svm_cv.py [--cases ep300,ep47848,dna32k] [--max-iter 40000] [--out profiles/svm_cv.json]
                          [--parent-lib PATH [--parent-seat first|second] [--rounds 5] [--key SUFFIX]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_svm import golden, synthetic  # noqa: E402

HALF_DECADES = [10.0 ** (k / 2.0) for k in range(-4, 3)]
CASES = {"ep300": dict(data=lambda: golden("EP300"), g=10, m=6, combos=None, Cs=HALF_DECADES, wg_max=None),
         "ep47848": dict(data=lambda: golden("EP300_47848"), g=10, m=6, combos=100, Cs=[0.1, 1.0, 10.0], wg_max=None),
         "dna32k": dict(data=lambda: synthetic(32000), g=12, m=8, combos=None, Cs=[0.1, 1.0, 10.0], wg_max=0)}


def resident(case, tok, off, rows=None):
    """An engine with the kernel of the sequences `rows` (all when None) finalized on the device."""
    from fastsk_amd import _native
    if rows is not None:
        tok = np.concatenate([tok[off[r]:off[r + 1]] for r in rows])
        off = np.concatenate([[0], np.cumsum(np.diff(off)[rows])]).astype(np.int64)
    e = _native.Engine(case["g"], case["m"])
    e.load_sequences(tok, off, len(off) - 1, 0)
    e.accumulate(np.arange(case["combos"] or e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
    e.finalize()
    return e


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def versus_parent(name, parent_path, parent_first, rounds, max_iter, eps, folds):
    """--parent-lib: the batch alone, this library and another build of it (the parent commit's) in turns on one device, as
    tools/bench_svm_weighted.py does for the single solve: both series of milliseconds a call (fsk_svm_cv_info.ms), this
    library's median against the other's own spread, and whether every problem and out-of-fold value is the other's bit for bit."""
    import statistics
    import fastsk_amd
    from fastsk_amd import _native
    case = CASES[name]
    tok, off, y = case["data"]()
    fold = fastsk_amd.stratified_folds(y, folds, seed=0)
    libs = [_native.Library(parent_path), None] if parent_first else [None, _native.Library(parent_path)]
    engines, ms, last = [], ([], []), [None, None]
    for lib in libs:   # (the seat: whose engine is made first and solves first)
        e = _native.Engine(case["g"], case["m"], lib=lib)
        e.load_sequences(tok, off, len(off) - 1, 0)
        e.accumulate(np.arange(case["combos"] or e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
        e.finalize()
        if case["wg_max"] is not None:
            e.set_tuning("svm_wg_max", case["wg_max"])
        e.svm_cv(y, fold, case["Cs"], eps, 50)   # warm: code objects, buffers
        engines.append(e)
    for _ in range(rounds):
        for k, e in enumerate(engines):
            last[k] = e.svm_cv(y, fold, case["Cs"], eps, max_iter)
            ms[k].append(round(last[k]["ms"], 3))
    same = last[0]["problems"] == last[1]["problems"] and np.array_equal(last[0]["decision"], last[1]["decision"]) and \
        last[0]["launches"] == last[1]["launches"] and last[0]["form"] == last[1]["form"]
    mine, theirs = (ms[1], ms[0]) if parent_first else (ms[0], ms[1])
    med = statistics.median(mine)
    for e in engines:
        e.close()
    return dict(case=name, n_train=len(y), problems=len(last[0]["problems"]), form=last[0]["form"], launches=last[0]["launches"],
                iterations=[q["iterations"] for q in last[0]["problems"]], parent_seat="first" if parent_first else "second", ms=mine,
                median_ms=med, parent=dict(ms=theirs, median_ms=statistics.median(theirs), lowest=min(theirs), highest=max(theirs)),
                results_equal_the_parents=bool(same), median_within_the_parents_spread=bool(min(theirs) <= med <= max(theirs)),
                median_over_parents_median=round(med / statistics.median(theirs), 4))


def run_case(name, max_iter, eps, folds, subset_max_n, host_max_n):
    import fastsk_amd
    case = CASES[name]
    tok, off, y = case["data"]()
    n, Cs = len(y), case["Cs"]
    fold = fastsk_amd.stratified_folds(y, folds, seed=0)
    e, kernel_ms = timed(lambda: resident(case, tok, off))
    if case["wg_max"] is not None:
        e.set_tuning("svm_wg_max", case["wg_max"])
    e.svm_cv(y, fold, Cs, eps, 50)   # warm: code objects, buffers
    e.svm_cv(y, fold, Cs, eps, max_iter)
    r, wall = timed(lambda: e.svm_cv(y, fold, Cs, eps, max_iter))
    its = [q["iterations"] for q in r["problems"]]
    out = dict(case=name, n_train=n, g=case["g"], m=case["m"], combos=case["combos"] or "all", folds=folds, Cs=Cs, eps=eps,
               max_iter=max_iter, kernel_ms=round(kernel_ms, 3), problems=len(its), form=r["form"], launches=r["launches"],
               batched_ms=round(wall, 3), batched_ms_library=round(r["ms"], 3), iterations=its,
               converged=[bool(q["converged"]) for q in r["problems"]], auc=[float(a) for a in r["auc"]],
               accuracy=[float(a) for a in r["accuracy"]])
    if not all(out["converged"]):
        out["note"] = "not every problem converged within max_iter: the times are those of a fixed iteration count"
    # sequential on the device, one value of C a call
    per_C = []
    for C in Cs:
        e.svm_cv(y, fold, [C], eps, 50)
        per_C.append(timed(lambda: e.svm_cv(y, fold, [C], eps, max_iter))[1])
    out["sequential_per_C_ms"] = dict(total=round(sum(per_C), 3), calls=[round(t, 3) for t in per_C])
    # sequential on the device, one problem a solve: fsk_svm_train on the kernel of each fold's training rows
    if n <= subset_max_n:
        solves, kernels, same = [[0.0] * folds for _ in Cs], 0.0, True
        for f in range(folds):
            rows = np.flatnonzero(fold != f)
            sub, ms = timed(lambda: resident(case, tok, off, rows))
            kernels += ms
            if case["wg_max"] is not None:
                sub.set_tuning("svm_wg_max", case["wg_max"])
            sub.svm_train(y[rows], Cs[0], eps, 50)
            for ci, C in enumerate(Cs):
                info, solves[ci][f] = timed(lambda: sub.svm_train(y[rows], C, eps, max_iter))
                same = same and info["iterations"] == its[ci * folds + f]
            sub.close()
        flat = [t for row in solves for t in row]
        out["sequential_per_problem_ms"] = dict(total=round(sum(flat), 3), solves=[round(t, 3) for t in flat], subset_kernels_ms=round(kernels, 3))
        out["slowest_problem_alone_ms"] = round(max(flat), 3)
        out["per_problem_iterations_equal_the_batch"] = same
    else:
        out["sequential_per_problem_ms"] = dict(not_run="%d rows: the kernels of %d training subsets are not recomputed here" % (n, folds))
    # the host: scikit-learn over the same folds
    if n <= host_max_n:
        from sklearn.svm import SVC
        K, getter = timed(e.get_train)
        t0 = time.perf_counter()
        dec = np.empty((len(Cs), n))
        for f in range(folds):
            tr, te = np.flatnonzero(fold != f), np.flatnonzero(fold == f)
            Ktr, Kte = K[np.ix_(tr, tr)], K[np.ix_(te, tr)]
            for ci, C in enumerate(Cs):
                clf = SVC(kernel="precomputed", C=C, tol=eps, shrinking=False, cache_size=4000).fit(Ktr, y[tr])
                dec[ci, te] = clf.decision_function(Kte)
        fit = 1e3 * (time.perf_counter() - t0)
        out["host"] = dict(getter_ms=round(getter, 3), svc_ms=round(fit, 3), total_ms=round(getter + fit, 3),
                           largest_decision_difference=float(np.max(np.abs(dec - r["decision"]))))
    else:
        out["host"] = dict(not_run="the square matrix scikit-learn wants is %.1f GB on the host" % (8.0 * n * n / 1e9))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ep300,ep47848,dna32k")
    ap.add_argument("--max-iter", type=int, default=40000)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--subset-max-n", type=int, default=8192)
    ap.add_argument("--host-max-n", type=int, default=8192)
    ap.add_argument("--parent-lib", default=None, help="another build of libfastsk_amd.so: time the batch alone against it, in turns (nothing else runs)")
    ap.add_argument("--parent-seat", choices=("first", "second"), default="first", help="whose engine is made first and solves first in a round")
    ap.add_argument("--rounds", type=int, default=5, help="--parent-lib: calls a library")
    ap.add_argument("--key", default="", help="a suffix for the JSON keys of this run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_cv.json"))
    args = ap.parse_args()
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)
    if args.parent_lib:
        import torch  # noqa: F401  (one HIP runtime for both libraries: torch's, loaded first)
    for name in args.cases.split(","):
        if args.parent_lib:
            res = versus_parent(name, args.parent_lib, args.parent_seat == "first", args.rounds, args.max_iter, args.eps, args.folds)
        else:
            res = run_case(name, args.max_iter, args.eps, args.folds, args.subset_max_n, args.host_max_n)
        print(json.dumps(res), flush=True)
        cur["case_" + name + args.key] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
