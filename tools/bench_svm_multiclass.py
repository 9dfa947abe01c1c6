#!/usr/bin/env python3
"""The one-vs-one multi-class C-SVC (fsk_svm_train_multiclass: the pairs of classes in one batch) on one GPU
-> profiles/svm_multiclass.json.

Workloads (--cases): synthetic 4-class DNA (tests/svm_multiclass_cases.dna: PCG64, one planted 8-mer a class, the classes
interleaved by row, 12 / 22 / 27 / 39 % of the rows as in the reference's WebKB data), 300 symbols a row, g = 12, m = 8 exact:
  dna2000, dna6500   the workgroup form (every pair below svm_wg_max = 8192 rows);
  dna32000           the two-launch form.
At most --max-iter steps a pair. Per case, host clock around calls that end in a device synchronise, the second of two calls:
  fit                fsk_svm_train_multiclass, the six pairs side by side; the pairs' iteration counts;
  pairs_alone        every pair solved alone, fsk_svm_train on an engine that holds the kernel of that pair's rows only (solve time
                     only; the sub-kernels' time beside it): the slowest of them and their sum ("one after another") against the fit;
  decision           fsk_svm_multiclass_decision over the training rows — the pair decisions and the vote in one launch, the copy
                     of the [n, 6] values included — and labels alone; the launch's share of the fit;
  cv                 fsk_svm_multiclass_cv, 5 stratified folds x Cs = 0.1, 1, 10: 90 problems in one batch;
  host               scikit-learn's SVC(kernel="precomputed", shrinking=False, decision_function_shape="ovo") on the matrix the
                     getter copies out, getter time included, where n <= --host-max-n.
None of these is a pass mark. What does not run says so in the JSON.

    tools/bench_svm_multiclass.py [--cases dna2000,dna6500,dna32000] [--max-iter 40000] [--out profiles/svm_multiclass.json]"""
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

from bench_svm_cv import resident, timed  # noqa: E402

SHARES = (0.12, 0.22, 0.27, 0.39)
G, M, LENGTH = 12, 8, 300
CS = [0.1, 1.0, 10.0]


def synthetic(n):
    import svm_multiclass_cases as mc
    sizes = [int(n * s) for s in SHARES[:-1]]
    sizes.append(n - sum(sizes))
    X, y = mc.dna(sizes, 0, LENGTH, 20201214 + n)
    return X.reshape(-1), np.arange(n + 1, dtype=np.int64) * LENGTH, y, sizes


def run_case(n, max_iter, eps, C, folds, host_max_n):
    import fastsk_amd
    import svm_multiclass_cases as mc
    case = dict(g=G, m=M, combos=None)
    tok, off, y, sizes = synthetic(n)
    e, kernel_ms = timed(lambda: resident(case, tok, off))
    e.n_test, e.N = 0, n
    e.svm_train_multiclass(y, C, eps, 50)   # warm: code objects, buffers
    e.svm_train_multiclass(y, C, eps, max_iter)
    info, wall = timed(lambda: e.svm_train_multiclass(y, C, eps, max_iter))
    model = e.svm_multiclass_model()
    its = [q["iterations"] for q in model["pairs"]]
    out = dict(case="dna%d" % n, n_train=n, class_sizes=sizes, g=G, m=M, length=LENGTH, C=C, eps=eps, max_iter=max_iter,
               kernel_ms=round(kernel_ms, 3), pairs=len(its), pair_rows=[q["n_rows"] for q in model["pairs"]], form=info["form"],
               launches=info["launches"], fit_ms=round(wall, 3), fit_ms_library=round(info["ms"], 3), iterations=its,
               converged=[bool(q["converged"]) for q in model["pairs"]], n_sv=info["n_sv"])
    if not all(out["converged"]):
        out["note"] = "not every pair converged within max_iter: the times are those of a fixed iteration count"
    # the decision-and-vote launch
    e.svm_multiclass_decision(0, n)
    (dec, pred), both = timed(lambda: e.svm_multiclass_decision(0, n))
    _, labels_only = timed(lambda: e.svm_multiclass_decision(0, n, decision=False))
    out["decision"] = dict(rows=n, values_and_labels_ms=round(both, 3), labels_only_ms=round(labels_only, 3),
                           share_of_fit=round(labels_only / wall, 4), train_accuracy=float((pred == y).mean()))
    # cross-validation: folds x Cs x pairs in one batch
    fold = fastsk_amd.stratified_folds(y, folds, seed=0)
    e.svm_multiclass_cv(y, fold, CS, eps, 50)
    r, cv_ms = timed(lambda: e.svm_multiclass_cv(y, fold, CS, eps, max_iter))
    out["cv"] = dict(folds=folds, Cs=CS, problems=len(r["problems"]), form=r["form"], launches=r["launches"], ms=round(cv_ms, 3),
                     accuracy=[float(a) for a in r["accuracy"]], slowest_problem_iterations=max(q["iterations"] for q in r["problems"]),
                     converged=sum(bool(q["converged"]) for q in r["problems"]))
    # the host: scikit-learn on the matrix the getter copies out
    if n <= host_max_n:
        from sklearn.svm import SVC
        K, getter = timed(e.get_train)
        clf, fit = timed(lambda: SVC(kernel="precomputed", C=C, tol=eps, shrinking=False, decision_function_shape="ovo", cache_size=4000).fit(K, y))
        theirs, predict = timed(lambda: clf.decision_function(K))
        out["host"] = dict(getter_ms=round(getter, 3), svc_fit_ms=round(fit, 3), svc_decision_ms=round(predict, 3),
                           total_ms=round(getter + fit, 3), largest_decision_difference=float(np.max(np.abs(theirs - dec))),
                           labels_equal=float((clf.predict(K) == pred).mean()))
        del K
    else:
        out["host"] = dict(not_run="NOT measured: the square matrix scikit-learn wants is %.1f GB on the host" % (8.0 * n * n / 1e9))
    e.close()
    # every pair alone: the kernel of its rows, fsk_svm_train
    _, pairs = mc.pairs_of(y)
    solves, kernels, same = [], 0.0, True
    for p, (a, b, idx, ys) in enumerate(pairs):
        sub, ms = timed(lambda: resident(case, tok, off, idx))
        kernels += ms
        sub.n_train = len(idx)
        sub.svm_train(ys, C, eps, 50)
        sub.svm_train(ys, C, eps, max_iter)
        got, ms = timed(lambda: sub.svm_train(ys, C, eps, max_iter))
        solves.append(ms)
        same = same and got["iterations"] == its[p]
        sub.close()
    out["pairs_alone"] = dict(solves_ms=[round(t, 3) for t in solves], slowest_ms=round(max(solves), 3), one_after_another_ms=round(sum(solves), 3),
                              sub_kernels_ms=round(kernels, 3), iterations_equal_the_batch=bool(same),
                              fit_over_slowest=round(wall / max(solves), 3), fit_over_one_after_another=round(wall / sum(solves), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="dna2000,dna6500,dna32000")
    ap.add_argument("--max-iter", type=int, default=40000)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--host-max-n", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_multiclass.json"))
    args = ap.parse_args()
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)
    for name in args.cases.split(","):
        res = run_case(int(name[3:]), args.max_iter, args.eps, args.C, args.folds, args.host_max_n)
        print(json.dumps(res), flush=True)
        cur["case_" + name] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
