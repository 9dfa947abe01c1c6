#!/usr/bin/env python3
"""The multi-class probabilities (fsk_svm_multiclass_calibrate: a Platt sigmoid a pair from one batch of fold solves;
fsk_svm_multiclass_proba: the pairs' decisions, the sigmoids and the pairwise coupling in one launch) on one GPU
-> profiles/svm_multiclass_proba.json.

Workloads: the synthetic 4-class DNA of tools/bench_svm_multiclass.py (300 symbols a row, g = 12, m = 8 exact) at --cases rows,
and the same generator with 16 and 64 equal classes at --many-rows rows. Host clock around calls that end in a device
synchronise, the second of two calls (the best of --reps for the two launches that are compared). Per case:
  calibrate          fsk_svm_multiclass_calibrate, 5 stratified folds x 6 pairs = 30 problems in one batch, beside the fit and
                     beside its slowest (fold, pair) problem solved alone (fsk_svm_train on an engine that holds the kernel of
                     that problem's rows only; which problem is the slowest is read off fsk_svm_multiclass_cv at the same C);
  proba              fsk_svm_multiclass_proba over the training rows beside fsk_svm_multiclass_decision over the same rows in
                     the same process — labels alone (4 bytes a row copied either way) and with the values ([n, k] probabilities
                     against [n, P] decisions) — and the coupling's iteration counts;
  many_classes       the two launches again at 16 and 64 classes under seeded sigmoids (fsk_svm_multiclass_set_calibration: the
                     fit runs 200 steps a pair at most, its model only has to exist), where the k sequential steps of a
                     coupling iteration begin to show.
None of these is a pass mark. What does not run says so in the JSON.

    tools/bench_svm_multiclass_proba.py [--cases dna2000,dna6500,dna32000] [--many 16,64] [--out profiles/svm_multiclass_proba.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_svm_cv import resident, timed  # noqa: E402
from bench_svm_multiclass import G, LENGTH, M, synthetic  # noqa: E402


def best(fn, reps):
    fn()
    return min(timed(fn)[1] for _ in range(reps))


def launches(e, n, reps):
    """The proba launch beside the decision launch over rows [0, n)."""
    lab_d = best(lambda: e.svm_multiclass_decision(0, n, decision=False), reps)
    lab_p = best(lambda: e.svm_multiclass_proba(0, n, proba=False, iterations=False), reps)
    val_d = best(lambda: e.svm_multiclass_decision(0, n), reps)
    val_p = best(lambda: e.svm_multiclass_proba(0, n), reps)
    prob, pred, iters = e.svm_multiclass_proba(0, n)
    vote = e.svm_multiclass_decision(0, n, decision=False)[1]
    return dict(rows=n, decision_labels_ms=round(lab_d, 3), proba_labels_ms=round(lab_p, 3), labels_ratio=round(lab_p / lab_d, 3),
                decision_values_ms=round(val_d, 3), proba_values_ms=round(val_p, 3), values_ratio=round(val_p / val_d, 3),
                iterations_mean=float(iters.mean()), iterations_max=int(iters.max()),
                largest_row_sum_error=float(np.abs(prob.sum(axis=1) - 1.0).max()), argmax_differs_from_vote=float((pred != vote).mean())), pred


def run_case(n, max_iter, eps, C, folds, reps):
    import fastsk_amd
    import svm_multiclass_cases as mc
    case = dict(g=G, m=M, combos=None)
    tok, off, y, sizes = synthetic(n)
    e = resident(case, tok, off)
    e.n_test, e.N = 0, n
    e.svm_train_multiclass(y, C, eps, 50)   # warm: code objects, buffers
    e.svm_train_multiclass(y, C, eps, max_iter)
    info, fit_ms = timed(lambda: e.svm_train_multiclass(y, C, eps, max_iter))
    fold = fastsk_amd.stratified_folds(y, folds, seed=0)
    e.svm_multiclass_calibrate(fold, folds)
    fits, cal_ms = timed(lambda: e.svm_multiclass_calibrate(fold, folds))
    out = dict(case="dna%d" % n, n_train=n, class_sizes=sizes, g=G, m=M, length=LENGTH, C=C, eps=eps, max_iter=max_iter, form=info["form"],
               fit_ms=round(fit_ms, 3), fit_launches=info["launches"])
    out["calibrate"] = dict(folds=folds, problems=folds * len(fits), form=fits[0]["form"], launches=fits[0]["launches"], ms=round(cal_ms, 3),
                            ms_library=round(fits[0]["ms"], 3), over_fit=round(cal_ms / fit_ms, 3), A=[f["A"] for f in fits], B=[f["B"] for f in fits],
                            fit_iterations=[f["iterations"] for f in fits], fit_status=[f["status"] for f in fits])
    out["proba"], pred = launches(e, n, reps)
    out["proba"]["train_accuracy_argmax"] = float((pred == y).mean())
    # the slowest (fold, pair) problem alone
    cv = e.svm_multiclass_cv(y, fold, [C], eps, max_iter)
    e.close()
    slow = max(range(len(cv["problems"])), key=lambda p: cv["problems"][p]["iterations"])
    q = cv["problems"][slow]
    classes = np.unique(y)
    idx = np.flatnonzero(((y == q["class_a"]) | (y == q["class_b"])) & (fold != q["fold"]))
    ys = np.where(y[idx] == q["class_a"], 1, -1).astype(np.int32)
    sub = resident(case, tok, off, idx)
    sub.n_train = len(idx)
    sub.svm_train(ys, C, eps, 50)
    sub.svm_train(ys, C, eps, max_iter)
    got, alone_ms = timed(lambda: sub.svm_train(ys, C, eps, max_iter))
    sub.close()
    out["calibrate"].update(slowest_problem=dict(fold=q["fold"], class_a=q["class_a"], class_b=q["class_b"], rows=len(idx),
                                                 iterations=q["iterations"], iterations_alone=got["iterations"], alone_ms=round(alone_ms, 3)),
                            over_slowest_problem=round(cal_ms / alone_ms, 3), classes=classes.tolist())
    return out


def run_many(k, n, eps, C, reps):
    import svm_multiclass_cases as mc
    import svm_multiclass_proba_cases as pc
    case = dict(g=G, m=M, combos=None)
    X, y = mc.dna([n // k] * k, 0, LENGTH, 20201214 + k)
    rows = len(y)
    e = resident(case, X.reshape(-1), np.arange(rows + 1, dtype=np.int64) * LENGTH)
    e.n_test, e.N = 0, rows
    info = e.svm_train_multiclass(y, C, eps, 200)
    A, B = pc.seeded_sigmoids(k, k)
    e.svm_multiclass_set_calibration(A, B)
    out, _ = launches(e, rows, reps)
    out.update(k=k, pairs=k * (k - 1) // 2, lds_bytes_a_workgroup=32 * (k * (k - 1) // 2), fit_form=info["form"])
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="dna2000,dna6500,dna32000")
    ap.add_argument("--many", default="16,64")
    ap.add_argument("--many-rows", type=int, default=2048)
    ap.add_argument("--max-iter", type=int, default=40000)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_multiclass_proba.json"))
    args = ap.parse_args()
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)

    def keep(key, res):
        print(json.dumps(res), flush=True)
        cur[key] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")

    for name in [c for c in args.cases.split(",") if c]:
        keep("case_" + name, run_case(int(name[3:]), args.max_iter, args.eps, args.C, args.folds, args.reps))
    for k in [int(v) for v in args.many.split(",") if v]:
        keep("many_classes_%d" % k, run_many(k, args.many_rows, args.eps, args.C, args.reps))


if __name__ == "__main__":
    main()
