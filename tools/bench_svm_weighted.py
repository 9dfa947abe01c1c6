#!/usr/bin/env python3
"""The class-weighted C-SVC and the Platt calibration (fsk_svm_set_class_weights, fsk_svm_calibrate) on one GPU
-> profiles/svm_weighted.json.

Workloads (--cases), those of tools/bench_svm.py:
  ep300     tests/golden/tokens_EP300.npz, 2000 train rows, g = 10, m = 6 exact, the workgroup form;
  dna32k    synthetic DNA 32,000 x 300, g = 12, m = 8 exact, the two-launch form, at most --max-iter steps.
Per case:
  unweighted   fsk_svm_train with the weights left at (1, 1), --rounds times, microseconds an iteration from fsk_svm_info.ms.
               With --parent-lib (a build of the commit before the class weights) the same solve on that library, on the same
               device, alternating with this one: both series, and this library's median against the parent's own spread
               (the model must be the parent's, iteration for iteration and bit for bit). --parent-seat second swaps who goes
               first; --parent-lib pointed at this tree's own library measures the seat alone;
  weighted     the labels turned 1 : 9 (every tenth row positive, taken evenly from the positives; every other row negative):
               the solve with (1, 1) and with "balanced" (5, 5 / 9), iterations and time;
  calibration  fsk_svm_train alone against fsk_svm_train + fsk_svm_calibrate on 5 stratified folds (what
               fit_svm(probability=True) runs), with the fold solves' iteration counts (fsk_svm_cv at the one C). The
               expectation written down before the first measurement: the five fold solves run side by side and cost about
               what the slowest of them costs alone, `slowest_fold_alone_ms_estimate` = its iterations x the unweighted solve's
               microseconds an iteration.

    tools/bench_svm_weighted.py [--cases ep300,dna32k] [--parent-lib PATH] [--parent-seat first|second] [--key SUFFIX] [--rounds 5]
                                [--max-iter 40000] [--out profiles/svm_weighted.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_svm import golden, synthetic  # noqa: E402

CASES = {"ep300": dict(data=lambda: golden("EP300"), g=10, m=6, wg_max=None),
         "dna32k": dict(data=lambda: synthetic(32000), g=12, m=8, wg_max=0)}
NEW = ("fsk_svm_set_class_weights", "fsk_svm_get_class_weights", "fsk_svm_platt_fit", "fsk_svm_calibrate", "fsk_svm_get_calibration",
       "fsk_svm_proba")


def parent_library(path):
    """A build from before the class weights: the symbols it lacks are left unbound."""
    from fastsk_amd import _native
    return _native.Library(path, optional=NEW)


def resident(case, tok, off, lib=None):
    from fastsk_amd import _native
    e = _native.Engine(case["g"], case["m"], lib=lib)
    e.load_sequences(tok, off, len(off) - 1, 0)
    e.accumulate(np.arange(e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
    e.finalize()
    if case["wg_max"] is not None:
        e.set_tuning("svm_wg_max", case["wg_max"])
    return e


def one_in_ten(y):
    """Every tenth row positive, taken evenly from the positives; every other row negative."""
    pos = np.flatnonzero(y > 0)
    keep = pos[np.linspace(0, len(pos) - 1, len(y) // 10).astype(np.int64)]
    out = -np.ones(len(y), dtype=np.int32)
    out[keep] = 1
    return out


def solve(e, y, C, eps, max_iter):
    info = e.svm_train(y, C, eps, max_iter)
    return dict(iterations=info["iterations"], converged=info["converged"], ms=round(info["ms"], 3), n_sv=info["n_sv"], n_bsv=info["n_bsv"],
                form=info["form"], launches=info["launches"], us_per_iteration=round(1e3 * info["ms"] / max(info["iterations"], 1), 3))


def run_case(name, parent, rounds, max_iter, C, eps, parent_first=True):
    import fastsk_amd
    case = CASES[name]
    tok, off, y = case["data"]()
    n = len(y)
    out = dict(case=name, n_train=n, g=case["g"], m=case["m"], C=C, eps=eps, max_iter=max_iter, rounds=rounds)
    # ---- the unweighted solve, this library and the parent's in turns (the seat: whose engine is made first and solves first)
    old = resident(case, tok, off, parent) if parent is not None and parent_first else None
    e = resident(case, tok, off)
    if parent is not None and not parent_first:
        old = resident(case, tok, off, parent)
    for x in (e, old):
        if x is not None:
            x.svm_train(y, C, eps, 50)   # warm: code objects, buffers
    mine, theirs, same = [], [], True
    for _ in range(rounds):
        if old is not None and parent_first:
            theirs.append(solve(old, y, C, eps, max_iter))
        mine.append(solve(e, y, C, eps, max_iter))
        if old is not None and not parent_first:
            theirs.append(solve(old, y, C, eps, max_iter))
        if old is not None:
            a, b = e.svm_model(), old.svm_model()
            same = same and np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2]["iterations"] == b[2]["iterations"] and a[2]["launches"] == b[2]["launches"]
    series = lambda runs: [r["us_per_iteration"] for r in runs]
    out["unweighted"] = dict(solve=mine[-1], us_per_iteration=series(mine), median_us_per_iteration=statistics.median(series(mine)))
    if old is not None:
        p = series(theirs)
        med = statistics.median(series(mine))
        out["unweighted"]["parent"] = dict(seat="first" if parent_first else "second", us_per_iteration=p, median_us_per_iteration=statistics.median(p), lowest=min(p), highest=max(p))
        out["unweighted"]["model_equals_the_parents"] = bool(same)
        out["unweighted"]["median_within_the_parents_spread"] = bool(min(p) <= med <= max(p))
        out["unweighted"]["median_over_parents_median"] = round(med / statistics.median(p), 4)
        old.close()
    per_it = out["unweighted"]["median_us_per_iteration"]
    # ---- 1 : 9 labels, (1, 1) against "balanced"
    y19 = one_in_ten(y)
    w = fastsk_amd.class_weights(y19, "balanced")
    plain = solve(e, y19, C, eps, max_iter)
    e.svm_set_class_weights(*w)
    e.svm_train(y19, C, eps, 50)
    balanced = solve(e, y19, C, eps, max_iter)
    dec = e.svm_decision(0, n)
    out["weighted"] = dict(positives=int((y19 > 0).sum()), weights=list(w), unweighted_solve=plain, balanced_solve=balanced,
                           balanced_train_recall=float(np.mean(dec[y19 > 0] > 0)), balanced_train_specificity=float(np.mean(dec[y19 < 0] <= 0)))
    # ---- the calibration beside the fit (the original labels, weights (1, 1))
    e.svm_set_class_weights(1.0, 1.0)
    fold = fastsk_amd.stratified_folds(y, 5, seed=0)
    fit = solve(e, y, C, eps, max_iter)
    e.svm_calibrate(fold, 5)             # warm: the batch kernels' code objects, buffers
    platt = e.svm_calibrate(fold, 5)
    its = [q["iterations"] for q in e.svm_cv(y, fold, [C], eps, max_iter)["problems"]]
    out["calibration"] = dict(fit_ms=fit["ms"], calibrate_ms=round(platt["ms"], 3), fit_and_calibrate_ms=round(fit["ms"] + platt["ms"], 3),
                              calibrate_over_fit=round(platt["ms"] / fit["ms"], 3), fit_iterations=fit["iterations"], fold_iterations=its,
                              slowest_fold_alone_ms_estimate=round(max(its) * per_it / 1e3, 3), form=platt["form"], launches=platt["launches"],
                              A=platt["A"], B=platt["B"], newton_iterations=platt["iterations"], status=platt["status"])
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ep300,dna32k")
    ap.add_argument("--parent-lib", default=None, help="libfastsk_amd.so built from the commit before the class weights")
    ap.add_argument("--parent-seat", choices=("first", "second"), default="first", help="whose engine is made first and solves first in a round")
    ap.add_argument("--key", default="", help="a suffix for the JSON keys of this run (e.g. a second seat, a library against itself)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=40000)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_weighted.json"))
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime for both libraries: torch's, loaded first)
    from fastsk_amd import _native
    _native.library()
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)
    for name in args.cases.split(","):
        res = run_case(name, parent, args.rounds, args.max_iter, args.C, args.eps, args.parent_seat == "first")
        print(json.dumps(res), flush=True)
        cur["case_" + name + args.key] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
