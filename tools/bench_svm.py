#!/usr/bin/env python3
"""The SVM stage on the resident triangle (fsk_svm_train) on one GPU -> profiles/svm.json.

Workloads (--cases):
  ep300        tests/golden/tokens_EP300.npz, 2000 train rows, g = 10, m = 6 exact, the form the engine picks (one workgroup);
  ep47848      tests/golden/tokens_EP300_47848.npz, its 6506 train rows (of 7230 sequences), g = 10, m = 6, a SAMPLE of the
               kernel — the first 100 of the 210 combos, as BASELINE config 3 —, BOTH forms
               (svm_wg_max forced to 8192 and to 0);
  dna32k       synthetic DNA 32,000 x 300 (tests/svm_cases.dna: PCG64, classes alternating, a 10-mer planted in 80 % of the
  dna100k      positives) and 100,000 x 300, g = 12, m = 8 exact, the two-launch form, at most --max-iter steps.
Per solve: fit_svm host time (fsk_svm_info.ms), iterations, microseconds an iteration, launches; for the two-launch form
the bytes an iteration moves as fastsk_amd/csrc/fsk_engine_svm.hip states them (74 n at the least, 130 n with a 64-byte
line for every strided cell of two middle rows), over the measured time. The host yardstick, scikit-learn's
SVC(kernel="precomputed", shrinking=False) on the matrix the getter copies out, getter time included, runs where n <= --host-max-n; beyond, the JSON says why it did not.

    tools/bench_svm.py [--cases ep300,ep47848,dna32k,dna100k] [--max-iter 20000] [--host-max-n 8192] [--out profiles/svm.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def golden(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tokens_%s.npz" % name))
    n = int(z["n_train"])
    off = z["offsets"].astype(np.int64)[:n + 1]
    tok = z["tokens"].astype(np.int32)[:off[-1]]
    return tok, off, np.where(np.asarray(z["y_train"]) > 0, 1, -1).astype(np.int32)


def synthetic(n):
    import svm_cases
    X, y = svm_cases.dna(n, 300, 20201214 + n)
    return X.reshape(-1), np.arange(n + 1, dtype=np.int64) * 300, y


CASES = {"ep300": dict(data=lambda: golden("EP300"), g=10, m=6, combos=None, forms=(None,)),
         "ep47848": dict(data=lambda: golden("EP300_47848"), g=10, m=6, combos=100, forms=(8192, 0)),
         "dna32k": dict(data=lambda: synthetic(32000), g=12, m=8, combos=None, forms=(0,)),
         "dna100k": dict(data=lambda: synthetic(100000), g=12, m=8, combos=None, forms=(0,))}


def run_case(name, max_iter, host_max_n, C, eps):
    from fastsk_amd import _native
    case = CASES[name]
    tok, off, y = case["data"]()
    n = len(y)
    e = _native.Engine(case["g"], case["m"])
    t0 = time.perf_counter()
    e.load_sequences(tok, off, n, 0)
    e.accumulate(np.arange(case["combos"] or e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
    e.finalize()
    out = dict(case=name, n_train=n, g=case["g"], m=case["m"], combos=case["combos"] or "all", C=C, eps=eps, max_iter=max_iter, kernel_ms=round(1e3 * (time.perf_counter() - t0), 3), solves=[])
    for wg_max in case["forms"]:
        if wg_max is not None:
            e.set_tuning("svm_wg_max", wg_max)
        e.svm_train(y, C, eps, 50)   # warm: code objects, buffers
        t0 = time.perf_counter()
        info = e.svm_train(y, C, eps, max_iter)
        wall = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        dec = e.svm_decision(0, n)
        dec_ms = 1e3 * (time.perf_counter() - t0)
        it = max(info["iterations"], 1)
        s = dict(info, wall_ms=round(wall, 3), us_per_iteration=round(1e3 * info["ms"] / it, 3), decision_train_ms=round(dec_ms, 3),
                 train_accuracy=float(np.mean((dec > 0) == (y > 0))))
        if info["form"] == "two-launch":
            sec = 1e-3 * info["ms"] / it
            s["GBps_least_bytes"] = round(74.0 * n / sec / 1e9, 2)       # (fsk_engine_svm.hip: bytes an iteration)
            s["GBps_with_64B_lines"] = round(130.0 * n / sec / 1e9, 2)
        out["solves"].append(s)
    if n <= host_max_n:
        from sklearn.svm import SVC
        t0 = time.perf_counter()
        K = e.get_train()
        t1 = time.perf_counter()
        clf = SVC(kernel="precomputed", C=C, tol=eps, shrinking=False, cache_size=4000).fit(K, y)
        t2 = time.perf_counter()
        out["host"] = dict(getter_ms=round(1e3 * (t1 - t0), 3), svc_fit_ms=round(1e3 * (t2 - t1), 3), total_ms=round(1e3 * (t2 - t0), 3),
                           n_sv=int(clf.n_support_.sum()), matrix_GB=round(K.nbytes / 1e9, 3))
    else:
        gb = 8.0 * n * n / 1e9
        out["host"] = dict(not_run="the square matrix scikit-learn wants is %.1f GB on the host%s" %
                           (gb, "" if gb < 64 else ": it cannot be held"))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ep300,ep47848,dna32k,dna100k")
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--host-max-n", type=int, default=8192)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm.json"))
    args = ap.parse_args()
    cur = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            cur = json.load(f)
    for name in args.cases.split(","):
        res = run_case(name, args.max_iter, args.host_max_n, args.C, args.eps)
        print(json.dumps(res), flush=True)
        cur["case_" + name] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
