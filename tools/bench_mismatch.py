#!/usr/bin/env python3
"""The mismatch-weighted mode on one GPU -> profiles/mismatch_levels.json.

LS-GKM's default setting on this engine: 16,000 x 300 bp DNA (PCG64(20201214), tokens 1..4, i.i.d. uniform), g = 11, m = 4,
max_mismatches = 3, reverse complement on: the levels (11, m = 0 .. 3), k = 11, 10, 9, 8, each folded into the result by
k_tri_fold. One warm compute, then --rounds timed ones: the wall time of fsk_compute, the host time of each level and the
HIP-event time of each fold (fsk_get_mismatch_times). The yardstick of the fold is k_triangle over the same triangle
(fsk_get_triangle_device into a resident tensor, wall time around the call, which ends in a synchronise), timed in the same
run: both are streaming passes without reuse, the fold moves 16 (the first level, a store) or 24 bytes a cell, k_triangle
16. A seeded sample of cells is checked against the brute-force Hamming profile of the two sequences.

    tools/bench_mismatch.py [--n 16000] [--rounds 3] [--out profiles/mismatch_levels.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMP = {1: 4, 4: 1, 2: 3, 3: 2}
G, M, D, L = 11, 4, 3, 300


def brute_cell(x, y, weights):
    """sum_h c_h N_h(x, y) over both strands of both sequences, from the Hamming distance of every window pair."""
    lut = np.zeros(5, dtype=np.int64)
    for a, b in COMP.items():
        lut[a] = b
    total = 0
    for xs in (x, lut[x[::-1]]):
        wx = np.lib.stride_tricks.sliding_window_view(xs, G)
        for ys in (y, lut[y[::-1]]):
            wy = np.lib.stride_tricks.sliding_window_view(ys, G)
            dist = (wx[:, None, :] != wy[None, :, :]).sum(axis=2)
            for h, c in enumerate(weights):
                total += int(c) * int((dist == h).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch_levels.json"))
    args = ap.parse_args()
    import torch
    from fastsk_amd import _native

    N = args.n
    rng = np.random.Generator(np.random.PCG64(20201214))
    X = rng.integers(1, 5, size=(N, L), dtype=np.int32)
    tokens, offsets = _native.flatten(X)
    e = _native.Engine(G, M, max_mismatches=D, revcomp=COMP)
    weights = e.weights
    e.compute(tokens, offsets, N, 0)   # warm
    rounds = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        e.compute(tokens, offsets, N, 0)
        wall = time.perf_counter() - t0
        info = e.mismatch_info()
        rounds.append({"compute_ms": wall * 1e3,
                       "levels": [{"m": lv["m"], "k": lv["k"], "a": lv["a"], "path": lv["path"], "ms": lv["ms"], "fold_ms": lv["fold_ms"]}
                                  for lv in info["levels"]]})
    pairs = N * (N + 1) // 2
    out = torch.empty(pairs, dtype=torch.float64, device="cuda")
    e.get_triangle_torch(out)   # warm
    tri_ms = []
    for _ in range(max(3, args.rounds)):
        t0 = time.perf_counter()
        e.get_triangle_torch(out)
        tri_ms.append((time.perf_counter() - t0) * 1e3)
    # spot check
    srng = np.random.Generator(np.random.PCG64(7))
    rows = srng.integers(0, N, size=40)
    cols = srng.integers(0, N, size=40)
    rows[:4] = cols[:4]   # a few diagonal cells
    got = e.get_counts_cells(rows, cols)
    want = [brute_cell(X[i].astype(np.int64), X[j].astype(np.int64), weights) for i, j in zip(rows, cols)]
    ok = [int(g) for g in got] == want
    best = min(rounds, key=lambda r: r["compute_ms"])
    tri_best = min(tri_ms)
    tri_bps = 16.0 * pairs / (tri_best * 1e-3)
    folds = []
    first_m = best["levels"][0]["m"]
    for lv in best["levels"]:
        nbytes = (16.0 if lv["m"] == first_m else 24.0) * pairs
        bps = nbytes / (lv["fold_ms"] * 1e-3) if lv["fold_ms"] > 0 else 0.0
        folds.append({"m": lv["m"], "fold_ms": lv["fold_ms"], "bytes": nbytes, "bytes_per_s": bps, "of_k_triangle": bps / tri_bps})
    result = {"workload": {"N": N, "L": L, "g": G, "m": M, "max_mismatches": D, "revcomp": True, "weights": weights, "cells": pairs},
              "device": torch.cuda.get_device_name(0), "rounds": rounds, "best_compute_ms": best["compute_ms"],
              "k_triangle_ms": tri_ms, "k_triangle_bytes_per_s": tri_bps, "folds": folds,
              "fold_share_of_compute": sum(f["fold_ms"] for f in folds) / best["compute_ms"],
              "sample_cells_match_brute_force": ok, "stats": {k: v for k, v in e.stats().items() if k in ("launches", "combos_done", "cell_updates", "sort_records")}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"best_compute_ms": best["compute_ms"], "k_triangle_ms": tri_best,
                      "folds": [(f["m"], round(f["fold_ms"], 3), round(f["of_k_triangle"], 3)) for f in folds], "sample_ok": ok}))
    e.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
