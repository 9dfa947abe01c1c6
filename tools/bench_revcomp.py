#!/usr/bin/env python3
"""Reverse-complement mode against its alternatives, on one GPU -> profiles/revcomp.json.

Three cases, data from the PCG64(20201214) generator (tokens 1..4, i.i.d. uniform):
  ep300   EP300-shaped 4,000 x 100 bp, g = 10, m = 6, exact (all 210 combos)
  dense   DNA 16,000 x 300 bp, g = 12, m = 8, exact (all 495 combos)
  sparse  DNA 32,000 x 300 bp, g = 12, m = 4, 8 combos
For each, three variants are timed in ONE process, warm, alternating, over --rounds rounds (wall time of reset + accumulate +
finalize, which ends in a synchronise; the sequences are resident):
  (a) plain     the kernel without the mode;
  (b) revcomp   the mode in the engine (fsk_set_complement);
  (c) twoN      what a caller can do without it: the 2N rows [X ; rc(X)] through the plain engine into a torch tensor, and the
                four N x N blocks of that triangle added on the device (timed with and without the fold).
(b) is checked against (c) on a seeded sample of cells in the same run.

    tools/bench_revcomp.py [--cases ep300,dense,sparse] [--rounds 5] [--out profiles/revcomp.json]
    tools/bench_revcomp.py --plain-bench PARENT_TREE [--repeats 3]   bench.py (plain) of a built checkout of the parent commit and
                                                                     of this tree, alternating: both ms_per_step series
    tools/bench_revcomp.py --trace dense --variant revcomp           one warm step + two steps of one variant, nothing else: the
                                                                     program to put behind `rocprofv3 --kernel-trace --stats --`
    tools/bench_revcomp.py --kernel-stats PLAIN.csv REVCOMP.csv      the two traces' kernel totals into the JSON
Every invocation merges its section into --out."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMP = {1: 4, 4: 1, 2: 3, 3: 2}
CASES = {"ep300": dict(N=4000, L=100, g=10, m=6, combos=None),
         "dense": dict(N=16000, L=300, g=12, m=8, combos=None),
         "sparse": dict(N=32000, L=300, g=12, m=4, combos=8)}
SAMPLE = 20000


def make_data(N, L):
    rng = np.random.Generator(np.random.PCG64(20201214))
    X = rng.integers(1, 5, size=(N, L), dtype=np.int32)
    return X, np.arange(N + 1, dtype=np.int64) * L


def rc_rows(X):
    lut = np.zeros(5, dtype=np.int32)
    for a, b in COMP.items():
        lut[a] = b
    return lut[X[:, ::-1]]


def cell(i):
    return i * (i + 1) // 2


def fold_on_device(torch, T, N):
    """The 2N-row triangle T (int64, row-major lower triangle) -> the N-row triangle of its four blocks' sum."""
    out = torch.empty(cell(N), dtype=torch.int64, device=T.device)
    a = 0
    while a < N:
        b = a + 1
        while b < N and cell(b + 1) - cell(a) <= (1 << 26):
            b += 1
        i = torch.arange(a, b, device=T.device, dtype=torch.int64)
        row = torch.repeat_interleave(i, i + 1)
        j = torch.arange(cell(a), cell(b), device=T.device, dtype=torch.int64) - row * (row + 1) // 2
        lower = (N + row) * (N + row + 1) // 2
        out[cell(a):cell(b)] = (T[row * (row + 1) // 2 + j] + T[lower + j] + T[(N + j) * (N + j + 1) // 2 + row] + T[lower + N + j])
        a = b
    return out


class Variant:
    def __init__(self, native, name, case, X, offsets, combos, torch=None):
        self.name, self.N, self.combos, self.torch = name, len(X), combos, torch
        self.e = native.Engine(case["g"], case["m"], revcomp=COMP if name == "revcomp" else None)
        self.T = None
        if name == "twoN":
            X = np.concatenate([X, rc_rows(X)])
            offsets = np.arange(len(X) + 1, dtype=np.int64) * X.shape[1]
            self.T = torch.zeros(cell(len(X)), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            self.e.bind_counts(self.T.data_ptr(), cell(len(X)), keepalive=self.T)
        self.e.load_sequences(X.reshape(-1), offsets, len(X), 0)
        self.folded = None

    def step(self, fold=True):
        t0 = time.perf_counter()
        self.e.reset_counts()
        self.e.accumulate(self.combos)
        self.e.finalize()
        t1 = time.perf_counter()
        if self.T is not None and fold:
            self.folded = fold_on_device(self.torch, self.T, self.N)
            self.torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t1


def run_case(native, torch, name, rounds, warmup=1):
    case = CASES[name]
    X, offsets = make_data(case["N"], case["L"])
    nc = native.library().num_combos(case["g"], case["m"])
    combos = np.arange(nc, dtype=np.int32) if case["combos"] is None else np.linspace(0, nc - 1, case["combos"]).astype(np.int32)
    variants = [Variant(native, v, case, X, offsets, combos, torch) for v in ("plain", "revcomp", "twoN")]
    for _ in range(warmup):
        for v in variants:
            v.step()
    times = {v.name: [] for v in variants}
    times["twoN_fold"] = []
    for _ in range(rounds):
        for v in variants:   # alternating: one step of each per round
            dt, dfold = v.step()
            times[v.name].append(dt)
            if v.name == "twoN":
                times["twoN_fold"].append(dfold)
    plain, rc, two = variants
    rng = np.random.Generator(np.random.PCG64(20201214 + 1))
    rows = rng.integers(0, case["N"], size=SAMPLE)
    cols = rng.integers(0, case["N"], size=SAMPLE)
    rows, cols = np.maximum(rows, cols), np.minimum(rows, cols)
    got = rc.e.get_counts_cells(rows, cols)
    idx = torch.as_tensor(rows * (rows + 1) // 2 + cols, device="cuda")
    want = two.folded[idx].cpu().numpy().astype(np.uint64)
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(case, case=name, combos=int(len(combos)), rounds=rounds,
               path={v.name: "dense" if v.e.stats()["path_used"] == 1 else "sparse" for v in variants},
               seconds={k: [round(x, 6) for x in v] for k, v in times.items()}, median_seconds={k: round(v, 6) for k, v in med.items()},
               revcomp_over_plain=round(med["revcomp"] / med["plain"], 3),
               twoN_with_fold_over_revcomp=round((med["twoN"] + med["twoN_fold"]) / med["revcomp"], 3),
               twoN_compute_only_over_revcomp=round(med["twoN"] / med["revcomp"], 3),
               revcomp_faster_than_twoN=bool(max(times["revcomp"]) < min(times["twoN"])),
               cells_checked=SAMPLE, revcomp_equals_twoN_fold=bool(np.array_equal(got, want)))
    for v in variants:
        v.e.close()
    return out


def trace(native, name, variant):
    import torch
    case = CASES[name]
    X, offsets = make_data(case["N"], case["L"])
    nc = native.library().num_combos(case["g"], case["m"])
    combos = np.arange(nc, dtype=np.int32) if case["combos"] is None else np.linspace(0, nc - 1, case["combos"]).astype(np.int32)
    v = Variant(native, variant, case, X, offsets, combos, torch)
    for _ in range(3):
        v.step(fold=False)
    v.e.close()


def plain_bench(parent, repeats, steps, warmup):
    """bench.py (plain: not --full) in a built checkout of the parent commit and in this tree, alternating."""
    series = {"parent": [], "this": []}
    for _ in range(repeats):
        for who, tree in (("parent", parent), ("this", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                               capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError("bench.py failed in %s:\n%s\n%s" % (tree, r.stdout[-2000:], r.stderr[-2000:]))
            series[who].append(round(json.loads(line[-1])["ms_per_step"], 3))
    lo, hi = min(series["parent"]), max(series["parent"])
    return dict(cmd="bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), repeats=repeats, ms_per_step=series,
                parent_spread=[lo, hi], this_median=float(np.median(series["this"])),
                this_within_parent_spread=bool(lo <= float(np.median(series["this"])) <= hi),
                this_not_slower_than_parent_max=bool(float(np.median(series["this"])) <= hi))


def kernel_stats(plain_csv, revcomp_csv):
    def read(path):
        out = {}
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                key = next((k for k in ("k_dense_tile_dma", "k_dense_count") if k in name), None)
                if key:
                    d = out.setdefault(key, dict(calls=0, total_ns=0))
                    d["calls"] += int(row["Calls"])
                    d["total_ns"] += int(float(row["TotalDurationNs"]))
                out["all_kernels_ns"] = out.get("all_kernels_ns", 0) + int(float(row["TotalDurationNs"]))
        return out
    return dict(case="dense", steps=3, plain=read(plain_csv), revcomp=read(revcomp_csv))


def merge(path, section, value):
    cur = {}
    if os.path.exists(path):
        with open(path) as f:
            cur = json.load(f)
    cur[section] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(cur, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ep300,dense,sparse")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "revcomp.json"))
    ap.add_argument("--plain-bench", metavar="PARENT_TREE", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", choices=sorted(CASES), default=None)
    ap.add_argument("--variant", choices=["plain", "revcomp", "twoN"], default="revcomp")
    ap.add_argument("--kernel-stats", nargs=2, metavar="CSV", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        merge(args.out, "kernel_stats_dense", kernel_stats(*args.kernel_stats))
        return
    if args.plain_bench:
        res = plain_bench(args.plain_bench, args.repeats, args.steps, args.warmup)
        print(json.dumps(res), flush=True)
        merge(args.out, "plain_bench", res)
        return
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from fastsk_amd import _native
    if args.trace:
        trace(_native, args.trace, args.variant)
        return
    if args.rounds < 5:
        raise SystemExit("--rounds must be at least 5")
    for name in args.cases.split(","):
        res = run_case(_native, torch, name, args.rounds)
        print(json.dumps(res), flush=True)
        merge(args.out, "case_" + name, res)
        if not res["revcomp_equals_twoN_fold"]:
            raise SystemExit("%s: the engine's reverse-complement counts differ from the folded 2N-row counts" % name)


if __name__ == "__main__":
    main()
