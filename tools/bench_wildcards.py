#!/usr/bin/env python3
"""Wildcard mode against the engine without it, on one GPU -> profiles/wildcards.json.

Two inputs:
  ep47848   BASELINE config 3's input: tests/golden/tokens_EP300_47848.npz, 7,230 x 200 with 288 n in five sequences,
            g = 10, m = 6, the first 100 combos;
  dna16k    synthetic DNA 16,000 x 300 from PCG64(20201214), 1 % of the sequences holding a run of 20 n, g = 12, m = 8, all 495
            combos, the dense dataflow.
Three variants, each in a process of its own (one warm compute, three timed; wall time of load_sequences + accumulate +
finalize, which ends in a synchronise), alternating over --rounds rounds:
  parent_letter   a built checkout of the parent commit (--parent TREE), n as a fifth letter: the yardstick;
  this_letter     this tree, the mode off: the same work, launch for launch;
  this_wildcard   this tree, wildcards = [n].
Without --parent only the last two run. Every invocation merges its section into --out.

    tools/bench_wildcards.py [--parent TREE] [--cases ep47848,dna16k] [--rounds 3] [--out profiles/wildcards.json]
    tools/bench_wildcards.py --plain-bench PARENT_TREE [--repeats 3]   bench.py of the parent checkout and of this tree, alternating,
                                                                      `repeats` pairs in each order: both ms_per_step series"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TOKEN = 5
CASES = {"ep47848": dict(g=10, m=6, combos=100, path=0), "dna16k": dict(g=12, m=8, combos=495, path=1)}


def make_data(name):
    if name == "ep47848":
        z = np.load(os.path.join(ROOT, "tests", "golden", "tokens_EP300_47848.npz"))
        return z["tokens"].astype(np.int32), z["offsets"].astype(np.int64), int(z["n_train"]), int(z["n_test"])
    rng = np.random.Generator(np.random.PCG64(20201214))
    N, L = 16000, 300
    X = rng.integers(1, 5, size=(N, L), dtype=np.int32)
    for i in rng.choice(N, size=N // 100, replace=False):
        a = int(rng.integers(0, L - 20))
        X[i, a:a + 20] = N_TOKEN
    return X.reshape(-1), np.arange(N + 1, dtype=np.int64) * L, N, 0


def worker(tree, name, wildcard):
    """One process: one warm compute, three timed; prints one JSON line."""
    sys.path.insert(0, tree)
    from fastsk_amd import _native
    case = CASES[name]
    tokens, offsets, ntr, nte = make_data(name)
    kw = {"wildcards": [N_TOKEN]} if wildcard else {}
    e = _native.Engine(case["g"], case["m"], path=case["path"], **kw)
    combos = np.arange(case["combos"], dtype=np.int32)
    times = []
    for _ in range(4):
        t0 = time.perf_counter()
        e.load_sequences(tokens, offsets, ntr, nte)
        t1 = time.perf_counter()
        e.accumulate(combos)
        e.finalize()
        times.append((time.perf_counter() - t0, t1 - t0))
    st = e.stats()
    print(json.dumps(dict(ms=[round(1e3 * t, 4) for t, _ in times[1:]], load_ms=[round(1e3 * t, 4) for _, t in times[1:]],
                          path="dense" if st["path_used"] == 1 else "sparse", alphabet=st["alphabet"], key_space=st["key_space"],
                          n_feat=st["n_feat"], launches=st["launches"], compact_keys_avg=st["compact_keys_avg"],
                          digest=[int(x) for x in e.counts_digest()])), flush=True)
    e.close()


def spawn(tree, name, wildcard):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--cases", name] + (["--wildcard"] if wildcard else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not line:
        raise RuntimeError("worker failed (%s):\n%s\n%s" % (" ".join(cmd), r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(line[-1])


def run_case(name, parent, rounds):
    variants = ([("parent_letter", parent, False)] if parent else []) + [("this_letter", ROOT, False), ("this_wildcard", ROOT, True)]
    runs = {v: [] for v, _, _ in variants}
    for _ in range(rounds):
        for v, tree, wild in variants:
            runs[v].append(spawn(tree, name, wild))
    out = dict(CASES[name], case=name, rounds=rounds)
    for v, rs in runs.items():
        ms = [x for r in rs for x in r["ms"]]
        out[v] = dict(ms=ms, min=min(ms), max=max(ms), mean=round(float(np.mean(ms)), 4), load_ms_mean=round(float(np.mean([x for r in rs for x in r["load_ms"]])), 4),
                      **{k: rs[0][k] for k in ("path", "alphabet", "key_space", "n_feat", "launches", "compact_keys_avg")})
    base = out.get("parent_letter", out["this_letter"])
    out["wildcard_mean_over_yardstick_mean"] = round(out["this_wildcard"]["mean"] / base["mean"], 4)
    out["wildcard_not_slower_than_yardstick_max"] = bool(out["this_wildcard"]["mean"] <= base["max"])
    if parent:
        out["letter_digest_equals_parent"] = runs["this_letter"][0]["digest"] == runs["parent_letter"][0]["digest"]
    return out


def plain_bench(parent, repeats, steps, warmup):
    """bench.py in a built checkout of the parent commit and in this tree, alternating: `repeats` pairs parent-first, then
    `repeats` pairs this-first."""
    series = {"parent": [], "this": []}
    order = [("parent", parent), ("this", ROOT)]
    for pairs in (order, order[::-1]):
        for _ in range(repeats):
            for who, tree in pairs:
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode != 0 or not line:
                    raise RuntimeError("bench.py failed in %s:\n%s\n%s" % (tree, r.stdout[-2000:], r.stderr[-2000:]))
                series[who].append(round(json.loads(line[-1])["ms_per_step"], 3))
    lo, hi = min(series["parent"]), max(series["parent"])
    mean = float(np.mean(series["this"]))
    return dict(cmd="bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), pairs_each_order=repeats, ms_per_step=series,
                parent_range=[lo, hi], parent_mean=round(float(np.mean(series["parent"])), 3), this_mean=round(mean, 3),
                this_mean_within_parent_range=bool(lo <= mean <= hi), this_mean_not_above_parent_max=bool(mean <= hi))


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
    ap.add_argument("--cases", default="ep47848,dna16k")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wildcards.json"))
    ap.add_argument("--plain-bench", metavar="PARENT_TREE", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--worker", metavar="TREE", default=None)
    ap.add_argument("--wildcard", action="store_true")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.cases, args.wildcard)
        return
    if args.plain_bench:
        res = plain_bench(os.path.abspath(args.plain_bench), args.repeats, args.steps, args.warmup)
        print(json.dumps(res), flush=True)
        merge(args.out, "plain_bench", res)
        return
    for name in args.cases.split(","):
        res = run_case(name, os.path.abspath(args.parent) if args.parent else None, args.rounds)
        print(json.dumps(res), flush=True)
        merge(args.out, "case_" + name, res)


if __name__ == "__main__":
    main()
