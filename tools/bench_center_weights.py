#!/usr/bin/env python3
"""Centre-weighted mode against the engine without it, on one GPU -> profiles/center_weights.json.

Two inputs, synthetic DNA from PCG64(20201214):
  dna16k_dense    16,000 x 300 bp, g = 12, m = 8, all 495 combos, the dense dataflow (the README's workload of the other modes);
  dna4k_sparse    4,000 x 300 bp, g = 12, m = 4 (k = 8), the first 24 combos, the sparse dataflow.
One process per run (`--worker`), one warm round, then --reps timed ones: wall time of load_sequences + accumulate + finalize,
which ends in a synchronise. Three shapes of process:
  alt     an engine with the mode off and one with center_weights = center_profile(25, 50), ALTERNATING call by call (`this_off`,
          `this_on`), and afterwards one call each with profile = 1 for ms_count and the other stage times;
  busy    the mode-off engine alternating with a second mode-off engine that makes `busy` calls in a row, untimed — as much GPU
          work between two timed calls as the mode-on call puts there (7 calls on the dense input, 3 on the sparse one), in a
          form the parent commit can run too;
  alone   the mode-off engine by itself;
  alt_parent   as `alt`, but the mode-off engine is the PARENT's library (its package imported under another name into the same
          process) while the mode-on engine is this tree's: the parent's code in the very call sequence of `alt`.
Recorded per variant: every timed call, n_feat, max_windows, sort_records (sparse: the record factor is on / off), launches.

With --parent TREE (a built checkout of the parent commit, which has no such keyword) the parent runs `alt_parent`, `busy` and
`alone`, each BEFORE and AFTER this tree's runs. The rule: this tree's mode-off median of the `alt` process must lie within
the spread the two parent runs show, [lower parent median - spread, higher parent median + spread] with spread = the
difference of the two parent medians — against the parent's `alt_parent` runs, the same call sequence
(`off_within_parent_spread`), and, written beside it, against the parent's `alone` runs (`off_within_parent_alone_spread`),
together with this tree's own `busy` and `alone` medians against the parent's runs of those shapes. The counts digest and the launches of the mode off are compared with the parent's.

    tools/bench_center_weights.py [--parent TREE] [--cases dna16k_dense,dna4k_sparse] [--reps 3] [--out profiles/center_weights.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"dna16k_dense": dict(n=16000, length=300, g=12, m=8, combos=495, path=1, busy=7),
         "dna4k_sparse": dict(n=4000, length=300, g=12, m=4, combos=24, path=2, busy=3)}
PROFILE_ARGS = (25, 50)


def make_data(case):
    rng = np.random.Generator(np.random.PCG64(20201214))
    X = rng.integers(1, 5, size=(case["n"], case["length"]), dtype=np.int32)
    return X.reshape(-1), np.arange(case["n"] + 1, dtype=np.int64) * case["length"], case["n"], 0


def parent_native(parent):
    """The parent checkout's fastsk_amd._native, imported as fastsk_amd_parent._native: it binds the parent's own library."""
    import importlib
    import importlib.util
    pkg = os.path.join(parent, "fastsk_amd")
    spec = importlib.util.spec_from_file_location("fastsk_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["fastsk_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("fastsk_amd_parent._native")


def worker(tree, name, reps, shape, parent=None):
    """One process; prints one JSON line."""
    sys.path.insert(0, tree)
    from fastsk_amd import _native
    case = CASES[name]
    tokens, offsets, ntr, nte = make_data(case)
    combos = np.arange(case["combos"], dtype=np.int32)
    variants = [("off", {}, 1, True)]   # (name, keywords, calls a round, timed)
    if shape in ("alt", "alt_parent"):
        variants.append(("on", {"center_weights": _native.center_profile(*PROFILE_ARGS)}, 1, True))
    elif shape == "busy":
        variants.append(("partner", {}, case["busy"], False))

    def call(e):
        t0 = time.perf_counter()
        e.load_sequences(tokens, offsets, ntr, nte)
        e.accumulate(combos)
        e.finalize()
        return 1e3 * (time.perf_counter() - t0)

    engines = {v: _native.Engine(case["g"], case["m"], path=case["path"], **kw) for v, kw, _, _ in variants}
    if shape == "alt_parent":
        engines["off"].close()
        pn = parent_native(parent)
        assert os.path.realpath(pn.library().path).startswith(os.path.realpath(parent))
        engines["off"] = pn.Engine(case["g"], case["m"], path=case["path"])
    out = {v: {"ms": []} for v, _, _, timed in variants if timed}
    for rnd in range(reps + 1):
        for v, _, calls, timed in variants:   # alternating
            for _ in range(calls):
                t = call(engines[v])
            if rnd and timed:
                out[v]["ms"].append(round(t, 4))
    for v, kw, _, timed in variants:
        st = engines[v].stats()
        if timed:
            out[v].update(path="dense" if st["path_used"] == 1 else "sparse", n_feat=st["n_feat"], max_windows=st["max_windows"],
                          sort_records=st["sort_records"], launches=st["launches"], digest=[int(x) for x in engines[v].counts_digest()])
        engines[v].close()
        if timed and shape == "alt":
            p = _native.Engine(case["g"], case["m"], path=case["path"], profile=True, **kw)
            call(p)
            call(p)
            st = p.stats()
            out[v]["stages_ms"] = {k: round(float(st[k]), 4) for k in sorted(st) if k.startswith("ms_") and st[k]}
            p.close()
    print(json.dumps(out), flush=True)


def spawn(tree, name, reps, shape, parent=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--cases", name, "--reps", str(reps), "--shape", shape]
    if parent:
        cmd += ["--parent", parent]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not line:
        raise RuntimeError("worker failed (%s):\n%s\n%s" % (" ".join(cmd), r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(line[-1])


def summary(ms):
    return dict(ms=ms, min=min(ms), max=max(ms), median=round(float(np.median(ms)), 4))


def within(median, runs):
    """The rule: inside [lower parent median - spread, higher parent median + spread], spread = their difference."""
    a, b = sorted(r["median"] for r in runs)
    return bool(a - (b - a) <= median <= b + (b - a))


def run_case(name, parent, reps):
    out = dict(CASES[name], case=name, reps=reps, profile="center_profile(%d, %d)" % PROFILE_ARGS)
    before = {sh: spawn(parent, name, reps, sh) for sh in ("busy", "alone")} if parent else None
    if parent:
        before["alt_parent"] = spawn(ROOT, name, reps, "alt_parent", parent)
    alone = spawn(ROOT, name, reps, "alone")
    this = spawn(ROOT, name, reps, "alt")
    busy = spawn(ROOT, name, reps, "busy")
    after = {sh: spawn(parent, name, reps, sh) for sh in ("alone", "busy")} if parent else None
    if parent:
        after["alt_parent"] = spawn(ROOT, name, reps, "alt_parent", parent)
    for v in ("off", "on"):
        out["this_" + v] = dict(summary(this[v]["ms"]), **{k: this[v][k] for k in ("path", "n_feat", "max_windows", "sort_records", "launches", "stages_ms")})
    out["this_off_alone"] = dict(summary(alone["off"]["ms"]), launches=alone["off"]["launches"])
    out["this_off_busy"] = dict(summary(busy["off"]["ms"]), launches=busy["off"]["launches"])
    out["on_over_off_median"] = round(out["this_on"]["median"] / out["this_off"]["median"], 4)
    out["n_feat_factor"] = round(this["on"]["n_feat"] / this["off"]["n_feat"], 4)
    if this["off"]["sort_records"]:
        out["record_factor"] = round(this["on"]["sort_records"] / this["off"]["sort_records"], 4)
    if parent:
        for sh in ("alt_parent", "busy", "alone"):
            runs = [summary(before[sh]["off"]["ms"]), summary(after[sh]["off"]["ms"])]
            out["parent_off_%s_runs" % sh] = runs
            out["parent_%s_spread_of_medians" % sh] = round(abs(runs[0]["median"] - runs[1]["median"]), 4)
        out["off_within_parent_spread"] = within(out["this_off"]["median"], out["parent_off_alt_parent_runs"])
        out["off_within_parent_alone_spread"] = within(out["this_off"]["median"], out["parent_off_alone_runs"])
        out["off_busy_within_parent_busy_spread"] = within(out["this_off_busy"]["median"], out["parent_off_busy_runs"])
        out["off_alone_within_parent_alone_spread"] = within(out["this_off_alone"]["median"], out["parent_off_alone_runs"])
        out["off_digest_equals_parent"] = this["off"]["digest"] == before["alone"]["off"]["digest"]
        out["off_launches_equal_parent"] = this["off"]["launches"] == before["alone"]["off"]["launches"]
    return out


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
    ap.add_argument("--cases", default="dna16k_dense,dna4k_sparse")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "center_weights.json"))
    ap.add_argument("--worker", metavar="TREE", default=None)
    ap.add_argument("--shape", choices=["alt", "alt_parent", "busy", "alone"], default="alt")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.cases, args.reps, args.shape, args.parent)
        return
    for name in args.cases.split(","):
        res = run_case(name, os.path.abspath(args.parent) if args.parent else None, args.reps)
        print(json.dumps(res), flush=True)
        merge(args.out, "case_" + name, res)


if __name__ == "__main__":
    main()
