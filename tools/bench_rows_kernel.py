#!/usr/bin/env python3
"""The rows kernel (fsk_rows_build: L(r, c) = <K(r, train), K(c, train)>, kernel_type="linear") on one GPU
-> profiles/rows_kernel.json.

Workloads (--cases):
  ep300     tests/golden/tokens_EP300.npz, 2000 train + 2000 test rows, g = 10, m = 6 exact;
  ep47848   tests/golden/tokens_EP300_47848.npz, 6506 train rows and its test rows, g = 10, m = 6, the first 100 of the 210
            combos (BASELINE config 3: the rows kernel's cost does not depend on what the cells hold);
  dna8k     synthetic DNA 8,000 x 300 (tests/svm_cases.dna), train only, g = 10, m = 6, 100 combos: the size the tile is chosen at;
  dna32k    32,000 x 300, the same.
Per case: one warm build, then --reps builds (fsk_finalize drops the rows kernel, fsk_rows_build builds it again); medians of
the scratch pass and of the product (fsk_rows_info.ms_scratch / ms_product, host clock around stream syncs), clocks as found.
Multiply-adds as fastsk_amd/csrc/fsk_engine_rows.hip counts them, per second, and the fraction of 19.6 10^12 a second — the
ceiling of one fp64 multiply and one fp64 add a term, DERIVED from the data sheet's 78.6 TFLOP/s of vector fp64 (an FMA counted
as two), not measured. For scale only: torch.matmul in fp64 of the same A on the same GPU (rocBLAS: free to use FMA, MFMA and any
order, so no bar to meet; its multiply-adds are N n N, the full square) and numpy on the host up to --host-max-n rows.

    tools/bench_rows_kernel.py [--cases ep300,ep47848,dna8k,dna32k] [--reps 5] [--lib PATH] [--label TEXT] [--out profiles/rows_kernel.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CEILING = 19.6e12   # multiply-adds a second: 78.6e12 / 2 instructions a second, two instructions a multiply-add (derived)


def golden(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tokens_%s.npz" % name))
    return z["tokens"].astype(np.int32), z["offsets"].astype(np.int64), int(z["n_train"]), int(z["n_test"])


def synthetic(n):
    import svm_cases
    X, _ = svm_cases.dna(n, 300, 20201214 + n)
    return X.reshape(-1), np.arange(n + 1, dtype=np.int64) * 300, n, 0


CASES = {"ep300": dict(data=lambda: golden("EP300"), g=10, m=6, combos=None),
         "ep47848": dict(data=lambda: golden("EP300_47848"), g=10, m=6, combos=100),
         "dna8k": dict(data=lambda: synthetic(8000), g=10, m=6, combos=100),
         "dna32k": dict(data=lambda: synthetic(32000), g=10, m=6, combos=100)}


def multiply_adds(n, N):
    return (n * (n + 1) // 2 + (N - n) * n) * n + (N - n) * n


def run_case(name, reps, lib, host_max_n, matmul):
    import torch
    from fastsk_amd import _native
    case = CASES[name]
    tok, off, n, n_test = case["data"]()
    N = n + n_test
    e = _native.Engine(case["g"], case["m"], lib=lib, skip_test_block=True)
    t0 = time.perf_counter()
    e.load_sequences(tok, off, n, n_test)
    e.accumulate(np.arange(case["combos"] or e.lib.num_combos(case["g"], case["m"]), dtype=np.int32))
    e.finalize()
    kernel_ms = 1e3 * (time.perf_counter() - t0)
    e.rows_build()   # warm: code objects, the allocations' first touch
    scratch, product = [], []
    for _ in range(reps):
        e.finalize()   # a new result: the rows kernel is dropped
        info = e.rows_build()
        scratch.append(info["ms_scratch"])
        product.append(info["ms_product"])
    ma = multiply_adds(n, N)
    ms = statistics.median(product)
    out = dict(case=name, n_train=n, n_seq=N, g=case["g"], m=case["m"], combos=case["combos"] or "all", tile=info["tile"], panel=info["panel"],
               tiles=tiles_of(n, N, info["tile"]), kernel_ms=round(kernel_ms, 3), reps=reps, scratch_ms=round(statistics.median(scratch), 3),
               product_ms=round(ms, 3), product_ms_all=[round(x, 3) for x in product], scratch_bytes=info["scratch_bytes"],
               resident_bytes=info["resident_bytes"], multiply_adds=ma, multiply_adds_per_s=ma / (ms * 1e-3),
               fraction_of_derived_ceiling=round(ma / (ms * 1e-3) / CEILING, 4))
    if matmul:
        A = e.get_block_torch(0, N, 0, n)
        torch.cuda.synchronize()
        (A @ A.T)[0, 0].item()   # warm
        times = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            G = A @ A.T
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        out["torch_matmul_fp64_ms"] = round(statistics.median(times), 3)
        out["torch_matmul_multiply_adds"] = N * N * n
        L = e.rows_block(0, min(N, 64), 0, min(n, 64), raw=True)
        out["max_rel_diff_to_torch_64x64"] = float(np.max(np.abs(L - G[:min(N, 64), :min(n, 64)].cpu().numpy()) / np.abs(L)))
        if N <= host_max_n:
            Ah = A.cpu().numpy()
            t0 = time.perf_counter()
            Ah @ Ah.T
            out["numpy_host_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        else:
            out["numpy_host_ms"] = None
            out["numpy_host_why_not"] = "N = %d rows is past --host-max-n = %d" % (N, host_max_n)
        del A, G
    e.close()
    return out


def tiles_of(n, N, T):
    ncb, nrb = -(-n // T), -(-N // T)
    return ncb * (ncb + 1) // 2 + (nrb - ncb) * ncb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="ep300,ep47848,dna8k,dna32k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libfastsk_amd.so (the tile A/B)")
    ap.add_argument("--label", default=None)
    ap.add_argument("--host-max-n", type=int, default=8192)
    ap.add_argument("--no-matmul", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_kernel.json"))
    args = ap.parse_args()
    import torch
    from fastsk_amd import _native
    lib = _native.Library(args.lib) if args.lib else None
    result = dict(tool="tools/bench_rows_kernel.py", label=args.label, device=torch.cuda.get_device_name(0),
                  ceiling_multiply_adds_per_s=CEILING,
                  ceiling_note="derived: data sheet 78.6 TFLOP/s vector fp64 with an FMA counted as two -> 39.3e12 instructions/s, a multiply and an add a term; not measured",
                  cases=[])
    for name in args.cases.split(","):
        r = run_case(name, args.reps, lib, args.host_max_n, not args.no_matmul)
        print(json.dumps(r), flush=True)
        result["cases"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
