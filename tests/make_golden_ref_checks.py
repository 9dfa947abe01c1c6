#!/usr/bin/env python3
"""Generate tests/golden/ref_checks.npz (build container only): what the compiled reference (oracle/_ref) returns for
the inputs of test_oracle.py's checks against it, so that those checks run where oracle/_ref was not built:
  shuffle__<n>__<seed>   sha256 of ref_shuffle_order(seed, n) (the reference's std::shuffle of 0..n-1);
  fresh<i>_exact         full_triangle of fresh input i, exact, t = 3;
  fresh<i>_approx_tri / _approx_sd / _order   the same in approx mode (t = 1, seed 42) and the order it drew;
  edge<i>                full_triangle of conftest.EDGE_CASES[i], t = 1.
Only data travels."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "ref_checks.npz")

SHUFFLE_N = (1, 2, 3, 4, 210, 495, 1001, 38760, 46340, 46341, 50000, 184756)
SHUFFLE_SEEDS = (0, 1, 42, 777, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 1759622400, 2 ** 40 + 12345)
FRESH = [(4, 8, 4, 30), (20, 7, 3, 25), (3, 6, 5, 12)]   # (sigma, g, m, n)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fresh_cases():
    """Random ragged inputs: (tokens, offsets, n_train, n_test, g, m), the last 7 sequences the test set."""
    rng = np.random.default_rng(11)
    for sigma, g, m, n in FRESH:
        X = [rng.integers(1, sigma + 1, size=int(L)).astype(np.int32) for L in rng.integers(g, 60, size=n)]
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(x) for x in X])
        yield np.concatenate(X), offsets, n - 7, 7, g, m


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import loader
    from conftest import EDGE_CASES
    from fastsk_amd import _native
    ref = loader.ref()
    out = {}
    for n in SHUFFLE_N:
        for seed in SHUFFLE_SEEDS:
            out["shuffle__%d__%d" % (n, seed)] = np.array(sha(ref.shuffle_order(seed, n)))
    for i, (tokens, offsets, ntr, nte, g, m) in enumerate(fresh_cases()):
        out["fresh%d_exact" % i], _ = ref.full_triangle(tokens, offsets, ntr, nte, g, m, t=3)
        nc = int(loader.port().num_combos(g, m))
        out["fresh%d_order" % i] = ref.shuffle_order(42, nc)
        out["fresh%d_approx_tri" % i], out["fresh%d_approx_sd" % i] = ref.full_triangle(tokens, offsets, ntr, nte, g, m, t=1,
                                                                                        approx=True, seed=42)
    for i, (X, ntr, nte, g, m) in enumerate(EDGE_CASES):
        tokens, offsets = _native.flatten(X)
        out["edge%d" % i], _ = ref.full_triangle(tokens, offsets, ntr, nte, g, m, t=1)
    np.savez_compressed(OUT, **out)
    print("%s: %d arrays" % (OUT, len(out)))


if __name__ == "__main__":
    main()
