#!/usr/bin/env python3
"""Generate tests/golden/center_weights.npz (build container only): centre-weighted mode on 40 training + 20 test sequences of
the committed token fixture tests/golden/tokens_EP300.npz, g = 10, m = 6, exact, all 210 combinations, under the profile
fastsk_amd.center_profile(8, 16, levels=4, floor=1), as the COMPILED REFERENCE (oracle/_ref)
counts it (the generator refuses to run without it, and the fixture says so in ``reference``): its raw counts of the level rows — per sequence and level t = 1 .. 4 the central substring that covers the windows
of weight >= t — folded onto the sequences they came from (tests/center_weight_cases.py:layer_fold):
  tokens, offsets, n_train   the 60 sequences (the fixture's ids);
  profile                    the weights w[0 .. n - 1];
  n_feat, max_windows        the sum of all weights, the largest sum of one sequence;
  counts                     uint64[60 * 61 / 2], the folded raw counts;
  tri                        float64, K[i,j] / sqrt(K[i,i] K[j,j]) of the fold (fastsk_kernel.cpp:96-103).
Only data travels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "center_weights.npz")
G, M = 10, 6


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import loader
    from conftest import load_tokens
    from fastsk_amd import center_profile
    import center_weight_cases as cases
    tokens, offsets, n_train, n_test, _, _ = load_tokens("EP300")
    rows = list(range(0, 40)) + list(range(n_train, n_train + 20))
    seqs = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in rows]
    profile = center_profile(8, 16, levels=4, floor=1)
    assert profile[0] == 4 and profile[-1] == 1 and max(len(s) for s in seqs) - G > 2 * len(profile)
    if not loader.have_ref():
        raise SystemExit("the compiled reference (oracle/_ref) is not built: this fixture is made from it alone")
    raw = loader.ref().raw_counts
    port = loader.port()
    nc = int(port.num_combos(G, M))
    counts = cases.layer_fold(port, seqs, profile, G, M, np.arange(nc, dtype=np.int32), raw=raw)
    tri = port.normalise(counts.astype(np.float64), len(seqs))
    nfeat, maxw = cases.expected_stats(seqs, G, profile)
    tok, off = loader.flatten(seqs)
    np.savez_compressed(OUT, tokens=tok.astype(np.int32), offsets=off.astype(np.int64), n_train=np.int64(40),
                        profile=np.array(profile, dtype=np.int64), n_feat=np.int64(nfeat), max_windows=np.int64(maxw), counts=counts,
                        tri=tri, g=np.int64(G), m=np.int64(M), rows=np.array(rows, dtype=np.int64), reference=np.array("compiled"))
    print("%s: %d sequences, %d cells, profile of %d entries, reference: %s" % (OUT, len(seqs), len(counts), len(profile),
                                                                                "compiled"))


if __name__ == "__main__":
    main()
