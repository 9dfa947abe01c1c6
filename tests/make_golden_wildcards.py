#!/usr/bin/env python3
"""Generate tests/golden/wildcards_ep47848_60.npz (build container only): wildcard mode on 40 training + 20 test sequences of
the committed token fixture tests/golden/tokens_EP300_47848.npz — the five training rows that hold n (3507, 4000, 4001, 4002,
5153) among them —, g = 10, m = 6, exact, with n as the wildcard, as the COMPILED REFERENCE (oracle/_ref, the CPU port where it
is absent) counts it: its raw counts of the FRAGMENTS (the maximal n-free runs of at least g symbols) as rows, the blocks
summed onto the rows they came from (tests/wildcard_cases.py:fragment_fold):
  tokens, offsets, n_train   the 60 sequences (the fixture's ids);
  wildcard                   the id of n;
  n_feat                     the windows free of n;
  counts                     uint64[60 * 61 / 2], the folded raw counts;
  tri                        float64, K[i,j] / sqrt(K[i,i] K[j,j]) of the fold (fastsk_kernel.cpp:96-103).
Only data travels."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "wildcards_ep47848_60.npz")
WITH_N = [3507, 4000, 4001, 4002, 5153]
G, M = 10, 6


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import loader
    from conftest import load_tokens, reference_fasta
    from fastsk_amd import FastaUtility
    import wildcard_cases as cases
    tokens, offsets, n_train, n_test, _, _ = load_tokens("EP300_47848")
    with tempfile.TemporaryDirectory() as tmp:
        reader = FastaUtility()
        t2, o2, _ = reader.read_packed(reference_fasta("EP300_47848.train", tmp))
    assert np.array_equal(t2, tokens[:offsets[n_train]]), "the fixture is not this reader's"
    wild = reader.wildcards("n")
    rows = sorted(set(range(0, 35)) | set(WITH_N))[:40]
    assert len(rows) == 40 and set(WITH_N) <= set(rows)
    rows += list(range(n_train, n_train + 20))
    seqs = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in rows]
    raw = loader.ref().raw_counts if loader.have_ref() else None
    port = loader.port()
    nc = int(port.num_combos(G, M))
    counts = cases.fragment_fold(port, seqs, set(wild), G, M, np.arange(nc, dtype=np.int32), raw=raw)
    tri = port.normalise(counts.astype(np.float64), len(seqs))
    tok, off = loader.flatten(seqs)
    np.savez_compressed(OUT, tokens=tok.astype(np.int32), offsets=off.astype(np.int64), n_train=np.int64(40), wildcard=np.int64(wild[0]),
                        n_feat=np.int64(sum(cases.valid_counts(seqs, set(wild), G))), counts=counts, tri=tri, g=np.int64(G), m=np.int64(M),
                        rows=np.array(rows, dtype=np.int64))
    print("%s: %d sequences, %d cells, wildcard %s, reference: %s" % (OUT, len(seqs), len(counts), wild, "compiled" if raw else "port"))


if __name__ == "__main__":
    main()
