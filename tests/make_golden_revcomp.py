#!/usr/bin/env python3
"""Generate tests/golden/revcomp_ep300_60.npz (build container only): reverse-complement mode on the first 60 EP300
training sequences of the committed token fixture (tests/golden/tokens_EP300.npz), g = 10, m = 6, exact, as the COMPILED
REFERENCE (oracle/_ref) counts it — its raw counts of the 120 sequences [X ; rc(X)], the four 60 x 60 blocks added:
  tokens, offsets      the 60 sequences (the fixture's ids);
  comp_tokens, comp_complements   the complement map of those ids (a<->t, c<->g, from the reader's vocabulary);
  counts               uint64[60 * 61 / 2], the folded raw counts;
  tri                  float64, K[i,j] / sqrt(K[i,i] K[j,j]) of the fold (fastsk_kernel.cpp:96-103).
Only data travels."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "golden", "revcomp_ep300_60.npz")
N, G, M = 60, 10, 6


def fold_blocks(tri2, n):
    """The 2n x 2n lower triangle of [X ; rc(X)] -> the n x n lower triangle of the four blocks' sum."""
    sq = np.zeros((2 * n, 2 * n), dtype=tri2.dtype)
    il = np.tril_indices(2 * n)
    sq[il] = tri2
    sq.T[il] = tri2
    f = sq[:n, :n] + sq[:n, n:] + sq[n:, :n] + sq[n:, n:]
    return f[np.tril_indices(n)]


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import loader
    from conftest import load_tokens, reference_fasta
    from fastsk_amd import FastaUtility
    tokens, offsets, _, _, _, _ = load_tokens("EP300")
    tokens, offsets = tokens[:offsets[N]].copy(), offsets[:N + 1].copy()
    with tempfile.TemporaryDirectory() as tmp:
        reader = FastaUtility()
        t2, o2, _ = reader.read_packed(reference_fasta("EP300.train", tmp))
    assert np.array_equal(t2[:o2[N]], tokens) and np.array_equal(o2[:N + 1], offsets), "the fixture is not this reader's"
    comp = reader.complement()
    seqs = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in range(N)]
    both = seqs + [[comp[t] for t in reversed(s)] for s in seqs]
    tok2, off2 = loader.flatten(both)
    nc = int(loader.port().num_combos(G, M))
    tri2, _ = loader.ref().raw_counts(tok2, off2, G, M, np.arange(nc, dtype=np.int32))
    counts = fold_blocks(tri2, N)
    tri = loader.port().normalise(counts.astype(np.float64), N)
    keys = sorted(comp)
    np.savez_compressed(OUT, tokens=tokens, offsets=offsets, comp_tokens=np.array(keys, dtype=np.int32),
                        comp_complements=np.array([comp[k] for k in keys], dtype=np.int32), counts=counts, tri=tri,
                        g=np.int64(G), m=np.int64(M))
    print("%s: %d sequences, %d cells, map %s" % (OUT, N, len(counts), comp))


if __name__ == "__main__":
    main()
