"""Yardsticks and inputs of the mismatch-weighted kernels (fsk_set_mismatch_weights, ``weights=`` / ``max_mismatches=``), shared by
tests/test_mismatch_host.py, tests/test_emu_mismatch.py and tests/test_gpu_mismatch.py. Nothing here touches an engine.

Two independent expectations of W = sum_h c_h N_h:
  ``brute_weighted``    from the definition: the Hamming distance of every pair of g-windows, counted per distance h, in numpy;
  ``levels_reference``  the algebra the engine uses, sum_j a_j S_j, with S_j from the CPU oracle (``port.raw_counts`` over all
                        C(g, j) combinations of (g, m = j)) and the a_j solved here in Python integers."""
from math import comb

import numpy as np

DNA = {1: 4, 4: 1, 2: 3, 3: 2, 5: 5}   # a = 1, c = 2, g = 3, t = 4, n = 5
MASK = (1 << 64) - 1


def solve_levels(g, c):
    """a_0..a_d in Python integers: d the last h with c_h != 0, a_d = c_d, a_h = c_h - sum_{j>h} a_j C(g-h, j-h)."""
    c = [int(x) for x in c]
    d = max(h for h, x in enumerate(c) if x)
    a = [0] * (d + 1)
    for h in range(d, -1, -1):
        a[h] = c[h] - sum(a[j] * comb(g - h, j - h) for j in range(h + 1, d + 1))
    return a


def gkm_weights(g, m, d=None):
    """c_h = C(g-h, m-h): the weights of the plain gapped k-mer kernel (d: truncated at d mismatches)."""
    d = m if d is None else d
    return [comb(g - h, m - h) if h <= d else 0 for h in range(m + 1)]


def ragged(n, lo, hi, sigma=4, seed=0):
    """n sequences over 1..sigma, lengths uniform in [lo, hi], one of exactly lo and one of exactly hi when n >= 2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(lo, hi + 1, size=n)
    if n >= 2:
        lens[0], lens[n - 1] = hi, lo
    return [rng.integers(1, sigma + 1, size=int(L)).tolist() for L in lens]


def _windows(seqs, g, comp=None):
    """(all g-windows as rows, the row at which every sequence's windows start); comp: of the reverse complements."""
    rows, starts = [], [0]
    for s in seqs:
        x = np.asarray(s if comp is None else [comp[t] for t in reversed(s)], dtype=np.int64)
        w = np.lib.stride_tricks.sliding_window_view(x, g)
        rows.append(w)
        starts.append(starts[-1] + len(w))
    return np.concatenate(rows), np.asarray(starts[:-1], dtype=np.int64)


def _block_counts(wa, sa, wb, sb, hmax):
    """[h][i, j] = pairs (a window of sequence i in wa, one of sequence j in wb) at Hamming distance exactly h, h <= hmax."""
    dist = np.zeros((len(wa), len(wb)), dtype=np.uint8)
    for p in range(wa.shape[1]):
        dist += wa[:, p][:, None] != wb[:, p][None, :]
    out = []
    for h in range(hmax + 1):
        eq = (dist == h).astype(np.int64)
        out.append(np.add.reduceat(np.add.reduceat(eq, sa, axis=0), sb, axis=1))
    return out


def brute_profile(seqs, g, hmax, comp=None):
    """N_h, h <= hmax, as (N, N) int64 matrices, straight from the definition. Reverse-complement mode (``comp``): the four strand
    blocks N_h(x, y) + N_h(x, rc y) + N_h(rc x, y) + N_h(rc x, rc y)."""
    wf, sf = _windows(seqs, g)
    prof = _block_counts(wf, sf, wf, sf, hmax)
    if comp is not None:
        wr, sr = _windows(seqs, g, comp)
        for other in (_block_counts(wf, sf, wr, sr, hmax), _block_counts(wr, sr, wf, sf, hmax), _block_counts(wr, sr, wr, sr, hmax)):
            prof = [a + b for a, b in zip(prof, other)]
    return prof


def brute_weighted(seqs, g, c, comp=None):
    """sum_h c_h N_h mod 2^64 as the uint64 lower triangle (row-major, cell (i, j <= i) at i (i + 1) / 2 + j)."""
    n = len(seqs)
    prof = brute_profile(seqs, g, len(c) - 1, comp)
    total = np.zeros((n, n), dtype=object)
    for h, ch in enumerate(c):
        if ch:
            total = total + int(ch) * prof[h].astype(object)
    assert (total == total.T).all()
    return np.array([int(v) & MASK for v in total[np.tril_indices(n)]], dtype=np.uint64)


def raw_level(port, seqs, g, j, comp=None):
    """S_j: the oracle's raw triangle of (g, m = j) over all C(g, j) combinations; reverse-complement mode: on [X ; rc(X)],
    the four blocks added."""
    from oracle import loader
    n = len(seqs)
    combos = np.arange(port.num_combos(g, j), dtype=np.int32)
    if comp is None:
        tok, off = loader.flatten([list(s) for s in seqs])
        return port.raw_counts(tok, off, g, j, combos)[0]
    both = [list(s) for s in seqs] + [[comp[t] for t in reversed(list(s))] for s in seqs]
    tok, off = loader.flatten(both)
    tri2 = port.raw_counts(tok, off, g, j, combos)[0]
    sq = np.zeros((2 * n, 2 * n), dtype=tri2.dtype)
    il = np.tril_indices(2 * n)
    sq[il] = tri2
    sq.T[il] = tri2
    f = sq[:n, :n] + sq[:n, n:] + sq[n:, :n] + sq[n:, n:]
    return f[np.tril_indices(n)]


def levels_reference(port, seqs, g, c, comp=None):
    """sum_j a_j S_j in Python integers reduced mod 2^64; returns (uint64 triangle, the partial sums after each level in
    ascending order of j, as Python-int lists before reduction, for the levels that run)."""
    a = solve_levels(g, c)
    total, partial = None, []
    for j, aj in enumerate(a):
        if aj == 0:
            continue
        s = raw_level(port, seqs, g, j, comp).astype(object) * aj
        total = s if total is None else total + s
        partial.append(total.copy())
    return np.array([int(v) & MASK for v in total], dtype=np.uint64), partial


def normalised(port, counts, n):
    """The expression the parity tests use for K, applied to W."""
    return port.normalise(counts.astype(np.float64), n)


# ---- the cases -------------------------------------------------------------------------------------------------------------
DEFINITION_WEIGHTS = [[1, 1, 1, 1], [20, 10, 4, 0], [1, 0, 0, 0], [2 ** 40, 1, 0, 0]]
FOLD_EDGE_N = [1, 2, 22, 23, 91, 724]   # 1, 3, 253, 276 (an odd count), 4186 and 262,450 cells


def definition_case():
    """40 ragged DNA sequences of 20..60 tokens, g = 6, m = 3."""
    return {"seqs": ragged(40, 20, 60, seed=406), "g": 6, "m": 3}


def fold_edge_case(n):
    """n DNA sequences of 4..9 tokens, g = 4, m = 2, weights [6, 3, 0]: d = 1, a = (-6, 3)."""
    return {"seqs": ragged(n, 4, 9, seed=4200 + n), "g": 4, "m": 2, "weights": [6, 3, 0]}


def protein_case():
    """30 sequences over 20 tokens, 25..70 long, g = 8, m = 4, truncated at 2 mismatches: levels k = 8, 7, 6."""
    return {"seqs": ragged(30, 25, 70, sigma=20, seed=84), "g": 8, "m": 4, "max_mismatches": 2}


def revcomp_case():
    """32 ragged DNA sequences with a run of n in one of them, g = 6, m = 3."""
    seqs = ragged(32, 12, 50, seed=63)
    seqs[3][2:7] = [5] * 5
    return {"seqs": seqs, "g": 6, "m": 3, "weights": [20, 10, 4, 0]}


def skip_case():
    """n_train = 20, n_test = 12."""
    return {"seqs": ragged(32, 15, 45, seed=2012), "g": 6, "m": 3, "weights": [5, 3, 1, 0], "n_train": 20, "n_test": 12}


def wide_key_case():
    """65 distinct tokens (7 bits a symbol), g = 14: level 0's 14-mer needs 98 bits, the parent's 13-mer (m = 1) 91."""
    rng = np.random.Generator(np.random.PCG64(65))
    seqs = [rng.integers(1, 66, size=int(L)).tolist() for L in (40, 33, 28, 37, 30, 25)]
    seqs[0][:40] = list(range(1, 41))
    seqs[1][:25] = list(range(41, 66))
    seqs[2][:20] = seqs[0][5:25]   # something shared
    assert len({t for s in seqs for t in s}) == 65
    return {"seqs": seqs, "g": 14, "m": 1, "weights": [7, 2]}
