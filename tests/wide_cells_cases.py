"""Inputs and the 64-bit reference of the wide-cell tests, shared by tests/test_gpu_wide_cells.py (the device) and
tests/test_emu_wide_cells.py (the emulator). Both dataflows sum a launch's or a batch's contributions to a cell of K in
32-bit accumulators and add into the 64-bit triangle at the end; each relies on one host-side bound:

    dense   fsk_engine_dense.hip:96, 106, 177 (accumulate_dense)   by_overflow = (2^32 - 1) // maxW^2 combos a tile launch
    sparse  fsk_engine_sparse.hip:963 (accumulate_sparse)          by_cells = max(1, (2^32 - 1) // maxW^2) combos a batch

The cases here are the smallest inputs that reach those bounds. ``port.raw_counts`` cannot be their reference as it
stands: it mirrors the reference's ``unsigned int Ks`` and wraps mod 2^32 WITHIN one call, so the reference here is
``counts_by_definition`` (numpy, int64), proved against the oracle one combination at a time modulo 2^32
(``check_reference``). A builder returns a dict: ``seqs`` (lists of tokens 1..4), ``g``, ``m``, ``combos`` and what else its
test needs; ``reference`` computes a case's triangle and U once and hands out read-only arrays. Nothing here touches an
engine."""
from itertools import combinations

import numpy as np

DNA = {1: 4, 4: 1, 2: 3, 3: 2}   # a = 1, c = 2, g = 3, t = 4
THREADS = 16                     # oracle threads: never sized by the machine's CPU count
U32 = 2 ** 32


# ---- the reference ------------------------------------------------------------------------------------------------------
_POSITIONS = {}


def combo_positions(g, k, combo):
    """The combo-th k-subset of range(g) in lexicographic order (what oracle/fastsk_oracle.c:orc_combo_positions lists)."""
    if (g, k) not in _POSITIONS:
        _POSITIONS[g, k] = list(combinations(range(g), k))
    return _POSITIONS[g, k][combo]


def window_index(X, g):
    """(tokens - 1 of all sequences in one array, where every window starts in it, the sequence of every window)."""
    lens = np.array([len(s) for s in X], dtype=np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in X]) - 1
    assert flat.min() >= 0 and flat.max() <= 3
    off = np.concatenate([[0], np.cumsum(lens)])[:-1]
    nw = np.maximum(lens - g + 1, 0)
    seq = np.repeat(np.arange(len(X), dtype=np.int64), nw)
    start = np.arange(int(nw.sum()), dtype=np.int64) - np.repeat(np.cumsum(nw) - nw, nw) + np.repeat(off, nw)
    return flat, start, seq


def count_matrix(index, n, g, m, combo):
    """C[i, v] = windows of sequence i whose kept positions spell key v (tokens 1..4, k = g - m <= 4): int64, N x 4^k, one
    np.bincount over the window keys of all sequences."""
    k = g - m
    assert 1 <= k <= 4
    flat, start, seq = index
    key = np.zeros(len(start), dtype=np.int64)
    for p in combo_positions(g, k, int(combo)):
        key = key * 4 + flat[start + p]
    return np.bincount(seq * 4 ** k + key, minlength=n * 4 ** k).reshape(n, 4 ** k)


def counts_by_definition(X, g, m, combos):
    """K = sum over the combos of C C^T in int64 (no cell of these cases comes near 2^63) -> (lower triangle as uint64,
    U = sum over combos and keys of d (d + 1) / 2 with d the sequences that hold the key, largest count of one key in one
    sequence)."""
    n = len(X)
    index = window_index(X, g)
    K = np.zeros((n, n), dtype=np.int64)
    U, top = 0, 0
    for c in combos:
        C = count_matrix(index, n, g, m, c)
        K += C @ C.T
        d = (C > 0).sum(axis=0).astype(np.int64)
        U += int((d * (d + 1) // 2).sum())
        top = max(top, int(C.max()))
    return K[np.tril_indices(n)].astype(np.uint64), U, top


def fold_by_definition(X, comp, g, m, combos):
    """Reverse-complement mode from the same definition: the reference on [X ; rc X], its four N x N blocks added (what
    tests/test_emu_revcomp.py:folded_oracle does with the oracle's counts) -> uint64 lower triangle."""
    n = len(X)
    both = [list(s) for s in X] + [[comp[int(t)] for t in reversed(list(s))] for s in X]
    tri2, _, _ = counts_by_definition(both, g, m, combos)
    sq = np.zeros((2 * n, 2 * n), dtype=np.uint64)
    il = np.tril_indices(2 * n)
    sq[il] = tri2
    sq.T[il] = tri2
    f = sq[:n, :n] + sq[:n, n:] + sq[n:, :n] + sq[n:, n:]
    return f[np.tril_indices(n)]


def check_reference(port, case, combos=None):
    """counts_by_definition against the independent oracle, one combination a call: equal modulo 2^32 (the oracle's
    ``unsigned int`` cells wrap within a call), and the U of every combination equal as it stands."""
    from oracle import loader
    tok, off = loader.flatten(case["seqs"])
    for c in (case["combos"] if combos is None else combos):
        one = np.array([c], dtype=np.int32)
        mine, U, _ = counts_by_definition(case["seqs"], case["g"], case["m"], one)
        theirs, _, U_orc = port.raw_counts(tok, off, case["g"], case["m"], one, threads=1)
        assert np.array_equal(mine & np.uint64(0xffffffff), theirs), int(c)
        assert U == U_orc, int(c)


_REFERENCES = {}


def reference(key, case):
    """(triangle, U, largest k-mer count) of a case, computed once per process and shared: the arrays are read-only."""
    if key not in _REFERENCES:
        tri, U, top = counts_by_definition(case["seqs"], case["g"], case["m"], case["combos"])
        tri.setflags(write=False)
        _REFERENCES[key] = (tri, U, top)
    return _REFERENCES[key]


def max_windows(case, strands=1):
    return strands * max(len(s) - case["g"] + 1 for s in case["seqs"])


def cell(tri, i, j):
    return int(tri[i * (i + 1) // 2 + j])


# ---- sparse: one combination alone puts 2^32 into a cell ------------------------------------------------------------
def wide_one_combo():
    """300 random DNA sequences 40..120 long (default_rng(66), as test_sparse_unpacked_entries_one_very_long_sequence) with
    two homopolymers of one letter, 70,000 and 66,000 windows, at rows 137 and 250; g = 4, m = 2, combos [0, 3]. Their three
    cells take 70000^2, 66000^2 and 70000 x 66000 a combination: by_cells = max(1, 0) = 1 holds nothing."""
    g, m = 4, 2
    rng = np.random.default_rng(66)
    seqs = [rng.integers(1, 5, size=int(L)).tolist() for L in rng.integers(40, 120, size=300)]
    seqs.insert(137, [1] * (70000 + g - 1))
    seqs.insert(250, [1] * (66000 + g - 1))
    return {"seqs": seqs, "g": g, "m": m, "combos": np.array([0, 3], dtype=np.int32), "n_train": 200, "rows": (137, 250),
            "windows": (70000, 66000)}


def wide_edge(windows):
    """Six random 30-long sequences and one homopolymer of ``windows`` windows, g = 4, m = 2, combo [0]. An entry's own cell
    takes c (c - 1) from the streams (the windows themselves come from k_sx_diag_windows): 65536 x 65535 < 2^32 <= 65537 x
    65536 — 65,537 is the first count whose own cell does not fit 32 bits."""
    g, m = 4, 2
    rng = np.random.default_rng(65536)
    seqs = [rng.integers(1, 5, size=30).tolist() for _ in range(6)]
    seqs.insert(3, [2] * (windows + g - 1))
    return {"seqs": seqs, "g": g, "m": m, "combos": np.array([0], dtype=np.int32), "n_train": 5, "rows": (3,),
            "windows": (windows,)}


def wide_edge_preconditions(case):
    W = case["windows"][0]
    assert (W * (W - 1) < U32) == (W <= 65536) and W * W >= U32


# ---- sparse: the batch bound binds ------------------------------------------------------------------------------------
def batch_bound():
    """Eight random 40-long sequences and homopolymers of 20,000 and 15,000 windows of one letter, g = 6, m = 2, all 15 combos:
    by_cells = (2^32 - 1) // 20000^2 = 10 < 15 — two batches at least — and an eleventh combo in a batch would wrap
    (11 x 20000^2 > 2^32)."""
    g, m = 6, 2
    rng = np.random.default_rng(20000)
    seqs = [rng.integers(1, 5, size=40).tolist() for _ in range(8)]
    seqs.insert(2, [3] * (20000 + g - 1))
    seqs.insert(7, [3] * (15000 + g - 1))
    return {"seqs": seqs, "g": g, "m": m, "combos": np.arange(15, dtype=np.int32), "rows": (2, 7), "windows": (20000, 15000)}


def batch_bound_preconditions(case, tri):
    maxW = max_windows(case)
    assert maxW == 20000 and (U32 - 1) // maxW ** 2 == 10 < len(case["combos"]) and 11 * maxW ** 2 > U32
    assert int(tri.max()) == 15 * 20000 ** 2 == 6 * 10 ** 9 and cell(tri, 2, 2) == 6 * 10 ** 9


# ---- dense: the chunk loop takes a second trip ----------------------------------------------------------------------
def dense_chunks():
    """140 random DNA sequences 20..60 long and one random sequence of 9,000 windows at row 77 (N = 141: two tile rows, three
    tiles), g = 8, m = 4, all 70 combos: by_overflow = (2^32 - 1) // 9000^2 = 53 < 70 — two tile launches a call."""
    g, m = 8, 4
    rng = np.random.default_rng(9000)
    seqs = [rng.integers(1, 5, size=int(L)).tolist() for L in rng.integers(20, 61, size=140)]
    seqs.insert(77, rng.integers(1, 5, size=9000 + g - 1).tolist())
    return {"seqs": seqs, "g": g, "m": m, "combos": np.arange(70, dtype=np.int32), "bands": [(0, 128), (128, 141)], "long_at": 77}


def dense_chunks_preconditions(case, top, strands=1):
    maxW = max_windows(case, strands)
    assert maxW == 9000 * strands and (U32 - 1) // maxW ** 2 == (53 if strands == 1 else 13)
    assert top <= 255   # (no k-mer count leaves the u8 panels: no chunk is handed to the sparse dataflow)


def dense_wrap(n_combos=1001):
    """128 random sequences 20..60 long and one random sequence of 45,000 windows (PCG64(45000)), g = 14, m = 10, the first
    ``n_combos`` of the 1001 combos: by_overflow = (2^32 - 1) // 45000^2 = 2 — a tile launch every two combos — and the long
    sequence's diagonal cell passes 2^32 (7,965,024,256 over all 1001): without the chunks the u32 registers would wrap."""
    g, m = 14, 10
    rng = np.random.Generator(np.random.PCG64(45000))
    long = rng.integers(1, 5, size=45000 + g - 1).tolist()   # (the generator's first draw: the diagonal quoted above)
    seqs = [rng.integers(1, 5, size=int(L)).tolist() for L in rng.integers(20, 61, size=128)]
    seqs.append(long)                                        # row 128: the second tile row
    return {"seqs": seqs, "g": g, "m": m, "combos": np.arange(n_combos, dtype=np.int32), "long_at": 128}


def dense_wrap_preconditions(case, tri, top):
    maxW = max_windows(case)
    at = case["long_at"]
    assert maxW == 45000 and (U32 - 1) // maxW ** 2 == 2 and top <= 255 and len(case["combos"]) >= 600
    assert cell(tri, at, at) > U32 and (len(case["combos"]) < 1001 or cell(tri, at, at) == 7965024256)


# ---- the tunings the sparse cases run in ----------------------------------------------------------------------------
# (tuning, sparse_form the stats must show, sparse_desc the stats must show; None: not forced)
BASE_TUNINGS = [({}, 0, None),                      # (the update streams of the owner bands are in use: form 0)
                ({"sparse_desc": -1}, 0, 0),
                ({"sparse_global": 1}, 1, None),
                ({"sparse_form": 2}, 2, None),
                ({"sparse_form": 2, "sparse_desc": 1}, 2, 1)]
DESC_TUNINGS = [({"sparse_desc": 1, "sparse_desc_cols": c}, 0, 1) for c in (0, 1, 2, 3)]   # (1: the default format)
PARTS_TUNING = ({"sparse_desc": 1, "sparse_parts_target": 256, "sparse_desc_parts": 48, "sparse_pairs": 0}, 0, 1)
# the word form with 32-bit words only: on a handful of sequences a word's product field is then 27 bits wide, a cell's words
# are few and no cut between the parts of a stream falls among them — the u32 cell of k_sx_consume gets their whole sum
WORDS_TUNING = ({"sparse_pairs": 0, "sparse_desc": -1}, 0, 0)


def tuning_id(t):
    return ",".join("%s=%s" % kv for kv in t[0].items()) or "default"
