"""Inputs, the restated plan and the numpy yardsticks of the sparse dataflow's front end — the record extraction with its
first-digit histogram, the LSD radix sort (k_sx_hist, k_sx_scan_slot, k_sx_scatter<RecT, NB>, driven by sx_sort) and the segment
kernels (k_sx_seg_count, k_sx_seg_scan, k_sx_seg_write) — shared by tests/test_emu_sort_edges.py and
tests/test_gpu_sort_edges.py. Nothing here touches an engine.

Four yardsticks:
  the counts         ``counts_by_definition_wide``: any alphabet, k-mers of any length (the rows of kept symbols go through
                     np.unique, never through a number), K = sum over the combinations of C C^T in int64. Proved against
                     ``port.raw_counts`` one combination at a time (``check_reference``) before an engine is asked;
  the plan           ``sort_plan``: what fsk_engine.hip:733-746, 944-950 (plan_words, the commit of a load), sx_sort and
                     sx_batch_begin derive from (sigma, k, g, N, nfeat): key bits, record type, passes and their widths, tiles.
                     No stat names the record type: the plan stands in for it and its other fields are asserted against the stats;
  the sorted slot    ``sorted_records``: the records (key << sb) | sequence of one slot in sorted order (key the mixed-radix number
                     of the ranked symbols, first kept position most significant);
  the segment tiles  ``segment_tiles``: per 2048 records what k_sx_seg_count writes — entries, tile-local index of the last entry
                     that heads a run (-1: none), likewise of the last test head.
The last two only prove that a case of group H reaches the edge it names; they are never compared with an engine."""
from itertools import combinations
from math import ceil

import numpy as np

SX_TILE, SG_TILE = 4096, 2048
THREADS = 4   # oracle threads: never sized by the machine's CPU count

# the update forms groups G and H run in: (tuning, sparse_form the stats must show, sparse_desc the stats must show; None: not forced)
FORMS = {"default": ({}, 0, None), "desc": ({"sparse_desc": 1}, 0, 1), "nodesc": ({"sparse_desc": -1}, 0, 0),
         "blocks": ({"sparse_form": 2}, 2, None), "atomics": ({"sparse_global": 1}, 1, None)}


# ---- the reference ------------------------------------------------------------------------------------------------------
_POSITIONS = {}


def combo_positions(g, k, combo):
    """The combo-th k-subset of range(g) in lexicographic order (as wide_cells_cases.combo_positions)."""
    if (g, k) not in _POSITIONS:
        _POSITIONS[g, k] = list(combinations(range(g), k))
    return _POSITIONS[g, k][int(combo)]


def windows_of(X, g):
    """(all g-windows of all sequences as rows of one array, the sequence of every row), sequences in order, windows in order."""
    rows, seq = [], []
    for i, s in enumerate(X):
        s = np.asarray(s, dtype=np.int32)
        if len(s) >= g:
            w = np.lib.stride_tricks.sliding_window_view(s, g)
            rows.append(w)
            seq.append(np.full(len(w), i, dtype=np.int64))
    return np.concatenate(rows), np.concatenate(seq)


def counts_by_definition_wide(X, g, m, combos):
    """K = sum over the combos of C C^T, C[sequence, key] = windows of the sequence whose kept positions spell the key, keys
    numbered by np.unique over the rows of kept symbols -> (lower triangle as uint64, U = sum over combos and keys of
    d (d + 1) / 2 with d the sequences that hold the key, the largest count of one key in one sequence)."""
    n, k = len(X), g - m
    win, seq = windows_of(X, g)
    K = np.zeros((n, n), dtype=np.int64)
    U, top = 0, 0
    for c in combos:
        kept = np.ascontiguousarray(win[:, list(combo_positions(g, k, c))])
        keys, inv = np.unique(kept, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        C = np.bincount(seq * len(keys) + inv, minlength=n * len(keys)).reshape(n, len(keys)).astype(np.int64)
        K += C @ C.T
        d = (C > 0).sum(axis=0).astype(np.int64)
        U += int((d * (d + 1) // 2).sum())
        top = max(top, int(C.max()))
    assert int(K.max()) < 2 ** 53   # (get_triangle's reference goes through float64)
    return K[np.tril_indices(n)].astype(np.uint64), U, top


def check_reference(port, case):
    """counts_by_definition_wide against the independent CPU oracle, one combination a call: cells and U equal."""
    from oracle import loader
    tok, off = loader.flatten(case["X"])
    for c in case["combos"]:
        one = np.array([c], dtype=np.int32)
        mine, U, _ = counts_by_definition_wide(case["X"], case["g"], case["m"], one)
        theirs, _, U_orc = port.raw_counts(tok, off, case["g"], case["m"], one, threads=THREADS)
        assert int(mine.max()) < 2 ** 32   # (the oracle's cells are unsigned int within a call)
        assert np.array_equal(mine, theirs), int(c)
        assert U == U_orc, int(c)


# ---- the plan -----------------------------------------------------------------------------------------------------------
def bits_below(v):
    """The smallest b with 2^b >= v (sx_bits_below)."""
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def pass_widths(bits):
    """sx_sort: ``bits`` split evenly over ceil(bits / 8) passes, the wider ones first."""
    passes = (bits + 7) // 8
    return [bits // passes + (1 if p < bits % passes else 0) for p in range(passes)]


def sort_plan(sigma, k, g, N, nfeat):
    """What the load and a batch derive from the shape alone. V is the engine's key_space: sigma^k while that stays <= 2^62,
    else 2^62 and the key is the symbols' bit fields side by side."""
    V, symbits = 1, 0
    for _ in range(k):
        if V > (1 << 62) // sigma:
            symbits = bits_below(sigma)
            V = 1 << 62
            break
        V *= sigma
    keybits = symbits * k if symbits else min(max(bits_below(V), 1), 62)
    sb = max(bits_below(N), 1)
    recbits = keybits + sb
    bits = 2 if sigma <= 4 else 4 if sigma <= 16 else 8 if sigma <= 256 else 16
    widths = pass_widths(keybits)
    return dict(V=V, symbits=symbits, keybits=keybits, sb=sb, recbits=recbits, rec_bytes=4 if recbits <= 32 else 8 if recbits <= 64 else 16,
                passes=len(widths), widths=widths, NB=sorted({max(w, 4) for w in widths}), tps=ceil(nfeat / SX_TILE),
                tpg=ceil(nfeat / SG_TILE), bits=bits, win_words=2 if g * bits <= 64 else 4 if g * bits <= 128 else 0,
                small=recbits <= 32 and V <= 1 << 24)


def hist_heads(nfeat, slots):
    """k_sx_hist's 16-byte path: the records before the first 16-byte boundary of every full tile of every slot (u32 records)."""
    return {(4 - (s * nfeat + t * SX_TILE) % 4) % 4 for s in range(slots) for t in range(nfeat // SX_TILE)}


def digit_spread(keys, widths):
    """For every pass of the LSD sort over ``keys`` (a slot's keys in extraction order): (the most source tiles one digit value
    comes from, whether some digit value occurs in all four wave quarters of one source tile)."""
    keys = np.asarray(keys, dtype=np.int64)
    out, shift = [], 0
    for w in widths:
        d = (keys >> shift) & ((1 << w) - 1)
        at = np.arange(len(keys))
        tiles = max(len(np.unique(at[d == v] // SX_TILE)) for v in np.unique(d))
        quarters = any(len(np.unique(at[(d == v) & (at // SX_TILE == t)] % SX_TILE // (SX_TILE // 4))) == 4
                       for v in np.unique(d) for t in range(ceil(len(keys) / SX_TILE)))
        out.append((tiles, quarters))
        keys = keys[np.argsort(d, kind="stable")]
        shift += w
    return out


def slot_keys(X, g, combo, m=1):
    """The keys of one slot in extraction order (sequence by sequence, window by window): the mixed-radix number of the ranked
    symbols at the kept positions, the first most significant, int64 (sigma^k must fit)."""
    k = g - m
    win, _ = windows_of(X, g)
    tokens = np.unique(np.concatenate([np.asarray(s) for s in X]))
    assert len(tokens) ** k < 2 ** 62
    rank = np.searchsorted(tokens, win[:, list(combo_positions(g, k, combo))]).astype(np.int64)
    key = np.zeros(len(win), dtype=np.int64)
    for c in range(k):
        key = key * len(tokens) + rank[:, c]
    return key


# ---- the sorted slot and its segment tiles ------------------------------------------------------------------------------
def sorted_records(X, g, combo, m=1):
    """The records (key << sb) | sequence of one slot (combination ``combo`` of (g, m)) in sorted order, int64 (sigma^k * 2^sb
    must fit), and sb."""
    key = slot_keys(X, g, combo, m)
    _, seq = windows_of(X, g)
    sb = max(bits_below(len(X)), 1)
    assert (int(key.max()) + 1) << sb < 2 ** 62
    return np.sort((key << sb) | seq), sb


def segment_tiles(records, sb, skip_from=None):
    """Per tile of 2048 records (entries, lrh, lth) as k_sx_seg_count states them: record j starts an ENTRY when it differs
    from record j - 1 and a RUN when its key does (j = 0 starts both); the first test entry (sequence >= skip_from) of a run
    is a TEST HEAD. lrh / lth: the index, among the tile's entries, of the last one that heads a run / is a test head; -1:
    none (lth also without skip_from)."""
    r = np.asarray(records, dtype=np.int64)
    prev = np.concatenate([[-1], r[:-1]])
    entry = r != prev
    run_head = entry & ((r >> sb) != (prev >> sb))
    run_head[0] = entry[0] = True
    seq, pseq = r & ((1 << sb) - 1), prev & ((1 << sb) - 1)
    test_head = np.zeros(len(r), dtype=bool) if skip_from is None else entry & (seq >= skip_from) & (run_head | (pseq < skip_from))
    out = []
    for t0 in range(0, len(r), SG_TILE):
        e, h, th = entry[t0:t0 + SG_TILE], run_head[t0:t0 + SG_TILE], test_head[t0:t0 + SG_TILE]
        idx = np.cumsum(e) - 1   # (the entry index of every record that is one)
        out.append((int(e.sum()), int(idx[h][-1]) if h.any() else -1, int(idx[th][-1]) if th.any() else -1))
    return out


# ---- sequences ----------------------------------------------------------------------------------------------------------
def related_sequences(sigma, g, N, nfeat, seed):
    """N sequences over tokens 1..sigma whose window counts sum to exactly nfeat: cut from one random parent at offsets 0..7
    with about 3 % point mutations, so that even k-mers of 30 and 62 symbols are shared between rows. Every token occurs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.multinomial(nfeat - N, np.full(N, 1.0 / N)) + 1 if N > 1 else np.array([nfeat])
    assert w.sum() == nfeat and w.min() >= 1
    L = w + g - 1
    parent = rng.integers(1, sigma + 1, size=int(L.max()) + 8)
    plant = min(len(parent) - 1, 7)
    room = min(sigma, len(parent) - plant)
    parent[plant:plant + room] = rng.permutation(sigma)[:room] + 1   # (every symbol within reach of every offset)
    X = []
    for i in range(N):
        o = int(rng.integers(0, 8))
        s = parent[o:o + int(L[i])].copy()
        hit = rng.random(len(s)) < 0.03
        s[hit] = (s[hit] - 1 + rng.integers(1, sigma, size=int(hit.sum()))) % sigma + 1 if sigma > 1 else s[hit]
        X.append(s.tolist())
    return X


def periodic_sequences(seed=7):
    """Group G: 24 sequences of 300..900 symbols, each one repeated unit of period 1, 2, 3 or 5 over {1, 2}; every third has
    one flipped symbol."""
    rng = np.random.Generator(np.random.PCG64(seed))
    units = {1: [[1], [2]], 2: [[1, 2]], 3: [[1, 1, 2], [1, 2, 2]], 5: [[1, 1, 2, 1, 2], [1, 2, 2, 2, 1], [1, 1, 1, 1, 2]]}
    X = []
    for i in range(24):
        period = (1, 2, 3, 5)[i % 4]
        unit = units[period][int(rng.integers(0, len(units[period])))]
        n = int(rng.integers(300, 901))
        s = (unit * (n // period + 1))[:n]
        if i % 3 == 2:
            at = int(rng.integers(20, n - 20))
            s[at] = 3 - s[at]
        X.append(s)
    return X


def homopolymers():
    """Group H (i): ones of length 5009 and 2059, [1, 2] x 30, ones of length 40, 4107 and 12."""
    return [[1] * 5009, [1] * 2059, [1, 2] * 30, [1] * 40, [1] * 4107, [1] * 12]


def k1_sequences(ones, twos):
    """Group H (ii), g = 2: sequence i has ones[i] windows that start with 1, then twos[i] that start with 2."""
    return [[1] * a + [2] * b + [2 if b or not a else 1] for a, b in zip(ones, twos)]


# group H (ii): name -> windows starting with 1, with 2, n_train, the tile and the feature it must show there
K1_CASES = {
    # run 1 starts at record sum(ones): the last record of tile 0, the first and the second of tile 1
    "run_head_2047": dict(ones=[1000, 700, 347, 0, 0], twos=[10, 0, 700, 2500, 5], n_train=3, head_at=2047),
    "run_head_2048": dict(ones=[1000, 700, 348, 0, 0], twos=[10, 0, 700, 2500, 5], n_train=3, head_at=2048, tile=1, lrh=0),
    "run_head_2049": dict(ones=[1000, 700, 349, 0, 0], twos=[10, 0, 700, 2500, 5], n_train=3, head_at=2049, tile=1, lrh=0),
    # the first test entry of run 0 (sequence 2 with n_train = 2) on the first record of tile 1 and on the last of tile 0; run 1
    # starts in tile 2 only: tile 1 has entries and no run head
    "test_head_2048": dict(ones=[1000, 1048, 500, 200, 1500], twos=[10, 0, 700, 900, 5], n_train=2, test_at=2048, tile=1, lth=0, lrh=-1),
    "test_head_2047": dict(ones=[1000, 1047, 501, 200, 1500], twos=[10, 0, 700, 900, 5], n_train=2, test_at=2047, tile=1, lrh=-1),
    # two entries in tile 1, neither a run head; the run of the twos starts in tile 2
    "entries_no_run_head": dict(ones=[2500, 1000, 900, 0, 3], twos=[0, 40, 700, 2100, 5], n_train=1, tile=1, lrh=-1),
}


# ---- the cases ----------------------------------------------------------------------------------------------------------
def case(sigma, k, m, N, nfeat, combos, seed=None, X=None, n_train=None):
    """A case: sequences (made here unless given), combinations, the plan. The reference comes from ``reference``."""
    g = k + m
    if X is None:
        X = related_sequences(sigma, g, N, nfeat, seed if seed is not None else 1000 * sigma + 10 * k + N + nfeat)
    assert len(X) == N and sum(len(s) - g + 1 for s in X) == nfeat
    assert set(np.unique(np.concatenate([np.asarray(s) for s in X])).tolist()) == set(range(1, sigma + 1))   # (token t is rank t - 1)
    return dict(X=X, sigma=sigma, k=k, g=g, m=m, N=N, nfeat=nfeat, combos=np.asarray(combos, dtype=np.int32),
                n_train=N if n_train is None else n_train, plan=sort_plan(sigma, k, g, N, nfeat))


_ONCE = {}


def once(key, build):
    """A case and its reference (``want``, ``U``, ``top``), computed once per process and shared: the arrays are read-only."""
    if key not in _ONCE:
        c = build()
        want, U, top = counts_by_definition_wide(c["X"], c["g"], c["m"], c["combos"])
        want.setflags(write=False)
        _ONCE[key] = dict(c, want=want, U=U, top=top)
    return _ONCE[key]


def group_a(k):
    """sigma = 2, N = 4, nfeat = 4 * 4096 + 1: tps = 5, one record in the last sort tile and in the last segment tile."""
    return once(("A", k), lambda: case(2, k, 1, 4, 4 * SX_TILE + 1, [0, k]))


def group_b(k, m=1):
    from math import comb
    return once(("B", k, m), lambda: case(2, k, m, 4, SX_TILE + 1, [0, comb(k + m, m) - 1]))


def group_c(sigma, k):
    return once(("C", sigma, k), lambda: case(sigma, k, 1, 40, SX_TILE + 1, [0, k]))


def group_d(sigma, k):
    return once(("D", sigma, k), lambda: case(sigma, k, 1, 64, 2 * SX_TILE + 1, [0, k]))


def group_e(sigma, k, N, nfeat):
    return once(("E", sigma, k, N), lambda: case(sigma, k, 1, N, nfeat, [0, k]))


def group_f(N, nfeat):
    return once(("F", N, nfeat), lambda: case(2, 12, 1, N, nfeat, [0, 5, 9, 12]))


def group_g():
    def build():
        X = periodic_sequences()
        return case(2, 9, 2, 24, sum(len(s) - 10 for s in X), [0, 17, 54], X=X, n_train=15)
    return once("G", build)


def group_h_homopolymers(n_train):
    """One reference for the six sequences; only the train / test split differs between the variants."""
    def build():
        X = homopolymers()
        return case(2, 8, 2, 6, sum(len(s) - 9 for s in X), [0, 44], X=X)
    return dict(once("H1", build), n_train=n_train)


def group_h_k1(name):
    def build():
        spec = K1_CASES[name]
        X = k1_sequences(spec["ones"], spec["twos"])
        return dict(case(2, 1, 1, len(X), sum(len(s) - 1 for s in X), [0, 1], X=X, n_train=spec["n_train"]), spec=spec)
    return once(("H2", name), build)


def group_i():
    """sigma = 2, k = 24, all 25 combinations in one batch of more than 16 slots, nfeat = 8193: wb = 14."""
    return once("I", lambda: case(2, 24, 1, 16, 2 * SX_TILE + 1, np.arange(25)))


A_KS = list(range(1, 31))
B_KS = [31, 32, 33, 40, 41, 48, 49, 55, 56, 57, 62]
C_CASES = [(20, 15), (20, 19), (65, 13)]
D_CASES = [(3, 5), (3, 6), (5, 7), (20, 4), (20, 6)]
E_CASES = [(2, 24, 255, 8195), (2, 24, 256, 8195), (2, 24, 257, 8195), (4, 28, 255, 4097), (4, 28, 256, 4097), (4, 28, 257, 4097)]
F_NFEAT = [16, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8191, 8192, 8193, 8194, 8195, 12289, 16384]
H1_TRAIN = [1, 2, 3, 5, 6]
