"""Yardsticks and inputs of wildcard mode (fsk_set_wildcards, ``wildcards=``), shared by tests/test_wildcards_host.py,
tests/test_emu_wildcards.py (scale < 1) and tests/test_gpu_wildcards.py (scale = 1). Nothing here touches an engine.

The definition: a g-window that holds a wildcard at ANY of its g positions is not a window; everything else is the plain
algorithm on the windows that remain. Two independent expectations:
  ``brute_counts`` / ``brute_weighted``  from the definition, in numpy: the valid windows of every sequence enumerated, per
                   combination the pairs equal at the kept positions (weighted mode: the Hamming distance of every pair of
                   valid windows); reverse complement as the four strand blocks;
  ``fragment_fold``  the CPU oracle (``port.raw_counts``) on the FRAGMENTS — the maximal wildcard-free runs of at least g
                   symbols — as rows, the blocks summed onto the rows they came from; reverse complement: on
                   [frags ; rc(frags)]."""
from math import comb

import numpy as np

import mismatch_cases
import revcomp_cases

A, C_, G_, T, N_, R_ = 1, 2, 3, 4, 5, 6
DNA = {1: 4, 4: 1, 2: 3, 3: 2}             # a wildcard need not be listed in the complement map ...
DNA_N = {1: 4, 4: 1, 2: 3, 3: 2, 5: 5}     # ... and may be, as its own complement
MASK = (1 << 64) - 1
THREADS = 16                               # oracle threads: never sized by the machine's CPU count
PANEL, SYM_CAP, LDS_BUDGET = 64, 64 << 10, 150 << 10


# ---- the definition ---------------------------------------------------------------------------------------------------------
def fragments(seq, wild, g):
    """The maximal wildcard-free runs of ``seq`` that are at least g long."""
    out, run = [], []
    for t in list(seq) + [None]:
        if t is None or t in wild:
            if len(run) >= g:
                out.append(run)
            run = []
        else:
            run.append(int(t))
    return out


def valid_windows(seq, wild, g):
    """The g-windows of ``seq`` free of wildcards, as rows, in order."""
    x = np.asarray(seq, dtype=np.int64)
    w = np.lib.stride_tricks.sliding_window_view(x, g)
    return w[~np.isin(w, list(wild)).any(axis=1)]


def valid_counts(seqs, wild, g):
    return [len(valid_windows(s, wild, g)) for s in seqs]


def _strand_windows(seqs, wild, g, comp):
    """(valid windows of every sequence stacked, the row each sequence starts at); comp: of the reverse complements — the
    reversed, complemented valid windows."""
    rows, starts = [], [0]
    for s in seqs:
        w = valid_windows(s, wild, g)
        if comp is not None:
            lut = np.zeros(max(max(comp), int(w.max())) + 1, dtype=np.int64)
            for a, b in comp.items():
                lut[a] = b
            w = lut[w[::-1, ::-1]]
        rows.append(w)
        starts.append(starts[-1] + len(w))
    return np.concatenate(rows), np.asarray(starts[:-1], dtype=np.int64)


def brute_counts(port, seqs, wild, g, m, combos, comp=None):
    """Sum over ``combos`` of the pairs of valid windows equal at the kept positions -> uint64 lower triangle."""
    n, k = len(seqs), g - m
    strands = [_strand_windows(seqs, wild, g, None)]
    if comp is not None:
        strands.append(_strand_windows(seqs, wild, g, comp))
    total = np.zeros((n, n), dtype=np.uint64)
    for c in combos:
        pos = np.asarray(port.combo_positions(g, k, int(c)), dtype=np.int64)
        keys = np.concatenate([w[:, pos] for w, _ in strands])
        _, kid = np.unique(keys, axis=0, return_inverse=True)
        kid = np.asarray(kid).reshape(-1)
        cnt = np.zeros((n, int(kid.max()) + 1), dtype=np.uint64)
        at = 0
        for w, st in strands:   # both strands of a sequence land in the one counter
            owner = np.searchsorted(st, np.arange(len(w)), side="right") - 1
            np.add.at(cnt, (owner, kid[at:at + len(w)]), np.uint64(1))
            at += len(w)
        total += cnt @ cnt.T
    return total[np.tril_indices(n)]


def brute_weighted(seqs, wild, g, c, comp=None):
    """sum_h c_h N_h over the pairs of VALID windows, mod 2^64, as the uint64 lower triangle."""
    n = len(seqs)
    wf, sf = _strand_windows(seqs, wild, g, None)
    prof = mismatch_cases._block_counts(wf, sf, wf, sf, len(c) - 1)
    if comp is not None:
        wr, sr = _strand_windows(seqs, wild, g, comp)
        for other in (mismatch_cases._block_counts(wf, sf, wr, sr, len(c) - 1), mismatch_cases._block_counts(wr, sr, wf, sf, len(c) - 1),
                      mismatch_cases._block_counts(wr, sr, wr, sr, len(c) - 1)):
            prof = [a + b for a, b in zip(prof, other)]
    total = np.zeros((n, n), dtype=object)
    for h, ch in enumerate(c):
        if ch:
            total = total + int(ch) * prof[h].astype(object)
    return np.array([int(v) & MASK for v in total[np.tril_indices(n)]], dtype=np.uint64)


def fold_rows(tri, owner, n):
    """The triangle over rows ``owner[a]`` -> the n x n sums of its blocks, as the uint64 lower triangle (on the diagonal
    the full sum over ordered pairs)."""
    f = len(owner)
    sq = np.zeros((f, f), dtype=np.uint64)
    il = np.tril_indices(f)
    sq[il] = tri
    sq.T[il] = tri
    p = np.zeros((n, f), dtype=np.uint64)
    p[np.asarray(owner), np.arange(f)] = 1
    out = p @ sq @ p.T
    assert np.array_equal(out, out.T)
    return out[np.tril_indices(n)]


def fragment_rows(seqs, wild, g, comp=None):
    """(the fragments of every sequence — with ``comp`` followed by their reverse complements —, the sequence of each)."""
    frags, owner = [], []
    for i, s in enumerate(seqs):
        for f in fragments(s, wild, g):
            frags.append(f)
            owner.append(i)
    if comp is not None:
        frags = frags + [[comp[t] for t in reversed(f)] for f in frags]
        owner = owner + owner
    return frags, owner


def fragment_fold(port, seqs, wild, g, m, combos, comp=None, threads=THREADS, raw=None):
    """``port.raw_counts`` (or ``raw``, the same call of the compiled reference) on the fragments as rows, folded."""
    from oracle import loader
    frags, owner = fragment_rows(seqs, wild, g, comp)
    tok, off = loader.flatten(frags)
    tri = (raw or port.raw_counts)(tok, off, g, m, np.asarray(combos, dtype=np.int32), threads=threads)[0]
    return fold_rows(tri, owner, len(seqs))


def plant(seq, places, token=N_):
    for p in places:
        seq[p] = token
    return seq


def sprinkle(rng, seqs, g, wild, frac):
    """About ``frac`` of the symbols of every sequence become the wildcard, as long as a valid window remains."""
    for s in seqs:
        for p in rng.integers(0, len(s), size=int(round(frac * len(s)))):
            old = s[p]
            s[p] = wild
            if not fragments(s, {wild}, g):
                s[p] = old
    return seqs


# ---- 1. the definition case ---------------------------------------------------------------------------------------------------
def definition_case():
    """Tokens 1..4, wildcards 5 and 6, lengths 12..40, g = 5, m = 2, all 10 combos. Planted: a wildcard at position 0, at
    len - 1 and at g - 1; two wildcards exactly g apart (no valid window between) and g + 1 apart (exactly one); a run of
    seven; a sequence with exactly one valid window; one with no wildcard; one whose only wildcard is token 6."""
    g, m = 5, 2
    rng = np.random.Generator(np.random.PCG64(55))
    lens = [12, 40, 17, 23, 31, 12, 28, 36, 19, 25, 33, 14, 22]
    seqs = [rng.integers(1, 5, size=L).tolist() for L in lens]
    plant(seqs[0], [0])
    plant(seqs[1], [len(seqs[1]) - 1])
    plant(seqs[2], [g - 1])
    plant(seqs[3], [6, 6 + g])            # windows 7 .. 6 would lie between: none
    plant(seqs[4], [8, 8 + g + 1])        # window 9 alone lies between
    plant(seqs[5], [g, 11])               # 12 symbols: window 0 before the first wildcard; positions 6..10 would hold a second ...
    seqs[5][6] = 6                        # ... and lose it to a wildcard of the other kind: exactly one valid window
    plant(seqs[6], range(10, 17))         # a run of seven
    plant(seqs[8], [7], token=6)          # only token 6
    plant(seqs[9], [0, 3, len(seqs[9]) - 1])
    plant(seqs[9], [12], token=6)
    plant(seqs[10], range(0, 4))          # a wildcard prefix
    plant(seqs[11], range(10, 14))        # a wildcard suffix
    case = {"seqs": seqs, "g": g, "m": m, "wild": [5, 6], "combos": np.arange(10, dtype=np.int32), "n_train": 9}
    v = valid_counts(seqs, {5, 6}, g)
    assert v[5] == 1 and v[7] == lens[7] - g + 1 and min(v) >= 1
    assert len(valid_windows(seqs[3][6:6 + g + 1], {5}, g)) == 0 and len(valid_windows(seqs[4][8:8 + g + 2], {5}, g)) == 1
    return case


# ---- 2. one panel, every place ------------------------------------------------------------------------------------------------
def panel_case(ragged_lengths):
    """64 sequences at g = 12, m = 8: sequence i holds a single wildcard at position i mod its length. One panel of the count
    kernel then has a differently placed hole in every lane, across the four-waves x four-windows trip and its tail loop.
    Lengths g + 31, or ragged g .. g + 40 (a sequence of exactly g symbols would lose its only window: those keep it)."""
    g, m = 12, 8
    rng = np.random.Generator(np.random.PCG64(64 + int(ragged_lengths)))
    seqs = []
    for i in range(64):
        L = g + 31 if not ragged_lengths else g + (i * 7) % 41
        s = rng.integers(1, 5, size=L).tolist()
        if L > 2 * g or (L > g and (i % L == 0 or i % L >= g)):
            s[i % L] = N_
        if not fragments(s, {N_}, g):
            s[i % L] = A
        seqs.append(s)
    return {"seqs": seqs, "g": g, "m": m, "wild": [N_], "combos": revcomp_cases.spread(495, 4)}


# ---- 3. the dense staging regimes -----------------------------------------------------------------------------------------------
def dense_plan(lmax, g, keys, table, strands, dense_chunk=0, cache_ok=True):
    """fsk_engine_dense.hip:accumulate_dense restated for wildcard mode: (windows a staging chunk, histogram sweeps, second
    strand resident, window-key cache). The validity words take strands * ceil(min(windows, 1024) / 32) * 256 + 4 bytes."""
    w1, vq = lmax - g + 1, (keys + 3) // 4
    extra = (2 * keys if table else 0) + strands * ((min(w1, 1024) + 31) // 32) * 256 + 4
    ch, vcq = revcomp_cases.dense_plan(w1, g, vq, extra)
    assert ch > 0
    resident = False
    if strands == 2 and ch >= w1 and not dense_chunk:
        ch2, vcq2 = revcomp_cases.dense_plan(w1, g, vq, extra + (w1 + g - 1) * PANEL)
        if ch2 >= w1:
            ch, vcq, resident, extra = ch2, vcq2, True, extra + (w1 + g - 1) * PANEL
    if dense_chunk:
        ch = max(1, min(ch, dense_chunk))
    cache = False
    if vcq < vq and ch >= w1 and not dense_chunk and strands == 1:
        ch2, vcq2 = revcomp_cases.dense_plan(w1, g, vq, extra + w1 * PANEL * 2)
        if ch2 >= w1 and vcq2 >= 64:
            ch, vcq, cache = ch2, vcq2, True
    return ch, -(-vq // vcq), resident, cache


def regime_case(lmax, m, scale=1.0, rare=False, strands=1):
    """Ragged DNA at g = 12 (revcomp_cases.dense_regime_case's shapes), 2 % wildcards planted at random, and — where the
    staging is chunked — wildcards at positions CH - 1, CH and CH + g - 2 of the long sequences: they fall in the overlap rows
    a chunk shares with the next. ``rare``: a rare real symbol r beside the wildcard, every r with a wildcard within g of it
    in some sequences."""
    g = 12
    n = revcomp_cases.scaled(200, scale, 70)
    rng = np.random.Generator(np.random.PCG64(7000 * lmax + m))
    seqs = revcomp_cases.ragged(rng, n, g, lmax)
    if scale < 1.0:
        for i, s in enumerate(seqs):
            if i % 8 and g < len(s) < lmax:
                del s[int(rng.integers(g, 151)):]
    keys = (5 if rare else 4) ** (g - m)
    ch = dense_plan(lmax, g, keys, rare, strands)[0]
    sprinkle(rng, seqs, g, N_, 0.02)
    for s in seqs:
        if len(s) > ch + g - 2:   # (the longest sequence gets all three)
            for p in (ch - 1, ch, ch + g - 2):
                if len(s) == lmax or rng.integers(0, 3):
                    s[p] = N_
    if rare:
        long = [i for i, s in enumerate(seqs) if len(s) > 4 * g]
        for q, i in enumerate(long[:12]):
            p = int(rng.integers(g, len(seqs[i]) - g))
            seqs[i][p] = R_
            if q % 3:
                d = (q % g) - g // 2
                seqs[i][p + (d or 1)] = N_   # a wildcard within g of the rare symbol (never on it)
    for s in seqs:
        assert fragments(s, {N_}, g)
    return {"seqs": seqs, "g": g, "m": m, "wild": [N_], "combos": revcomp_cases.spread(comb(g, m), 5 if scale >= 1.0 else 2),
            "keys": keys, "chunk": ch}


def poly_a_case(period, length, scale=1.0):
    """Poly-a interrupted by a single n every ``period`` symbols, among ordinary ragged DNA, g = 5, m = 2: every valid window of
    such a sequence is the one k-mer, so its count is the sequence's valid windows, ``top`` (150 at period 20 and 200 symbols:
    the hi plane; 885 at period 300 and 900 symbols: the overflow flag and the recount on the sparse dataflow)."""
    g, m = 5, 2
    n = revcomp_cases.scaled(140, scale, 72)
    rng = np.random.Generator(np.random.PCG64(period))
    seqs = revcomp_cases.ragged(rng, n, g, 60)
    for at in (3, n // 2, n - 2):
        s = [A] * length
        for p in range(period - 1, length, period):
            s[p] = N_
        seqs[at] = s
    return {"seqs": seqs, "g": g, "m": m, "wild": [N_], "combos": np.arange(10, dtype=np.int32), "top": len(valid_windows(seqs[3], {N_}, g))}


# ---- 4. sparse ------------------------------------------------------------------------------------------------------------------
def low_complexity_case(scale=1.0):
    """revcomp_cases.low_complexity_case with runs of n (1 .. 12 symbols) planted in every third sequence."""
    case = revcomp_cases.low_complexity_case(scale)
    g = case["g"]
    rng = np.random.Generator(np.random.PCG64(31))
    for i, s in enumerate(case["seqs"]):
        if i % 3 == 0 and len(s) > 2 * g:
            a, r = int(rng.integers(0, len(s))), int(rng.integers(1, 13))
            old = list(s)
            s[a:a + r] = [N_] * len(s[a:a + r])
            if not fragments(s, {N_}, g):
                s[:] = old
    case["wild"] = [N_]
    return case


def wide_window_case(port, scale=1.0):
    """A protein-like alphabet of 20 symbols and x (21) as the wildcard: 8 bits a symbol — the wildcard costs no code, but
    20 symbols need 5 > 4 bits —, g = 17 is 136 bits: no packed window array, k_sx_extract gathers the symbols itself."""
    g, m = 17, 12
    n = revcomp_cases.scaled(300, scale, 24)
    rng = np.random.Generator(np.random.PCG64(1721))
    seqs = revcomp_cases.ragged(rng, n, g, 90, sigma=20)
    sprinkle(rng, seqs, g, 21, 0.03)
    nc = port.num_combos(g, m)
    return {"seqs": seqs, "g": g, "m": m, "wild": [21], "combos": np.array([0, 1, nc // 2, nc - 1], dtype=np.int32)}


def wide_key_case():
    """65 real symbols and a wildcard (66), g = 14, m = 3: 65^11 > 2^62, keys travel as bit fields in 128-bit records."""
    case = mismatch_cases.wide_key_case()
    seqs = case["seqs"]
    plant(seqs[0], [16], token=66)
    plant(seqs[3], [0, 20], token=66)
    plant(seqs[4], [len(seqs[4]) - 1], token=66)
    for s in seqs:
        assert fragments(s, {66}, 14)
    return {"seqs": seqs, "g": 14, "m": 3, "wild": [66], "combos": np.array([0, 100, 363], dtype=np.int32)}


# ---- 6. mismatch weights ----------------------------------------------------------------------------------------------------------
def mismatch_case():
    """24 ragged DNA sequences of 14..45 tokens with wildcards, g = 6, m = 3."""
    rng = np.random.Generator(np.random.PCG64(63))
    seqs = mismatch_cases.ragged(24, 14, 45, seed=636)
    sprinkle(rng, seqs, 6, N_, 0.05)
    plant(seqs[2], [0])
    plant(seqs[5], range(6, 11))
    return {"seqs": seqs, "g": 6, "m": 3, "wild": [N_]}


# ---- 7. padding ---------------------------------------------------------------------------------------------------------------------
def padded_case(n=40, seed=77):
    """Sequences padded with 0 .. 15 n at either end (zero included): the kernel must be the plain one of the trimmed ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    core = mismatch_cases.ragged(n, 10, 40, seed=seed)
    pads = [(int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in range(n)]
    pads[0], pads[1], pads[2] = (0, 0), (15, 0), (0, 15)
    return {"core": core, "seqs": [[N_] * a + c + [N_] * b for c, (a, b) in zip(core, pads)], "g": 8, "m": 4, "wild": [N_]}
