"""Inputs of the reverse-complement edge cases, shared by tests/test_gpu_revcomp.py (scale = 1: the sizes that reach each
branch on the device) and tests/test_emu_revcomp.py (scale < 1: the same cases with fewer ordinary sequences, the
edge-defining lengths kept wherever the emulator can afford them). A builder returns a dict: ``seqs`` (lists of tokens), ``g``,
``m``, ``combos`` and whatever else its test needs. Nothing here touches an engine: the checks that run the cases are in
tests/test_emu_revcomp.py."""
import numpy as np

DNA = {1: 4, 4: 1, 2: 3, 3: 2, 5: 5}   # a = 1, c = 2, g = 3, t = 4, n = 5
A, C_, G_, T, N_ = 1, 2, 3, 4, 5
THREADS = 16                          # oracle threads: never sized by the machine's CPU count


def scaled(n, scale, floor):
    return max(floor, int(round(n * scale)))


def ragged(rng, n, lo, hi, sigma=4):
    """n sequences over 1..sigma, lengths uniform in [lo, hi]; one has exactly hi symbols and one exactly lo (at seeded
    places)."""
    lens = rng.integers(lo, hi + 1, size=n)
    a, b = rng.choice(n, size=2, replace=False)
    lens[a], lens[b] = hi, lo
    return [rng.integers(1, sigma + 1, size=int(L)).tolist() for L in lens]


def spread(nc, n=5):
    """n combination ids: the first, the last, the rest evenly between."""
    return np.unique(np.linspace(0, nc - 1, n).astype(np.int32))


# ---- the update count U of this mode, from the definition --------------------------------------------------------------
def fold_updates(port, seqs, comp, g, m, combos):
    """U of oracle/fastsk_oracle.c:count_runs for the folded feature sets: per combination and key, cu (cu + 1) / 2 with cu
    the number of sequences that hold the key on EITHER strand (a key held by one feature of one sequence: 1, the same
    formula). ``comp=None``: one strand, which must be the oracle's own U (tests/test_emu_revcomp.py checks that)."""
    k = g - m
    sigma = max(max(s) for s in seqs) + 1
    total = 0
    for c in combos:
        pos = np.asarray(port.combo_positions(g, k, int(c)), dtype=np.int64)
        keys, ids = [], []
        for i, s in enumerate(seqs):
            strands = [np.asarray(s, dtype=np.int64)]
            if comp is not None:
                strands.append(np.asarray([comp[t] for t in reversed(s)], dtype=np.int64))
            for x in strands:
                nw = len(x) - g + 1
                if nw <= 0:
                    continue
                key = np.zeros(nw, dtype=np.int64)
                for p in pos:
                    key = key * sigma + x[p:p + nw]
                keys.append(key)
                ids.append(np.full(nw, i, dtype=np.int64))
        keys, ids = np.concatenate(keys), np.concatenate(ids)
        held = np.unique(keys * len(seqs) + ids)           # (key, sequence) once each
        _, cu = np.unique(held // len(seqs), return_counts=True)
        total += int((cu * (cu + 1) // 2).sum())
    return total


def strand_maxima(port, seqs, comp, g, m, combos):
    """(largest count one strand of one sequence gives one key of one combination, the same with both strands in the one
    counter) — what k_dense_count's u16 counters hold, from the definition."""
    k = g - m
    sigma = max(max(s) for s in seqs) + 1
    one = both = 0
    for c in combos:
        pos = np.asarray(port.combo_positions(g, k, int(c)), dtype=np.int64)
        for s in seqs:
            keys = []
            for x in (np.asarray(s, dtype=np.int64), np.asarray([comp[t] for t in reversed(s)], dtype=np.int64)):
                nw = len(x) - g + 1
                key = np.zeros(nw, dtype=np.int64)
                for p in pos:
                    key = key * sigma + x[p:p + nw]
                keys.append(key)
                one = max(one, int(np.unique(key, return_counts=True)[1].max()))
            both = max(both, int(np.unique(np.concatenate(keys), return_counts=True)[1].max()))
    return one, both


# ---- 1. dense: the staging regimes of the strand loop -------------------------------------------------------------------
PANEL, SYM_CAP, LDS_BUDGET = 64, 64 << 10, 150 << 10


def dense_plan(max_win, g, vq, extra):
    """fsk_engine_dense.hip:dense_plan restated: (windows per staging chunk, key quads per histogram sweep); (0, 0) = no fit."""
    sym = min((max_win + g - 1) * PANEL, SYM_CAP)
    if sym + extra + 1024 > LDS_BUDGET:
        return 0, 0
    vcq = min(vq, (LDS_BUDGET - sym - extra) // 512)
    if vcq < vq:
        vcq &= ~1
        if vcq < 2:
            return 0, 0
    if sym // PANEL < g:
        return 0, 0
    return min(max_win, sym // PANEL - (g - 1)), vcq


def dense_regime(lmax, g, keys, compact, dense_chunk=0):
    """The regime accumulate_dense (fsk_engine_dense.hip:127-145) puts the strand loop of k_dense_count in for a longest
    sequence of lmax symbols, ``keys`` = alphabet^k, with the rank table of key compaction (2 bytes a key) or without, and
    the tuning key dense_chunk: (regime, histogram sweeps) with
    'A' both strands resident (rc_rows != 0): sweeps after the first reuse the staged symbols;
    'B' a strand is staged in one pass but there is no second buffer (CH >= max_win, rc_rows == 0): every sweep restages
        strand by strand;
    'C' chunked staging (CH < max_win, rc_rows == 0)."""
    w1, vq = lmax - g + 1, (keys + 3) // 4
    extra = 2 * keys if compact else 0
    ch, vcq = dense_plan(w1, g, vq, extra)
    assert ch > 0
    if ch >= w1 and not dense_chunk:
        ch2, vcq2 = dense_plan(w1, g, vq, extra + (w1 + g - 1) * PANEL)
        if ch2 >= w1:
            return "A", -(-vq // vcq2)
    if dense_chunk:
        ch = max(1, min(ch, dense_chunk))
    return ("B" if ch >= w1 else "C"), -(-vq // vcq)


WHOLE_STRAND = 1 << 20   # dense_chunk: no cap that binds, but no second buffer either (regime B wherever a strand fits)
# (longest sequence, m at g = 12, a few n among the symbols, (regime, histogram sweeps) as planned, the same with
#  dense_chunk=WHOLE_STRAND)
DENSE_REGIMES = [(300, 8, False, ("A", 1), ("B", 1)),
                 (1000, 8, False, ("A", 2), ("B", 1)),
                 (1025, 8, False, ("C", 1), ("C", 1)),
                 (2500, 8, False, ("C", 1), ("C", 1)),
                 (1000, 5, False, ("A", 82), ("B", 24)),
                 (1000, 7, True, ("A", 22), ("B", 5))]


def dense_regime_case(port, lmax, m, rare_n, scale=1.0):
    """Ragged DNA at g = 12, lengths in [g, lmax] with one sequence of exactly lmax and one of exactly g symbols. Scale 1:
    N = 200 (four panels of 64, the last one partly empty), lengths uniform, five combos (first, last, three between).
    Scaled down: N = 70 (two panels, the last one partly empty), every eighth length uniform in [g, lmax] and the rest in
    [g, 150] (the emulator's sort is slow; the longest sequence alone decides the regime), first and last combo, and the
    tiny staging chunk 67 windows instead of 7 at k = 7, where every chunk is staged once per histogram sweep.
    ``rare_n``: three n among the symbols: 5^5 = 3125 keys and key compaction by the engine's own rule (a rare symbol)."""
    g = 12
    full = scale >= 1.0
    n = scaled(200, scale, 70)
    rng = np.random.Generator(np.random.PCG64(1000 * lmax + m))
    seqs = ragged(rng, n, g, lmax)
    if not full:
        for i, s in enumerate(seqs):
            if i % 8 and g < len(s) < lmax:
                del s[int(rng.integers(g, 151)):]
    if rare_n:
        for i in (1, n // 2, n - 2):
            seqs[i][len(seqs[i]) // 2] = N_
    keys = (5 if rare_n else 4) ** (g - m)
    return {"seqs": seqs, "g": g, "m": m, "combos": spread(port.num_combos(g, m), 5 if full else 2), "keys": keys,
            "compact": rare_n, "max_windows": 2 * (lmax - g + 1), "tiny_chunk": 7 if full or keys <= 256 else 67}


# ---- 2. dense: counts that cross a plane because both strands land in one counter --------------------------------------
def plane_case(name, scale=1.0):
    """g = 5, m = 2 (k = 3), DNA + n. Low-complexity sequences scattered among ordinary ragged ones so that flagged rows sit
    in three panels and two tiles (N = 140 > 128).
      'hi_plane': no strand alone puts more than 15 into a counter, both together do, and nothing exceeds 255:
          a^12 t^12 is its own reverse complement: aaa counts 8 windows + up to 2 at the a|t border = 10 a strand, 20
          together; likewise t^12 a^12, c^11 g^11 and a^10 cg t^10; (at)^8, (acgt)^4 and (catg)^4 (x == rc x: every count
          doubles; 6 a strand for (at)^8); n^12 under the self-pair 5:5: 8 windows of nnn a strand, 16 in the one counter.
      'overflow': no strand alone exceeds 255, both together do: a^200 t^200 (<= 198 a strand, 396 together), (at)^150
          (<= 148 a strand, 296 together), (acgt)^200 (<= 199 a strand), n^140 (136 a strand, 272 together); plus the
          hi_plane sequences.
    (strand_maxima counts this from the definition and tests/test_emu_revcomp.py asserts it.)"""
    g, m = 5, 2
    n = scaled(140, scale, 72)
    rng = np.random.Generator(np.random.PCG64(52))
    seqs = ragged(rng, n, g, 60)
    hi = [[A] * 12 + [T] * 12, [T] * 12 + [A] * 12, [C_] * 11 + [G_] * 11, [A, T] * 8, [A, C_, G_, T] * 4, [N_] * 12,
          [A] * 10 + [C_, G_] + [T] * 10, [C_, A, T, G_] * 4]
    over = [[A] * 200 + [T] * 200, [A, T] * 150, [A, C_, G_, T] * 200, [N_] * 140, [G_] * 180 + [A] * 7 + [C_] * 190]
    special = hi + (over if name == "overflow" else [])
    # places: every panel of 64 and both sides of row 128 when n allows, ends included
    places = sorted(set(int(p) for p in np.linspace(0, n - 1, len(special)).round()))
    assert len(places) == len(special)
    for p, s in zip(places, special):
        seqs[p] = list(s)
    if n > 129:   # and on both sides of row 128, where the second tile row begins
        assert not {128, 129} & set(places)
        seqs[128], seqs[129] = list(special[0]), list(special[-1])
        places = sorted(places + [128, 129])
    return {"seqs": seqs, "g": g, "m": m, "combos": np.arange(10, dtype=np.int32), "flagged": places}


# ---- 3. sparse --------------------------------------------------------------------------------------------------------
def long_sequence_case(windows, scale=1.0):
    """300 ordinary sequences and one of ``windows`` windows (g = 9, m = 4, four combos): max_windows = 2 * windows decides the
    entry format (fsk_engine_sparse.hip: packed = N < 65535 && maxW < 65536). All but the last 500 windows of the long one
    are an (at) repeat — its own reverse complement, so its two keys take (windows - 500) / 2 from EACH strand:
    multiplicities of about 2^15 - 250, the largest two strands of one sequence can give two keys. n_train is two thirds of
    N: skip_test_block keeps every cell whose column is a train sequence, 8/9 of the triangle."""
    g, m = 9, 4
    n = scaled(300, scale, 30)
    rng = np.random.Generator(np.random.PCG64(66))
    seqs = ragged(rng, n, 40, 120)
    rep = windows - 500
    long = ([A, T] * ((rep + g) // 2 + 1))[:rep + g - 1] + rng.integers(1, 5, size=500).tolist()
    assert len(long) - g + 1 == windows
    at = n * 137 // 300
    seqs.insert(at, long)
    combos = np.array([3, 40, 77, 125] if scale >= 1.0 else [3, 125], dtype=np.int32)   # (scaled down: two of the four)
    return {"seqs": seqs, "g": g, "m": m, "combos": combos, "n_train": (2 * len(seqs)) // 3,
            "long_at": at, "max_windows": 2 * windows}


def products_case(scale=1.0):
    """A 1500-long poly-a, a 1400-long poly-t and an (at) repeat of 1200 among 300 ragged DNA sequences, g = 10, m = 6, every
    tenth combo: poly-a and poly-t share no k-mer until the second strand of each is counted, and then their cell takes
    2 * 1491 * 1391 a combination — multiplicity x windows far beyond the product field of one 32-bit update word."""
    g, m = 10, 6
    n = scaled(300, scale, 40)
    rng = np.random.Generator(np.random.PCG64(8))
    seqs = ragged(rng, n, 12, 90)
    ia, it, iat = n * 17 // 300, n * 201 // 300, n * 202 // 300 + 1
    seqs[ia], seqs[it], seqs[iat] = [A] * 1500, [T] * 1400, [A, T] * 600
    combos = np.arange(0, 210, 10 if scale >= 1.0 else 50, dtype=np.int32)   # (scaled down: every fiftieth)
    return {"seqs": seqs, "g": g, "m": m, "combos": combos, "poly_a": ia, "poly_t": it}


def wide_window_case(port, scale=1.0):
    """DNA + n packs to 4 bits a symbol; g = 33 is 132 bits: no packed window array, k_sx_extract<RecT, true> gathers the
    symbols itself, of the second strand backwards. 300 ragged sequences of 33..110 symbols (about 23,000 features)."""
    g, m = 33, 28
    n = scaled(300, scale, 24)
    rng = np.random.Generator(np.random.PCG64(3328))
    seqs = ragged(rng, n, g, 110, sigma=5)
    nc = port.num_combos(g, m)
    return {"seqs": seqs, "g": g, "m": m, "combos": np.array([0, 1, 777, nc // 2, nc - 1], dtype=np.int32)}


SPARSE_FORMS = [("owner bands", {"sparse_form": 1, "sparse_desc": -1}, 0),
                ("owner bands, descriptors", {"sparse_form": 1, "sparse_desc": 1, "sparse_desc_min": 5}, 0),
                ("two-level blocks", {"sparse_form": 2, "sparse_desc": -1}, 2),
                ("two-level blocks, descriptors", {"sparse_form": 2, "sparse_desc": 1, "sparse_desc_min": 5}, 2),
                ("unpacked entries", {"sparse_unpacked": 1}, None),
                ("direct atomics", {"sparse_form": 3}, 1)]
SMALL_BLOCKS = ("two-level blocks, forced small", {"sparse_form": 2, "blocks_sub_shift": 8, "blocks_max_bands": 7,
                                                   "blocks_band_shift_max": 12}, 2)


def low_complexity_case(scale=1.0):
    """About 1500 ragged low-complexity DNA sequences (g = 9, m = 4, three combos): each a short random motif (1..6 symbols)
    repeated to a length in 9..120 with a few point mutations, so that keys repeat inside a sequence (long entries,
    multiplicities) and across sequences built on the same motif; every eighth sequence is plain random. Row bands at
    multiples of 128. Scaled down: lengths 9..60 and two of the three combos."""
    g, m = 9, 4
    n = scaled(1500, scale, 150)
    top = 120 if scale >= 1.0 else 60
    rng = np.random.Generator(np.random.PCG64(1500))
    seqs = []
    for i in range(n):
        L = int(rng.integers(g, top + 1))
        if i % 8 == 7:
            seqs.append(rng.integers(1, 5, size=L).tolist())
            continue
        motif = rng.integers(1, 5, size=int(rng.integers(1, 7)))
        s = np.resize(motif, L)
        for p in rng.integers(0, L, size=int(rng.integers(0, 4))):
            s[p] = rng.integers(1, 5)
        seqs.append(s.tolist())
    seqs[5], seqs[n - 3] = [int(t) for t in rng.integers(1, 5, size=g)], [A, C_] * (top // 2)
    cut = max(128, (n // 3) // 128 * 128)
    bands = [(0, cut), (cut, min(n, 2 * cut)), (min(n, 2 * cut), n)]
    return {"seqs": seqs, "g": g, "m": m, "combos": np.array([0, 50, 125] if scale >= 1.0 else [0, 125], dtype=np.int32),
            "bands": [b for b in bands if b[0] < b[1]]}


# ---- 4. the group's int32 narrowing ----------------------------------------------------------------------------------
def narrowing_case(windows, scale=1.0):
    """130 short ragged sequences and one (at) repeat of ``windows`` windows, g = 6, m = 2, all 15 combos. The repeat is its
    own reverse complement and, at k = 4, has two keys of windows / 2 a strand: its diagonal cell is
    15 * 2 * windows^2 (each key (2 * windows / 2)^2). windows = 10,000: 15 * windows^2 = 1.5e9 < 2^31 (one strand's bound
    would narrow the exchange) while the cell is 3e9 >= 2^31. windows = 4,000: 15 * (2 * 4000)^2 = 9.6e8 < 2^31, narrow."""
    g, m = 6, 2
    n = scaled(130, scale, 20)
    rng = np.random.Generator(np.random.PCG64(21))
    seqs = ragged(rng, n, g, 80)
    at = n // 2
    seqs.insert(at, ([A, T] * (windows // 2 + g))[:windows + g - 1])
    return {"seqs": seqs, "g": g, "m": m, "combos": np.arange(15, dtype=np.int32), "long_at": at, "windows": windows,
            "diagonal": 15 * 2 * windows * windows, "n_train": len(seqs) - len(seqs) // 4}
