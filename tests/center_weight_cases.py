"""Yardsticks and inputs of centre-weighted mode (fsk_set_center_weights, ``center_weights=``), shared by
tests/test_center_weights_host.py, tests/test_emu_center_weights.py (scale < 1) and tests/test_gpu_center_weights.py
(scale = 1). Nothing here touches an engine.

The definition: window p (0 <= p <= L - g) of a sequence of length L lies d(p) = floor(|2p + g - L| / 2) from the
sequence's centre and counts w[min(d(p), n - 1)] times; a window of weight 0 is not a window; everything else is the plain
algorithm on these counts. Three independent expectations:
  ``brute`` / ``brute_mismatch``  from the definition, in numpy: every window enumerated, per combination a counter per
                   sequence filled with the windows' weights and multiplied out in uint64 (mismatch weights: the Hamming
                   distance of every pair of windows); reverse complement as the second strand's windows, reversed and
                   complemented, in the same counter (the four strand blocks);
  ``window_fold``  the CPU oracle (``port.raw_counts``) on EVERY SINGLE WINDOW as a row of length g, folded as
                   P M P^T with P[i, u] = the weight of window u when it belongs to sequence i;
  ``layer_fold``   for non-increasing profiles, where the weight is the number of levels t = 1 .. max w with w >= t: the
                   oracle on the rows {the central substring of x that covers the windows of weight >= t}, folded with
                   ``fold_rows``. Exact against the reference at any N."""
from math import comb

import numpy as np

import mismatch_cases
import revcomp_cases
import wildcard_cases

A, C_, G_, T, N_ = 1, 2, 3, 4, 5
DNA = wildcard_cases.DNA
MASK = (1 << 64) - 1
THREADS = wildcard_cases.THREADS
PANEL = 64


# ---- the definition ---------------------------------------------------------------------------------------------------------
def distances(length, g):
    """d(p) of every window of a sequence of ``length`` symbols."""
    p = np.arange(length - g + 1, dtype=np.int64)
    return np.abs(2 * p + g - length) // 2


def window_weights(length, g, profile):
    """The weight of every window position (wildcards not looked at)."""
    w = np.asarray(profile, dtype=np.int64)
    return w[np.minimum(distances(length, g), len(w) - 1)]


def weighted_windows(seq, g, profile, wild=()):
    """(the windows of ``seq`` that are windows — free of wildcards, weight above 0 — as rows in order, their weights)."""
    x = np.asarray(seq, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(x, g)
    wt = window_weights(len(x), g, profile)
    keep = wt > 0
    if wild:
        keep &= ~np.isin(win, list(wild)).any(axis=1)
    return win[keep], wt[keep]


def weight_sums(seqs, g, profile, wild=()):
    return [int(weighted_windows(s, g, profile, wild)[1].sum()) for s in seqs]


def expected_stats(seqs, g, profile, wild=(), comp=None):
    """(n_feat, max_windows): sums of weights, both strands in reverse-complement mode."""
    v = weight_sums(seqs, g, profile, wild)
    s = 2 if comp is not None else 1
    return s * sum(v), s * max(v)


def _complement_lut(comp, top):
    lut = np.arange(max(max(comp), top) + 1, dtype=np.int64)
    for a, b in comp.items():
        lut[a] = b
    return lut


def _all_windows(seqs, g, profile, wild=(), comp=None):
    """(windows stacked, their weights, their owner); with ``comp`` the second strand's windows follow the first's."""
    rows, wts, own = [], [], []
    for i, s in enumerate(seqs):
        w, t = weighted_windows(s, g, profile, wild)
        rows.append(w)
        wts.append(t)
        own.append(np.full(len(w), i, dtype=np.int64))
    if comp is not None:
        lut = _complement_lut(comp, max(int(r.max()) for r in rows if len(r)))
        for i in range(len(seqs)):
            rows.append(lut[rows[i][::-1, ::-1]])
            wts.append(wts[i][::-1])
            own.append(own[i])
    return np.concatenate(rows), np.concatenate(wts), np.concatenate(own)


def brute(port, seqs, profile, g, m, combos, comp=None, wild=()):
    """Sum over ``combos`` of cnt @ cnt.T, cnt[i, key] = the weights of the windows of sequence i (both strands) with that
    key at the kept positions -> uint64 lower triangle (wraps mod 2^64 as the engine's cells do)."""
    n, k = len(seqs), g - m
    win, wt, own = _all_windows(seqs, g, profile, wild, comp)
    total = np.zeros((n, n), dtype=np.uint64)
    for c in combos:
        pos = np.asarray(port.combo_positions(g, k, int(c)), dtype=np.int64)
        _, kid = np.unique(win[:, pos], axis=0, return_inverse=True)
        kid = np.asarray(kid).reshape(-1)
        cnt = np.zeros((n, int(kid.max()) + 1), dtype=np.uint64)
        np.add.at(cnt, (own, kid), wt.astype(np.uint64))
        total += cnt @ cnt.T
    return total[np.tril_indices(n)]


def brute_mismatch(seqs, profile, g, c, comp=None, wild=()):
    """sum_h c_h N_h, N_h(x, y) = sum over the pairs of windows at Hamming distance h of the product of their weights."""
    n = len(seqs)
    win, wt, own = _all_windows(seqs, g, profile, wild, comp)
    ham = (win[:, None, :] != win[None, :, :]).sum(axis=2)
    p = np.zeros((n, len(win)), dtype=object)
    p[own, np.arange(len(win))] = [int(t) for t in wt]
    total = np.zeros((n, n), dtype=object)
    for h, ch in enumerate(c):
        if ch:
            total = total + int(ch) * p.dot((ham == h).astype(object)).dot(p.T)
    return np.array([int(v) & MASK for v in total[np.tril_indices(n)]], dtype=np.uint64)


def window_fold(port, seqs, profile, g, m, combos, comp=None, wild=(), threads=THREADS):
    """The oracle on every single window as a row of length g (at most about 700 of them), folded with the weights."""
    from oracle import loader
    n = len(seqs)
    win, wt, own = _all_windows(seqs, g, profile, wild, comp)
    tok, off = loader.flatten([r.tolist() for r in win])
    tri = port.raw_counts(tok, off, g, m, np.asarray(combos, dtype=np.int32), threads=threads)[0]
    f = len(win)
    sq = np.zeros((f, f), dtype=np.uint64)
    il = np.tril_indices(f)
    sq[il] = tri
    sq.T[il] = tri
    p = np.zeros((n, f), dtype=np.uint64)
    p[own, np.arange(f)] = wt.astype(np.uint64)
    return (p @ sq @ p.T)[np.tril_indices(n)]


def layer_rows(seqs, profile, g, comp=None):
    """Non-increasing profiles: the rows of ``layer_fold`` and the sequence each belongs to. Level t = 1 .. max w: the
    windows of weight >= t are those with d <= D_t, a central run p_lo .. p_hi of positions; the row is
    x[p_lo : p_hi + g]."""
    w = np.asarray(profile, dtype=np.int64)
    assert (np.diff(w) <= 0).all(), "layer_fold needs a non-increasing profile"
    rows, owner = [], []
    for i, s in enumerate(seqs):
        wt = window_weights(len(s), g, profile)
        for t in range(1, int(w.max()) + 1):
            at = np.nonzero(wt >= t)[0]
            if len(at):
                assert at[-1] - at[0] + 1 == len(at)
                rows.append([int(v) for v in s[at[0]:at[-1] + g]])
                owner.append(i)
    if comp is not None:
        rows = rows + [[comp[v] for v in reversed(r)] for r in rows]
        owner = owner + owner
    return rows, owner


def fold_rows(tri, owner, n):
    """wildcard_cases.fold_rows — the triangle over rows ``owner[a]`` -> the n x n sums of its blocks — by sorting the rows by
    owner and summing runs (thousands of rows: an integer matrix product over them takes a minute)."""
    owner = np.asarray(owner, dtype=np.int64)
    f = len(owner)
    sq = np.zeros((f, f), dtype=np.uint64)
    il = np.tril_indices(f)
    sq[il] = tri
    sq.T[il] = tri
    order = np.argsort(owner, kind="stable")
    sq = sq[order][:, order]
    assert np.array_equal(np.unique(owner), np.arange(n))   # every sequence has a row
    starts = np.searchsorted(owner[order], np.arange(n))
    out = np.add.reduceat(np.add.reduceat(sq, starts, axis=0), starts, axis=1)
    assert np.array_equal(out, out.T)
    return out[np.tril_indices(n)]


def layer_fold(port, seqs, profile, g, m, combos, comp=None, threads=THREADS, raw=None):
    """``port.raw_counts`` (or ``raw``, the same call of the compiled reference) on the level rows, folded."""
    from oracle import loader
    rows, owner = layer_rows(seqs, profile, g, comp)
    tok, off = loader.flatten(rows)
    tri = (raw or port.raw_counts)(tok, off, g, m, np.asarray(combos, dtype=np.int32), threads=threads)[0]
    return fold_rows(tri, owner, len(seqs))


def brute_variance(port, seqs, profile, g, m, order, n_train, delta=0.025, max_iters=-1, comp=None, wild=()):
    """Variance mode with one chain (t = 1) on ``brute``'s per-combination triangles, taken in ``order``: the reference's
    Welford chain (fastsk_kernel.cpp:108-143, 188-262) restated on the host — per iteration the running mean K_hat of the
    triangles, the mean over the train cells of delta * delta2 summed SEQUENTIALLY in triangle order, sd = sqrt(that /
    (iter - 1) / iter) (9999999 / 1 at the first), stop when delta / sd > 1.96 or at max_iters — then the normalisation.
    Returns (normalised triangle, stdevs)."""
    n = len(seqs)
    pairs = n * (n + 1) // 2
    train_pairs = int((n_train / 2.0) * (n_train + 1))
    k_hat = np.zeros(pairs, dtype=np.float64)
    sds = []
    for it, c in enumerate(order, start=1):
        ks = brute(port, seqs, profile, g, m, [int(c)], comp, wild)
        assert int(ks.max()) < 2 ** 32   # (the per-combination cells of this mode are 32-bit)
        ks = ks.astype(np.float64)
        d1 = ks - k_hat
        k_hat += d1 / it
        d2 = ks - k_hat
        avg = 0.0
        for v in (d1 * d2)[:train_pairs]:
            avg += float(v)
        avg /= train_pairs
        avg = 9999999.0 if it == 1 else avg / (it - 1)
        sd = float(np.sqrt(avg / it))
        sds.append(sd)
        if delta / sd > 1.96 or (max_iters != -1 and it >= max_iters):
            break
    return port.normalise(k_hat, n), np.array(sds)


def trimmed(seqs, g, plateau):
    """The sequences cut to the windows with d < plateau: what the 0/1 profile [1] * plateau + [0] keeps."""
    out = []
    for s in seqs:
        at = np.nonzero(distances(len(s), g) < plateau)[0]
        out.append([int(v) for v in s[at[0]:at[-1] + g]])
    return out


def center_profile_definition(plateau, halflife, levels=8, floor=0):
    """fastsk_amd.center_profile restated from its formula, entry by entry, and cut at the first final constant."""
    full = [max(floor, int(levels * 2.0 ** (-max(0, d - plateau) / halflife) + 0.5)) for d in range(20000)]
    final = full[-1]
    return full[:full.index(final) + 1]


# ---- 1. the definition case ---------------------------------------------------------------------------------------------------
DEFINITION_PROFILE = [3, 3, 2, 2, 2, 1, 0, 0, 1]


def definition_case():
    """13 ragged DNA sequences, g = 5, m = 2, all 10 combos; lengths g, g + 1 and g + 2 among them (both parities of L - g,
    the one-window sequence) and up to 40 (d reaches 17: the tail extended past the profile's last index). The profile has
    zeros inside, neighbours that differ (a distance off by one shows) and a non-zero last entry."""
    g, m = 5, 2
    rng = np.random.Generator(np.random.PCG64(4105))
    lens = [5, 6, 7, 40, 17, 23, 31, 12, 28, 36, 19, 25, 14]
    seqs = [rng.integers(1, 5, size=L).tolist() for L in lens]
    reach = max(int(distances(L, g).max()) for L in lens)
    assert reach > len(DEFINITION_PROFILE) - 1 and {(L - g) % 2 for L in lens} == {0, 1}
    assert len(_all_windows(seqs, g, DEFINITION_PROFILE, comp=DNA)[0]) <= 700
    return {"seqs": seqs, "g": g, "m": m, "profile": list(DEFINITION_PROFILE), "combos": np.arange(10, dtype=np.int32), "n_train": 9}


# ---- 2. one panel -----------------------------------------------------------------------------------------------------------------
def panel_case():
    """64 sequences of lengths g .. g + 40 at g = 12, m = 8 and w[d] = 1 + (7 d mod 13): every lane of the one panel has its
    centre elsewhere across the four-waves x four-windows trip and its tail, and no two neighbouring distances weigh alike."""
    g, m = 12, 8
    rng = np.random.Generator(np.random.PCG64(6412))
    seqs = [rng.integers(1, 5, size=g + (i * 7) % 41).tolist() for i in range(64)]
    assert {len(s) for s in seqs} >= {g, g + 40}
    profile = [1 + (7 * d) % 13 for d in range(21)]
    return {"seqs": seqs, "g": g, "m": m, "profile": profile, "combos": revcomp_cases.spread(comb(g, m), 4)}


# ---- 3. the dense staging regimes -----------------------------------------------------------------------------------------------
def monotone_profile(lmax, g):
    """Four levels, non-increasing, reaching 1 at about a third of the longest sequence's half (the last entry extends)."""
    half = max(8, (lmax - g) // 2)
    step = max(2, half // 6)
    return [4] * step + [3] * step + [2] * step + [1]


def regime_case(lmax, m, scale=1.0, rare=False):
    """Ragged DNA at g = 12 (revcomp_cases.dense_regime_case's shapes): about 200 sequences (70 scaled down), one of exactly
    lmax and one of exactly g symbols. ``rare``: a few of a fifth real symbol (key compaction with the marking pass)."""
    g = 12
    n = revcomp_cases.scaled(200, scale, 70)
    rng = np.random.Generator(np.random.PCG64(9000 * lmax + m))
    seqs = revcomp_cases.ragged(rng, n, g, lmax)
    if scale < 1.0:
        for i, s in enumerate(seqs):
            if i % 8 and g < len(s) < lmax:
                del s[int(rng.integers(g, 151)):]
    if rare:
        for i in (1, n // 2, n - 2):
            seqs[i][len(seqs[i]) // 2] = N_
    keys = (5 if rare else 4) ** (g - m)
    return {"seqs": seqs, "g": g, "m": m, "profile": monotone_profile(lmax, g),
            "combos": revcomp_cases.spread(comb(g, m), 5 if scale >= 1.0 else 2), "keys": keys}


def dense_plan(lmax, g, keys, table, strands, profile_len, zeros, dense_chunk=0):
    """fsk_engine_dense.hip:accumulate_dense restated for this mode: (windows a staging chunk, histogram sweeps, second
    strand resident, window-key cache). The profile takes its length rounded up to 4 bytes, plus 4 when no validity words
    (``zeros``: a weight of 0 is reached, so wildcard_cases.dense_plan's validity words are staged too) bring them."""
    w1, vq = lmax - g + 1, (keys + 3) // 4
    extra = 2 * keys if table else 0
    if zeros:
        extra += strands * ((min(w1, 1024) + 31) // 32) * 256 + 4
    extra += (profile_len + 3) // 4 * 4 + (0 if zeros else 4)
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


# ---- 4. counts that cross a plane by weight alone -------------------------------------------------------------------------------
def poly_a_case(windows, scale=1.0):
    """Poly-a of ``windows`` + g - 1 symbols among ordinary ragged DNA, g = 5, m = 2, w = [8]: the one k-mer of such a
    sequence counts 8 x windows — 80 at 10 windows (the hi plane, where unit counts would stay below 16), 320 at 40 (above
    255: the overflow flag, the batch recounted on the sparse dataflow, where unit counts would not even leave the lo and hi
    planes)."""
    g, m = 5, 2
    n = revcomp_cases.scaled(140, scale, 72)
    rng = np.random.Generator(np.random.PCG64(800 + windows))
    seqs = revcomp_cases.ragged(rng, n, g, 30)
    for at in (3, n // 2, n - 2):
        seqs[at] = [A] * (windows + g - 1)
    return {"seqs": seqs, "g": g, "m": m, "profile": [8], "combos": np.arange(10, dtype=np.int32), "top": 8 * windows}


# ---- 5. weighted sums past 65,535 -------------------------------------------------------------------------------------------------
def heavy_case(scale=1.0):
    """Three sequences of 300 windows under w = [255] among short ragged ones (g = 9, m = 4, two combos): 76,500 a sequence,
    so max_windows^2 > 2^32 — unpacked sparse entries, wide cells, no dense path — with 300 windows only. Two of the three
    are low-complexity (an (ac) repeat and poly-a with a random tail): multiplicities of tens of thousands."""
    g, m = 9, 4
    n = revcomp_cases.scaled(60, scale, 24)
    rng = np.random.Generator(np.random.PCG64(76500))
    seqs = revcomp_cases.ragged(rng, n, g, 40)
    L = 300 + g - 1
    seqs[2] = ([A, C_] * L)[:L]
    seqs[n // 2] = [A] * (L - 60) + rng.integers(1, 5, size=60).tolist()
    seqs[n - 1] = rng.integers(1, 5, size=L).tolist()
    return {"seqs": seqs, "g": g, "m": m, "profile": [255], "combos": np.array([0, 125], dtype=np.int32), "max_windows": 76500}


# ---- 6. sparse forms --------------------------------------------------------------------------------------------------------------
def low_complexity_case(scale=1.0):
    """revcomp_cases.low_complexity_case under a 4-level non-increasing profile."""
    case = dict(revcomp_cases.low_complexity_case(scale))
    case["profile"] = [4] * 6 + [3] * 6 + [2] * 8 + [1]
    return case


# ---- 7. with the other modes --------------------------------------------------------------------------------------------------------
def wildcard_case():
    """The definition case with n planted: at an end, in the middle (the heaviest windows go), and a sequence whose valid
    windows all lie at distances 6 and 7, where the profile is 0 — it has no window left."""
    case = definition_case()
    seqs = case["seqs"]
    wildcard_cases.plant(seqs[3], [0, 20])
    wildcard_cases.plant(seqs[5], [len(seqs[5]) - 1])
    wildcard_cases.plant(seqs[8], [14])
    case["wild"] = [N_]
    # 17 + g - 1 = 21 symbols, 17 windows, d = 8 .. 0 .. 8: n at positions 6 .. 14 leaves windows 0, 1 (d = 8, 7) and
    # 15, 16 (d = 7, 8); a second n at 0 and 20 removes the two of d = 8, whose weight is 1
    dead = np.random.Generator(np.random.PCG64(2)).integers(1, 5, size=21).tolist()
    wildcard_cases.plant(dead, list(range(6, 15)) + [0, 20])
    left = weighted_windows(dead, case["g"], [1], {N_})[0]
    assert len(left) == 2 and len(weighted_windows(dead, case["g"], case["profile"], {N_})[0]) == 0
    case["dead"] = dead
    return case


def mismatch_case():
    """20 ragged DNA sequences of 6..34 tokens, g = 6, m = 3, the definition profile."""
    seqs = mismatch_cases.ragged(20, 6, 34, seed=414)
    return {"seqs": seqs, "g": 6, "m": 3, "profile": list(DEFINITION_PROFILE)}
