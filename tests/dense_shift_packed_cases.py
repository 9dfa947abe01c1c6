"""Inputs and the numpy statement of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_keymajor,
k_dense_shift_packed; tuning dense_shift_packed), shared by tests/test_emu_dense_shift_packed.py and
tests/test_gpu_dense_shift_packed.py. Nothing here touches an engine. tests/dense_shift_cases.py has the identity and the plan.

The packed kernel reads a key's 4-bit counts of 8 sequences in one dword and forms the weighted sums without a multiply:

    D'    = (lo(sigma) | 16) - lo(delta)            per term and cell, in [1, 31]: a byte, no borrow
    R_r   = sum_{u <= r} D'_u                        inside a chain, in [r + 1, 31 (r + 1)]: a byte for 8 steps
    acc  += R_r (row term) + R_r (column term)       sum_r R_r = sum_u (t1 - u) D_u + 16 x the chain's weights
    acc  += 16 w (hi(sigma) - hi(delta))             the counts above 15, at the step's weight w
    K    += acc - 32 x the sum of all weights

``packed_sum`` evaluates exactly that (uint32 sums, chains cut at nine members) and asserts the byte ranges on the way; the tests
hold it against ``dense_shift_cases.identity_sum`` before any engine is asked."""
import numpy as np

import dense_shift_cases as cases

A, C, G_, T = 1, 2, 3, 4          # the four letters as tokens (key digit = token - 1)
MAX_CHAIN = 9                     # members of a chain at most when the packed kernel runs
TUNING = dict(cases.TUNING)
PACKED, PARENT = {"dense_shift_packed": 0}, {"dense_shift_packed": -1}
NO_ROOM = {"dense_shift_plane_kb": 1}   # the key-major planes may take 1 KiB: they never fit


def cut(chains, max_chain=MAX_CHAIN):
    out = []
    for ch in chains:
        for i in range(0, len(ch), max_chain):
            out.append(ch[i:i + max_chain])
    return out


def counts(seqs, pos, g):
    """[sequence][key]: the count vectors under kept positions ``pos`` at window length g (four letters, k = len(pos))."""
    out = np.zeros((len(seqs), cases.SIGMA ** len(pos)), dtype=np.int64)
    for i, x in enumerate(seqs):
        a = np.asarray(x, dtype=np.int64) - 1
        nw = len(a) - g + 1
        key = np.zeros(nw, dtype=np.int64)
        for p in pos:
            key = key * cases.SIGMA + a[p:p + nw]
        out[i] = np.bincount(key, minlength=out.shape[1])
    return out


def edge_keys(seqs, lower, upper, g):
    def key(x, start, pos):
        k = 0
        for p in pos:
            k = k * cases.SIGMA + int(x[start + p]) - 1
        return k
    return (np.array([key(x, 0, lower) for x in seqs]), np.array([key(x, len(x) - g, upper) for x in seqs]))


def direct_sum(seqs, positions, g):
    total = np.zeros((len(seqs), len(seqs)), dtype=np.int64)
    for pos in positions:
        c = counts(seqs, pos, g)
        total += c @ c.T
    return total


def packed_sum(seqs, positions, g=cases.G, max_chain=MAX_CHAIN):
    """The packed kernel's arithmetic (every sequence has a window). Returns (the sum over ``positions``, what was seen: the
    largest stored R of either term, the smallest stored R at the eighth step of a chain per term, the largest count, the steps
    with a count above 15 on their upper or lower side)."""
    n = len(seqs)
    total = np.zeros((n, n), dtype=np.int64)
    acc = np.zeros((n, n), dtype=np.int64)
    wsum = 0
    seen = {"r_max": {"row": 0, "col": 0}, "r_min_at_8": {"row": None, "col": None}, "top": 0, "flagged_steps": []}
    for chain in cut(cases.chains(positions), max_chain):
        length = len(chain)
        assert length <= max_chain
        c_lo = counts(seqs, positions[chain[0]], g)
        total += length * (c_lo @ c_lo.T)
        r_row = np.zeros((n, n), dtype=np.int64)   # the prefix sums restart at a chain base
        r_col = np.zeros((n, n), dtype=np.int64)
        for u in range(length - 1):
            lower, upper = positions[chain[u]], positions[chain[u + 1]]
            delta, sigma = edge_keys(seqs, lower, upper, g)
            c_up = counts(seqs, upper, g)
            seen["top"] = max(seen["top"], int(c_lo.max()), int(c_up.max()))
            if c_lo.max() > 15 or c_up.max() > 15:
                seen["flagged_steps"].append((chain[u], chain[u + 1]))
            d_row = ((c_up & 15)[:, sigma] | 16) - (c_up & 15)[:, delta]          # [i, j]: row i's counts at column j's keys
            d_col = (((c_lo & 15)[:, sigma] | 16) - (c_lo & 15)[:, delta]).T      # [i, j]: column j's counts at row i's keys
            for d in (d_row, d_col):
                assert d.min() >= 1 and d.max() <= 31
            r_row += d_row
            r_col += d_col
            for name, r in (("row", r_row), ("col", r_col)):
                assert u + 1 <= r.min() and r.max() <= 31 * (u + 1) <= 255, "a stored prefix sum leaves its byte"
                seen["r_max"][name] = max(seen["r_max"][name], int(r.max()))
                if u == 7:
                    low = seen["r_min_at_8"][name]
                    seen["r_min_at_8"][name] = int(r.min()) if low is None else min(low, int(r.min()))
            w = length - 1 - u
            wsum += w
            hi = ((c_up >> 4)[:, sigma] - (c_up >> 4)[:, delta]) + ((c_lo >> 4)[:, sigma] - (c_lo >> 4)[:, delta]).T
            acc = (acc + r_row + r_col + 16 * w * hi) & 0xffffffff
            c_lo = c_up
    assert (2 * max(len(x) - g + 1 for x in seqs) + 32) * wsum < 2 ** 31   # the host's bound
    v = (acc - 32 * wsum) & 0xffffffff
    total += np.where(v >= 2 ** 31, v - 2 ** 32, v)
    return total, seen


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def span4(positions):
    """The class of nine shifts, (0, 1, 2, 3) + t: one chain of eight steps."""
    ids = [c for c, pos in enumerate(positions) if tuple(p - pos[0] for p in pos) == (0, 1, 2, 3)]
    assert len(ids) == 9
    return np.array(ids, dtype=np.int32)


# The byte range at its ends (L = 40, 29 windows). RUN holds A^18 at 8 .. 25: its 15 AAAA starts lie inside the window range of
# every shift, so AAAA counts 15 under all nine, and it holds no G. PLUS begins G^11 and ends A^12: its eight delta keys are GGGG,
# its eight sigma keys AAAA, so against RUN a term is + 15 at every step (stored R: 31, 62 .. 248); MINUS is the mirror image
# (- 15 at every step: stored R stays r + 1). The row term meets them where RUN is the row, the column term where RUN is the column.
RUN = [C] * 8 + [A] * 18 + [C, T] * 7
PLUS = [G_] * 11 + [T] * 17 + [A] * 12
MINUS = [A] * 11 + [T] * 17 + [G_] * 12
EXTREMES_AT = {10: RUN, 100: RUN, 128: RUN, 3: PLUS, 90: PLUS, 129: PLUS, 66: MINUS, 120: MINUS}
# (row, column): tile (1, 0): (128, 3) row +, (128, 66) row -, (129, 10) and (129, 100) column +; tile (0, 0): (100, 3) row +,
# (100, 66) row -, (90, 10) column +, (120, 10) and (120, 100) column -; tile (1, 1): (129, 128) column +
EXTREME_CELLS = {"row+": [(128, 3), (100, 3)], "row-": [(128, 66), (100, 66)], "col+": [(129, 10), (90, 10), (129, 128)], "col-": [(120, 10), (120, 100)]}


def extremes(n=cases.N, seed=21):
    seqs = cases.uniform(n, 40, seed)
    for i, x in EXTREMES_AT.items():
        assert len(x) == 40
        seqs[i] = list(x)
    return seqs


# A count that crosses 15 in the middle of the nine-shift class only (L = 60, 49 windows): A^12 at 4 .. 15 keeps its nine AAAA
# starts up to shift 4 and loses one a shift from there; A^12 at 44 .. 55 gains one a shift up to shift 4 and keeps nine from
# there. AAAA counts 14 15 16 17 18 17 16 15 14 under shifts 0 .. 8: the steps 1 -> 2 .. 6 -> 7 run the hi pass inside one chain.
CROSSING = [T] * 4 + [A] * 12 + [C, G_, T, C] * 7 + [A] * 12 + [T] * 4
CROSSING_COUNTS = [14, 15, 16, 17, 18, 17, 16, 15, 14]
CROSSING_AT = (70, 129)   # a column of tile (1, 0) and of tile (0, 0) ... and a row of tiles (1, 0) and (1, 1)


def crossing(n=cases.N, seed=22):
    seqs = cases.uniform(n, 40, seed)
    assert len(CROSSING) == 60
    for i in CROSSING_AT:
        seqs[i] = list(CROSSING)
    return seqs


# The chain cut: g = 14, m = 10 (k = 4: 256 keys, 1001 combinations) has a class of eleven shifts, (0, 1, 2, 3) + 0 .. 10.
CUT_G, CUT_M = 14, 10


def cut_list(port):
    """The eleven-shift class, a class of ten and two lone combinations, in call order: ids and their kept positions."""
    n = 1001
    pos = [tuple(int(p) for p in port.combo_positions(CUT_G, cases.K, c)) for c in range(n)]
    eleven = [c for c in range(n) if tuple(p - pos[c][0] for p in pos[c]) == (0, 1, 2, 3)]
    ten = [c for c in range(n) if tuple(p - pos[c][0] for p in pos[c]) == (0, 1, 2, 4)]
    assert len(eleven) == 11 and len(ten) == 10
    ids = eleven + ten + [500, 900]
    return np.array(ids, dtype=np.int32), [pos[c] for c in ids]


def cut_seqs(n=cases.N, seed=23):
    """L = 40 and, in every tile row and the last tile's rows, L = 14 (one window), 15 and 24 (eleven windows: as many as shifts)."""
    seqs = cases.uniform(n, 40, seed)
    for base in (0, 61, 126):
        for i, L in enumerate((14, 15, 24)):
            seqs[base + i] = seqs[base + i][:L]
    seqs[n - 1] = seqs[n - 1][:14]
    return seqs
