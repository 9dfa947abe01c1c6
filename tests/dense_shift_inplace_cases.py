"""Inputs and numpy preconditions for the in-place form of the packed shift corrections (fsk_kernels_dense_shift.h:
k_dense_shift_packed<true>; tuning dense_shift_inplace), shared by tests/test_emu_dense_shift_inplace.py and
tests/test_gpu_dense_shift_inplace.py. Nothing here touches an engine. tests/dense_shift_packed_cases.py has the arithmetic,
tests/dense_shift_lanes_cases.py the positions inside a tile.

The in-place form stages a chain's key-major planes once and makes the planes of every further step in LDS:

    A (row side):     c_up(s+1) = c_up(s) + e(sigma) - e(delta)   with the keys of step s + 1
    B (column side):  c_lo(s+1) = c_lo(s) + e(sigma) - e(delta)   with the keys of step s

one 4-bit increment and one decrement a sequence, at nibble ``lanes.nibble(p)`` of dword ``lanes.group(p)`` for in-tile
position p. What it can get wrong: the nibble or the dword of a position, the step whose keys a side takes, a sequence whose
two keys are equal (nothing moves; a padded row's zero plane must stay zero), a count that would leave its nibble (a step that
meets one in the tile, and the step behind it, must be staged), and the hand-over between chains. ``chain_facts`` states in numpy what an input meets."""
import numpy as np

import dense_shift_cases as cases
import dense_shift_lanes_cases as lanes
import dense_shift_packed_cases as packed

TILE = cases.TILE
TUNING = {"tile_splits": 1, "dense_shift": 1, "dense_shift_packed": 0}
FORMS = (1, 0)   # dense_shift_inplace: the in-place form, and every step staged


def chain_facts(seqs, span, g=cases.G):
    """The chain of consecutive shifts ``span`` (kept positions), step by step, every sequence with a window. Asserts the
    identity the updates rest on and returns what they meet: the (sequence, step) pairs whose keys are equal ("stay"), whose
    delta count goes 1 -> 0 ("down_to_0"), whose sigma count goes 0 -> 1 ("up_from_0"), the largest count of every tile side
    over all the slots the chain visits ("top": tile side -> count), and the largest count reached by an update ("top_moved")."""
    n = len(seqs)
    rows = np.arange(n)
    sides = (n + TILE - 1) // TILE
    facts = {"stay": set(), "down_to_0": set(), "up_from_0": set(), "top": {t: 0 for t in range(sides)}, "top_moved": 0}

    def tops(c):
        for t in range(sides):
            facts["top"][t] = max(facts["top"][t], int(c[t * TILE:(t + 1) * TILE].max()))
    c = packed.counts(seqs, span[0], g)
    tops(c)
    for u in range(len(span) - 1):
        delta, sigma = packed.edge_keys(seqs, span[u], span[u + 1], g)
        c_up = c.copy()
        c_up[rows, delta] -= 1
        c_up[rows, sigma] += 1
        assert np.array_equal(c_up, packed.counts(seqs, span[u + 1], g)), "c_{t+1} = c_t + e(sigma) - e(delta)"
        moved = delta != sigma
        facts["stay"] |= {(int(i), u) for i in np.flatnonzero(~moved)}
        facts["down_to_0"] |= {(int(i), u) for i in np.flatnonzero(moved & (c[rows, delta] == 1))}
        facts["up_from_0"] |= {(int(i), u) for i in np.flatnonzero(moved & (c[rows, sigma] == 0))}
        if moved.any():
            facts["top_moved"] = max(facts["top_moved"], int(c_up[rows[moved], sigma[moved]].max()))
        tops(c_up)
        c = c_up
    return facts


# ---- 1. every nibble position -------------------------------------------------------------------------------------------------
NIBBLES_N = 258   # two full tile rows and a third with two real rows


def same_row(n=NIBBLES_N, seed=41):
    """The 128 sequences of tile row 1 are one and the same: in every step all 8 nibbles of all 16 dwords of a key take the same
    update, as rows of the diagonal tile (1, 1) and of tile (1, 0) and as columns of tiles (1, 1) and (2, 1). The rest is uniform."""
    seqs = cases.uniform(n, 40, seed)
    for i in range(TILE, 2 * TILE):
        seqs[i] = list(seqs[TILE])
    assert sorted((lanes.nibble(i % TILE), lanes.group(i % TILE)) for i in range(TILE, 2 * TILE)) == [(e, t) for e in range(8) for t in range(16)]
    return seqs


# ---- 2. steps that move nothing next to steps that empty and open a key, and the nibble's top --------------------------------------
# STAY: the first window of shift t and the last window of shift t + 1 show the same 4-mer of (0, 1, 2, 3) at t = 0, 5 and 6
# (x[t .. t + 3] = x[29 + t .. 32 + t]), and different ones at the other steps, each of which empties one key and opens another.
STAY = [1, 2, 3, 4, 2, 2, 4, 1, 3, 3] + [4, 1] * 9 + [3] + [1, 2, 3, 4, 3, 2, 4, 1, 3, 3, 2]
STAY_STEPS = [0, 5, 6]
assert [t for t in range(8) if STAY[t:t + 4] == STAY[29 + t:33 + t]] == STAY_STEPS
STAY_AT = (7, 66, 128 + 21, 256 + 90, 385)   # (i mod 3 = 1, 0, 2, 1, 1: every type gives up a place; every tile row holds one)
MOVES_N = lanes.EVERYWHERE_N


def moves_and_stays(n=MOVES_N):
    """RUN / PLUS / MINUS by i mod 3 (tests/dense_shift_lanes_cases.py: a count of 15 under all nine shifts, counts that run
    down to 0 and up from 1) with STAY in every tile row."""
    assert len(STAY) == 40
    seqs = lanes.everywhere(n)
    for i in STAY_AT:
        seqs[i] = list(STAY)
    return seqs


# ---- 3. a count that leaves its nibble, and one that only reaches its top -------------------------------------------------------------
# PEAK15: packed.CROSSING with nine A instead of twelve in front: AAAA counts 11 .. 15 .. 11 under the nine shifts and never 16.
PEAK15 = [4] * 4 + [1] * 9 + [4] * 3 + [2, 3, 4, 2] * 7 + [1] * 12 + [4] * 4
PEAK15_COUNTS = [11, 12, 13, 14, 15, 14, 13, 12, 11]
CROSSING_N = 386   # four tile rows: the planted sequences sit in tile rows 0 and 1, tile rows 2 and 3 hold none
CROSSING_AT = lanes.HI_AT   # an even and an odd nibble of the column side and of the row side of tile (1, 0)


def crossing(which, n=CROSSING_N, seed=42):
    """``which`` = packed.CROSSING (the steps of tile rows 0 and 1 that meet the count above 15 must be staged, with the hi
    pass) or PEAK15 (every step stays in place), with partners whose sigma or delta key is AAAA at every step."""
    assert len(which) == 60 and [lanes.nibble(x % TILE) for x in CROSSING_AT] == [0, 1, 4, 5]
    seqs = cases.uniform(n, 40, seed)
    for x in CROSSING_AT:
        seqs[x] = list(which)
    for x in lanes.HI_PLUS_AT:
        seqs[x] = list(packed.PLUS)
    for x in lanes.HI_MINUS_AT:
        seqs[x] = list(packed.MINUS)
    return seqs


# ---- 4. one window, ragged lengths, padded positions ----------------------------------------------------------------------------------
RAGGED_N = 258


def ragged(n=RAGGED_N, seed=43):
    """Every length of cases.RAGGED (g = 12: one window .. nine, plenty) in every tile row, at both ends of a tile side and
    across its panels' border, and one window and two in the last tile's two real rows, which 126 padded positions follow."""
    seqs = cases.uniform(n, 40, seed)
    at = {}
    for base in (0, 61, 122, 128, 189, 250):
        for i, L in enumerate(cases.RAGGED):
            at[base + i] = L
    at[n - 2], at[n - 1] = 13, 12
    for i, L in at.items():
        seqs[i] = seqs[i][:L]
    assert n % TILE == 2 and sum(len(x) == cases.G for x in seqs) == 7
    return seqs
