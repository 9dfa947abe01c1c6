"""Inputs and numpy preconditions for the lane layout of the packed shift corrections (fsk_kernels_dense_shift.h:
k_dense_shift_packed), shared by tests/test_emu_dense_shift_lanes.py and tests/test_gpu_dense_shift_lanes.py. Nothing here
touches an engine. tests/dense_shift_packed_cases.py has the arithmetic.

What a lane layout can get wrong, it gets wrong per in-tile position: a key-major dword holds the 8 sequences of a lane group as
nibbles, a lane owns the rows of a row group and columns of a column group, and which half of the tile, which nibble parity and
which byte a cell's sum comes from all follow from the cell's position inside the 128 x 128 tile. The cases of
tests/dense_shift_packed_cases.py touch a dozen cells. The cases here put the byte range's ends at EVERY in-tile position, as a
row and as a column, and the counts above 15 at both parities on both sides, in a diagonal and in an off-diagonal tile. They hold
for any assignment of cells to lanes: they were written for a form of 512 threads with 8 x 4 cells a lane, which was measured
and not kept (docs/history.md), and they pin the 8 x 8 form as well."""
import numpy as np

import dense_shift_cases as cases
import dense_shift_packed_cases as packed

TILE = cases.TILE


def nibble(p):
    """The nibble (0..7) of a key-major dword at which in-tile position p (0..127) sits: the inverse of the kernels'
    tile_index(t, n) = (n >> 2) * 64 + t + 16 * (n & 3)."""
    return (p >> 6) * 4 + ((p & 63) >> 4)


def group(p):
    """The lane group t (0..15) of in-tile position p."""
    return p & 15


assert sorted((nibble(p), group(p)) for p in range(TILE)) == [(n, t) for n in range(8) for t in range(16)]
assert all((nibble(p) >> 2) * 64 + group(p) + 16 * (nibble(p) & 3) == p for p in range(TILE))


# ---- every position at the byte ends ------------------------------------------------------------------------------------------
EVERYWHERE_N = 386   # three full tile rows and a fourth with two real rows
TYPES = (packed.RUN, packed.PLUS, packed.MINUS)   # sequence i is TYPES[i mod 3]


def everywhere(n=EVERYWHERE_N):
    """Since 128 mod 3 = 2, in-tile position p holds type (p + 2 t) mod 3 in tile row t: each of the three in some full tile row."""
    for p in range(TILE):
        assert {(p + TILE * t) % 3 for t in range(3)} == {0, 1, 2}
    return [list(TYPES[i % 3]) for i in range(n)]


def byte_end_positions(seqs, span, g=cases.G):
    """The stored prefix sums of the eighth step of the nine-shift chain ``span``, in numpy: for each term and each end of the
    byte range (R = 248, a term of + 15 at every step, and R = 8, - 15 at every step) the in-tile row positions and the in-tile
    column positions of the cells j <= i at which that end is stored. -> {"row+": (rows, columns), "row-": ..., "col+": ..., "col-": ...}"""
    n = len(seqs)
    assert len(span) == 9
    r_row = np.zeros((n, n), dtype=np.int64)
    r_col = np.zeros((n, n), dtype=np.int64)
    c_lo = packed.counts(seqs, span[0], g)
    for u in range(8):
        delta, sigma = packed.edge_keys(seqs, span[u], span[u + 1], g)
        c_up = packed.counts(seqs, span[u + 1], g)
        assert c_lo.max() <= 15 and c_up.max() <= 15
        r_row += (c_up[:, sigma] | 16) - c_up[:, delta]
        r_col += ((c_lo[:, sigma] | 16) - c_lo[:, delta]).T
        c_lo = c_up
    lower = np.tril(np.ones((n, n), dtype=bool))
    out = {}
    for name, r, end in (("row+", r_row, 248), ("row-", r_row, 8), ("col+", r_col, 248), ("col-", r_col, 8)):
        assert r.min() >= 8 and r.max() <= 248
        i, j = np.nonzero((r == end) & lower)
        out[name] = (set((i % TILE).tolist()), set((j % TILE).tolist()))
    return out


# ---- counts above 15 at both parities, both sides, both kinds of tile ------------------------------------------------------------
HI_N = 258   # two full tile rows and a third with two real rows
# CROSSING (AAAA counts 14 .. 18 .. 14 under the nine shifts, and its own edge keys are AAAA at some steps) at an even and an
# odd nibble of the first tile row and of the second: as a column and as a row, in diagonal and off-diagonal tiles
HI_AT = (5, 21, 128 + 70, 128 + 90)
assert [nibble(x % TILE) for x in HI_AT] == [0, 1, 4, 5]
# partners whose sigma (PLUS) or delta (MINUS) key is AAAA at every step: the hi difference against CROSSING is never zero
HI_PLUS_AT = (2, 40, 100, 127, 128, 150, 200, 256)
HI_MINUS_AT = (9, 33, 77, 129, 180, 255, 257)


def hi_seqs(n=HI_N, seed=31):
    seqs = cases.uniform(n, 40, seed)
    for x in HI_AT:
        seqs[x] = list(packed.CROSSING)
    for x in HI_PLUS_AT:
        seqs[x] = list(packed.PLUS)
    for x in HI_MINUS_AT:
        seqs[x] = list(packed.MINUS)
    return seqs


def hi_cells(seqs, span, g=cases.G):
    """Where the hi pass has something to add under the nine-shift chain ``span``: the set of (term, parity of the nibble the
    term reads for the cell, "diagonal" or "off-diagonal" tile) over the cells j <= i with a non-zero hi difference. The row term
    reads the ROW's nibble of A[key of the column], the column term the COLUMN's nibble of B[key of the row]."""
    n = len(seqs)
    out = set()
    c_lo = packed.counts(seqs, span[0], g)
    for u in range(8):
        delta, sigma = packed.edge_keys(seqs, span[u], span[u + 1], g)
        c_up = packed.counts(seqs, span[u + 1], g)
        hi_row = (c_up >> 4)[:, sigma] - (c_up >> 4)[:, delta]
        hi_col = ((c_lo >> 4)[:, sigma] - (c_lo >> 4)[:, delta]).T
        for term, hi in (("row", hi_row), ("col", hi_col)):
            for i, j in zip(*np.nonzero(np.tril(hi))):
                reads = nibble((i if term == "row" else j) % TILE)
                out.add((term, "odd" if reads & 1 else "even", "diagonal" if i // TILE == j // TILE else "off-diagonal"))
        c_lo = c_up
    return out


HI_CELLS = {(t, p, k) for t in ("row", "col") for p in ("even", "odd") for k in ("diagonal", "off-diagonal")}

# ---- ragged lengths and the chain cut with a full second tile row -------------------------------------------------------------------
CUT_N = 258


def cut_seqs():
    return packed.cut_seqs(CUT_N, seed=33)
