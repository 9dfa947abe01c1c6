"""The lane layout of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_shift_packed) at every place where it
decides something: the nibble position and parity, the lane group, the side. tests/dense_shift_lanes_cases.py holds the inputs
and the numpy preconditions; the check functions here state the contract and tests/test_gpu_dense_shift_lanes.py runs them on
the device. ``make(g, m, **kw)`` creates an engine; no expected value comes from one: counts are compared cell for cell, over
the whole triangle, with the CPU oracle (``port.raw_counts``), after numpy has shown that the inputs reach what they are meant
to reach.

The emulator runs the class of nine shifts and the 23 combinations of the chain cut; all 495 combinations run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
import dense_shift_lanes_cases as lanes  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift import differ, once, positions  # noqa: E402

EVERY = set(range(cases.TILE))


def oracle(port, name, seqs_of, ids, g=cases.G, m=cases.M):
    """(sequences, tokens, offsets, the oracle's counts over ``ids``), computed once and read-only."""
    from oracle import loader

    def build():
        seqs = seqs_of()
        tok, off = loader.flatten(seqs)
        want = port.raw_counts(tok, off, g, m, np.asarray(ids, dtype=np.int32), threads=4)[0]
        for a in (tok, off, want):
            a.setflags(write=False)
        return seqs, tok, off, want
    return once(("lanes", name, g, tuple(int(c) for c in ids)), build)


def run(make, tok, off, n, ids, plist, g=cases.G, m=cases.M):
    """One call over ``ids`` (kept positions ``plist``) on the packed kernel after reset_counts -> counts. The launches are
    stated from the plan alone, as in tests/test_emu_dense_shift_packed.py: the count, the edge keys, one base launch per
    distinct chain length, ONE launch of corrections, and the two key-major planes and the key offsets."""
    e = make(g, m, path=1, tuning=dict(packed.TUNING, **packed.PACKED))
    e.load_sequences(tok, off, n, 0)
    e.reset_counts()
    before = e.stats()
    e.accumulate(np.asarray(ids, dtype=np.int32))
    e.finalize()
    st = e.stats()
    got = e.get_counts()
    e.close()
    assert st["path_used"] == 1 and st["n_tile_launches"] - before["n_tile_launches"] == 1
    want_launches = 1 + 1 + len({len(c) for c in packed.cut(cases.chains(plist))}) + 1 + 3
    assert st["launches"] - before["launches"] == want_launches, (st["launches"] - before["launches"], want_launches)
    return got


def check_every_position(make, port, ids):
    """Sequence i is RUN, PLUS or MINUS by i mod 3 (N = 386): the stored prefix sum reaches 248 and stays at r + 1, in the row
    term and in the column term, at every in-tile row position and every in-tile column position."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "everywhere", lanes.everywhere, ids)
    span = [pos[c] for c in packed.span4(pos)]

    def statement():
        total, seen = packed.packed_sum(seqs, span)
        assert np.array_equal(total, packed.direct_sum(seqs, span, cases.G))
        return seen, lanes.byte_end_positions(seqs, span)
    seen, ends = once("everywhere statement", statement)
    assert seen["r_max"] == {"row": 248, "col": 248} and seen["r_min_at_8"] == {"row": 8, "col": 8} and seen["top"] == 15
    for name in ("row+", "row-", "col+", "col-"):
        assert ends[name] == (EVERY, EVERY), name
    got = run(make, tok, off, len(seqs), ids, [pos[c] for c in ids])
    assert not differ(got, want), differ(got, want)


def check_hi_positions(make, port, ids):
    """CROSSING at an even and an odd nibble of either tile row (N = 258): the hi pass adds a non-zero difference through the
    row term and through the column term, from an even and from an odd nibble, in a diagonal and in an off-diagonal tile."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "hi", lanes.hi_seqs, ids)
    span = [pos[c] for c in packed.span4(pos)]
    assert [int(packed.counts([packed.CROSSING], p, cases.G)[0][0]) for p in span] == packed.CROSSING_COUNTS

    def statement():
        total, seen = packed.packed_sum(seqs, span)
        assert np.array_equal(total, packed.direct_sum(seqs, span, cases.G))
        return seen, lanes.hi_cells(seqs, span)
    seen, cells = once("hi statement", statement)
    assert seen["top"] == 18 and seen["flagged_steps"] == [(u, u + 1) for u in range(1, 7)]
    assert cells == lanes.HI_CELLS
    got = run(make, tok, off, len(seqs), ids, [pos[c] for c in ids])
    assert not differ(got, want), differ(got, want)


def check_cut_full_row(make, port):
    """g = 14, m = 10, N = 258: ragged lengths (one window .. eleven) in the first tile row and at the end, the second tile row
    full, the eleven-shift class cut into nine and two."""
    ids, plist = once("cut list", lambda: packed.cut_list(port))
    seqs, tok, off, want = oracle(port, "cut", lanes.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    assert sorted(len(x) for x in seqs)[:4] == [14, 14, 14, 14] and all(len(x) == 40 for x in seqs[129:256])
    assert sorted(len(c) for c in packed.cut(cases.chains(plist))) == [1, 1, 1, 2, 9, 9]

    def statement():
        some = seqs[:4] + seqs[60:65] + seqs[124:132] + seqs[-2:]
        total, seen = packed.packed_sum(some, plist, packed.CUT_G)
        assert np.array_equal(total, packed.direct_sum(some, plist, packed.CUT_G))
        return seen
    assert once("lanes cut statement", statement)["top"] <= 15
    got = run(make, tok, off, len(seqs), ids, plist, packed.CUT_G, packed.CUT_M)
    assert not differ(got, want), differ(got, want)


# ---- the emulator runs ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


def test_emu_byte_ends_at_every_position(make_emu, port):
    check_every_position(make_emu, port, packed.span4(positions(port)))


def test_emu_hi_pass_at_both_parities(make_emu, port):
    check_hi_positions(make_emu, port, packed.span4(positions(port)))


def test_emu_chain_cut_with_a_full_tile_row(make_emu, port):
    check_cut_full_row(make_emu, port)
