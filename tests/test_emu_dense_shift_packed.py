"""The packed shift corrections (tuning dense_shift_packed; fsk_kernels_dense_shift.h: k_dense_keymajor, k_dense_edge_offs,
k_dense_shift_packed) at the edges their arithmetic has. tests/dense_shift_packed_cases.py holds the inputs and the numpy
statement of the arithmetic; the check functions here state the contract and tests/test_gpu_dense_shift_packed.py runs them on
the device. ``make(g, m, **kw)`` creates an engine; no expected value comes from one.

Every case is N = 130 (three tiles, the last with two real rows), four letters, tile_splits=1 and dense_shift=1. Counts are
compared bit for bit with the CPU oracle (``port.raw_counts``), and the numpy statement is held against
``dense_shift_cases.identity_sum`` (g = 14: against the direct sum) before any engine is asked.

The emulator runs the class of nine shifts, the small list of tests/test_emu_dense_shift.py and the 23 combinations of the chain
cut; all 495 combinations run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift import differ, once, positions  # noqa: E402


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
    return once(("packed", name, g, tuple(int(c) for c in ids)), build)


def run(make, tok, off, ids, plist, tuning, g=cases.G, m=cases.M):
    """One call over ``ids`` (kept positions ``plist``) after reset_counts -> (counts, dense_macs of the call). Which
    corrections ran shows in the launch count, stated here from the plan alone: one count launch, one of the edge keys, one
    base launch per distinct chain length (chains cut at nine members unless dense_shift_packed = -1), the corrections — and,
    where the packed kernel runs, the key-major lo plane, the key-major hi plane and the key offsets: three more."""
    e = make(g, m, path=1, tuning=dict(packed.TUNING, **tuning))
    e.load_sequences(tok, off, cases.N, 0)
    e.reset_counts()
    before = e.stats()
    e.accumulate(np.asarray(ids, dtype=np.int32))
    e.finalize()
    st = e.stats()
    got = e.get_counts()
    e.close()
    assert st["path_used"] == 1 and st["n_tile_launches"] - before["n_tile_launches"] == 1
    asked = tuning.get("dense_shift_packed", 0) == 0
    chains = packed.cut(cases.chains(plist)) if asked else cases.chains(plist)
    ran_packed = asked and "dense_shift_plane_kb" not in tuning
    want_launches = 1 + 1 + len({len(c) for c in chains}) + 1 + (3 if ran_packed else 0)
    assert st["launches"] - before["launches"] == want_launches, (st["launches"] - before["launches"], want_launches)
    return got, st["dense_macs"] - before["dense_macs"]


def numpy_statement(seqs, plist, key, g=cases.G):
    """packed_sum == the identity (g = 12) or the direct sum, once per case; returns what packed_sum saw."""
    def build():
        total, seen = packed.packed_sum(seqs, plist, g)
        want = cases.identity_sum(seqs, plist) if g == cases.G else packed.direct_sum(seqs, plist, g)
        assert np.array_equal(total, want)
        return seen
    return once(("statement", key), build)


def check_extremes(make, port, ids, key):
    """A term of + 15 at every one of eight steps (stored R reaches 248) and of - 15 (stored R stays r + 1), in the row term
    and the column term, in tile (1, 0) and in diagonal tiles; no count above 15, so only the lo planes are read."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "extremes", packed.extremes, ids)
    span = [pos[c] for c in packed.span4(pos)]
    seen = numpy_statement(seqs, span, "extremes")
    assert seen["r_max"] == {"row": 248, "col": 248} and seen["r_min_at_8"] == {"row": 8, "col": 8}
    # no count of any of the 130 sequences under any of the 495 combinations exceeds 15: the lo planes alone are what runs
    assert len(pos) == cases.N_COMBOS and len(seqs) == cases.N
    assert once("extremes top", lambda: max(int(packed.counts(seqs, p, cases.G).max()) for p in pos)) == 15
    assert once("extremes high", lambda: cases.high_panels(seqs, span)) == (set(), 15)
    c_run = packed.counts([packed.RUN], span[3], cases.G)[0]
    assert c_run[0] == 15 and c_run[170] == 0   # AAAA and GGGG
    for name, cells in packed.EXTREME_CELLS.items():   # the cells the comment in the case module names are what it says
        for i, j in cells:
            d, s = packed.edge_keys([seqs[j if name[:3] == "row" else i]], span[2], span[3], cases.G)
            assert (int(d[0]), int(s[0])) == ((170, 0) if name[3] == "+" else (0, 170)), (name, i, j)
            assert seqs[i if name[:3] == "row" else j] == packed.RUN
    got, _ = run(make, tok, off, ids, [pos[c] for c in ids], packed.PACKED)
    assert not differ(got, want), differ(got, want)


def check_both_kernels(make, port, name, ids):
    """dense_shift_packed = -1 and 0: equal triangles (the oracle's) and, no chain being cut at g = 12, equal dense_macs."""
    pos = positions(port)
    seqs_of = {"uniform": cases.uniform, "ragged": cases.ragged}[name]
    seqs, tok, off, want = oracle(port, name, seqs_of, ids)
    bases = len(cases.chains([pos[c] for c in ids]))
    assert len(packed.cut(cases.chains([pos[c] for c in ids]))) == bases
    got_new, macs_new = run(make, tok, off, ids, [pos[c] for c in ids], packed.PACKED)
    got_old, macs_old = run(make, tok, off, ids, [pos[c] for c in ids], packed.PARENT)
    assert not differ(got_new, want), differ(got_new, want)
    assert np.array_equal(got_old, got_new)
    assert macs_new == macs_old == cases.expected_macs(cases.n_tiles(), bases)


def check_chain_cut(make, port):
    """g = 14, m = 10: the eleven-shift class is two chains (nine and two) under the packed kernel — one more product than the
    plan of dense_shift_packed = -1, which runs the eleven members uncut — and the oracle's counts either way."""
    ids, plist = once("cut list", lambda: packed.cut_list(port))
    seqs, tok, off, want = oracle(port, "cut", packed.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    uncut = cases.chains(plist)
    assert sorted(len(c) for c in uncut) == [1, 1, 10, 11] and sorted(len(c) for c in packed.cut(uncut)) == [1, 1, 1, 2, 9, 9]
    seen = numpy_statement(seqs[:40] + seqs[120:], plist, "cut", packed.CUT_G)
    assert seen["top"] <= 15
    got_new, macs_new = run(make, tok, off, ids, plist, packed.PACKED, packed.CUT_G, packed.CUT_M)
    got_old, macs_old = run(make, tok, off, ids, plist, packed.PARENT, packed.CUT_G, packed.CUT_M)
    assert not differ(got_new, want), differ(got_new, want)
    assert not differ(got_old, want), differ(got_old, want)
    assert macs_old == cases.expected_macs(cases.n_tiles(), len(uncut))
    assert macs_new == cases.expected_macs(cases.n_tiles(), len(uncut) + 2)   # (the class of eleven and the class of ten: one more each)


def check_crossing(make, port, ids):
    """One planted sequence whose AAAA count is 14 15 16 17 18 17 16 15 14 under the nine shifts: the hi pass runs in the middle
    steps of one chain, whose lo prefix sums go on through them."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "crossing", packed.crossing, ids)
    span_ids = packed.span4(pos)
    span = [pos[c] for c in span_ids]
    assert [int(packed.counts([packed.CROSSING], p, cases.G)[0][0]) for p in span] == packed.CROSSING_COUNTS
    seen = numpy_statement(seqs, span, "crossing")
    assert seen["top"] == 18 and seen["flagged_steps"] == [(u, u + 1) for u in range(1, 7)]
    got, _ = run(make, tok, off, ids, [pos[c] for c in ids], packed.PACKED)
    assert not differ(got, want), differ(got, want)


def check_fallback(make, port, ids, capfd):
    """The key-major planes do not fit (a tuning cap of 1 KiB): k_dense_shift_fix runs the plan, the oracle's counts come out,
    and under trace=1 the call says on stderr that it fell back (the packed run of the same list does not)."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "ragged", cases.ragged, ids)
    capfd.readouterr()
    got, macs = run(make, tok, off, ids, plist, dict(packed.PACKED, trace=1, **packed.NO_ROOM))
    said = capfd.readouterr().err
    assert "over the dense_shift_plane_kb cap: k_dense_shift_fix runs the corrections" in said, said
    assert not differ(got, want), differ(got, want)
    assert macs == cases.expected_macs(cases.n_tiles(), len(packed.cut(cases.chains(plist))))
    run(make, tok, off, ids, plist, dict(packed.PACKED, trace=1))
    assert "k_dense_shift_fix runs" not in capfd.readouterr().err


# ---- the numpy statement itself -----------------------------------------------------------------------------------------------
def test_packed_arithmetic_is_the_identity(port):
    """Ragged lengths (one window .. nine, the edges overlapping) and counts above 15 on three classes and two lone combinations."""
    pos = positions(port)
    plist = [pos[c] for c in cases.small_list(pos)]
    rng = np.random.Generator(np.random.PCG64(12))
    seqs = [rng.integers(1, 5, size=L).tolist() for L in (12, 13, 14, 19, 20, 40, 33, 12, 16)] + [[2] * 50, [1, 3] * 30, packed.CROSSING]
    total, seen = packed.packed_sum(seqs, plist)
    assert np.array_equal(total, cases.identity_sum(seqs, plist)) and np.array_equal(total, cases.direct_sum(seqs, plist))
    assert seen["top"] == 39 and seen["flagged_steps"]


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


def test_emu_byte_range_at_its_ends(make_emu, port):
    check_extremes(make_emu, port, packed.span4(positions(port)), "emu")


@pytest.mark.parametrize("name", ["uniform", "ragged"])
def test_emu_both_kernels(make_emu, port, name):
    check_both_kernels(make_emu, port, name, cases.small_list(positions(port)))


def test_emu_chain_cut(make_emu, port):
    check_chain_cut(make_emu, port)


def test_emu_flagged_steps_inside_a_long_chain(make_emu, port):
    check_crossing(make_emu, port, packed.span4(positions(port)))


def test_emu_planes_do_not_fit(make_emu, port, capfd):
    check_fallback(make_emu, port, cases.small_list(positions(port)), capfd)
