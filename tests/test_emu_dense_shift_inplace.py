"""The in-place form of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_shift_packed<true>; tuning
dense_shift_inplace): a chain's key-major planes are staged at its first step and every further unflagged step's are made in
LDS, one nibble up and one down a sequence. tests/dense_shift_inplace_cases.py holds the inputs and the numpy preconditions; the check functions here state
the contract and tests/test_gpu_dense_shift_inplace.py runs them on the device. ``make(g, m, **kw)`` creates an engine; no
expected value comes from one: counts are compared cell for cell, over the whole triangle, with the CPU oracle
(``port.raw_counts``), after numpy has shown that the inputs reach what they are meant to reach. Every case runs with
dense_shift_inplace = 1 and = 0 (every step staged): the same counts, the same launches.

The emulator runs the class of nine shifts and the 23 combinations of the chain cut; all 495 combinations run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
import dense_shift_inplace_cases as inplace  # noqa: E402
import dense_shift_lanes_cases as lanes  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift import differ, once, positions  # noqa: E402
from test_emu_dense_shift_lanes import oracle  # noqa: E402


def run(make, form, tok, off, n, ids, plist, g=cases.G, m=cases.M, calls=1):
    """``calls`` calls over ``ids`` (kept positions ``plist``) after reset_counts -> counts. The launches of a call are stated
    from the plan alone and do not depend on the form: the count, the edge keys, one base launch per distinct chain length, ONE
    launch of corrections, and the two key-major planes and the key offsets."""
    e = make(g, m, path=1, tuning=dict(inplace.TUNING, dense_shift_inplace=form))
    e.load_sequences(tok, off, n, 0)
    e.reset_counts()
    want_launches = 1 + 1 + len({len(c) for c in packed.cut(cases.chains(plist))}) + 1 + 3
    for _ in range(calls):
        before = e.stats()
        e.accumulate(np.asarray(ids, dtype=np.int32))
        st = e.stats()
        assert st["path_used"] == 1 and st["n_tile_launches"] - before["n_tile_launches"] == 1
        assert st["launches"] - before["launches"] == want_launches, (st["launches"] - before["launches"], want_launches)
    e.finalize()
    got = e.get_counts()
    e.close()
    return got


def span_of(port):
    pos = positions(port)
    return [pos[c] for c in packed.span4(pos)]


def check_every_nibble(make, port, ids, form, calls=1):
    """Tile row 1 holds one sequence 128 times (N = 258): its keys differ at every step, so in every step all 8 nibbles of all
    16 dwords of two keys move together, on the row side and on the column side, in a diagonal and in off-diagonal tiles.
    ``calls`` = 2: a second call on the same load adds the same counts again (the planes in memory are as the first call read them)."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "inplace nibbles", inplace.same_row, ids)
    facts = once("inplace nibbles facts", lambda: inplace.chain_facts(seqs, span_of(port)))
    assert not {u for i, u in facts["stay"] if i == cases.TILE} and max(facts["top"].values()) <= 15
    got = run(make, form, tok, off, len(seqs), ids, [pos[c] for c in ids], calls=calls)
    assert not differ(got, calls * want), differ(got, calls * want)


def check_moves_and_stays(make, port, ids, form):
    """RUN / PLUS / MINUS by i mod 3 with STAY in every tile row (N = 386): steps that move nothing (equal keys) sit next to
    steps that take a count 1 -> 0 and 0 -> 1, counts of 15 stay where they are, and no count leaves its nibble."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "inplace moves", inplace.moves_and_stays, ids)
    facts = once("inplace moves facts", lambda: inplace.chain_facts(seqs, span_of(port)))
    for i in inplace.STAY_AT:
        assert sorted(u for q, u in facts["stay"] if q == i) == inplace.STAY_STEPS
        assert {u for q, u in facts["down_to_0"] if q == i} and {u for q, u in facts["up_from_0"] if q == i}
    assert {u for q, u in facts["down_to_0"] if q % 3 == 1 and q not in inplace.STAY_AT} == {7}   # PLUS: its last GGGG
    assert set(facts["top"].values()) == {15}                                                # RUN, in every tile row
    got = run(make, form, tok, off, len(seqs), ids, [pos[c] for c in ids])
    assert not differ(got, want), differ(got, want)


def check_crossing(make, port, ids, form, which):
    """A count of 14 .. 18 .. 14 over the nine shifts (packed.CROSSING) at an even and an odd nibble of both sides of tile
    (1, 0), N = 386: in the tiles of tile rows 0 and 1 the steps that meet a count above 15 are staged and run the hi pass, and
    so is the step behind them; where the sequence is a column only (tiles (2, 0), (3, 1), ...) the chain's second step is still
    made in place before the count crosses. Tile rows 2 and 3 hold no count above 15 and their tiles (2, 2), (3, 2), (3, 3) stay
    in place throughout. With inplace.PEAK15 (11 .. 15 .. 11) no step is flagged and an update takes a nibble to exactly 15: the
    two sides of the condition."""
    pos = positions(port)
    name = "crossing" if which is packed.CROSSING else "peak15"
    seqs, tok, off, want = oracle(port, "inplace " + name, lambda: inplace.crossing(which), ids)
    span = span_of(port)
    shown = [int(packed.counts([which], p, cases.G)[0][0]) for p in span]
    facts = once("inplace %s facts" % name, lambda: inplace.chain_facts(seqs, span))
    if which is packed.CROSSING:
        assert shown == packed.CROSSING_COUNTS
        assert facts["top"][0] == 18 and facts["top"][1] == 18 and facts["top"][2] <= 15 and facts["top"][3] <= 15
    else:
        assert shown == inplace.PEAK15_COUNTS
        assert max(facts["top"].values()) == 15 and facts["top_moved"] == 15
    got = run(make, form, tok, off, len(seqs), ids, [pos[c] for c in ids])
    assert not differ(got, want), differ(got, want)


def check_ragged(make, port, ids, form):
    """Sequences of one window (length g) and ragged lengths in every tile row, N = 258: the last tile side holds two real rows
    and 126 padded positions, whose keys are 0 | 0 and whose zero planes stay zero."""
    pos = positions(port)
    seqs, tok, off, want = oracle(port, "inplace ragged", inplace.ragged, ids)
    facts = once("inplace ragged facts", lambda: inplace.chain_facts(seqs, span_of(port)))
    one_window = [i for i, x in enumerate(seqs) if len(x) == cases.G]
    for i in one_window:   # its one key moves at a step, 1 -> 0 and 0 -> 1, or stays
        moved = {u for q, u in facts["down_to_0"] if q == i}
        assert moved == {u for q, u in facts["up_from_0"] if q == i} and moved | {u for q, u in facts["stay"] if q == i} == set(range(8))
    assert len(seqs) - 1 in one_window and max(facts["top"].values()) <= 15
    got = run(make, form, tok, off, len(seqs), ids, [pos[c] for c in ids])
    assert not differ(got, want), differ(got, want)


def check_cut(make, port, form):
    """g = 14, m = 10, N = 258: the class of eleven shifts is cut into nine + two, so a chain of one step directly follows a
    chain of eight and the hand-over of the next chain's first planes crosses it; lone combinations add no step."""
    ids, plist = once("cut list", lambda: packed.cut_list(port))
    seqs, tok, off, want = oracle(port, "cut", lanes.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    assert sorted(len(c) for c in packed.cut(cases.chains(plist))) == [1, 1, 1, 2, 9, 9]
    got = run(make, form, tok, off, len(seqs), ids, plist, packed.CUT_G, packed.CUT_M)
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


def span4(port):
    return packed.span4(positions(port))


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_every_nibble_position(make_emu, port, form):
    check_every_nibble(make_emu, port, span4(port), form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_moves_and_stays(make_emu, port, form):
    check_moves_and_stays(make_emu, port, span4(port), form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_crossing_falls_back(make_emu, port, form):
    check_crossing(make_emu, port, span4(port), form, packed.CROSSING)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_peak_of_15_stays_in_place(make_emu, port, form):
    check_crossing(make_emu, port, span4(port), form, inplace.PEAK15)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_one_window_and_ragged(make_emu, port, form):
    check_ragged(make_emu, port, span4(port), form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_chain_cut_hands_over(make_emu, port, form):
    check_cut(make_emu, port, form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_two_calls_on_one_load(make_emu, port, form):
    check_every_nibble(make_emu, port, span4(port), form, calls=2)
