"""The straight chains of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_shift_packed<true, true, true>; tuning
dense_shift_straight): the ahead schedule's loop runs over chains, a chain none of whose steps meets a count above 15 in its tile
runs lookups and barrier - update - barrier with a step counter, the ring position and the unpack bits, every other chain runs the
step loop's body, and both hand over through the same tail. tests/dense_shift_straight_cases.py holds the inputs and the numpy
preconditions; the check functions here state the contract and tests/test_gpu_dense_shift_straight.py runs them on the device.
``make(g, m, **kw)`` creates an engine; no expected value comes from one: counts are compared cell for cell, over the whole
triangle, with the CPU oracle (``port.raw_counts``). Every case runs with dense_shift_straight = 1 and = 0, and the two are held
against each other; launches and dense_macs are stated from the plan alone.

Like its sibling for the ahead schedule, the emulator lands a load when it is issued and sees the bookkeeping only: which chain
takes which path, what the straight path carries, the buffer and the ring half at the hand-over. The device cases compare every
cell of every tile, and that is the race check. The emulator runs lists of up to 49 combinations; all 495 run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_ahead_cases as ahead  # noqa: E402
import dense_shift_batch_cases as batch  # noqa: E402
import dense_shift_cases as cases  # noqa: E402
import dense_shift_inplace_cases as inplace  # noqa: E402
import dense_shift_lanes_cases as lanes  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
import dense_shift_straight_cases as straight  # noqa: E402
from test_emu_dense_shift import differ, once, positions  # noqa: E402
from test_emu_dense_shift_lanes import oracle  # noqa: E402


def run(make, tok, off, n, ids, plist, g=cases.G, m=cases.M, calls=1, bands=None, **tuning):
    """``calls`` calls over ``ids`` (kept positions ``plist``) after reset_counts, with dense_shift_straight = 1 and = 0 -> the
    counts of the two, which must be equal. The launches and the dense_macs of a call are stated from the plan alone and do not
    depend on the key: the count, the edge keys, one base launch per distinct chain length, ONE launch of corrections, the two
    key-major planes and the key offsets; one product per chain. ``bands``: row bands of accumulate_rows instead of one call.
    ``tuning``: further keys (the forms under which the new key is ignored)."""
    got = {}
    chains = batch.plan_chains(plist)
    want_launches = 1 + 1 + len({len(c) for c in chains}) + 1 + 3
    want_macs = ahead.expected_macs(n, len(chains), g - m)
    for key in straight.STRAIGHT:
        e = make(g, m, path=1, tuning=dict(straight.TUNING, dense_shift_straight=key, **tuning))
        e.load_sequences(tok, off, n, 0)
        e.reset_counts()
        for _ in range(calls):
            before = e.stats()
            if bands:
                for r0, r1 in bands:
                    e.accumulate_rows(np.asarray(ids, dtype=np.int32), r0, r1)
                assert e.stats()["count_launches"] - before["count_launches"] == 1   # the later bands reuse the panels, the planes and the tables
            else:
                e.accumulate(np.asarray(ids, dtype=np.int32))
                st = e.stats()
                assert st["n_tile_launches"] - before["n_tile_launches"] == 1
                assert st["launches"] - before["launches"] == want_launches, (st["launches"] - before["launches"], want_launches)
                assert st["dense_macs"] - before["dense_macs"] == want_macs, (st["dense_macs"] - before["dense_macs"], want_macs)
            assert e.stats()["path_used"] == 1
        e.finalize()
        got[key] = e.get_counts()
        e.close()
    assert np.array_equal(got[1], got[0]), "dense_shift_straight = 1 and = 0 differ: " + differ(got[1], got[0])
    return got[1]


def check_mixed(make, port, ids, name, n=inplace.NIBBLES_N, calls=1, bands=None, **tuning):
    """Uniform sequences at N = 258 (two full tile rows and one with two rows: every chain of every tile is clean) over a list
    with chains of several lengths, chains of one step among them, and a last chain without a successor."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    lengths = [len(c) for c in batch.plan_chains(plist)]
    assert sum(n > 1 for n in lengths) > 1, "several chains with steps: the last of them has no successor"
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(n, 40, 51), ids)
    got = run(make, tok, off, n, ids, plist, calls=calls, bands=bands, **tuning)
    assert not differ(got, calls * want), differ(got, calls * want)


def check_list(make, port, ids, name, lengths=None):
    """A list as a call may bring it, over clean tiles: one chain of one, two and eight steps (nine members: the longest the
    plan makes), a long chain and two one-step chains, a class with a gap, a rank's share of a sharded run."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    if lengths is not None:
        assert [len(c) for c in batch.plan_chains(plist)] == lengths
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(inplace.NIBBLES_N, 40, 52), ids)
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


def check_cut(make, port):
    """g = 14, m = 10, N = 258: the class of eleven shifts cut into nine + two, a class of ten into nine + one: two straight
    chains of eight steps fill a ring half each, a chain of one step follows them."""
    ids, plist = once("cut list", lambda: packed.cut_list(port))
    seqs, tok, off, want = oracle(port, "cut", lanes.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    assert [len(c) for c in batch.plan_chains(plist)] == [9, 9, 2, 1, 1, 1]
    got = run(make, tok, off, len(seqs), ids, plist, packed.CUT_G, packed.CUT_M)
    assert not differ(got, want), differ(got, want)


def check_placed(make, port, place, where, ids=None):
    """A count of 12 .. 16 .. 12 over the nine shifts (PEAK16) at an even and an odd nibble of both sides of tile (1, 0), N = 386,
    and a list that puts the flagged step at its chain's first, middle or last step, the flagged chain between two clean chains,
    first in the call or last in it (straight.placed_list). In the tiles of tile rows 0 and 1 that chain runs the step loop's
    body — staged steps, the hi pass, a lost prefetch, the late stage of the next start — between chains that run straight; tile
    rows 2 and 3 hold no count above 15 and in tiles (2, 2), (3, 2), (3, 3) every chain is straight. ``ids``: a larger list that
    holds the case's (the device: all 495, in which the class of nine is the first chain and its steps 3 and 4 are flagged)."""
    pos = positions(port)
    if ids is None:
        ids, at = straight.placed_list(pos, place, where)
        want_flagged = [(at, u) for u in straight.PLACES[place][1]]
    else:
        want_flagged = None
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "ahead peak16", lambda: inplace.crossing(straight.PEAK16), ids)
    planted = [seqs[x] for x in inplace.CROSSING_AT]
    flagged = once(("straight flagged", place, where, len(ids)), lambda: ahead.flagged_steps(planted, plist))
    if want_flagged is not None:
        assert flagged == want_flagged, (flagged, want_flagged)
    else:
        assert flagged[:2] == [(0, 3), (0, 4)], flagged
    rest = [x for i, x in enumerate(seqs) if i >= 2 * cases.TILE]
    assert not once(("straight unflagged", place, where, len(ids)), lambda: ahead.flagged_steps(rest, plist))
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


def check_one_side(make, port):
    """PEAK16 in tile row 1 only, the middle place between two clean chains: tile (1, 0) meets the count above 15 on its row
    side only, tiles (2, 1) and (3, 1) on their column side only, tile (1, 1) on both; the test that picks the path must look at
    both sides' masks, and at every step's."""
    pos = positions(port)
    ids, at = straight.placed_list(pos, "middle", "between")
    plist = [pos[c] for c in ids]
    seqs, planted_at = once("straight one side seqs", lambda: straight.one_side(straight.PEAK16))
    seqs, tok, off, want = oracle(port, "straight one side", lambda: seqs, ids)
    by_row = once("straight one side flagged", lambda: straight.flagged_by_tile_row(seqs, plist))
    assert by_row == [[], [(at, u) for u in straight.PLACES["middle"][1]], [], []], by_row
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


# ---- numpy alone ------------------------------------------------------------------------------------------------------------
def test_the_plan_orders_chains_longest_first(port):
    """Why no list has a one-step chain between two longer ones: in every list of these cases the chains' lengths never rise."""
    pos = positions(port)
    for ids in (batch.mixed_list(pos), straight.long_one_one(pos), straight.placed_list(pos, "middle", "between")[0], np.arange(cases.N_COMBOS)):
        lengths = [len(c) for c in batch.plan_chains([pos[c] for c in ids])]
        assert lengths == sorted(lengths, reverse=True)


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


def test_emu_one_chain_of_one_step(make_emu, port):
    check_list(make_emu, port, batch.one_step_list(positions(port)), "one step", lengths=[2])


def test_emu_one_chain_of_two_steps(make_emu, port):
    check_list(make_emu, port, straight.two_step_list(positions(port)), "two steps", lengths=[3])


def test_emu_one_chain_of_nine_members(make_emu, port):
    check_list(make_emu, port, ahead.one_chain_list(positions(port)), "one chain", lengths=[9])


def test_emu_one_step_chains_behind_a_long_one(make_emu, port):
    check_list(make_emu, port, straight.long_one_one(positions(port)), "long one one", lengths=[9, 2, 2])


def test_emu_a_rank_of_a_sharded_run(make_emu, port):
    check_list(make_emu, port, batch.rank_list(1, 8), "rank 1 of 8")


def test_emu_a_class_with_a_gap(make_emu, port):
    check_list(make_emu, port, cases.lists(positions(port))["gap"], "gap", lengths=[4, 4])


def test_emu_chain_cut(make_emu, port):
    check_cut(make_emu, port)


@pytest.mark.parametrize("where", straight.WHERE)
@pytest.mark.parametrize("place", sorted(straight.PLACES))
def test_emu_flagged_chain_among_straight_ones(make_emu, port, place, where):
    check_placed(make_emu, port, place, where)


def test_emu_flag_on_one_side_only(make_emu, port):
    check_one_side(make_emu, port)


def test_emu_chains_of_every_kind(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed")


def test_emu_two_calls_without_a_reset(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", calls=2)


def test_emu_two_row_bands(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", bands=((0, 128), (128, inplace.NIBBLES_N)))


@pytest.mark.parametrize("off", ("dense_shift_inplace", "dense_shift_ahead"))
def test_emu_key_is_ignored_without_the_ahead_schedule(make_emu, port, off):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", **{off: 0})
