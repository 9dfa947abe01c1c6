"""The ahead schedule of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_shift_packed<true, true>; tuning
dense_shift_ahead): at a chain's first step the next chain's first planes go into the idle stage buffer and its key offsets into
the idle half of an offsets ring, and no step inside a chain loads from memory. tests/dense_shift_ahead_cases.py holds the
inputs and the numpy preconditions; the check functions here state the contract and tests/test_gpu_dense_shift_ahead.py runs
them on the device. ``make(g, m, **kw)`` creates an engine; no expected value comes from one: counts are compared cell for
cell, over the whole triangle, with the CPU oracle (``port.raw_counts``). Every case runs with dense_shift_ahead = 1 and = 0,
and the two are held against each other; launches and dense_macs are stated from the plan alone.

The emulator runs a workgroup's threads one after another between barriers and a direct-to-LDS load lands when it is issued: it
CANNOT see the timing of the prefetch — a load still in flight when its buffer is read, a barrier that does not order what a
load landed. What it checks is the schedule's bookkeeping: the chain table, the buffers, the ring halves, the lost prefetch. The
device cases compare every cell of every tile, and that is the race check. The emulator runs lists of up to 49 combinations;
all 495 run on the device."""
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
from test_emu_dense_shift import differ, once, positions  # noqa: E402
from test_emu_dense_shift_lanes import oracle  # noqa: E402


def run(make, tok, off, n, ids, plist, g=cases.G, m=cases.M, calls=1, bands=None, inplace_form=1):
    """``calls`` calls over ``ids`` (kept positions ``plist``) after reset_counts, with dense_shift_ahead = 1 and = 0 -> the
    counts of the two, which must be equal. The launches and the dense_macs of a call are stated from the plan alone and do not
    depend on the key: the count, the edge keys, one base launch per distinct chain length, ONE launch of corrections, the two
    key-major planes and the key offsets; one product per chain. ``bands``: row bands of accumulate_rows instead of one call."""
    got = {}
    chains = batch.plan_chains(plist)
    want_launches = 1 + 1 + len({len(c) for c in chains}) + 1 + 3
    want_macs = ahead.expected_macs(n, len(chains), g - m)
    for key in ahead.AHEAD:
        e = make(g, m, path=1, tuning=dict(ahead.TUNING, dense_shift_ahead=key, dense_shift_inplace=inplace_form))
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
    assert np.array_equal(got[1], got[0]), "dense_shift_ahead = 1 and = 0 differ: " + differ(got[1], got[0])
    return got[1]


def check_mixed(make, port, ids, name, n=inplace.NIBBLES_N, calls=1, bands=None, inplace_form=1):
    """Uniform sequences at N = 258 (two full tile rows and one with two rows) over a list with chains of several lengths, chains
    of one step among them, and a last chain without a successor."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    lengths = [len(c) for c in batch.plan_chains(plist)]
    assert sum(n > 1 for n in lengths) > 1, "several chains with steps: the last of them has no successor"
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(n, 40, 51), ids)
    got = run(make, tok, off, n, ids, plist, calls=calls, bands=bands, inplace_form=inplace_form)
    assert not differ(got, calls * want), differ(got, calls * want)


def check_list(make, port, ids, name, lengths=None):
    """A list as a call may bring it: one chain, one chain of one step, a class with a gap, a rank's share of a sharded run."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    if lengths is not None:
        assert [len(c) for c in batch.plan_chains(plist)] == lengths
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(inplace.NIBBLES_N, 40, 52), ids)
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


def check_cut(make, port):
    """g = 14, m = 10, N = 258: the class of eleven shifts cut into nine + two, a class of ten into nine + one: two chains of
    eight steps fill a ring half each, a chain of one step follows them, lone combinations add no chain to the table."""
    ids, plist = once("cut list", lambda: packed.cut_list(port))
    seqs, tok, off, want = oracle(port, "cut", lanes.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    assert [len(c) for c in batch.plan_chains(plist)] == [9, 9, 2, 1, 1, 1]
    got = run(make, tok, off, len(seqs), ids, plist, packed.CUT_G, packed.CUT_M)
    assert not differ(got, want), differ(got, want)


def check_small_keys(make, port, m, take=None):
    """k = 3 (64 keys) and k = 2 (16 keys) at g = 12, N = 258: a staged plane is 4 KB and 1 KB instead of 16 KB, one load a side
    (the waves past the plane's end land nothing), so a prefetch has fewer loads in flight."""
    g = cases.G
    ids, plist = once(("ahead small keys", m, take), lambda: ahead.small_keys(port, g, m, take))
    assert max(len(c) for c in batch.plan_chains(plist)) == packed.MAX_CHAIN and g - m < 4
    seqs, tok, off, want = oracle(port, "ahead small keys", lambda: cases.uniform(inplace.NIBBLES_N, 40, 54), ids, g, m)
    got = run(make, tok, off, len(seqs), ids, plist, g, m)
    assert not differ(got, want), differ(got, want)


def check_placed(make, port, place, ids=None):
    """A count of 12 .. 16 .. 12 over the nine shifts (ahead.PEAK16) at an even and an odd nibble of both sides of tile (1, 0),
    N = 386, and a list that puts the flagged step at a chain's first, middle or last step or at the NEXT chain's first step
    (ahead.PLACES). In the tiles of tile rows 0 and 1 the prefetch is not issued or is overwritten, and the chain must still
    finish — the steps behind the flagged ones are made in place again — and hand over to the chains behind it; tile rows 2 and 3
    hold no count above 15 and their tiles (2, 2), (3, 2), (3, 3) keep every prefetch. ``ids``: a larger list that holds the case's
    (the device: all 495, in which the class of nine is the first chain and its steps 3 and 4 are flagged)."""
    pos = positions(port)
    ids = ahead.placed_list(pos, place) if ids is None else ids
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "ahead peak16", lambda: inplace.crossing(ahead.PEAK16), ids)
    span = [pos[c] for c in packed.span4(pos)]
    assert [int(packed.counts([ahead.PEAK16], p, cases.G)[0][0]) for p in span] == ahead.PEAK16_COUNTS
    planted = [seqs[x] for x in inplace.CROSSING_AT]
    assert [lanes.nibble(x % cases.TILE) for x in inplace.CROSSING_AT] == [0, 1, 4, 5] and {x // cases.TILE for x in inplace.CROSSING_AT} == {0, 1}
    flagged = once(("ahead flagged", place, len(ids)), lambda: ahead.flagged_steps(planted, plist))
    if len(ids) < cases.N_COMBOS:
        assert flagged == ahead.PLACES[place][1], flagged
    else:
        assert flagged[:2] == [(0, 3), (0, 4)], flagged
    rest = [x for i, x in enumerate(seqs) if i >= 2 * cases.TILE]
    assert not once(("ahead unflagged", place, len(ids)), lambda: ahead.flagged_steps(rest, plist))
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


# ---- numpy alone ------------------------------------------------------------------------------------------------------------
def test_the_plan_of_config_5_has_every_chain_length(port):
    """All 495 combinations: 120 chains with steps, of every length from two to nine members, a run of 36 chains of one step, and
    84 chains whose first step is not their last."""
    lengths = [len(c) for c in batch.plan_chains(positions(port))]
    with_steps = [n for n in lengths if n > 1]
    assert len(with_steps) == 120 and sum(n - 1 for n in with_steps) == 330 and set(with_steps) == set(range(2, 10))
    assert with_steps.count(2) == 36 and with_steps[-36:] == [2] * 36 and sum(n > 2 for n in with_steps) == 84


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


def test_emu_chains_of_every_kind(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed")


def test_emu_one_chain(make_emu, port):
    check_list(make_emu, port, ahead.one_chain_list(positions(port)), "one chain", lengths=[9])


def test_emu_one_chain_of_one_step(make_emu, port):
    check_list(make_emu, port, batch.one_step_list(positions(port)), "one step", lengths=[2])


def test_emu_a_class_with_a_gap(make_emu, port):
    check_list(make_emu, port, cases.lists(positions(port))["gap"], "gap", lengths=[4, 4])


def test_emu_a_rank_of_a_sharded_run(make_emu, port):
    check_list(make_emu, port, batch.rank_list(1, 8), "rank 1 of 8")


def test_emu_chain_cut(make_emu, port):
    check_cut(make_emu, port)


@pytest.mark.parametrize("m", (9, 10))
def test_emu_fewer_than_256_keys(make_emu, port, m):
    check_small_keys(make_emu, port, m, take=3)


@pytest.mark.parametrize("place", sorted(ahead.PLACES))
def test_emu_flagged_step_loses_the_prefetch(make_emu, port, place):
    check_placed(make_emu, port, place)


def test_emu_two_calls_without_a_reset(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", calls=2)


def test_emu_two_row_bands(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", bands=((0, 128), (128, inplace.NIBBLES_N)))


def test_emu_key_is_ignored_without_the_in_place_form(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", inplace_form=0)
