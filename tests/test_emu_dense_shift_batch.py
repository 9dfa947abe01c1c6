"""The batched unpack of the packed shift corrections (fsk_kernels_dense_shift.h: k_dense_shift_packed; tuning
dense_shift_batch): the prefix sums of a batch of steps are added byte to byte and leave for the int32 sums where the step table
carries the flag. tests/dense_shift_batch_cases.py holds the inputs, the walk and the numpy statement; the check functions here
state the contract and tests/test_gpu_dense_shift_batch.py runs them on the device. ``make(g, m, **kw)`` creates an engine; no
expected value comes from one: counts are compared cell for cell, over the whole triangle, with the CPU oracle
(``port.raw_counts``), after numpy has shown what the inputs make a byte of Q reach. Every case runs with dense_shift_batch = 1
(by the bound) and = 0 (after every step), and the two are held against each other.

The emulator runs lists of up to 49 combinations; all 495 run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_batch_cases as batch  # noqa: E402
import dense_shift_cases as cases  # noqa: E402
import dense_shift_inplace_cases as inplace  # noqa: E402
import dense_shift_lanes_cases as lanes  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift import differ, once, positions  # noqa: E402
from test_emu_dense_shift_lanes import oracle  # noqa: E402


def run(make, tok, off, n, ids, plist, g=cases.G, m=cases.M, calls=1, bands=None, inplace_form=1):
    """``calls`` calls over ``ids`` (kept positions ``plist``) after reset_counts, with dense_shift_batch = 1 and = 0 ->
    the counts of the two, which must be equal. The launches of a call are stated from the plan alone and do not depend on the
    key: the count, the edge keys, one base launch per distinct chain length, ONE launch of corrections, and the two key-major
    planes and the key offsets. ``bands``: row bands of accumulate_rows instead of one call."""
    got = {}
    want_launches = 1 + 1 + len({len(c) for c in batch.plan_chains(plist)}) + 1 + 3
    for key in batch.BATCH:
        e = make(g, m, path=1, tuning=dict(batch.TUNING, dense_shift_batch=key, dense_shift_inplace=inplace_form))
        e.load_sequences(tok, off, n, 0)
        e.reset_counts()
        for _ in range(calls):
            before = e.stats()
            if bands:
                for r0, r1 in bands:
                    e.accumulate_rows(np.asarray(ids, dtype=np.int32), r0, r1)
                assert e.stats()["count_launches"] - before["count_launches"] == 1   # the later bands reuse the panels and the step table
            else:
                e.accumulate(np.asarray(ids, dtype=np.int32))
                st = e.stats()
                assert st["n_tile_launches"] - before["n_tile_launches"] == 1
                assert st["launches"] - before["launches"] == want_launches, (st["launches"] - before["launches"], want_launches)
            assert e.stats()["path_used"] == 1
        e.finalize()
        got[key] = e.get_counts()
        e.close()
    assert np.array_equal(got[1], got[0]), "dense_shift_batch = 1 and = 0 differ: " + differ(got[1], got[0])
    return got[1]


def numpy_statement(name, seqs, plist, g=cases.G):
    """batched_sum (the new arithmetic) == the identity (g = 12) or the direct sum, with the flags of either key; returns what
    batched_sum saw under the bound's flags."""
    def build():
        total, seen = batch.batched_sum(seqs, plist, g, batch=1)
        every, _ = batch.batched_sum(seqs, plist, g, batch=0)
        want = cases.identity_sum(seqs, plist) if g == cases.G else packed.direct_sum(seqs, plist, g)
        assert np.array_equal(total, want) and np.array_equal(every, want)
        return seen
    return once(("batch numpy", name, g), build)


def check_mixed(make, port, ids, name, n=inplace.NIBBLES_N, calls=1, bands=None, uniform_seed=51):
    """Uniform sequences at N = 258 (two full tile rows and one with two rows) over a list with chains of several lengths:
    batches inside a chain, batches that span chains, a partial last batch."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(n, 40, uniform_seed), ids)
    numpy_statement(name, seqs[:40 if len(ids) <= 64 else 12], plist)   # (the arithmetic does not depend on N: the first sequences of the same input)
    got = run(make, tok, off, n, ids, plist, calls=calls, bands=bands)
    assert not differ(got, calls * want), differ(got, calls * want)


def check_extremes(make, port, ids, all_combos=False):
    """RUN / PLUS / MINUS by i mod 3 at N = 386: under the class of nine shifts a byte of Q sits AT the bound of each of its six
    batches (180, 120, 150, 180, 210, 240: the largest byte of Q over the run is 240) and one sits at 0, in the row term and in
    the column term, at even and odd nibbles. numpy shows it before the engine is asked."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "batch extremes", lanes.everywhere, ids)
    span = [pos[c] for c in packed.span4(pos)]
    seen = numpy_statement("extremes", seqs, span)
    assert batch.extremes_facts(seen) == 240
    if all_combos:   # what the batches of the other shapes reach under these inputs (the walk is the bound, not this)
        full = once("batch extremes 495", lambda: batch.batched_sum(seqs[:48], plist)[1])
        assert [b["top"] for b in full["batches"][:6]] == [{"row": x, "col": x} for x in batch.SPAN4_BOUNDS]
        short = batch.shortfall(full)
        print("batches short of their bound: %d of %d; the largest byte of Q %d; (batch, bound, reached) %s"
              % (len(short), len(full["batches"]), max(max(b["top"].values()) for b in full["batches"]), short[:12]))
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


def check_cut(make, port):
    """g = 14, m = 10, N = 258: chains of 9, 9, 2 and lone combinations. Batches end in the middle of a chain and exactly at a
    chain's last step (240 of 255), and the last chain's one step is a batch of its own."""
    ids, plist = once("batch cut list", lambda: batch.cut_flags(port))
    seqs, tok, off, want = oracle(port, "cut", lanes.cut_seqs, ids, packed.CUT_G, packed.CUT_M)
    numpy_statement("cut", [x for x in seqs if len(x) == 40][:24], plist, packed.CUT_G)
    got = run(make, tok, off, len(seqs), ids, plist, packed.CUT_G, packed.CUT_M)
    assert not differ(got, want), differ(got, want)


def check_crossing(make, port, ids, form):
    """A count of 14 .. 18 .. 14 over the nine shifts (packed.CROSSING) at N = 386: the steps 1 .. 6 of the chain are flagged
    (a count above 15), two of them inside the batch {0, 1, 2}: their hi pass adds to the int32 sums directly while the batch's
    bytes are still in Q. With the in-place form on and off."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    seqs, tok, off, want = oracle(port, "inplace crossing", lambda: inplace.crossing(packed.CROSSING), ids)
    span = [pos[c] for c in packed.span4(pos)]
    planted = [seqs[x] for x in inplace.CROSSING_AT] + [seqs[x] for x in lanes.HI_PLUS_AT[:2] + lanes.HI_MINUS_AT[:2]]
    seen = numpy_statement("crossing", planted, span)
    assert seen["flagged_steps"] == [(0, 1), (0, 2), (1, 0), (2, 0), (3, 0), (4, 0)]   # (batch, place in the batch)
    got = run(make, tok, off, len(seqs), ids, plist, inplace_form=form)
    assert not differ(got, want), differ(got, want)


def check_list(make, port, ids, name, only_flag=False):
    """A list as a call may bring it: a rank's share of a combo-sharded run, a class with a gap, one chain of one step."""
    pos = positions(port)
    plist = [pos[c] for c in ids]
    flags = batch.unpack_flags([len(c) for c in batch.plan_chains(plist)])
    assert flags and flags[-1][2] and (not only_flag or [f for c, r, f in flags] == [True])
    seqs, tok, off, want = oracle(port, "batch " + name, lambda: cases.uniform(inplace.NIBBLES_N, 40, 52), ids)
    numpy_statement(name, seqs[:24], plist)
    got = run(make, tok, off, len(seqs), ids, plist)
    assert not differ(got, want), differ(got, want)


# ---- numpy alone ------------------------------------------------------------------------------------------------------------
def test_the_walk_on_config_5(port):
    """The plan of all 495 combinations: chain lengths as the case module states them, 125 unpack points for 330 steps, every
    batch inside the byte; the key at 0 flags every step."""
    pos = positions(port)
    lengths = [len(c) for c in batch.plan_chains(pos)]
    assert lengths == batch.CONFIG5_LENGTHS
    got, bounds = batch.batches(lengths)
    assert len(got) == 125 and max(bounds) <= batch.BYTE and sum(map(len, got)) == 330
    assert any(len({c for c, r in b}) > 1 for b in got) and bounds[-1] < 240   # batches span chains; the last one is partial


def test_batched_arithmetic_is_the_identity(port):
    """Ragged lengths are the engine cases' business; the arithmetic is held against the identity on the mixed list, with counts
    above 15 in it (packed.CROSSING among uniform sequences)."""
    pos = positions(port)
    ids = batch.mixed_list(pos)
    seqs = cases.uniform(24, 60, 53)
    seqs[3] = list(packed.CROSSING)
    seqs[17] = list(packed.CROSSING)
    seen = numpy_statement("mixed crossing", seqs, [pos[c] for c in ids])
    assert seen["flagged_steps"] and len(seen["batches"]) == 14


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


def test_emu_batches_inside_and_across_chains(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed")


def test_emu_bytes_of_q_at_their_bound_and_at_zero(make_emu, port):
    check_extremes(make_emu, port, packed.span4(positions(port)))


def test_emu_chain_cut(make_emu, port):
    check_cut(make_emu, port)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_emu_flagged_steps_inside_a_batch(make_emu, port, form):
    check_crossing(make_emu, port, packed.span4(positions(port)), form)


def test_emu_a_rank_of_a_sharded_run(make_emu, port):
    check_list(make_emu, port, batch.rank_list(1, 8), "rank 1 of 8")


def test_emu_a_class_with_a_gap(make_emu, port):
    check_list(make_emu, port, cases.lists(positions(port))["gap"], "gap")


def test_emu_one_chain_of_one_step(make_emu, port):
    check_list(make_emu, port, batch.one_step_list(positions(port)), "one step", only_flag=True)


def test_emu_two_calls_without_a_reset(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", calls=2)


def test_emu_two_row_bands(make_emu, port):
    check_mixed(make_emu, port, batch.mixed_list(positions(port)), "mixed", bands=((0, 128), (128, inplace.NIBBLES_N)))
