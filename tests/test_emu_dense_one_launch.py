"""The one base launch over all chain-length groups of the shift-class plan (fsk_tile_kernel_dma.inc with FSK_DMA_SHIFT 2:
k_dense_tile_shift_all; tuning dense_shift_one_launch): one workgroup a tile runs the groups in descending chain length and
flushes at every group end WITHOUT clearing its sums, each flush multiplied by the weight step to the next group's length.
tests/dense_one_launch_cases.py states the group table and the numpy preconditions; the check functions here state the contract
and tests/test_gpu_dense_one_launch.py runs them on the device. ``make(g, m, **kw)`` creates an engine; no expected value comes
from one: counts are compared cell for cell, over the whole triangle, with the CPU oracle (``port.raw_counts``).

Every case is N = 130 (three tiles, the last with two real rows) on tuning tile_splits = 1, dense_shift = 1, and runs with
dense_shift_one_launch = 1 and = -1 (one k_dense_tile_shift launch a group, the form before): the same counts, the same
dense_macs, one tile pass, and the launches apart by the distinct chain lengths minus one.

The emulator affords some tens of combinations on three tiles: the full list's nine groups with every weight step 1 run as
one chain of each length 9 .. 1 (45 combinations); all 495 combinations, and the lists of 100, run on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_one_launch_cases as one  # noqa: E402
import dense_shift_cases as cases  # noqa: E402
from test_emu_dense_shift import differ, inputs, once, positions  # noqa: E402

STATS = ("dense_macs", "n_tile_launches", "launches")


def run(make, key, tok, off, ids, calls=1, bands=None):
    """``calls`` calls over ``ids`` after reset_counts (K held other data: the first flush of the first call stores, every other
    flush adds) -> the counts and each call's stats. ``bands``: every call as accumulate_rows over these row ranges."""
    ids = np.asarray(ids, dtype=np.int32)
    e = make(cases.G, cases.M, path=1, tuning=dict(one.TUNING, dense_shift_one_launch=key))
    e.load_sequences(tok, off, cases.N, 0)
    e.accumulate(ids[:1])
    e.reset_counts()
    deltas = []
    for _ in range(calls):
        before = e.stats()
        if bands:
            for lo, hi in bands:
                e.accumulate_rows(ids, lo, hi)
        else:
            e.accumulate(ids)
        st = e.stats()
        assert st["path_used"] == 1
        deltas.append({k: st[k] - before[k] for k in STATS})
    e.finalize()
    got = e.get_counts()
    e.close()
    return got, deltas


def check_pair(make, port, name, ids, calls=1, bands=None):
    """The case with the key at 1 and at -1 against the oracle and against each other. Returns the group table."""
    ids = np.asarray(ids, dtype=np.int32)
    pos = positions(port)
    plist = [pos[c] for c in ids]
    table = one.groups(plist)
    bases = len(one.plan_chains(plist))
    seqs, tok, off, want = inputs(port, name, ids)
    got = {}
    for key in one.KEYS:
        got[key] = run(make, key, tok, off, ids, calls=calls, bands=bands)
        print("%s, %d combinations, key %d: groups %s, %s" % (name, len(ids), key, table, got[key][1]))
    passes = len(bands) if bands else 1
    for (counts, deltas) in got.values():
        assert not differ(counts, calls * want), differ(counts, calls * want)
        for d in deltas:
            assert d["n_tile_launches"] == passes
            assert d["dense_macs"] == cases.expected_macs(cases.n_tiles(), bases)   # (over the bands: one tile, then two)
    assert np.array_equal(got[1][0], got[-1][0])
    for d_one, d_each in zip(got[1][1], got[-1][1]):
        assert d_one["dense_macs"] == d_each["dense_macs"]
        assert d_each["launches"] - d_one["launches"] == passes * (len(table) - 1), (d_each, d_one, table)
    return table


def check_nine_groups(make, port, ids):
    """Nine groups, every weight step 1; and the data's own zeros: cells that the first flush stores as zero and a later flush
    adds to."""
    pos = positions(port)
    seqs = inputs(port, "uniform", ids)[0]
    zeros, added = once(("stored zeros", "uniform", len(ids)), lambda: one.stored_zeros(seqs, [pos[c] for c in ids]))
    assert zeros >= 100 and added >= 100, (zeros, added)
    table = check_pair(make, port, "uniform", ids)
    assert len(table) == 9 and all(d == 1 for _, d in table)


def check_uneven_steps(make, port, ids):
    """small_list: chain lengths 9, 8, 8, 1, 1 — weight steps 1, 7 and 1 at end slots 1, 3 and 5. A flush that forgets its step,
    takes the chain length for it or clears the sums gives other counts."""
    pos = positions(port)
    seqs = inputs(port, "uniform", ids)[0]
    zeros, added = once(("stored zeros", "uniform small"), lambda: one.stored_zeros(seqs, [pos[c] for c in ids]))
    assert zeros >= 100 and added >= 100, (zeros, added)
    assert check_pair(make, port, "uniform", ids) == [(1, 1), (3, 7), (5, 1)]


def check_list(make, port, name):
    """The lists a combo-sharded rank passes: arbitrary lengths in any order, one group only, a lone combination (not eligible
    for the shift path: it runs as before, and the key changes nothing)."""
    ids = cases.lists(positions(port))[name]
    table = check_pair(make, port, "ragged", ids)
    assert {"one": table == [(1, 1)], "gap": table == [(2, 4)]}.get(name, len(table) >= 1)


def check_planted(make, port, which, ids):
    """Counts of 79 on the row side, the column side and both sides of tile (1, 0): the hi-plane remainder runs in stages that a
    flush follows. From numpy: the flagged panels are the ones the case names."""
    pos = positions(port)
    seqs = inputs(port, which, ids)[0]
    panels, top = once(("high", which), lambda: cases.high_panels(seqs, [pos[c] for c in (0, 100, 494)]))
    assert top == 79 and panels == {"rows": {2}, "cols": {0, 1}, "both": {0, 1, 2}}[which]
    assert len(check_pair(make, port, which, ids)) >= 3


def check_ragged(make, port, ids):
    """Padded rows and the last tile's i >= N rows, lengths from one window up."""
    assert len(check_pair(make, port, "ragged", ids)) >= 3


def check_twice(make, port, ids):
    """Two accumulates on one load without a reset: the second call adds at EVERY flush, its first included — twice the oracle."""
    assert len(check_pair(make, port, "ragged", ids, calls=2)) >= 3


def check_row_bands(make, port, ids):
    """Rows [0, 128) and [128, 130) over one counted list: the second band reuses the panels, the edge keys and the group table,
    and each band's first flush stores (the rows are still zero by contract, from their lower edge)."""
    assert len(check_pair(make, port, "ragged", ids, bands=((0, 128), (128, cases.N)))) >= 3


# ---- the case module's own statements ---------------------------------------------------------------------------------------
def test_group_tables(port):
    pos = positions(port)
    full = one.groups(pos)
    assert [e for e, _ in full] == [1, 4, 10, 20, 35, 56, 84, 120, 165] and all(d == 1 for _, d in full)
    each = one.one_chain_of_each_length(pos)
    assert one.groups([pos[c] for c in each]) == [(b, 1) for b in range(1, 10)]
    assert one.groups([pos[c] for c in cases.small_list(pos)]) == [(1, 1), (3, 7), (5, 1)]
    ls = cases.lists(pos)
    assert one.groups([pos[c] for c in ls["gap"]]) == [(2, 4)] and one.groups([pos[c] for c in ls["repeated"]]) == [(1, 3), (2, 2)]
    assert one.groups([pos[c] for c in ls["one"]]) == [(1, 1)]
    assert one.groups([pos[c] for c in ls["subset"]]) == one.groups([pos[c] for c in ls["shuffled"]])


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


def test_emu_nine_groups_of_step_one(make_emu, port):
    check_nine_groups(make_emu, port, one.one_chain_of_each_length(positions(port)))


def test_emu_uneven_weight_steps(make_emu, port):
    check_uneven_steps(make_emu, port, cases.small_list(positions(port)))


@pytest.mark.parametrize("name", ["gap", "repeated", "one"])
def test_emu_lists(make_emu, port, name):
    check_list(make_emu, port, name)


def test_emu_counts_above_15(make_emu, port):
    check_planted(make_emu, port, "both", cases.small_list(positions(port)))


def test_emu_ragged(make_emu, port):
    check_ragged(make_emu, port, cases.small_list(positions(port)))


def test_emu_two_calls_without_a_reset(make_emu, port):
    check_twice(make_emu, port, cases.small_list(positions(port)))


def test_emu_row_bands(make_emu, port):
    check_row_bands(make_emu, port, cases.small_list(positions(port)))
