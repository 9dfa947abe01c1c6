"""The dense tile kernels (fsk_tile_kernel_dma.inc) at the edges of their loops: a second trip of the mask-chunk loop (the row
masks restaged, the double-buffered direct-to-LDS pipeline restarted from cold), flagged rows (counts above 15, the hi-plane
remainder) in mask words above 0, in the upper 16 rows of a word, in word 63 of 16,384 keys, in the first stage after a restart
and in a final stage of fewer than 16 rows, two and three hi-plane rounds in one stage, and the compact kernels' side-aware
remainder with one side flagged. tests/tile_edges_cases.py holds the inputs and the numpy yardsticks; the check functions here
state the contract and tests/test_gpu_tile_edges.py runs them on the device. Before a check calls the engine it asserts, from
the yardstick's flagged rows alone, that its case reaches the edges it names: a case that drifts off its edge fails.
``make(g, m, **kw)`` creates an engine; no expected value comes from an engine.

Counts are compared bit for bit with the CPU oracle. The non-compact kernels' ``dense_macs`` (profile mode) must equal
cases.expected_macs, which ties the yardstick's flagged rows to the kernel's row masks; the compact kernels index rows by
compacted rank: for them the counts and ``compact_keys_avg > 0``.

The emulator stands plain copies in for the direct-to-LDS loads, their waits and the M0 save and restore. A chunk crossing of a
non-compact kernel is at least 1024 * 32 dword rows a tile, and profile mode's k_dense_distinct is one emulated workgroup a
(row, combination) — 85 of case B's 99 seconds on one tile. So the emulator runs A, B, C and F on one tile (N = 66), A to C
without profile mode (dense_macs is then the plain rows alone, asserted as such), and D, E (the sides need tile (1, 0)), G and H
whole; H is the small case whose dense_macs has flagged rows in mask words above 0. Every form of A to C at three tiles in
profile mode, and the skip_test_block pass, run on the device only.

Case F: the issue of this suite supposed that the uncapped branch chunk_slots = 960 / (2 nst) < 64 needs more than the 4096
keys key compaction accepts. It needs nst >= 8, that is Vq8 >= 225 dword rows of 8 keys: V >= 1793. Five symbols at k = 5 are
3125 keys, nst = 13, chunk_slots = 36.

Not reachable from sequences: the compact kernels' skip of a combination with no key at all (FSK_ROWS_OF(slot) == 0) — any
window gives its combination a key."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tile_edges_cases as cases  # noqa: E402

_ONCE = {}


def once(port, name, N):
    """A case's inputs and yardsticks, computed once per session and shared: read-only."""
    if (name, N) not in _ONCE:
        _ONCE[(name, N)] = cases.build(port, name, N)
    return _ONCE[(name, N)]


def check_case(make, port, name, form, N=130, profile=True):
    """``profile``: the non-compact kernels' dense_macs with the flagged rows' remainder term (profile mode); without it the
    engine states the plain rows alone. The compact cases never need the mode."""
    c = once(port, name, N)
    g, m, compact = c["g"], c["m"], c["compact"]
    profile = profile and not compact
    tuning = dict(cases.FORMS[form], compact=compact)
    geo = cases.geometry(c["sigma"], c["k"], len(c["combos"]), tuning["tile_splits"], compact)
    tiles = cases.tiles_of(N)
    cases.assert_edges(c, geo, form, tiles)
    assert not compact or geo["V"] <= 4096   # (key compaction takes no more)
    print("%s/%s N=%d: V=%d Vq8=%d nst=%d chunk_slots=%d slots_per_split=%d" % (name, form, N, geo["V"], geo["Vq8"], geo["nst"],
                                                                             geo["chunk_slots"], geo["slots_per_split"]))
    e = make(g, m, path=1, profile=profile, tuning=tuning)
    before = {"dense_macs": 0, "n_tile_launches": 0}
    if form == "store":   # K holds other data; the reset leaves the zeros to the launch, which stores its sums
        assert not compact
        e.load_sequences(c["tok"], c["off"], N, 0)
        e.accumulate(c["combos"][1:4])
        before = e.stats()
        assert e.get_counts().any()
        e.reset_counts()
        e.accumulate(c["combos"])
        e.finalize()
    else:
        e.compute(c["tok"], c["off"], N, 0)
    st = e.stats()
    got = e.get_counts()
    e.close()
    assert st["path_used"] == 1 and st["n_tile_launches"] - before["n_tile_launches"] == 1
    assert st["key_space"] == geo["V"]
    bad = np.flatnonzero(got != c["want"])
    assert bad.size == 0, "%d cells differ, the first at %d: %d against %d" % (bad.size, bad[0], got[bad[0]], c["want"][bad[0]])
    if compact:
        assert 0 < st["compact_keys_avg"] <= geo["V"]
    else:
        macs = st["dense_macs"] - before["dense_macs"]
        expected = cases.expected_macs(c["F"], tiles, remainder=profile)
        print("dense_macs %d, expected %d" % (macs, expected))
        assert macs == expected


def check_skip_test_block(make, port, n_train, N=300):
    """Case B with the test x test tiles off the diagonal left out: first_test_tile = ceil(n_train / 128). Computed cells equal
    the oracle, skipped tiles stay zero, dense_macs counts the tiles of the launch."""
    c = once(port, "B", N)
    tuning = dict(cases.FORMS["one"], compact=0)
    geo = cases.geometry(c["sigma"], c["k"], len(c["combos"]), 1, 0)
    ftt = (n_train + cases.TILE - 1) // cases.TILE
    assert ftt == {127: 1, 128: 1, 129: 2}[n_train]
    tiles = cases.tiles_of(N, ftt)
    assert len(tiles) == {1: 5, 2: 6}[ftt]
    cases.assert_edges(c, geo, "one", tiles)
    e = make(c["g"], c["m"], path=1, profile=True, tuning=tuning, skip_test_block=True)
    e.compute(c["tok"], c["off"], n_train, N - n_train)
    st = e.stats()
    got = tri_to_square(e.get_counts(), N)
    e.close()
    want = tri_to_square(c["want"], N)
    i, j = np.tril_indices(N)
    kept = np.array([(a, b) in set(tiles) for a, b in zip((i // cases.TILE).tolist(), (j // cases.TILE).tolist())])
    assert st["path_used"] == 1 and st["n_tile_launches"] == 1
    assert np.array_equal(got[i[kept], j[kept]], want[i[kept], j[kept]])
    assert not got[i[~kept], j[~kept]].any()
    assert kept.all() if ftt == 2 else want[i[~kept], j[~kept]].any()
    assert st["dense_macs"] == cases.expected_macs(c["F"], tiles)


# ---- the yardstick itself ------------------------------------------------------------------------------------------------
def test_geometry_of_the_cases(port):
    """The table of the cases: keys, rows, mask words, combinations and chunk_slots."""
    want = {"A": (256, 32, 1, 1820, 1024), "B": (4096, 512, 16, 84, 64), "C": (16384, 2048, 64, 36, 16), "D": (243, 31, 1, 126, 1024),
            "E": (625, 79, 3, 70, 64), "F": (3125, 391, 13, 126, 36), "G": (256, 32, 1, 70, 1024), "H": (1024, 128, 4, 6, 256)}
    for name, spec in cases.CASES.items():
        n = port.num_combos(spec["g"], spec["m"])
        geo = cases.geometry(spec["sigma"], spec["g"] - spec["m"], n, 1, spec["compact"])
        assert (geo["V"], geo["Vq8"], geo["nst"], n, geo["chunk_slots"]) == want[name], name
    assert cases.geometry(4, 7, 36, 2, 0)["slots_per_split"] == 18


def test_flagged_rows_against_counting_by_hand():
    """Poly-4 over four letters at k = 3 is key 63, dword row 7; 20 windows of it are flagged, 15 are not; a panel past the end
    of the sequences has none; 256 windows are refused."""
    pos = [np.array([0, 1, 3]), np.array([1, 2, 3])]
    X = np.ones((70, 23), dtype=np.int32)
    X[65] = 4
    X[2, :18] = [1, 2, 3] * 6   # keys of period 3, five windows each, then two more keys once each: nothing above 15
    F = cases.flagged_rows(X, 4, 4, pos)
    assert F.shape == (2, 2, 8)
    assert F[0].sum() == 2 and F[0, :, 0].all()   # poly-1: key 0, row 0, in both combinations
    assert F[1].sum() == 4 and F[1, :, 0].all() and F[1, :, 7].all()   # sequences 64..69: poly-1 and the one poly-4
    F = cases.flagged_rows(X[:, :18], 4, 4, pos)   # 15 windows: nothing above 15
    assert not F.any()
    with pytest.raises(ValueError):
        cases.flagged_rows(np.ones((3, 259), dtype=np.int32), 4, 4, pos)
    assert cases.tiles_of(300, 1) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 2)] and len(cases.tiles_of(130)) == 3


def test_a_case_off_its_edge_fails_at_the_precondition(port):
    """Without its low-complexity sequences, or launched under chunk_slots, a case fails before any engine is asked."""
    for name in ("D", "E", "G"):
        c = cases.build(port, name, 130, low_complexity=False)
        geo = cases.geometry(c["sigma"], c["k"], len(c["combos"]), 1, c["compact"])
        with pytest.raises(AssertionError):
            cases.assert_edges(c, geo, "one", cases.tiles_of(130))
    c = once(port, "E", 130)
    with pytest.raises(AssertionError, match="slots_per_split 35 against chunk_slots 64"):
        cases.assert_edges(dict(c, cross=("atomics",)), cases.geometry(5, 4, 70, 2, 1), "atomics", cases.tiles_of(130))


# ---- the emulator runs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


@pytest.mark.parametrize("name,form", [("A", "one"), ("B", "one"), ("C", "staged")])
def test_second_chunk_on_one_tile(make_emu, port, name, form):
    check_case(make_emu, port, name, form, N=66, profile=False)


@pytest.mark.parametrize("form", ["one", "atomics", "staged", "store"])
def test_dense_macs_with_flagged_rows_in_four_mask_words(make_emu, port, form):
    check_case(make_emu, port, "H", form)


@pytest.mark.parametrize("form", ["one", "store"])
def test_stage_tail_of_15_rows(make_emu, port, form):
    check_case(make_emu, port, "D", form)


@pytest.mark.parametrize("form", ["one", "atomics", "staged"])
def test_compact_row_slots_cap_and_one_sided_rows(make_emu, port, form):
    check_case(make_emu, port, "E", form)


def test_compact_chunk_below_the_cap_on_one_tile(make_emu, port):
    check_case(make_emu, port, "F", "one", N=66)


@pytest.mark.parametrize("form", ["one", "staged"])
def test_two_and_three_hi_plane_rounds(make_emu, port, form):
    check_case(make_emu, port, "G", form)
