"""The dense dataflow by shift classes (fsk_engine_dense_shift.hip): one weighted Gram product per chain of combinations that
differ by a shift of all kept positions, the other members by edge lookups. tests/dense_shift_cases.py holds the inputs, the
plan and the numpy yardstick of the identity; the check functions here state the contract and tests/test_gpu_dense_shift.py
runs them on the device over all 495 combinations. ``make(g, m, **kw)`` creates an engine; no expected value comes from one.

Every case is N = 130 (three tiles, the last with two real rows), four letters, g = 12, m = 8, with tile_splits=1 and
dense_shift=1. Counts are compared bit for bit with the CPU oracle, and ``dense_macs`` must equal 8 * 128^2 * tiles * 32 rows *
chain bases: that the path ran, and how many products it did.

The emulator runs the direct-to-LDS loads as plain copies and a wave's key broadcast (v_readlane) as a wave collective of 64
fibers, so it affords three classes and two lone combinations (27 combinations, 22 derived steps) on three tiles; all 495, the
combination lists of 100 and the batch that leaves for the sparse dataflow run on the device only."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402

_ONCE = {}


def once(key, build):
    """Inputs and yardsticks computed once per session and shared: read-only."""
    if key not in _ONCE:
        _ONCE[key] = build()
    return _ONCE[key]


def positions(port):
    return once("positions", lambda: cases.all_positions(port))


def inputs(port, name, ids):
    """(tokens, offsets, the oracle's counts over ``ids``) of the named sequences."""
    from oracle import loader

    def build():
        seqs = {"uniform": cases.uniform, "ragged": cases.ragged, "long": cases.long_homopolymer}.get(name) or (lambda: cases.planted(name))
        seqs = seqs()
        tok, off = loader.flatten(seqs)
        want = port.raw_counts(tok, off, cases.G, cases.M, np.asarray(ids, dtype=np.int32), threads=4)[0]
        for a in (tok, off, want):
            a.setflags(write=False)
        return seqs, tok, off, want
    return once((name, tuple(int(c) for c in ids)), build)


def differ(got, want):
    bad = np.flatnonzero(got != want)
    return "" if bad.size == 0 else "%d cells differ, the first at %d: %d against %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


def check_shift(make, port, name, ids, twice=False, tuning=None):
    """One call over ``ids`` after reset_counts (the storing first flush); ``twice``: a second call on top (adding flushes) gives
    exactly twice the counts. dense_macs with the chain bases the case module plans."""
    ids = np.asarray(ids, dtype=np.int32)
    pos = positions(port)
    bases = len(cases.chains([pos[c] for c in ids]))
    seqs, tok, off, want = inputs(port, name, ids)
    e = make(cases.G, cases.M, path=1, tuning=dict(cases.TUNING, **(tuning or {})))
    e.load_sequences(tok, off, cases.N, 0)
    e.accumulate(ids[:1])          # K holds other data; the reset leaves the zeros to the launch, which stores
    before = e.stats()
    e.reset_counts()
    e.accumulate(ids)
    st = e.stats()
    got = e.get_counts()
    assert st["path_used"] == 1
    d = {k: st[k] - before[k] for k in ("dense_macs", "n_tile_launches", "count_launches")}
    print("%s, %d combinations: %d chain bases, dense_macs %d" % (name, len(ids), bases, d["dense_macs"]))
    assert d == {"dense_macs": cases.expected_macs(cases.n_tiles(), bases), "n_tile_launches": 1, "count_launches": 1}, d
    assert not differ(got, want), differ(got, want)
    if twice:
        e.accumulate(ids)
        e.finalize()
        got2 = e.get_counts()
        assert e.stats()["dense_macs"] - st["dense_macs"] == cases.expected_macs(cases.n_tiles(), bases)
        assert not differ(got2, 2 * want), differ(got2, 2 * want)
    e.close()
    return bases


def check_planted(make, port, which, ids):
    """Counts of 79 (and 40 / 39 of the period-2 sequences): the hi-plane lookups on the row side only, the column side only
    and both, in tile (1, 0) and in a diagonal tile. From numpy: the flagged panels are the ones the case names."""
    pos = positions(port)
    seqs = inputs(port, which, ids)[0]
    panels, top = once(("high", which), lambda: cases.high_panels(seqs, [pos[c] for c in (0, 100, 494)]))
    assert top == 79 and panels == {"rows": {2}, "cols": {0, 1}, "both": {0, 1, 2}}[which]
    return check_shift(make, port, which, ids)


def check_row_bands(make, port, ids):
    """accumulate_rows over [0, 128) and [128, 130) against one call: identical triangles; the second band reuses the panels and
    the edge keys."""
    ids = np.asarray(ids, dtype=np.int32)
    pos = positions(port)
    bases = len(cases.chains([pos[c] for c in ids]))
    seqs, tok, off, want = inputs(port, "ragged", ids)
    e = make(cases.G, cases.M, path=1, tuning=cases.TUNING)
    e.load_sequences(tok, off, cases.N, 0)
    e.reset_counts()
    e.accumulate(ids)
    whole = e.get_counts()
    st0 = e.stats()
    e.reset_counts()
    e.accumulate_rows(ids, 0, 128)
    e.accumulate_rows(ids, 128, cases.N)
    e.finalize()
    st = e.stats()
    bands = e.get_counts()
    e.close()
    assert not differ(whole, want), differ(whole, want)
    assert np.array_equal(bands, whole)
    assert st["count_launches"] - st0["count_launches"] == 1 and st0["count_launches"] == 1
    assert st["n_tile_launches"] - st0["n_tile_launches"] == 2
    assert st["dense_macs"] - st0["dense_macs"] == cases.expected_macs(cases.n_tiles(), bases)   # one tile, then two


def check_old_path(make, port, ids, how):
    """dense_shift=1 on a call that is not eligible, dense_shift=-1 and the default at N = 130: the old path (dense_macs with every
    combination of the call) and the oracle's counts."""
    import wildcard_cases
    from oracle import loader
    ids = np.asarray(ids, dtype=np.int32)
    kw, tuning, compact = {}, dict(cases.TUNING), False
    seqs = [list(s) for s in cases.ragged()]
    if how == "revcomp":
        kw["revcomp"] = wildcard_cases.DNA
    elif how == "wildcards":
        kw["wildcards"] = [wildcard_cases.N_]
        for i, p in ((10, 0), (30, 20), (100, 39), (110, 15)):   # (sequences of 40: each keeps a window)
            assert len(seqs[i]) == 40
            seqs[i][p] = wildcard_cases.N_
    elif how == "compact":
        seqs[20][7] = seqs[90][30] = 5   # a rare fifth symbol: 625 keys, key compaction
        compact = True
    elif how == "splits":
        tuning["tile_splits"] = 2
    elif how == "never":
        tuning["dense_shift"] = -1
    elif how == "default":
        tuning = {"tile_splits": 1}
    else:
        raise ValueError(how)
    tok, off = loader.flatten(seqs)
    if how == "revcomp":
        want = wildcard_cases.brute_counts(port, seqs, (), cases.G, cases.M, ids, comp=wildcard_cases.DNA)
    elif how == "wildcards":
        want = wildcard_cases.brute_counts(port, seqs, (wildcard_cases.N_,), cases.G, cases.M, ids)
    else:
        want = port.raw_counts(tok, off, cases.G, cases.M, ids, threads=4)[0]
    e = make(cases.G, cases.M, path=1, tuning=tuning, **kw)
    e.load_sequences(tok, off, cases.N, 0)
    e.reset_counts()
    e.accumulate(ids)
    st = e.stats()
    got = e.get_counts()
    e.close()
    assert st["path_used"] == 1 and st["n_tile_launches"] == 1
    assert not differ(got, want), differ(got, want)
    if compact:
        assert st["key_space"] == 625 and 0 < st["compact_keys_avg"] <= 625
    else:
        assert st["key_space"] == cases.V and st["dense_macs"] == cases.expected_macs(cases.n_tiles(), len(ids))


# ---- the yardstick itself ---------------------------------------------------------------------------------------------------
def test_the_classes_of_config_5(port):
    """495 kept-position sets of (g = 12, k = 4): 165 classes of 13 - span shifts each; 330 derived steps."""
    ch = cases.chains(positions(port))
    sizes = {}
    for c in ch:
        sizes[len(c)] = sizes.get(len(c), 0) + 1
    assert sizes == cases.CLASS_SIZES and len(ch) == 165 and sum(len(c) - 1 for c in ch) == 330
    ls = cases.lists(positions(port))
    pos = positions(port)
    assert len(cases.chains([pos[c] for c in ls["gap"]])) == 2 and len(cases.chains([pos[c] for c in ls["repeated"]])) == 2
    assert len(cases.chains([pos[c] for c in ls["subset"]])) == len(cases.chains([pos[c] for c in ls["shuffled"]])) < 100
    assert len(cases.chains([pos[c] for c in ls["one"]])) == 1


def test_identity_against_the_direct_sum_and_the_oracle(port):
    """Ragged lengths: L < g (no window), L = g, sequences with fewer windows than a class has shifts, planted repeats. The
    oracle, like the engine (FSK_ESHORT) and the reference, refuses a sequence shorter than g: it is asked without that one."""
    from oracle import loader
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [rng.integers(1, 5, size=L).tolist() for L in (5, 12, 13, 14, 19, 20, 40, 33, 12, 16)] + [[2] * 30, [1, 3] * 12]
    pos = positions(port)
    ls = cases.lists(pos)
    for ids in (np.arange(cases.N_COMBOS), ls["shuffled"], ls["repeated"], ls["gap"]):
        plist = [pos[c] for c in ids]
        direct = cases.direct_sum(seqs, plist)
        assert np.array_equal(cases.identity_sum(seqs, plist), direct)
        assert len(seqs[0]) < cases.G and not direct[0].any() and not direct[:, 0].any()
        tok, off = loader.flatten(seqs[1:])
        want = port.raw_counts(tok, off, cases.G, cases.M, np.asarray(ids, dtype=np.int32))[0]
        assert np.array_equal(direct[1:, 1:][np.tril_indices(len(seqs) - 1)].astype(np.uint64), want)


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


def test_emu_a_sequence_without_a_window_is_refused(make_emu):
    """L = 5 < g: the load fails as the reference does, so no engine case can hold such a sequence (the edge-key kernel's
    delta = sigma = 0 for it serves the padding rows of the last panel)."""
    from fastsk_amd import _native
    from oracle import loader
    seqs = cases.ragged()
    seqs[3] = seqs[3][:5]
    tok, off = loader.flatten(seqs)
    e = make_emu(cases.G, cases.M, path=1, tuning=cases.TUNING)
    with pytest.raises(_native.FskError):
        e.load_sequences(tok, off, cases.N, 0)
    e.close()


def test_emu_ragged_lengths_store_then_add(make_emu, port):
    ids = cases.small_list(positions(port))
    assert check_shift(make_emu, port, "ragged", ids, twice=True) == 5


@pytest.mark.parametrize("which", ["rows", "cols", "both"])
def test_emu_counts_above_15(make_emu, port, which):
    check_planted(make_emu, port, which, cases.small_list(positions(port))[:9])


@pytest.mark.parametrize("name", ["one", "gap", "repeated"])
def test_emu_lists(make_emu, port, name):
    check_shift(make_emu, port, "ragged", cases.lists(positions(port))[name])


def test_emu_row_bands(make_emu, port):
    check_row_bands(make_emu, port, cases.small_list(positions(port)))


@pytest.mark.parametrize("how", ["revcomp", "wildcards", "compact", "splits", "never", "default"])
def test_emu_old_path(make_emu, port, how):
    check_old_path(make_emu, port, cases.small_list(positions(port)), how)
