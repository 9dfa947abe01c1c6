"""Cells of K beyond 32 bits, on the CPU: the engine's HIP source compiled against tests/emu/hip_emu.h must give the exact
64-bit sum in every form of both dataflows where a launch's or a batch's share of a cell comes up to — or, for one
combination alone, passes — what its 32-bit accumulators hold. The contract (include/fastsk_amd.h:fsk_get_counts): the
integer triangle of the exact and skip-variance modes is the exact 64-bit sum for every form and every tuning. The cases and
the 64-bit reference are tests/wide_cells_cases.py (``port.raw_counts`` wraps mod 2^32 within a call: it only PROVES the
reference here, one combination at a time); the checks below are shared with tests/test_gpu_wide_cells.py, which runs all of
them on the device.

Variance mode is out of scope: its by-slot triangles are u32 / u16 by design, like the reference's ``unsigned int Ks``,
which wrap (test_variance_mode_count_above_255 stays as it is).

Cut to what the emulator finishes in about two minutes — dropped here for time and run on the device only: DENSE_WRAP (501
tile launches); of WIDE_ONE_COMBO every tuning but the default, descriptors and the two-level blocks, and its skip_test_block
runs; of BATCH_BOUND every tuning but the default and blocks + descriptors, each in one call only; of DENSE_CHUNKS every
tuning but the default (one call; two calls) and tile_splits=1 (one call; row bands), and reverse-complement mode. (Measured:
about two and a half minutes, 60 s of them the five emulated passes of DENSE_CHUNKS.)"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import wide_cells_cases as cases  # noqa: E402


@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


# ---- the checks, shared with tests/test_gpu_wide_cells.py: ``make(g, m, **kw)`` creates an engine -------------------------
def loaded(make, case, path, tuning, n_train=None, **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(case["seqs"])
    n = len(case["seqs"])
    e = make(case["g"], case["m"], path=path, tuning=dict(tuning), **kw)
    e.load_sequences(tok, off, n if n_train is None else n_train, 0 if n_train is None else n - n_train)
    return e


def assert_forced(st, form, desc, what):
    assert st["path_used"] == 2, what
    assert form is None or st["sparse_form"] == form, (what, st["sparse_form"])
    assert desc is None or st["sparse_desc"] == desc, (what, st["sparse_desc"])


def assert_kept_cells(got, want, n, n_train):
    """skip_test_block: every cell whose column is a train sequence or that lies on the diagonal equals the reference's; the
    rest is zero in the engine and is not all zero in the reference."""
    a, b = np.tril_indices(n)
    keep = (b < n_train) | (a == b)
    assert keep.mean() >= 0.5
    assert np.array_equal(got[keep], want[keep]) and not got[~keep].any() and want[~keep].any()


def check_wide(make, key, case, tuning, skip):
    """One combination alone puts 2^32 and more into a cell (a sequence of 65,536 windows or more). Pins
    fsk_engine_sparse.hip:963 (accumulate_sparse), ``by_cells = max(1, (2^32 - 1) / maxW^2)``: the max(1, .) holds nothing, what
    does is ``cwide = (2^32 - 1) / maxW`` of fsk_engine_sparse.hip:300 (sx_batch_begin) — an entry of a larger multiplicity adds its
    products into K as 64-bit atomics (fsk_sparse_kernels.inc:sx_wide_entry) whatever form the update stage takes. The form
    and the descriptors that the tuning forces must be the ones the batch took: the update streams stay in use."""
    tun, form, desc = tuning
    want, U, _ = cases.reference(key, case)
    n, ntr = len(case["seqs"]), case["n_train"]
    e = loaded(make, case, 2, tun, n_train=ntr if skip else None, skip_test_block=skip)
    e.accumulate(case["combos"])
    e.finalize()
    st = e.stats()
    assert_forced(st, form, desc, tun)
    assert st["max_windows"] == case["windows"][0] == cases.max_windows(case)
    got = e.get_counts()
    a, b = np.tril_indices(n)
    bad = np.nonzero((got != want) & ((b < ntr) | (a == b) | (not skip)))[0]   # (the figures first: what differs is a multiple of 2^32)
    print(key, tun, "skip_test_block" if skip else "whole", "cells that differ:", len(bad), "by",
          sorted(set((want[bad].astype(np.int64) - got[bad].astype(np.int64)).tolist()))[:4])
    if skip:
        assert_kept_cells(got, want, n, ntr)
        assert st["cell_updates"] < U
    else:
        assert np.array_equal(got, want)
        assert st["cell_updates"] == U
    e.close()


def check_batch_bound(make, tuning, how):
    """A batch of the sparse dataflow may hold (2^32 - 1) / maxW^2 = 10 of this case's 15 combinations and not one more.
    Pins fsk_engine_sparse.hip:963-975 (accumulate_sparse), ``by_cells`` inside ``batch_combos`` — in one call, in three calls (5 + 5
    + 5: below the bound) and as a row band."""
    tun, form, desc = tuning
    case = cases.batch_bound()
    want, U, _ = cases.reference("batch_bound", case)
    cases.batch_bound_preconditions(case, want)
    n, combos = len(case["seqs"]), case["combos"]
    e = loaded(make, case, 2, tun)
    if how == "whole":
        e.accumulate(combos)
    elif how == "three calls":
        for part in np.array_split(combos, 3):
            e.accumulate(part)
    else:   # (N < 128: the one band there is)
        e.accumulate_rows(combos, 0, n)
    e.finalize()
    st = e.stats()
    assert_forced(st, form, desc, (tun, how))
    assert st["max_windows"] == 20000 and st["combos_done"] == len(combos)
    assert np.array_equal(e.get_counts(), want), (tun, how)
    assert st["cell_updates"] == U, (tun, how)
    e.close()


def check_dense_chunks(make, tuning, stages=("whole", "row bands", "two calls")):
    """The chunk loop of the dense dataflow takes a second trip: 70 combinations at (2^32 - 1) / 9000^2 = 53 a tile launch.
    Pins fsk_engine_dense.hip:96-106 and 177 (accumulate_dense), ``by_overflow`` and ``for (int s = 0; s < n; s += chunk)``: several tile
    launches a call (with tile_splits=1 a storing one, then an adding one), U summed over the chunks, row bands that
    recount per chunk (``cached`` needs a single chunk), and the chunk boundary as two calls."""
    case = cases.dense_chunks()
    want, U, top = cases.reference("dense_chunks", case)
    cases.dense_chunks_preconditions(case, top)
    combos = case["combos"]
    e = loaded(make, case, 1, tuning, profile=True)
    before = e.stats()
    for stage in stages:
        e.reset_counts()
        if stage == "whole":
            e.accumulate(combos)
        elif stage == "row bands":
            for lo, hi in case["bands"]:
                e.accumulate_rows(combos, lo, hi)
        else:
            e.accumulate(combos[:53])
            e.accumulate(combos[53:])
        e.finalize()
        st = e.stats()
        assert st["path_used"] == 1 and st["max_windows"] == 9000
        d = {k: st[k] - before[k] for k in ("n_tile_launches", "count_launches", "cell_updates")}
        # (two chunks a call or a band; every band recounts both and counts their U again)
        times = 2 if stage == "row bands" else 1
        assert d == {"n_tile_launches": 2 * times, "count_launches": 2 * times, "cell_updates": U * times}, (tuning, stage, d)
        assert np.array_equal(e.get_counts(), want), (tuning, stage)
        before = st
    e.close()


def check_dense_chunks_revcomp(make, tuning):
    """The same input in reverse-complement mode: maxW counts both strands (18,000), so ``by_overflow`` of
    fsk_engine_dense.hip:96 (accumulate_dense) is (2^32 - 1) / 18000^2 = 13 and the 70 combinations take six tile launches. The
    reference is the fold of counts_by_definition on [X ; rc X]."""
    case = cases.dense_chunks()
    both = [list(s) for s in case["seqs"]] + [[cases.DNA[t] for t in reversed(s)] for s in case["seqs"]]
    _, _, top = cases.reference("dense_chunks both strands", dict(case, seqs=both))
    cases.dense_chunks_preconditions(case, 2 * top, strands=2)   # (a counter takes both strands: twice one strand's at most)
    want = cases.fold_by_definition(case["seqs"], cases.DNA, case["g"], case["m"], case["combos"])
    e = loaded(make, case, 1, tuning, profile=True, revcomp=cases.DNA)
    e.reset_counts()
    e.accumulate(case["combos"])
    e.finalize()
    st = e.stats()
    assert st["path_used"] == 1 and st["revcomp"] and st["max_windows"] == 18000
    assert st["n_tile_launches"] == 6 and st["count_launches"] == 6, (tuning, st["n_tile_launches"], st["count_launches"])
    assert np.array_equal(e.get_counts(), want), tuning
    e.close()


def check_dense_wrap(make, n_combos=1001):
    """(2^32 - 1) / 45000^2 = 2 combinations a tile launch while the long sequence's diagonal cell passes 2^32 over the call:
    without the chunks of fsk_engine_dense.hip:96-106 (accumulate_dense, ``by_overflow``) the u32 registers of the tile kernel
    would wrap."""
    case = cases.dense_wrap(n_combos)
    want, _, top = cases.reference(("dense_wrap", n_combos), case)
    cases.dense_wrap_preconditions(case, want, top)
    e = loaded(make, case, 1, {})
    e.accumulate(case["combos"])
    e.finalize()
    st = e.stats()
    assert st["path_used"] == 1 and st["max_windows"] == 45000
    assert st["n_tile_launches"] == (n_combos + 1) // 2
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- the reference --------------------------------------------------------------------------------------------------
REFERENCE_CASES = [("wide_one_combo", cases.wide_one_combo), ("wide_edge_65536", lambda: cases.wide_edge(65536)),
                   ("wide_edge_65537", lambda: cases.wide_edge(65537)), ("batch_bound", cases.batch_bound),
                   ("dense_chunks", cases.dense_chunks), ("dense_wrap", cases.dense_wrap)]


@pytest.mark.parametrize("name,build", REFERENCE_CASES, ids=[n for n, _ in REFERENCE_CASES])
def test_reference_is_the_oracle_modulo_2_32(port, name, build):
    """counts_by_definition against ``port.raw_counts``, combination by combination, cells modulo 2^32 and U as it stands:
    an independent implementation proves the reference even where it wraps. And every case is in the regime it is meant
    for, from the reference alone."""
    case = build()
    cases.check_reference(port, case)
    want, U, top = cases.reference(name if name != "dense_wrap" else ("dense_wrap", 1001), case)
    if name == "wide_one_combo":
        (a, b), (wa, wb) = case["rows"], case["windows"]
        one, _, _ = cases.counts_by_definition(case["seqs"], case["g"], case["m"], case["combos"][:1])
        assert int(one.max()) == wa * wa >= cases.U32   # (a single combination)
        assert (cases.cell(want, a, a), cases.cell(want, b, b), cases.cell(want, b, a)) == (2 * wa * wa, 2 * wb * wb, 2 * wa * wb)
        assert int(want.max()) == 9800000000
    elif name.startswith("wide_edge"):
        cases.wide_edge_preconditions(case)
        r, W = case["rows"][0], case["windows"][0]
        assert cases.cell(want, r, r) == W * W
    elif name == "batch_bound":
        cases.batch_bound_preconditions(case, want)
    elif name == "dense_chunks":
        cases.dense_chunks_preconditions(case, top)
    else:
        cases.dense_wrap_preconditions(case, want, top)


def test_the_oracle_wraps_within_a_call(port):
    """Why ``port.raw_counts`` is no reference for these cases: one call over the 15 combinations of BATCH_BOUND returns the
    wrapped cell, and 65,536 equal windows return 0."""
    from oracle import loader
    case = cases.batch_bound()
    tok, off = loader.flatten(case["seqs"])
    got, _, _ = port.raw_counts(tok, off, case["g"], case["m"], case["combos"], threads=1)
    assert cases.cell(got, 2, 2) == 6 * 10 ** 9 - cases.U32
    case = cases.wide_edge(65536)
    tok, off = loader.flatten(case["seqs"])
    got, _, _ = port.raw_counts(tok, off, case["g"], case["m"], case["combos"], threads=1)
    assert cases.cell(got, 3, 3) == 0


# ---- the engine under emulation -----------------------------------------------------------------------------------------
EDGE_TUNINGS = cases.BASE_TUNINGS + [cases.WORDS_TUNING]


@pytest.mark.parametrize("tuning", EDGE_TUNINGS, ids=cases.tuning_id)
@pytest.mark.parametrize("windows", [65536, 65537])
def test_emu_wide_edge(make_emu, windows, tuning):
    check_wide(make_emu, "wide_edge_%d" % windows, cases.wide_edge(windows), tuning, skip=False)


@pytest.mark.parametrize("tuning", [cases.BASE_TUNINGS[0], cases.DESC_TUNINGS[1], cases.BASE_TUNINGS[3]], ids=cases.tuning_id)
def test_emu_wide_one_combo(make_emu, tuning):
    check_wide(make_emu, "wide_one_combo", cases.wide_one_combo(), tuning, skip=False)


@pytest.mark.parametrize("tuning", [cases.BASE_TUNINGS[0], cases.BASE_TUNINGS[4]], ids=cases.tuning_id)
def test_emu_batch_bound(make_emu, tuning):
    check_batch_bound(make_emu, tuning, "whole")


@pytest.mark.parametrize("tuning,stages", [({}, ("whole", "two calls")), ({"tile_splits": 1}, ("whole", "row bands"))],
                         ids=["default", "tile_splits=1"])
def test_emu_dense_chunks(make_emu, tuning, stages):
    check_dense_chunks(make_emu, tuning, stages)
