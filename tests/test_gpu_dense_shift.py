"""The dense dataflow by shift classes on the MI355X: the product library through the C ABI, the check functions of
tests/test_emu_dense_shift.py (which state the contract) over all 495 combinations of (g = 12, m = 8) — the real direct-to-LDS
loads of whole panels, the wave-uniform key broadcasts and the signed 64-bit atomic flush, which the emulator replaces with
plain copies, fibers and plain adds. Every case is N = 130 sequences (three tiles, the last with two real rows)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
from test_emu_dense_shift import check_old_path, check_planted, check_row_bands, check_shift, differ, inputs, positions  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = np.arange(cases.N_COMBOS, dtype=np.int32)


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build_engine()    # no-op when fastsk_amd/lib/libfastsk_amd.so is current
    ge.build_bindings()
    from fastsk_amd import _native
    lib = _native.library()  # raises if the HIP library is missing: no fallback
    assert lib.device_count() >= 1
    return _native


@pytest.fixture(scope="module")
def make(native):
    return lambda g, m, **kw: native.Engine(g, m, **kw)


def test_all_combinations_store_then_add(make, port):
    """L = 40 uniform: after reset_counts the first flush stores; a second accumulate on top adds: exactly twice the counts."""
    assert check_shift(make, port, "uniform", ALL, twice=True) == 165


def test_ragged_lengths(make, port):
    """L = 12 .. 20 (one window to nine, the edges overlapping) and 40, in every tile and in the last tile's rows (L < g the
    engine refuses, as the reference does)."""
    assert check_shift(make, port, "ragged", ALL, twice=True) == 165


@pytest.mark.parametrize("which", ["rows", "cols", "both"])
def test_counts_above_15(make, port, which):
    assert check_planted(make, port, which, ALL) == 165


def test_a_count_above_255_leaves_for_the_sparse_dataflow(make, port):
    """One homopolymer of 289 windows: the batch goes to the sparse dataflow; the result is right and dense_macs is unchanged."""
    seqs, tok, off, want = inputs(port, "long", ALL)
    e = make(cases.G, cases.M, path=1, tuning=cases.TUNING)
    e.load_sequences(tok, off, cases.N, 0)
    before = e.stats()
    e.reset_counts()
    e.accumulate(ALL)
    e.finalize()
    st = e.stats()
    got = e.get_counts()
    e.close()
    assert st["max_windows"] == 289 and st["dense_macs"] == before["dense_macs"] == 0
    assert not differ(got, want), differ(got, want)


@pytest.mark.parametrize("name", ["subset", "shuffled", "one", "gap", "repeated"])
def test_lists(make, port, name):
    check_shift(make, port, "ragged", cases.lists(positions(port))[name])


def test_row_bands(make, port):
    check_row_bands(make, port, ALL)


@pytest.mark.parametrize("how", ["revcomp", "wildcards", "compact", "splits", "never", "default"])
def test_old_path(make, port, how):
    check_old_path(make, port, ALL, how)
