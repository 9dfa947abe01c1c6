"""The in-place form of the packed shift corrections on the MI355X: the product library through the C ABI, the check functions
of tests/test_emu_dense_shift_inplace.py (which state the contract) — the LDS atomic adds of up to 8 lanes on one dword, the
barriers around them, the direct-to-LDS load of the next chain's planes in flight under a whole chain, which the emulator replaces
with plain C++ run thread by thread. All 495 combinations of (g = 12, m = 8), and the chain cut of (g = 14, m = 10); every case
with dense_shift_inplace = 1 and = 0."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
import dense_shift_inplace_cases as inplace  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift_inplace import (check_crossing, check_cut, check_every_nibble, check_moves_and_stays,  # noqa: E402
                                          check_ragged)

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


@pytest.mark.parametrize("form", inplace.FORMS)
def test_every_nibble_position(make, port, form):
    check_every_nibble(make, port, ALL, form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_moves_and_stays(make, port, form):
    check_moves_and_stays(make, port, ALL, form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_crossing_falls_back(make, port, form):
    check_crossing(make, port, ALL, form, packed.CROSSING)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_peak_of_15_stays_in_place(make, port, form):
    check_crossing(make, port, ALL, form, inplace.PEAK15)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_one_window_and_ragged(make, port, form):
    check_ragged(make, port, ALL, form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_chain_cut_hands_over(make, port, form):
    check_cut(make, port, form)


@pytest.mark.parametrize("form", inplace.FORMS)
def test_two_calls_on_one_load(make, port, form):
    check_every_nibble(make, port, ALL, form, calls=2)
