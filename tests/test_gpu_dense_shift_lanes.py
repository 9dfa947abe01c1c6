"""The lane layout of the packed shift corrections on the MI355X: the product library through the C ABI, the check functions of
tests/test_emu_dense_shift_lanes.py (which state the contract) — the direct-to-LDS loads, the per-lane keys into swizzled LDS
rows with the reads kept in flight, the half-select xors, the byte-select adds and the atomic flush, which the emulator replaces
with plain copies and plain C++. The class of nine shifts and all 495 combinations of (g = 12, m = 8), and the chain cut of
(g = 14, m = 10)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
import dense_shift_packed_cases as packed  # noqa: E402
from test_emu_dense_shift import positions  # noqa: E402
from test_emu_dense_shift_lanes import check_cut_full_row, check_every_position, check_hi_positions  # noqa: E402

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


def ids_of(port, which):
    return ALL if which == "all" else packed.span4(positions(port))


@pytest.mark.parametrize("which", ["span4", "all"])
def test_byte_ends_at_every_position(make, port, which):
    check_every_position(make, port, ids_of(port, which))


@pytest.mark.parametrize("which", ["span4", "all"])
def test_hi_pass_at_both_parities(make, port, which):
    check_hi_positions(make, port, ids_of(port, which))


def test_chain_cut_with_a_full_tile_row(make, port):
    check_cut_full_row(make, port)
