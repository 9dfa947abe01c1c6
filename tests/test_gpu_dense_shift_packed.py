"""The packed shift corrections on the MI355X: the product library through the C ABI, the check functions of
tests/test_emu_dense_shift_packed.py (which state the contract) over all 495 combinations of (g = 12, m = 8) and the chain cut
of (g = 14, m = 10) — the real direct-to-LDS loads of key-major planes, per-lane keys into swizzled LDS rows, the byte-select
adds and the signed 64-bit atomic flush, which the emulator replaces with plain copies and plain C++. Every case is N = 130
sequences (three tiles, the last with two real rows)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_shift_cases as cases  # noqa: E402
from test_emu_dense_shift import positions  # noqa: E402
from test_emu_dense_shift_packed import check_both_kernels, check_chain_cut, check_crossing, check_extremes, check_fallback  # noqa: E402

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


def test_byte_range_at_its_ends(make, port):
    check_extremes(make, port, ALL, "gpu")


@pytest.mark.parametrize("name", ["uniform", "ragged"])
def test_both_kernels(make, port, name):
    check_both_kernels(make, port, name, ALL)


def test_chain_cut(make, port):
    check_chain_cut(make, port)


def test_flagged_steps_inside_a_long_chain(make, port):
    check_crossing(make, port, ALL)


def test_planes_do_not_fit(make, port, capfd):
    check_fallback(make, port, ALL, capfd)
