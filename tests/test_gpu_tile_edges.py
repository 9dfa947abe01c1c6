"""The dense tile kernels at the edges of their loops on the MI355X: the product library through the C ABI, the check functions
of tests/test_emu_tile_edges.py (which state the contract) over the whole matrix of cases and launch forms — the real
direct-to-LDS loads, their waits and the clamped buffer descriptor across a mask-chunk restart and a short final stage, which
the emulator replaces with plain copies. Every case is N = 130 sequences (three tiles, the last with two real rows); the
largest is 36 combinations x 2048 dword rows."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_emu_tile_edges import check_case, check_skip_test_block  # noqa: E402

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("profile", [True, False], ids=["profile", "plain"])
@pytest.mark.parametrize("form", ["one", "atomics", "staged", "store"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_mask_chunk_crossing(make, port, name, form, profile):
    """256, 4096 and 16,384 keys: 1820 combinations against a chunk of 1024, 84 against 64, 36 (18 a split) against 16. In
    profile mode (dense_macs with the remainder rows; the engine synchronises around its launches) and as the product runs."""
    check_case(make, port, name, form, profile=profile)


@pytest.mark.parametrize("form", ["one", "atomics", "staged", "store"])
def test_dense_macs_with_flagged_rows_in_four_mask_words(make, port, form):
    check_case(make, port, "H", form)


@pytest.mark.parametrize("form", ["one", "atomics", "staged", "store"])
def test_stage_tail_of_15_rows(make, port, form):
    check_case(make, port, "D", form)


@pytest.mark.parametrize("form", ["one", "atomics", "staged"])
def test_compact_row_slots_cap_and_one_sided_rows(make, port, form):
    check_case(make, port, "E", form)


@pytest.mark.parametrize("form", ["one", "atomics", "staged"])
def test_compact_chunk_below_the_cap(make, port, form):
    check_case(make, port, "F", form)


@pytest.mark.parametrize("form", ["one", "atomics", "staged", "store"])
def test_two_and_three_hi_plane_rounds(make, port, form):
    check_case(make, port, "G", form)


@pytest.mark.parametrize("n_train", [127, 128, 129])
def test_skip_test_block_at_the_tile_edges(make, port, n_train):
    check_skip_test_block(make, port, n_train)
