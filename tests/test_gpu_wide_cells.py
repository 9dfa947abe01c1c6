"""Cells of K beyond 32 bits, on the MI355X: the product library through the C ABI (``native.Engine``), ``get_counts()``
compared bit for bit with the 64-bit reference of tests/wide_cells_cases.py, at the two host-side bounds that keep the 32-bit
accumulators of the dataflows from wrapping —

    dense   fsk_engine_dense.hip:96, 106, 177 (accumulate_dense)   by_overflow = (2^32 - 1) // maxW^2 combos a tile launch
    sparse  fsk_engine_sparse.hip:963 (accumulate_sparse)          by_cells = max(1, (2^32 - 1) // maxW^2) combos a batch

— and beyond the second one, where a single combination puts more than 2^32 into a cell (a sequence of 65,536 windows or
more) and the entries that do so add into K themselves (fsk_sparse_kernels.inc:sx_wide_entry). The checks are those of
tests/test_emu_wide_cells.py, which states the contract and proves the reference against the oracle; here every tuning,
every way of calling and DENSE_WRAP run, on the real wave intrinsics and LDS atomics.

Variance mode is out of scope: its by-slot triangles are u32 / u16 by design, like the reference's ``unsigned int Ks``,
which wrap (test_variance_mode_count_above_255 stays as it is)."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import wide_cells_cases as cases  # noqa: E402
from test_emu_wide_cells import (check_batch_bound, check_dense_chunks, check_dense_chunks_revcomp, check_dense_wrap,  # noqa: E402
                                 check_wide)

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


# every form the sparse update stage can take, every partner format of sx_expand_descriptors, several parts a band (K
# written with atomics), and the word form whose parts do not cut a cell's words
SPARSE_TUNINGS = cases.BASE_TUNINGS + cases.DESC_TUNINGS + [cases.PARTS_TUNING, cases.WORDS_TUNING]
WIDE_CASES = {"wide_one_combo": cases.wide_one_combo, "wide_edge_65536": lambda: cases.wide_edge(65536),
              "wide_edge_65537": lambda: cases.wide_edge(65537)}


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip_test_block"])
@pytest.mark.parametrize("tuning", SPARSE_TUNINGS, ids=cases.tuning_id)
@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_sparse_one_combination_beyond_32_bits(make, name, tuning, skip):
    """WIDE_ONE_COMBO (homopolymers of 70,000 and 66,000 windows among 300 sequences: cells of 2 x 70000^2, 2 x 66000^2 and
    2 x 70000 x 66000) and WIDE_EDGE (one homopolymer of 65,536 / 65,537 windows: the first count whose c (c - 1) does not
    fit 32 bits). Pins ``by_cells`` of fsk_engine_sparse.hip:accumulate_sparse, whose max(1, .) holds nothing here, and
    ``cwide`` of fsk_engine_sparse.hip:sx_batch_begin, which does: see check_wide."""
    check_wide(make, name, WIDE_CASES[name](), tuning, skip)


@pytest.mark.parametrize("how", ["whole", "three calls", "row bands"])
@pytest.mark.parametrize("tuning", cases.BASE_TUNINGS, ids=cases.tuning_id)
def test_sparse_batch_bound(make, tuning, how):
    """BATCH_BOUND: 15 combinations where a batch may hold ten. Pins ``by_cells`` inside ``batch_combos`` of
    fsk_engine_sparse.hip:accumulate_sparse: see check_batch_bound."""
    check_batch_bound(make, tuning, how)


@pytest.mark.parametrize("tuning", [({"sparse_exact_lanes": 2}, 0, None), ({"sparse_exact_lanes": 2, "sparse_desc": 1}, 0, 1)], ids=cases.tuning_id)
def test_sparse_batch_bound_in_two_lanes(make, tuning):
    """The same with the batches of a call alternating between two lanes (tuning sparse_exact_lanes=2): the lanes and the
    cell bound meet in ``batch_combos`` of fsk_engine_sparse.hip:accumulate_sparse, which evens out what is left over an
    even number of batches and may never hand out more than ``by_cells``. (No run of this file sets sparse_batch_records:
    the record cap is far away, ``by_cells`` is what binds.)"""
    check_batch_bound(make, tuning, "whole")


DENSE_TUNINGS = [{}, {"tile_splits": 1}, {"dense_small": 1}, {"dense_small": 1, "tile_splits": 5}]


@pytest.mark.parametrize("tuning", DENSE_TUNINGS, ids=lambda t: cases.tuning_id((t,)))
def test_dense_chunk_loop_takes_a_second_trip(make, tuning):
    """DENSE_CHUNKS: 70 combinations at 53 a tile launch. Pins ``by_overflow`` and the chunk loop of
    fsk_engine_dense.hip:accumulate_dense: see check_dense_chunks."""
    check_dense_chunks(make, tuning)


@pytest.mark.parametrize("tuning", DENSE_TUNINGS, ids=lambda t: cases.tuning_id((t,)))
def test_dense_chunk_loop_reverse_complement(make, tuning):
    """DENSE_CHUNKS in reverse-complement mode: maxW counts both strands, ``by_overflow`` of
    fsk_engine_dense.hip:accumulate_dense is 13 and the call takes six tile launches: see check_dense_chunks_revcomp."""
    check_dense_chunks_revcomp(make, tuning)


def test_dense_registers_would_wrap_without_chunks(make):
    """DENSE_WRAP: all 1001 combinations at two a tile launch (501 launches), a diagonal cell of 7,965,024,256. Pins
    ``by_overflow`` of fsk_engine_dense.hip:accumulate_dense: see check_dense_wrap."""
    check_dense_wrap(make, 1001)
