"""The front end of the sparse dataflow at the edges of its digits, tiles and record types on the MI355X: the product library
through the C ABI, the check functions of tests/test_emu_sort_edges.py (which state the contract) at the same sizes and over the
whole sweeps — what the emulator replaces is what runs here: the wave64 ballot matching of k_sx_scatter (sbfe1, and_xnor, mbcnt),
its volatile per-wave LDS counters, the DPP scans of the segment kernels and the 16-byte loads of k_sx_hist. The largest case is
25 slots of 8193 records."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import sort_edges_cases as cases  # noqa: E402
from test_emu_sort_edges import (H1_CASES, check_a, check_b, check_c, check_d, check_e, check_f, check_g,  # noqa: E402
                                 check_h_homopolymers, check_h_k1, check_i)

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


@pytest.mark.parametrize("k", cases.A_KS)
def test_widths_in_32_bit_records(make, monkeypatch, port, k):
    """Digit widths 1..8 (NB 4..8), one to four passes, 32 record bits exactly at k = 30; tps = 5, one record in the last tile."""
    check_a(make, monkeypatch, port, k)


@pytest.mark.parametrize("k,m", [(k, 1) for k in cases.B_KS] + [(62, 3)])
def test_widths_in_64_bit_records(make, monkeypatch, port, k, m):
    """Four to eight passes; 64 record bits exactly at k = 62; g = 65 gathers its symbols (no window array)."""
    check_b(make, monkeypatch, port, k, m)


@pytest.mark.parametrize("sigma,k", cases.C_CASES)
def test_widths_in_128_bit_records(make, monkeypatch, port, sigma, k):
    check_c(make, monkeypatch, port, sigma, k)


@pytest.mark.parametrize("sigma,k", cases.D_CASES)
def test_mixed_radix_keys(make, monkeypatch, port, sigma, k):
    check_d(make, monkeypatch, port, sigma, k)


@pytest.mark.parametrize("sigma,k,N,nfeat", cases.E_CASES)
def test_record_type_boundaries(make, monkeypatch, port, sigma, k, N, nfeat):
    check_e(make, monkeypatch, port, sigma, k, N, nfeat)


@pytest.mark.parametrize("extract_slots", [1, 4])
@pytest.mark.parametrize("N,nfeat", [(16, n) for n in cases.F_NFEAT] + [(1, 1), (1, 2)])
def test_tile_tails_and_slot_alignment(make, monkeypatch, port, N, nfeat, extract_slots):
    check_f(make, monkeypatch, port, N, nfeat, extract_slots)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip_test_block"])
@pytest.mark.parametrize("form", sorted(cases.FORMS))
def test_buckets_across_tiles(make, monkeypatch, port, form, skip):
    check_g(make, monkeypatch, port, form, skip)


@pytest.mark.parametrize("n_train,form,skip", H1_CASES)
def test_entry_across_three_segment_tiles(make, monkeypatch, port, n_train, form, skip):
    check_h_homopolymers(make, monkeypatch, port, n_train, form, skip)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip_test_block"])
@pytest.mark.parametrize("name", sorted(cases.K1_CASES))
def test_heads_on_segment_tile_edges(make, monkeypatch, port, name, skip):
    check_h_k1(make, monkeypatch, port, name, skip)


@pytest.mark.parametrize("share", [18, 19])
def test_shared_positions_across_presort_width(make, monkeypatch, port, share):
    check_i(make, monkeypatch, port, share)
