"""The update stage of the sparse dataflow at the edges of its slots, bands, parts and sub-bands on the MI355X: the product library
through the C ABI, the check functions of tests/test_emu_update_edges.py (which state the contract) over every case — what the
emulator replaces is what runs here: the LDS atomics that reserve k_sx_emit's slots, the global 64-bit atomics of a band of several
parts beside the plain read-modify-write of a band of one, the 16-byte loads of the streams and of the descriptors' partners with
their masked heads and tails, the 16-byte stores of the slot triangles. Group A's N >= 4095, which the emulator file leaves out,
runs here; the largest case is N = 8192, a triangle of 268 MB."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_emu_update_edges import (A_RUNS, C_CASES, D_FAR, D_STRADDLE, E_FORMATS, E_TARGETS, F_RUNS, VARIANTS, check_a, check_b_cmax,  # noqa: E402
                                   check_b_partners, check_b_skip, check_c, check_c_fullest, check_d_e0, check_d_far, check_d_straddle,
                                   check_e_desc, check_e_desc_bands, check_e_long_part, check_e_parts, check_e_streams, check_e_two_rounds,
                                   check_f, check_g_crossing, check_g_passes, check_g_records, check_g_tile, vid)

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


@pytest.mark.parametrize("N,variant,sparse_form", A_RUNS, ids=lambda v: vid(v) if isinstance(v, tuple) else str(v))
def test_band_plan_boundaries(make, monkeypatch, port, N, variant, sparse_form):
    check_a(make, monkeypatch, port, N, variant, sparse_form)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_entry_classes(make, monkeypatch, port, variant):
    check_b_partners(make, monkeypatch, port, variant)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip"])
@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("desc_min", [1, 16, 48])
def test_entry_classes_descriptor_threshold(make, monkeypatch, port, desc_min, pairs, skip):
    check_b_partners(make, monkeypatch, port, ("desc", pairs, skip), desc_min)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_multiplicity_at_cmax(make, monkeypatch, port, variant):
    check_b_cmax(make, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v[2]], ids=vid)
def test_test_rows_of_0_1_48_49_train_partners(make, monkeypatch, port, variant):
    check_b_skip(make, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("name", sorted(C_CASES))
def test_slot_capacity(make, monkeypatch, port, name, variant):
    check_c(make, monkeypatch, port, name, variant)


@pytest.mark.parametrize("variant", [("default", 1, True), ("default", 0, True), ("default", 1, False), ("desc", 1, True), ("blocks", 1, True),
                                     ("atomics", 1, True)], ids=vid)
def test_fullest_tile(make, monkeypatch, port, variant):
    check_c_fullest(make, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("name", sorted(D_STRADDLE))
def test_runs_across_a_tile_edge(make, monkeypatch, port, name, variant):
    check_d_straddle(make, monkeypatch, port, name, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("e0", [1, 47, 48])
def test_entries_in_front_of_a_tile(make, monkeypatch, port, e0, variant):
    check_d_e0(make, monkeypatch, port, e0, variant)


@pytest.mark.parametrize("variant", D_FAR, ids=vid)
def test_run_that_began_two_tiles_back(make, monkeypatch, port, variant):
    check_d_far(make, monkeypatch, port, variant, **({"sparse_form": 1} if variant[0] == "desc" else {}))


@pytest.mark.parametrize("target", E_TARGETS)
@pytest.mark.parametrize("pairs", [1, 0])
def test_parts_side_by_side(make, monkeypatch, port, pairs, target):
    check_e_parts(make, monkeypatch, port, pairs, target)


@pytest.mark.parametrize("pairs", [1, 0])
def test_streams_of_a_few_words(make, monkeypatch, port, pairs):
    check_e_streams(make, monkeypatch, port, pairs)


@pytest.mark.parametrize("words", [16383, 16384, 16385])
def test_part_of_16384_words(make, monkeypatch, port, words):
    check_e_long_part(make, monkeypatch, port, words)


@pytest.mark.parametrize("desc_parts", [1, 64])
@pytest.mark.parametrize("cols,unpacked", E_FORMATS)
def test_descriptor_partner_formats(make, monkeypatch, port, cols, unpacked, desc_parts):
    check_e_desc(make, monkeypatch, port, cols, unpacked, desc_parts)


def test_descriptor_bands_without_words(make, monkeypatch, port):
    check_e_desc_bands(make, monkeypatch, port)


def test_descriptors_in_two_lds_rounds(make, monkeypatch, port):
    check_e_two_rounds(make, monkeypatch, port)


@pytest.mark.parametrize("N,slots16,t,top", F_RUNS)
def test_by_slot_stores(make, monkeypatch, port, N, slots16, t, top):
    check_f(make, monkeypatch, port, N, slots16, t, top)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip"])
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("sub_shift", [4, 6])
def test_lists_across_sub_bands(make, monkeypatch, port, sub_shift, desc, skip):
    check_g_crossing(make, monkeypatch, port, sub_shift, desc, skip)


@pytest.mark.parametrize("words", [8191, 8192, 8193])
def test_scatter_tile(make, monkeypatch, port, words):
    check_g_tile(make, monkeypatch, port, words)


@pytest.mark.parametrize("records", [8191, 8192, 8193])
def test_descriptor_record_piece(make, monkeypatch, port, records):
    check_g_records(make, monkeypatch, port, records)


@pytest.mark.parametrize("pass_words", [0, 30])
def test_blocks_passes(make, monkeypatch, port, pass_words):
    check_g_passes(make, monkeypatch, port, pass_words)
