"""Mismatch-weighted kernels (fsk_set_mismatch_weights, ``weights=`` / ``max_mismatches=``) on the MI355X: the product library
through the C ABI, the check functions of tests/test_emu_mismatch.py (which state the contract) at the same sizes — every
level on the real dataflows, k_tri_fold on the device (16-byte lanes, the scalar tail of an odd cell count, more than one
workgroup) — plus the one size only the device needs, and the pybind11 class once."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests"))

import mismatch_cases as cases  # noqa: E402
from test_emu_mismatch import (check_definition, check_fold_edges, check_identity, check_level_key_too_wide, check_profile_recipe,  # noqa: E402
                               check_protein, check_reuse, check_revcomp, check_skip_test_block,
                               check_staged_calls_and_unsupported_handles, check_weight_bound)

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


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("weights", cases.DEFINITION_WEIGHTS, ids=lambda w: "-".join(str(x) for x in w))
def test_definition(make, port, weights, path):
    check_definition(make, port, weights, path)


@pytest.mark.parametrize("path", [1, 2])
def test_identity_with_gkm_weights(make, port, path):
    check_identity(make, port, path)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", cases.FOLD_EDGE_N)
def test_fold_edges(make, port, n, order):
    check_fold_edges(make, port, n, order)


def test_fold_second_grid_stride_trip(make, port):
    """The fold's grid is at most 8 workgroups of 256 lanes a compute unit: 524,288 lanes of two cells on 256 compute units. The
    emulator (two compute units) strides from 8,192 cells on; on the device the 262,450 cells above are one trip. N = 1500 is
    1,125,750 cells = 562,875 pairs: the first 38,587 lanes take a second trip."""
    check_fold_edges(make, port, 1500, 0)


def test_fold_of_a_misaligned_triangle(native, make, port):
    """A bound result triangle that is 8 but not 16 bytes aligned (a torch tensor's second element on): the scalar form."""
    import torch
    case = cases.fold_edge_case(91)
    seqs, g, m, weights = case["seqs"], case["g"], case["m"], case["weights"]
    pairs = len(seqs) * (len(seqs) + 1) // 2
    buf = torch.zeros(pairs + 2, dtype=torch.int64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    tok, off = native.flatten(seqs)
    e = make(g, m, weights=weights)
    e.bind_counts(buf.data_ptr() + 8, pairs, keepalive=buf)
    e.compute(tok, off, len(seqs), 0)
    want = cases.levels_reference(port, seqs, g, weights)[0]
    assert np.array_equal(e.get_counts(), want)
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    assert np.array_equal(host[1:1 + pairs], want) and host[0] == 0 and host[pairs + 1] == 0
    e.close()


def test_protein_truncated_at_two_mismatches(make, port):
    check_protein(make, port)


@pytest.mark.parametrize("path", [1, 2])
def test_reverse_complement_with_weights(make, port, path):
    check_revcomp(make, port, path)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_test_block(make, port, path):
    check_skip_test_block(make, port, path)


def test_level_key_too_wide(make, port):
    check_level_key_too_wide(make, port)


def test_weight_bound(make, port):
    check_weight_bound(make, port)


def test_staged_calls_and_unsupported_handles(make, port):
    check_staged_calls_and_unsupported_handles(make, port)


def test_reuse_of_one_handle(make, port):
    check_reuse(make, port)


def test_mismatch_profile_recipe(make, port):
    check_profile_recipe(make, port)


def test_pybind_surface(native, port):
    """FastSK(g=6, m=3, max_mismatches=2).compute_kernel(lists, lists) against the brute force, getters as numpy."""
    from fastsk_amd import FastSK
    case = cases.definition_case()
    seqs, g, m = case["seqs"], case["g"], case["m"]
    ntr = 25
    weights = cases.gkm_weights(g, m, 2)
    want = cases.brute_weighted(seqs, g, weights)
    n = len(seqs)
    f = FastSK(g=g, m=m, max_mismatches=2)
    f.compute_kernel(seqs[:ntr], seqs[ntr:])
    assert np.array_equal(f.get_counts_np(), want)
    sq = tri_to_square(cases.normalised(port, want, n), n)
    assert np.array_equal(f.get_train_kernel_np(), sq[:ntr, :ntr]) and np.array_equal(f.get_test_kernel_np(), sq[ntr:, :ntr])
    assert np.array_equal(np.array(f.get_test_kernel()), sq[ntr:, :ntr])
    st = f.stats()
    assert st["weights"] == weights and [lv["m"] for lv in st["mismatch_levels"]] == [0, 1, 2]
    info = f.mismatch_info()
    assert info["a"] == cases.solve_levels(g, weights) and info["n_levels"] == 3
    # the same through weights=, with reverse complement
    h = FastSK(g=g, m=m, weights=weights, revcomp=cases.DNA)
    h.compute_train(seqs)
    assert np.array_equal(h.get_counts_np(), cases.brute_weighted(seqs, g, weights, cases.DNA))
