"""Centre-weighted mode (fsk_set_center_weights, ``FastSK(center_weights=...)``) on the MI355X: the product library against the
yardsticks of tests/center_weight_cases.py, through the check functions of tests/test_emu_center_weights.py at the sizes that
reach each branch on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import center_weight_cases as cases  # noqa: E402
from test_emu_center_weights import (REGIMES, check_constant, check_definition, check_errors, check_golden, check_group,  # noqa: E402
                                     check_heavy, check_mismatch, check_ones_is_off, check_panel, check_plateau, check_poly_a,
                                     check_rare_symbol, check_regime, check_shared_prefix, check_skip_test_block,
                                     check_skip_variance, check_sparse_forms, check_staged, check_too_many_features,
                                     check_variance, check_wildcards, check_zero_weights_in_a_regime)

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


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_definition(make, port, path, comp):
    check_definition(make, port, path, comp)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_ones_and_unreached_entries_are_the_mode_off(make, port, path, comp):
    check_ones_is_off(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_constant_profile_scales_by_its_square(make, port, path):
    check_constant(make, port, path)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_plateau_is_the_trimmed_kernel(make, port, path, comp):
    check_plateau(make, port, path, 1.0, comp)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_one_panel_every_centre(make, port, path, comp):
    check_panel(make, port, path, comp)


@pytest.mark.parametrize("name,lmax,m,tun,strands,planned", REGIMES, ids=[r[0] for r in REGIMES])
def test_dense_regimes(make, port, name, lmax, m, tun, strands, planned):
    check_regime(make, port, name, lmax, m, tun, strands, planned, 1.0)


@pytest.mark.parametrize("name,lmax,m,tun,strands", [r[:5] for r in REGIMES if r[0] in ("tiny chunks", "both strands resident", "both strands chunked")],
                         ids=["tiny chunks", "both strands resident", "both strands chunked"])
def test_zero_weights_in_a_dense_regime(make, port, name, lmax, m, tun, strands):
    check_zero_weights_in_a_regime(make, port, name, lmax, m, tun, strands, 1.0)


def test_rare_symbol_compaction(make, port):
    check_rare_symbol(make, port, 1.0)


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("windows", [10, 40])
def test_poly_a_crosses_the_planes_by_weight(make, port, windows, path):
    check_poly_a(make, port, windows, path, 1.0)


def test_weighted_sums_past_65535(make, port):
    check_heavy(make, port, 1.0)


def test_sparse_forms(make, port):
    check_sparse_forms(make, port, 1.0)


def test_shared_prefix_batches(make, port):
    check_shared_prefix(make, port, 1.0)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_with_wildcards(make, port, path, comp):
    check_wildcards(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
def test_with_mismatch_weights(make, port, path, comp):
    check_mismatch(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_variance(make, port, native, path):
    check_skip_variance(make, port, native.library(), path)


def test_variance_mode(make, port, native):
    check_variance(make, port, native.library())


@pytest.mark.parametrize("path", [1, 2])
def test_staged_calls_and_state(make, port, path):
    check_staged(make, port, path, 1.5)   # N = 300: the row band [128, 256)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_test_block(make, port, path):
    check_skip_test_block(make, port, path, 1.0)


def test_group_handle(make, port):
    check_group(make, port, 1.0)


def test_errors(make, port):
    check_errors(make, port)


def test_weighted_features_past_2_31_are_refused(make):
    check_too_many_features(make)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(make, path):
    check_golden(make, path)


@pytest.mark.parametrize("skip", [False, True, "lazy"])
def test_pybind_surface(native, port, skip):
    """``FastSK(center_weights=center_profile(...))``: the keyword reaches the engine, with every form of skip_test_block."""
    from fastsk_amd import FastSK, center_profile
    case = cases.definition_case()
    n, ntr = len(case["seqs"]), case["n_train"]
    prof = center_profile(2, 3, levels=5, floor=1)
    want = cases.brute(port, case["seqs"], prof, case["g"], case["m"], case["combos"])
    f = FastSK(g=case["g"], m=case["m"], t=1, center_weights=prof, skip_test_block=skip)
    f.compute_kernel(case["seqs"][:ntr], case["seqs"][ntr:])
    sq = np.zeros((n, n))
    sq[np.tril_indices(n)] = port.normalise(want.astype(np.float64), n)
    assert np.array_equal(np.array(f.get_test_kernel()), sq[ntr:, :ntr])
    full = sq + np.tril(sq, -1).T
    assert np.array_equal(np.array(f.get_train_kernel()), full[:ntr, :ntr])
    st = f.stats()
    assert st["center_weights"] == prof and st["n_feat"] == cases.expected_stats(case["seqs"], case["g"], prof)[0]
    assert FastSK(g=5, m=2).stats()["center_weights"] is None
