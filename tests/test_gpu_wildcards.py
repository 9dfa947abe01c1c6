"""Wildcard mode (fsk_set_wildcards, ``FastSK(wildcards=...)``) on the MI355X: the product library against the yardsticks of
tests/wildcard_cases.py, through the check functions of tests/test_emu_wildcards.py at the sizes that reach each branch on the
device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_tokens

sys.path.insert(0, os.path.join(ROOT, "tests"))

import wildcard_cases as cases  # noqa: E402
from test_emu_wildcards import (REGIMES, check_absent_wildcard, check_definition, check_errors, check_golden, check_group,  # noqa: E402
                                check_mismatch, check_padding_exact, check_panel, check_poly_a, check_rare_symbol, check_regime,
                                check_revcomp_errors, check_shared_prefix, check_skip_test_block, check_skip_variance,
                                check_sparse_forms, check_staged, check_variance_padding, check_wide_keys, check_wide_windows)

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


@pytest.mark.parametrize("comp", [None, cases.DNA, cases.DNA_N], ids=["one strand", "revcomp", "revcomp, n listed"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_definition(make, port, path, comp):
    check_definition(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_absent_wildcard_changes_nothing(make, port, path):
    check_absent_wildcard(make, port, path)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("ragged_lengths", [False, True])
def test_one_panel_every_place(make, port, ragged_lengths, path):
    check_panel(make, port, ragged_lengths, path)


@pytest.mark.parametrize("name,lmax,m,tun,strands,planned", REGIMES, ids=[r[0] for r in REGIMES])
def test_dense_regimes(make, port, name, lmax, m, tun, strands, planned):
    check_regime(make, port, name, lmax, m, tun, strands, planned, 1.0)


def test_rare_symbol_beside_the_wildcard(make, port):
    check_rare_symbol(make, port, 1.0)


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("period,length", [(20, 200), (300, 900)])
def test_poly_a_cut_by_wildcards(make, port, period, length, path):
    check_poly_a(make, port, period, length, path, 1.0)


def test_sparse_forms(make, port):
    check_sparse_forms(make, port, 1.0)


def test_shared_prefix_batches(make, port):
    check_shared_prefix(make, port, 1.0)


@pytest.mark.parametrize("path", [0, 2])
def test_windows_wider_than_128_bits(make, port, path):
    check_wide_windows(make, port, path, 1.0)


def test_keys_beyond_62_bits(make, port):
    check_wide_keys(make, port)


def test_wildcard_in_the_complement_map(make):
    check_revcomp_errors(make)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
def test_mismatch_weights(make, port, path, comp):
    check_mismatch(make, port, path, comp, max_mismatches=2)


def test_mismatch_weights_beyond_32_bits(make, port):
    check_mismatch(make, port, 0, None, weights=[2 ** 40, 1, 0, 0])


@pytest.mark.parametrize("path", [1, 2])
def test_skip_variance(make, port, native, path):
    check_skip_variance(make, port, native.library(), path)


@pytest.mark.parametrize("path", [1, 2])
def test_variance_mode_on_padded_sequences(make, port, native, path):
    check_variance_padding(make, port, native.library(), path)


@pytest.mark.parametrize("comp", [None, cases.DNA_N], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_padding_is_the_trimmed_kernel(make, port, path, comp):
    check_padding_exact(make, port, path, comp)


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


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(make, path):
    check_golden(make, path)


def test_pybind_surface(native, port):
    """``FastSK(wildcards=FastaUtility.wildcards())``: the keyword reaches the engine."""
    from fastsk_amd import FastSK
    case = cases.definition_case()
    n, ntr = len(case["seqs"]), case["n_train"]
    want = cases.fragment_fold(port, case["seqs"], set(case["wild"]), case["g"], case["m"], case["combos"])
    f = FastSK(g=case["g"], m=case["m"], t=1, wildcards=case["wild"])
    f.compute_kernel(case["seqs"][:ntr], case["seqs"][ntr:])
    sq = np.zeros((n, n))
    sq[np.tril_indices(n)] = port.normalise(want.astype(np.float64), n)
    assert np.array_equal(np.array(f.get_test_kernel()), sq[ntr:, :ntr])
    assert f.stats()["wildcards"] == [5, 6] and f.stats()["alphabet"] == 4


def test_config_3_input_with_n_as_wildcard(make, port):
    """The whole EP300_47848 input (7,230 x 200, five sequences with 288 n between them), g = 10, m = 6, the first 100 combos:
    the scattered cells of 300 sequences that contain the five, against the fragment fold."""
    tokens, offsets, n_train, n_test, _, _ = load_tokens("EP300_47848")
    with_n = [3507, 4000, 4001, 4002, 5153]
    rng = np.random.Generator(np.random.PCG64(3))
    idx = np.array(sorted(set(with_n) | set(rng.choice(n_train + n_test, size=295, replace=False).tolist()))[:300], dtype=np.int64)
    assert set(with_n) <= set(idx.tolist())
    seqs = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in idx]
    assert sum(s.count(5) for s in seqs) == 288
    combos = np.arange(100, dtype=np.int32)
    want = cases.fragment_fold(port, seqs, {5}, 10, 6, combos)
    e = make(10, 6, wildcards=[5])
    e.load_sequences(tokens, offsets, n_train, n_test)
    e.accumulate(combos)
    e.finalize()
    st = e.stats()
    assert st["alphabet"] == 4 and st["key_space"] == 256 and st["max_windows"] == 191
    assert st["n_feat"] == 7230 * 191 - (5 * 191 - sum(cases.valid_counts([seqs[list(idx).index(r)] for r in with_n], {5}, 10)))
    a, b = np.tril_indices(len(idx))
    assert np.array_equal(e.get_counts_cells(idx[a], idx[b]), want)
    e.close()
