"""Wildcard mode without a device: the keyword forms and their validation, the tokeniser helper, and the yardsticks of
tests/wildcard_cases.py against each other."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, reference_fasta

sys.path.insert(0, os.path.join(ROOT, "tests"))

import wildcard_cases as cases  # noqa: E402


def test_wildcard_array_forms():
    from fastsk_amd import _native
    for off in (None, False, [], ()):
        assert len(_native.wildcard_array(off)) == 0
    a = _native.wildcard_array([5, np.int32(6), -3])
    assert a.dtype == np.int32 and a.tolist() == [5, 6, -3]
    assert _native.wildcard_array(np.array([7, 9])).tolist() == [7, 9]
    assert _native.wildcard_array({5}).tolist() == [5]


@pytest.mark.parametrize("bad", [[5.0], ["n"], [True], [None], "n", 5, [2 ** 31], [-2 ** 31 - 1], [5, 6, 5]])
def test_wildcard_array_rejects(bad):
    from fastsk_amd import _native
    with pytest.raises(ValueError):
        _native.wildcard_array(bad)


def test_tokeniser_helper(tmp_path):
    from fastsk_amd import FastaUtility
    reader = FastaUtility()
    reader.read_data(reference_fasta("EP300_47848.train", tmp_path))
    comp = reader.complement()
    wild = reader.wildcards()
    assert len(wild) == 1 and comp[wild[0]] == wild[0] and wild == reader.wildcards("nN")
    fresh = FastaUtility()
    ids = fresh.wildcards("nx")   # not seen yet: they get their ids now ...
    assert ids == [1, 2] and fresh.wildcards("x") == [2]
    X, _ = fresh.read_data(reference_fasta("EP300_47848.train", tmp_path))   # ... and a file read later agrees
    assert sum(row.count(ids[0]) for row in X) == 288
    assert sorted(i for i, row in enumerate(X) if ids[0] in row) == [3507, 4000, 4001, 4002, 5153]
    assert len(cases.valid_windows(X[4000], set(ids), 10)) == 68


def test_fragments_are_the_valid_windows():
    case = cases.definition_case()
    g, wild = case["g"], set(case["wild"])
    for s in case["seqs"]:
        frs = cases.fragments(s, wild, g)
        assert sum(len(f) - g + 1 for f in frs) == len(cases.valid_windows(s, wild, g))
        assert all(len(f) >= g and not wild & set(f) for f in frs)


@pytest.mark.parametrize("comp", [None, cases.DNA, cases.DNA_N], ids=["one strand", "revcomp", "revcomp, n listed"])
def test_the_two_yardsticks_agree(port, comp):
    case = cases.definition_case()
    args = (port, case["seqs"], set(case["wild"]), case["g"], case["m"], case["combos"], comp)
    brute = cases.brute_counts(*args)
    assert np.array_equal(brute, cases.fragment_fold(*args)) and brute.any()
    # and the mode matters: with n as a letter the plain oracle counts more
    from oracle import loader
    tok, off = loader.flatten(case["seqs"])
    if comp is None:
        plain = port.raw_counts(tok, off, case["g"], case["m"], case["combos"])[0]
        assert (plain >= brute).all() and (plain > brute).any()


def test_the_weighted_yardstick_reduces_to_the_counts(port):
    """With the gapped k-mer kernel's own weights the Hamming brute force is the per-combination brute force."""
    import mismatch_cases
    case = cases.mismatch_case()
    g, m, wild = case["g"], case["m"], set(case["wild"])
    combos = np.arange(port.num_combos(g, m), dtype=np.int32)
    for comp in (None, cases.DNA):
        w = cases.brute_weighted(case["seqs"], wild, g, mismatch_cases.gkm_weights(g, m), comp)
        assert np.array_equal(w, cases.brute_counts(port, case["seqs"], wild, g, m, combos, comp))


@pytest.mark.parametrize("bad", [[5.0], ["n"], [True], "n", 5, [2 ** 31], [5, 6, 5]])
def test_pybind_keyword_rejects_before_any_device_call(bad):
    import re
    import __graft_entry__ as ge
    ge.build_engine()
    ge.build_bindings()
    from fastsk_amd import _fastsk
    with pytest.raises(ValueError):
        _fastsk.FastSK(6, 3, wildcards=bad)
    doc = _fastsk.FastSK.__init__.__doc__
    assert re.search(r"wildcards: [^,)]*= None\)", doc)   # the last keyword: nothing before it moved


def test_header_and_ctypes_view_agree():
    from fastsk_amd import _native
    src = open(os.path.join(ROOT, "include", "fastsk_amd.h")).read()
    assert "int fsk_set_wildcards(fsk_engine* e, const int32_t* tokens, int32_t n);" in src
    assert "fsk_set_wildcards" in _native.SYMBOLS and "#define FSK_ABI_VERSION 5" in src
