"""Centre-weighted mode without a device: the keyword forms and their validation, ``center_profile``, and the yardsticks of
tests/center_weight_cases.py against each other and against ``port.raw_counts``.

Six test cases here (five functions, one of them run twice) look at the yardsticks and the cases alone (test_distances_are_symmetric_and_start_at_zero,
test_the_yardsticks_agree, test_fold_rows_is_the_matrix_product, test_the_mismatch_yardstick_reduces_to_the_counts,
test_cases_reach_what_they_are_for): they check the references the other tests rely on and would pass on an engine without
the feature. Every other test of the three files needs the new symbol, keyword or helper and fails without it."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import center_weight_cases as cases  # noqa: E402


def test_center_weight_array_forms():
    from fastsk_amd import _native
    for off in (None, False, [], ()):
        assert len(_native.center_weight_array(off)) == 0
    a = _native.center_weight_array([5, np.int32(6), 0, 255])
    assert a.dtype == np.uint32 and a.tolist() == [5, 6, 0, 255]
    assert _native.center_weight_array(np.array([7, 9])).tolist() == [7, 9]
    assert len(_native.center_weight_array([1] * 4096)) == 4096


@pytest.mark.parametrize("bad", [[5.0], ["8"], [True], [None], "8", 5, [256], [-1], [0, 1], [1] * 4097])
def test_center_weight_array_rejects(bad):
    from fastsk_amd import _native
    with pytest.raises(ValueError):
        _native.center_weight_array(bad)


@pytest.mark.parametrize("bad", [[5.0], ["8"], [True], "8", 5, [256], [-1], [0, 1], [1] * 4097])
def test_pybind_keyword_rejects_before_any_device_call(bad):
    import __graft_entry__ as ge
    ge.build_engine()
    ge.build_bindings()
    from fastsk_amd import _fastsk
    with pytest.raises(ValueError):
        _fastsk.FastSK(6, 3, center_weights=bad)
    doc = _fastsk.FastSK.__init__.__doc__
    # an overload of its own: the signature that ends in wildcards is still there, and center_weights is keyword-only
    assert re.search(r"wildcards: [^,)]*= None\)", doc) and re.search(r"wildcards: [^,)]*= None, \*, center_weights: ", doc)


def test_pybind_wildcards_keep_their_place():
    """The 18th positional argument is still wildcards (checked before any device call: a bad one raises ValueError), and
    center_weights cannot be passed by position."""
    import __graft_entry__ as ge
    ge.build_engine()
    ge.build_bindings()
    from fastsk_amd import _fastsk
    head = (6, 3, -1, False, 0.025, -1, False, 0, "auto", None, False, None, "auto", 0, None, None, None)
    with pytest.raises(ValueError) as err:
        _fastsk.FastSK(*head, [5, 5])
    assert "twice" in str(err.value)
    with pytest.raises(TypeError):
        _fastsk.FastSK(*head, None, [1, 1])
    with pytest.raises(ValueError) as err:
        _fastsk.FastSK(*head, [5], center_weights=[0])
    assert "first" in str(err.value)


def test_center_profile_values_and_cut():
    from fastsk_amd import center_profile
    for args, kw in (((25, 50), {}), ((0, 1), {}), ((3, 2.5), {"levels": 255}), ((8, 16), {"levels": 4, "floor": 1}),
                     ((10, 7), {"levels": 3, "floor": 3}), ((100, 300), {"levels": 8, "floor": 2})):
        got = center_profile(*args, **kw)
        assert got == cases.center_profile_definition(*args, **kw), (args, kw)
        assert got[0] == kw.get("levels", 8) and got[-1] == kw.get("floor", 0) and got.count(got[-1]) == 1
        assert all(a >= b for a, b in zip(got, got[1:])) and len(got) <= 4096
    p = center_profile(25, 50)
    assert p[:26] == [8] * 26 and p[25 + 50] == 4 and p[25 + 100] == 2 and p[25 + 150] == 1 and p[-1] == 0 and len(p) == 227
    assert center_profile(10, 7, levels=3, floor=3) == [3]   # constant from the start: one entry
    from fastsk_amd import _native
    assert len(_native.center_weight_array(p)) == len(p)


@pytest.mark.parametrize("args,kw", [((25, 1100), {}), ((-1, 5), {}), ((5, 0), {}), ((5, 5), {"levels": 0}), ((5, 5), {"levels": 256}),
                                     ((5, 5), {"floor": -1}), ((2.5, 5), {}), ((4000, 50), {})])
def test_center_profile_rejects(args, kw):
    from fastsk_amd import center_profile
    with pytest.raises(ValueError):
        center_profile(*args, **kw)


def test_distances_are_symmetric_and_start_at_zero():
    for g in (5, 12):
        for L in range(g, g + 45):
            d = cases.distances(L, g)
            assert np.array_equal(d, d[::-1]) and d.min() == 0 and d.max() == (L - g) // 2
            assert np.array_equal(d, [abs(2 * p + g - L) // 2 for p in range(L - g + 1)])
            assert (np.abs(np.diff(d)) <= 1).all()


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
def test_the_yardsticks_agree(port, comp):
    """brute, window_fold and — on a non-increasing profile — layer_fold, all three; all ones is ``port.raw_counts``."""
    from oracle import loader
    case = cases.definition_case()
    seqs, g, m, combos = case["seqs"], case["g"], case["m"], case["combos"]
    want = cases.brute(port, seqs, case["profile"], g, m, combos, comp)
    assert np.array_equal(want, cases.window_fold(port, seqs, case["profile"], g, m, combos, comp)) and want.any()
    mono = [3, 3, 2, 2, 2, 1, 0]
    b = cases.brute(port, seqs, mono, g, m, combos, comp)
    assert np.array_equal(b, cases.window_fold(port, seqs, mono, g, m, combos, comp))
    assert np.array_equal(b, cases.layer_fold(port, seqs, mono, g, m, combos, comp))
    assert not np.array_equal(b, want)
    if comp is None:
        tok, off = loader.flatten(seqs)
        plain = port.raw_counts(tok, off, g, m, combos)[0]
        assert np.array_equal(cases.brute(port, seqs, [1], g, m, combos), plain)
        assert np.array_equal(cases.brute(port, seqs, [3], g, m, combos), plain * np.uint64(9))


def test_fold_rows_is_the_matrix_product():
    import wildcard_cases
    rng = np.random.Generator(np.random.PCG64(5))
    owner = rng.permutation(np.repeat(np.arange(7), 3)).tolist() + list(range(7))
    f = len(owner)
    tri = rng.integers(0, 2 ** 40, size=f * (f + 1) // 2).astype(np.uint64)
    assert np.array_equal(cases.fold_rows(tri, owner, 7), wildcard_cases.fold_rows(tri, owner, 7))


def test_the_mismatch_yardstick_reduces_to_the_counts(port):
    """With the gapped k-mer kernel's own weights the Hamming brute force is the per-combination brute force."""
    import mismatch_cases
    case = cases.mismatch_case()
    g, m = case["g"], case["m"]
    combos = np.arange(port.num_combos(g, m), dtype=np.int32)
    for comp in (None, cases.DNA):
        w = cases.brute_mismatch(case["seqs"], case["profile"], g, mismatch_cases.gkm_weights(g, m), comp)
        assert np.array_equal(w, cases.brute(port, case["seqs"], case["profile"], g, m, combos, comp))


def test_cases_reach_what_they_are_for():
    case = cases.wildcard_case()
    assert min(cases.weight_sums(case["seqs"], case["g"], case["profile"], {cases.N_})) >= 1
    heavy = cases.heavy_case(0.3)
    sums = cases.weight_sums(heavy["seqs"], heavy["g"], heavy["profile"])
    assert sorted(sums)[-3:] == [76500] * 3 and max(len(s) for s in heavy["seqs"]) - heavy["g"] + 1 == 300
    panel = cases.panel_case()
    assert len({tuple(cases.window_weights(len(s), panel["g"], panel["profile"])) for s in panel["seqs"]}) == 41


def test_header_and_ctypes_view_agree():
    from fastsk_amd import _native
    src = open(os.path.join(ROOT, "include", "fastsk_amd.h")).read()
    assert "int fsk_set_center_weights(fsk_engine* e, const uint32_t* w, int32_t n);" in src
    assert "fsk_set_center_weights" in _native.SYMBOLS and "#define FSK_ABI_VERSION 5" in src
