"""Mismatch-weighted kernels (fsk_set_mismatch_weights, ``weights=`` / ``max_mismatches=``) on the CPU: the engine's HIP source
compiled against tests/emu/hip_emu.h must give W = sum_h c_h N_h to the bit — against the brute-force Hamming profile and
against the level algebra on the CPU oracle's raw counts (tests/mismatch_cases.py). One check function per case;
tests/test_gpu_mismatch.py runs the same functions on the device. ``make(g, m, **kw)`` creates an engine; no expected value
comes from an engine."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mismatch_cases as cases  # noqa: E402

_ONCE = {}


def once(key, fn):
    """An expectation computed once per session and shared: read-only."""
    if key not in _ONCE:
        v = fn()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _ONCE[key] = v
    return _ONCE[key]


def run(make, seqs, g, m, n_train=None, **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(seqs)
    n = len(seqs)
    e = make(g, m, **kw)
    e.compute(tok, off, n if n_train is None else n_train, 0 if n_train is None else n - n_train)
    return e


# ---- definition ----------------------------------------------------------------------------------------------------------
def check_definition(make, port, weights, path):
    case = cases.definition_case()
    seqs, g, m = case["seqs"], case["g"], case["m"]
    n = len(seqs)
    want = once(("def", tuple(weights)), lambda: cases.brute_weighted(seqs, g, weights))
    levels = once(("def-levels", tuple(weights)), lambda: cases.levels_reference(port, seqs, g, weights)[0])
    assert np.array_equal(want, levels)   # (the two yardsticks agree before the engine is asked)
    e = run(make, seqs, g, m, path=path, weights=weights)
    got = e.get_counts()
    assert np.array_equal(got, want) and np.array_equal(got, levels)
    if weights[0] >= 2 ** 40:
        assert int(got.max()) >= 2 ** 32   # cells beyond 32 bits
    tri = cases.normalised(port, want, n)
    assert np.array_equal(e.get_triangle(), tri)
    sq = tri_to_square(tri, n)
    assert np.array_equal(e.get_train(), sq) and np.array_equal(e.get_block(3, 9, 1, 30), sq[3:9, 1:30])
    info = e.mismatch_info()
    a = cases.solve_levels(g, weights)
    assert info["a"] == a and info["n_levels"] == len(a)
    assert [lv["m"] for lv in info["levels"]] == [j for j, v in enumerate(a) if v]
    assert all(lv["path"] == path for lv in info["levels"])
    st = e.stats()
    assert st["weights"] == list(weights) and st["combos_done"] == sum(port.num_combos(g, j) for j, v in enumerate(a) if v)
    e.close()


# ---- identity ------------------------------------------------------------------------------------------------------------
def check_identity(make, port, path):
    """The gkm weights are today's kernel: same counts, same launches, one level, no scratch and no fold."""
    case = cases.definition_case()
    seqs, g, m = case["seqs"], case["g"], case["m"]
    plain = run(make, seqs, g, m, path=path)
    e = run(make, seqs, g, m, path=path, weights=cases.gkm_weights(g, m))
    assert np.array_equal(e.get_counts(), plain.get_counts())
    assert np.array_equal(e.get_counts(), once(("def", "gkm"), lambda: cases.brute_weighted(seqs, g, cases.gkm_weights(g, m))))
    assert e.stats()["launches"] == plain.stats()["launches"]
    info = e.mismatch_info()
    assert info["a"] == [0] * m + [1] and len(info["levels"]) == 1 and info["levels"][0]["m"] == m
    assert info["levels"][0]["path"] == path and info["levels"][0]["fold_ms"] == 0.0
    assert plain.mismatch_info() == {"n_levels": 0, "a": [], "levels": []}
    # max_mismatches = m is the same thing
    f = run(make, seqs, g, m, path=path, max_mismatches=m)
    assert np.array_equal(f.get_counts(), plain.get_counts()) and f.stats()["launches"] == plain.stats()["launches"]
    for x in (plain, e, f):
        x.close()


# ---- fold edges ----------------------------------------------------------------------------------------------------------
def check_fold_edges(make, port, n, order):
    """weights [6, 3, 0] at g = 4: a = (-6, 3). In ascending order of levels the partial sum is -6 S_0, negative mod 2^64 in
    every cell that is not zero, until the last level; ``order`` = the tuning key mismatch_order."""
    case = cases.fold_edge_case(n)
    seqs, g, m, weights = case["seqs"], case["g"], case["m"], case["weights"]
    assert len(seqs) * (len(seqs) + 1) // 2 == {1: 1, 2: 3, 22: 253, 23: 276, 91: 4186, 724: 262450, 1500: 1125750}[n]
    want, partial = once(("fold", n), lambda: cases.levels_reference(port, seqs, g, weights))
    assert len(partial) == 2 and all(int(v) < 0 for v in partial[0] if v) and any(partial[0]) and all(int(v) >= 0 for v in partial[1])
    if n <= 91:
        assert np.array_equal(want, cases.brute_weighted(seqs, g, weights))
    e = run(make, seqs, g, m, weights=weights, tuning={"mismatch_order": order})
    assert np.array_equal(e.get_counts(), want)
    assert e.mismatch_info()["a"] == [-6, 3]
    assert e.counts_digest()[0] == int(want.astype(object).sum()) & cases.MASK
    e.close()


# ---- protein -------------------------------------------------------------------------------------------------------------
def check_protein(make, port):
    case = cases.protein_case()
    seqs, g, m, d = case["seqs"], case["g"], case["m"], case["max_mismatches"]
    weights = cases.gkm_weights(g, m, d)
    want = once(("protein",), lambda: cases.brute_weighted(seqs, g, weights))
    assert np.array_equal(want, once(("protein-levels",), lambda: cases.levels_reference(port, seqs, g, weights)[0]))
    e = run(make, seqs, g, m, max_mismatches=d)
    assert np.array_equal(e.get_counts(), want)
    assert np.array_equal(e.get_triangle(), cases.normalised(port, want, len(seqs)))
    info = e.mismatch_info()
    assert [(lv["m"], lv["k"], lv["path"]) for lv in info["levels"]] == [(0, 8, 2), (1, 7, 2), (2, 6, 2)]
    assert info["a"] == cases.solve_levels(g, weights) and all(lv["ms"] > 0 for lv in info["levels"])
    e.close()


# ---- reverse complement --------------------------------------------------------------------------------------------------
def check_revcomp(make, port, path):
    case = cases.revcomp_case()
    seqs, g, m, weights = case["seqs"], case["g"], case["m"], case["weights"]
    want = once(("rc",), lambda: cases.brute_weighted(seqs, g, weights, cases.DNA))
    assert np.array_equal(want, once(("rc-levels",), lambda: cases.levels_reference(port, seqs, g, weights, cases.DNA)[0]))
    one_strand = once(("rc-off",), lambda: cases.brute_weighted(seqs, g, weights))
    assert not np.array_equal(want, one_strand)
    e = run(make, seqs, g, m, path=path, weights=weights, revcomp=cases.DNA)
    assert np.array_equal(e.get_counts(), want)
    assert np.array_equal(e.get_triangle(), cases.normalised(port, want, len(seqs)))
    assert e.stats()["revcomp"] is True
    e.close()


# ---- skip_test_block -----------------------------------------------------------------------------------------------------
def check_skip_test_block(make, port, path):
    case = cases.skip_case()
    seqs, g, m, weights, ntr, nte = case["seqs"], case["g"], case["m"], case["weights"], case["n_train"], case["n_test"]
    n = ntr + nte
    want = once(("skip",), lambda: cases.brute_weighted(seqs, g, weights))
    sq = tri_to_square(cases.normalised(port, want, n), n)
    whole = run(make, seqs, g, m, n_train=ntr, path=path, weights=weights)
    e = run(make, seqs, g, m, n_train=ntr, path=path, weights=weights, skip_test_block=True)
    for x in (whole, e):
        assert np.array_equal(x.get_train(), sq[:ntr, :ntr]) and np.array_equal(x.get_test(), sq[ntr:, :ntr])
    assert np.array_equal(whole.get_counts(), want)
    got = e.get_counts()
    a, b = np.tril_indices(n)
    keep = (b < ntr) | (a == b)
    assert np.array_equal(got[keep], want[keep]) and want[~keep].any()
    # the other cells "may be left at zero": the sparse dataflow leaves every one, in every level; the dense one leaves whole
    # tiles of 128 x 128 and there is none at this size — what it computes is computed in full
    if path == 2:
        assert not got[~keep].any()
    else:
        assert ((got[~keep] == 0) | (got[~keep] == want[~keep])).all()
    whole.close(); e.close()


# ---- errors --------------------------------------------------------------------------------------------------------------
def check_level_key_too_wide(make, port):
    """Level 0's 14-mer of 7-bit symbols is 98 bits: FSK_EUNSUPPORTED naming the level; the handle computes with the mode off."""
    from fastsk_amd import _native
    case = cases.wide_key_case()
    seqs, g, m, weights = case["seqs"], case["g"], case["m"], case["weights"]
    tok, off = _native.flatten(seqs)
    e = make(g, m, weights=weights)
    with pytest.raises(_native.FskError) as ei:
        e.compute(tok, off, len(seqs), 0)
    assert ei.value.code == -6 and "level 0" in str(ei.value)
    with pytest.raises(_native.FskError):   # nothing half-done is readable
        e.get_counts()
    e.set_mismatch_weights(None)
    e.compute(tok, off, len(seqs), 0)
    assert e.stats()["bits_per_symbol"] == 8 and e.stats()["alphabet"] == 65
    assert np.array_equal(e.get_counts(), cases.brute_weighted(seqs, g, cases.gkm_weights(g, m)))
    # weights whose level 0 is not needed run: [28, 2] is a = (0, 2), twice the plain kernel
    e.set_mismatch_weights([28, 2])
    assert _native.solve_mismatch_levels(g, [28, 2]) == [0, 2]
    e.compute(tok, off, len(seqs), 0)
    assert np.array_equal(e.get_counts(), cases.brute_weighted(seqs, g, [28, 2]))
    assert [lv["m"] for lv in e.mismatch_info()["levels"]] == [1]
    e.close()


def check_weight_bound(make, port):
    """max(c) * max_windows^2 >= 2^64 is refused at load; just below it runs."""
    from fastsk_amd import _native
    seqs = cases.ragged(5, 8, 20, seed=9)   # g = 5: max_windows = 16, 2^64 / 256 = 2^56
    tok, off = _native.flatten(seqs)
    e = make(5, 1, weights=[2 ** 56, 1])
    with pytest.raises(_native.FskError) as ei:
        e.compute(tok, off, 5, 0)
    assert ei.value.code == -6 and "2^64" in str(ei.value)
    e.set_mismatch_weights([2 ** 56 - 1, 1])
    e.compute(tok, off, 5, 0)
    assert np.array_equal(e.get_counts(), cases.brute_weighted(seqs, 5, [2 ** 56 - 1, 1]))
    e.close()


def check_staged_calls_and_unsupported_handles(make, port):
    from fastsk_amd import _native
    seqs = cases.ragged(6, 8, 20, seed=3)
    tok, off = _native.flatten(seqs)
    e = make(6, 3, weights=[4, 2, 1, 0])
    e.compute(tok, off, 6, 0)
    for call in (lambda: e.load_sequences(tok, off, 6, 0), lambda: e.accumulate([0]), lambda: e.accumulate_rows([0], 0, 6),
                 e.reset_counts, lambda: e.reset_counts_rows(0, 6), lambda: e.run_chains(0, 1)):
        with pytest.raises(_native.FskError) as ei:
            call()
        assert ei.value.code == -3 and "mismatch-weighted" in str(ei.value)
    e.finalize()   # (the diagonal of W again)
    assert np.array_equal(e.get_counts(), cases.brute_weighted(seqs, 6, [4, 2, 1, 0]))
    e.set_mismatch_weights(None)
    e.load_sequences(tok, off, 6, 0)   # the staged path is back with the mode off
    e.close()
    c = np.array([4, 2, 1, 0], dtype=np.uint64)
    for kw, word in ((dict(approx=True), "approx"), (dict(devices=[0, 0], collective=_native.COLL_P2P), "group")):
        h = make(6, 3, **kw)
        assert h.lib.L.fsk_set_mismatch_weights(h.h, c.ctypes.data, 4) == -6
        assert word in h.lib.L.fsk_last_error(h.h).decode()
        assert h.lib.L.fsk_set_mismatch_weights(h.h, None, 0) in (0, -6)
        h.close()
    # the C call's own argument checks
    h = make(6, 3)
    for arr in ([1, 1, 1], [0, 1, 1, 1], [1, 2 ** 62, 0, 0]):
        c = np.array(arr, dtype=np.uint64)
        assert h.lib.L.fsk_set_mismatch_weights(h.h, c.ctypes.data, len(arr)) == -1
    n = C.c_int32(-1)
    assert h.lib.L.fsk_get_mismatch_info(h.h, C.byref(n), None, None, 0) == 0 and n.value == 0
    h.close()


# ---- reuse ---------------------------------------------------------------------------------------------------------------
def check_reuse(make, port):
    from fastsk_amd import _native
    big, small = cases.ragged(37, 10, 40, seed=1), cases.ragged(9, 10, 30, seed=2)
    g, m, weights = 6, 3, [20, 10, 4, 0]
    e = make(g, m, weights=weights)
    for seqs in (big, small, big):
        tok, off = _native.flatten(seqs)
        e.compute(tok, off, len(seqs), 0)
        assert np.array_equal(e.get_counts(), cases.brute_weighted(seqs, g, weights))
    e.set_mismatch_weights(None)
    tok, off = _native.flatten(small)
    e.compute(tok, off, len(small), 0)
    assert np.array_equal(e.get_counts(), cases.brute_weighted(small, g, cases.gkm_weights(g, m)))
    assert e.mismatch_info()["n_levels"] == 0 and e.stats()["weights"] is None
    e.close()


def check_profile_recipe(make, port):
    """N_h itself: the difference of the raw counts under [1] * (h + 1) + [0] * (m - h) and [1] * h + [0] * (m - h + 1)."""
    seqs = cases.ragged(12, 10, 30, seed=77)
    g, m = 6, 3
    prof = cases.brute_profile(seqs, g, m)
    il = np.tril_indices(len(seqs))
    prev = None
    for h in range(m + 1):
        e = run(make, seqs, g, m, weights=[1] * (h + 1) + [0] * (m - h))
        cur = e.get_counts().astype(np.int64)
        e.close()
        assert np.array_equal(cur - (0 if prev is None else prev), prof[h][il])
        prev = cur


# ---- the emulator runs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("weights", cases.DEFINITION_WEIGHTS, ids=lambda w: "-".join(str(x) for x in w))
def test_definition(make_emu, port, weights, path):
    check_definition(make_emu, port, weights, path)


@pytest.mark.parametrize("path", [1, 2])
def test_identity_with_gkm_weights(make_emu, port, path):
    check_identity(make_emu, port, path)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", cases.FOLD_EDGE_N)
def test_fold_edges(make_emu, port, n, order):
    check_fold_edges(make_emu, port, n, order)


def test_fold_of_a_misaligned_triangle(make_emu, port):
    """A bound result triangle that is 8 but not 16 bytes aligned: the fold takes its scalar form for every cell."""
    from fastsk_amd import _native
    case = cases.fold_edge_case(23)
    seqs, g, m, weights = case["seqs"], case["g"], case["m"], case["weights"]
    pairs = len(seqs) * (len(seqs) + 1) // 2
    buf = np.zeros(pairs + 3, dtype=np.uint64)
    at = 1 if buf.ctypes.data % 16 == 0 else 0
    view = buf[at:at + pairs]
    assert view.ctypes.data % 16 == 8
    tok, off = _native.flatten(seqs)
    e = make_emu(g, m, weights=weights)
    e.bind_counts(view.ctypes.data, pairs, keepalive=buf)   # (the emulator's device memory is host memory)
    e.compute(tok, off, len(seqs), 0)
    want = cases.levels_reference(port, seqs, g, weights)[0]
    assert np.array_equal(e.get_counts(), want) and np.array_equal(view, want)
    assert buf[at + pairs] == 0 and (at == 0 or buf[0] == 0)
    e.close()


def test_protein_truncated_at_two_mismatches(make_emu, port):
    check_protein(make_emu, port)


@pytest.mark.parametrize("path", [1, 2])
def test_reverse_complement_with_weights(make_emu, port, path):
    check_revcomp(make_emu, port, path)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_test_block(make_emu, port, path):
    check_skip_test_block(make_emu, port, path)


def test_level_key_too_wide(make_emu, port):
    check_level_key_too_wide(make_emu, port)


def test_weight_bound(make_emu, port):
    check_weight_bound(make_emu, port)


def test_staged_calls_and_unsupported_handles(make_emu, port):
    check_staged_calls_and_unsupported_handles(make_emu, port)


def test_reuse_of_one_handle(make_emu, port):
    check_reuse(make_emu, port)


def test_mismatch_profile_recipe(make_emu, port):
    check_profile_recipe(make_emu, port)
