"""The rows kernel (fsk_rows_build, fsk_rows_get_block, fsk_svm_set_kernel) on the CPU: the engine's HIP source compiled against
tests/emu/hip_emu.h must reproduce, to the bit, the numpy yardstick of tests/rows_kernel_cases.py at every tile and panel edge,
for every kind of result and under skip_test_block; the SVM stage on it must equal tests/svm_cases.py fed with K2 from the
getter. The ``check_*`` functions take an engine factory; tests/test_gpu_rows_kernel.py runs them on the MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rows_kernel_cases as rk  # noqa: E402
import svm_cases as cases  # noqa: E402
import svm_cv_cases as cv  # noqa: E402
from test_emu_svm import computed, emu_lib, make, same_model  # noqa: E402,F401  (the fixtures: the emulator's library and engine factory)
from test_emu_svm_cv import same_problems  # noqa: E402

FORMS = (("workgroup", 8192), ("two-launch", 0))
REVCOMP = {1: 4, 4: 1, 2: 3, 3: 2}


def tile_and_panel(lib):
    keys = lib.tuning_keys()
    T, P = keys["rows_tile"][0], keys["rows_panel"][0]
    assert keys["rows_tile"][1:3] == (T, T) and keys["rows_panel"][1:3] == (P, P)   # read-only: one value in range
    assert T in (64, 128) and P == 16
    return T, P


def tiles_of(n, N, T):
    ncb, nrb = -(-n // T), -(-N // T)
    return ncb * (ncb + 1) // 2 + (nrb - ncb) * ncb


def check_against_yardstick(e, n, N, T=None, tiles_before=0):
    """Raw and normalised blocks over the whole square (every computable cell in both orders, the test x test off-diagonal
    cells, the test rows' diagonals) against the yardstick fed from the result's own get_block."""
    info = e.rows_build()
    L, K2, d = rk.reference(e.get_block(0, N, 0, n), n)
    got_L, got_K2 = e.rows_block(0, N, 0, N, raw=True), e.rows_block(0, N, 0, N)
    assert rk.same_bits(got_L, L), np.argwhere(got_L.view(np.uint64) != L.view(np.uint64))[:5]
    assert rk.same_bits(got_K2, K2), np.argwhere(got_K2.view(np.uint64) != K2.view(np.uint64))[:5]
    if N > n + 1:
        off = ~np.eye(N - n, dtype=bool)
        some = d[n:] > 0.0                                  # (a test row that shares nothing with the train set: 0 / sqrt(0))
        assert not got_L[n:, n:][off].any() and not got_K2[n:, n:][off & some[:, None] & some[None, :]].any()   # never computed: 0.0
    assert rk.same_bits(e.rows_block(n - 1, N, 0, n, raw=True), e.rows_block(0, n, n - 1, N, raw=True).T)   # either order of (r, c)
    assert info["n_train"] == n and info["n_seq"] == N and info["resident_bytes"] >= 8 * (N * (N + 1) // 2 + N)
    if T is not None:
        assert info["tile"] == T and info["tiles"] - tiles_before == tiles_of(n, N, T), info
    return info, L, K2


# ---- 1. tile and panel edges ------------------------------------------------------------------------------------------------------
def check_edge(make, lib, n_train, n_test):
    """n_train, n_test: expressions in T and P (rows_kernel_cases.EDGE_*), the library's own tile edge and panel depth."""
    T, P = tile_and_panel(lib)
    n, n_test = rk.size_of(n_train, T, P), rk.size_of(n_test, T, P)
    c = rk.case(n, n_test)
    e = computed(make, c)
    check_against_yardstick(e, n, n + n_test, T)
    e.close()


# ---- 2. result kinds ----------------------------------------------------------------------------------------------------------------
def check_result_kind(make, lib, kind):
    from fastsk_amd import _native
    T, P = tile_and_panel(lib)
    n, n_test = T + P + 1, 3
    kw = {"fp64": dict(approx=True, t=1, max_iters=6, seed=5), "mismatch": dict(max_mismatches=1), "revcomp": dict(revcomp=REVCOMP),
          "group": dict(devices=[0, 0], collective=_native.COLL_P2P)}[kind]
    c = rk.case(n, n_test, seed=77)
    e = computed(make, c, **kw)
    if kind == "group":
        assert e.multi_info()["ndev"] == 2
    if kind == "fp64":
        assert len(e.get_stdevs()) > 0
    plain = computed(make, c)
    assert np.array_equal(plain.get_train(), e.get_train()) == (kind == "group")   # (the mode is really on)
    plain.close()
    check_against_yardstick(e, n, n + n_test, T)
    e.close()


# ---- 3. skip_test_block -----------------------------------------------------------------------------------------------------------
def check_skip_test_block(make, lib):
    T, P = tile_and_panel(lib)
    n, n_test = T + 1, P + 1
    c = rk.case(n, n_test, seed=31)
    blocks = []
    for skip in (False, True):
        e = computed(make, c, skip_test_block=skip)
        check_against_yardstick(e, n, n + n_test, T)
        blocks.append((e.rows_block(0, n + n_test, 0, n + n_test, raw=True), e.rows_block(0, n + n_test, 0, n + n_test)))
        e.close()
    assert rk.same_bits(blocks[0][0], blocks[1][0]) and rk.same_bits(blocks[0][1], blocks[1][1])


# ---- 5. the SVM stage on the rows kernel ----------------------------------------------------------------------------------------
def check_svm(make, n, forms=FORMS, C=10.0, n_test=5, max_iter=-1, folds=True):
    """alpha, rho, objective and the iteration count equal svm_cases.solve fed with K2 from the getter, in both forms; the
    decision values of train and test rows lie within decision_reference's bound; 3 folds x 2 C equal svm_cv_cases on K2."""
    c = cases.edge_case(n, C=C, n_test=n_test)
    e = computed(make, c)
    N = n + n_test
    e.svm_set_kernel("linear")
    assert e.svm_get_kernel() == 1
    y, eps = c["y"], c["eps"]
    e.rows_build()
    K2 = e.rows_block(0, n, 0, n)
    assert np.all(np.diag(K2) == 1.0)
    want = cases.solve(K2, y, C, eps, max_iter)
    for form, limit in forms:
        e.set_tuning("svm_wg_max", limit)
        info = e.svm_train(y, C, eps, max_iter)
        assert info["form"] == form, (form, info)
        alpha, rho, _ = same_model(e, want, (n, form))
        dec = e.svm_decision(0, N)
        ref, bound = cases.decision_reference(e.rows_block(0, N, 0, n), y, alpha, rho)
        assert np.all(np.abs(dec - ref) <= bound), float(np.max(np.abs(dec - ref) - bound))
    if folds and n >= 12:
        fold, Cs = cv.paired(n, 3), (1.0, C)
        wantcv = cv.expected(K2, y, fold, Cs, eps, max_iter)
        for form, limit in forms:
            e.set_tuning("svm_wg_max", limit)
            got = e.svm_cv(y, fold, Cs, eps, max_iter)
            assert got["form"] == form
            same_problems(e, got, wantcv, (n, form))
            ref, bound = cv.oof_reference(K2, y, fold, wantcv, len(Cs))
            assert np.all(np.abs(got["decision"] - ref) <= bound)
    # the model follows the kind: the same call on the gapped-k-mer kernel is another model
    e.svm_set_kernel("fastsk")
    with pytest.raises(Exception):
        e.svm_model()
    e.close()
    return want


def check_svm_two_launch_by_tuning(make, max_iter=-1):
    """svm_wg_max lowered to 64: 65 rows take the two launches by the automatic switch, 64 the workgroup; one arithmetic."""
    for n, form in ((64, "workgroup"), (65, "two-launch")):
        c = cases.edge_case(n, C=10.0)
        e = computed(make, c, tuning={"svm_wg_max": 64})
        e.svm_set_kernel(1)
        e.rows_build()
        want = cases.solve(e.rows_block(0, n, 0, n), c["y"], 10.0, c["eps"], max_iter)
        assert e.svm_train(c["y"], 10.0, c["eps"], max_iter)["form"] == form
        same_model(e, want, form)
        e.close()


# ---- 6. life cycle and errors -------------------------------------------------------------------------------------------------------
def check_life_cycle(make, lib):
    from fastsk_amd import _native
    T, P = tile_and_panel(lib)
    c = cases.edge_case(20, n_test=3)
    tok, off = _native.flatten(c["X"])
    y = c["y"]
    e = make(c["g"], c["m"])

    def code(fn):
        with pytest.raises(_native.FskError) as err:
            fn()
        return err.value.code

    block = lambda: e.rows_block(0, 2, 0, 2)
    assert code(e.rows_build) == -3 and code(block) == -3                     # nothing computed
    e.load_sequences(tok, off, 20, 3)
    e.accumulate(np.arange(15, dtype=np.int32))
    assert code(e.rows_build) == -3 and code(block) == -3                     # accumulated, not finalized
    e.finalize()
    assert code(block) == -3                                                  # finalized, not built: the getter does not build
    first = e.rows_build()
    assert first["builds"] == 1 and first["tiles"] == tiles_of(20, 23, T) and first["scratch_bytes"] >= 8 * (210 + 60)
    again = e.rows_build()
    assert again["builds"] == 1 and again["tiles"] == first["tiles"]          # idempotent: no second launch
    L = e.rows_block(0, 23, 0, 23, raw=True)
    assert code(lambda: e.rows_block(-1, 2, 0, 2)) == -1 and code(lambda: e.rows_block(0, 24, 0, 2)) == -1
    assert code(lambda: e.rows_block(0, 2, 3, 2)) == -1 and e.lib.L.fsk_rows_get_block(e.h, 0, 2, 0, 2, 0, None) == -1
    assert e.rows_block(5, 5, 0, 3).shape == (0, 3)
    assert e.lib.L.fsk_rows_build(None) == -1 and e.lib.L.fsk_svm_set_kernel(e.h, 2) == -1 and e.lib.L.fsk_svm_set_kernel(e.h, -1) == -1
    # a model of kind rows, then everything that drops the result drops both
    e.svm_set_kernel(1)
    e.svm_train(y, 10.0)
    alpha1, rho1, info1 = e.svm_model()
    for drop in ("accumulate", "reset", "load", "compute"):
        if drop == "accumulate":
            e.accumulate(np.arange(3, dtype=np.int32))
        elif drop == "reset":
            e.reset_counts()
        elif drop == "load":
            e.load_sequences(tok, off, 20, 3)
        else:
            e.compute(tok, off, 20, 3)
        assert code(block) == -3 and code(e.svm_model) == -3, drop
        assert e.rows_info()["resident_bytes"] == 0
        e.compute(tok, off, 20, 3)
        assert code(block) == -3                                              # a new result: not built yet
        e.svm_train(y, 10.0)                                                  # kind rows: builds
        assert rk.same_bits(e.rows_block(0, 23, 0, 23, raw=True), L)
    assert e.rows_info()["builds"] == 5
    # switching the kind drops the model; switching back and refitting gives the first model's bits
    e.svm_set_kernel(0)
    assert code(e.svm_model) == -3
    e.svm_train(y, 10.0)
    alpha0, _, _ = e.svm_model()
    assert not np.array_equal(alpha0, alpha1)
    fold = cv.paired(20, 2)
    e.svm_cv(y, fold, (1.0,))
    e.svm_set_kernel(0)                                                       # the same kind: nothing dropped
    e.svm_model()
    e.svm_set_kernel(1)
    assert code(e.svm_model) == -3 and e.lib.L.fsk_svm_cv_get(e.h, None, None, None, None) == -3   # model and cross-validation gone
    e.svm_train(y, 10.0)
    alpha2, rho2, info2 = e.svm_model()
    assert np.array_equal(alpha2, alpha1) and rho2 == rho1 and info2["iterations"] == info1["iterations"] and info2["objective"] == info1["objective"]
    assert e.rows_info()["builds"] == 5                                       # the rows kernel stayed
    e.close()


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("n_test", rk.EDGE_N_TEST)
@pytest.mark.parametrize("n_train", rk.EDGE_N_TRAIN)
def test_tile_and_panel_edges(make, emu_lib, n_train, n_test):
    check_edge(make, emu_lib, n_train, n_test)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "revcomp", "group"])
def test_result_kinds(make, emu_lib, kind):
    check_result_kind(make, emu_lib, kind)


def test_skip_test_block_gives_the_same_bits(make, emu_lib):
    check_skip_test_block(make, emu_lib)


@pytest.mark.parametrize("n", [2, 64, 65, 300])
def test_svm_on_the_rows_kernel(make, n):
    check_svm(make, n, max_iter=-1 if n <= 65 else 60)


def test_svm_two_launch_form_by_lowered_wg_max(make):
    check_svm_two_launch_by_tuning(make)


def test_life_cycle_and_errors(make, emu_lib):
    check_life_cycle(make, emu_lib)
