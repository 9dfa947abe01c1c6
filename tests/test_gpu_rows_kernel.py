"""The rows kernel (fsk_rows_build / fsk_rows_get_block / fsk_svm_set_kernel, ``kernel_type="linear"``) on the MI355X: the product
library against the yardstick of tests/rows_kernel_cases.py through the check functions of tests/test_emu_rows_kernel.py — every
tile and panel edge, every kind of result, the SVM stage run to convergence —, cells past 2^32, the pybind11 class and EP300 end
to end."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_tokens

sys.path.insert(0, os.path.join(ROOT, "tests"))

import rows_kernel_cases as rk  # noqa: E402
import svm_cases as cases  # noqa: E402
from test_emu_rows_kernel import (check_edge, check_life_cycle, check_result_kind, check_skip_test_block, check_svm,  # noqa: E402
                                  check_svm_two_launch_by_tuning)

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


@pytest.mark.parametrize("n_test", rk.EDGE_N_TEST)
@pytest.mark.parametrize("n_train", rk.EDGE_N_TRAIN)
def test_tile_and_panel_edges(make, native, n_train, n_test):
    check_edge(make, native.library(), n_train, n_test)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "revcomp", "group"])
def test_result_kinds(make, native, kind):
    check_result_kind(make, native.library(), kind)


def test_skip_test_block_gives_the_same_bits(make, native):
    check_skip_test_block(make, native.library())


@pytest.mark.parametrize("n", [2, 64, 65, 300])
def test_svm_on_the_rows_kernel(make, n):
    want = check_svm(make, n)
    assert want["converged"]


def test_svm_two_launch_form_by_lowered_wg_max(make):
    check_svm_two_launch_by_tuning(make)


def test_life_cycle_and_errors(make, native):
    check_life_cycle(make, native.library())


def test_device_getter(make, native):
    """fsk_rows_get_block_device writes the host getter's bits into the caller's device memory."""
    import torch
    c = rk.case(40, 7)
    tok, off = native.flatten(c["X"])
    e = make(c["g"], c["m"])
    e.compute(tok, off, 40, 7)
    e.rows_build()
    for raw in (0, 1):
        t = torch.zeros((47, 40), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert e.lib.L.fsk_rows_get_block_device(e.h, 0, 47, 0, 40, raw, t.data_ptr()) == 0
        assert rk.same_bits(t.cpu().numpy(), e.rows_block(0, 47, 0, 40, raw=bool(raw)))
    assert e.lib.L.fsk_rows_get_block_device(e.h, 0, 47, 0, 40, 0, None) == -1
    assert e.lib.L.fsk_rows_get_block_device(e.h, 0, 48, 0, 40, 0, t.data_ptr()) == -1
    e.close()


def test_cells_past_2_to_the_32(make, native):
    """N = 92,700 sequences, 8 of them train, skip_test_block: the last rows of L lie past cell 2^32 of the packed triangle
    (tri_index(92,682, 0) > 2^32). L(N-1, 0..7), L(N-1, N-1) and the same cells of three other rows above 92,682 against the
    yardstick on those rows. The counts and L take 34.4 GB each; 1.2 s on the MI355X."""
    N, n = 92700, 8
    rng = np.random.Generator(np.random.PCG64(92700))
    X = rng.integers(1, 5, size=(N, 12), dtype=np.int32)
    tok, off = native.flatten(X)
    e = make(6, 2, skip_test_block=True)
    e.compute(tok, off, n, N - n)
    info = e.rows_build()
    assert info["n_seq"] == N and info["resident_bytes"] >= 8 * (N * (N + 1) // 2)
    rows = np.array([N - 1, 92683, 92690, 92698])
    assert all(r * (r + 1) // 2 > 2 ** 32 for r in rows.tolist())
    A_train = e.get_block(0, n, 0, n)
    for r in rows.tolist():
        A_row = e.get_block(r, r + 1, 0, n)
        want, d = rk.reference_rows(A_row, A_train, n)
        assert rk.same_bits(e.rows_block(r, r + 1, 0, n, raw=True), want), r
        assert rk.same_bits(e.rows_block(0, n, r, r + 1, raw=True), want.T), r
        assert rk.same_bits(e.rows_block(r, r + 1, r, r + 1, raw=True), d.reshape(1, 1)), r
        assert not e.rows_block(r, r + 1, r - 3, r, raw=True).any()       # test x test: never computed
    assert np.all(e.rows_block(N - 2, N, N - 2, N) [[0, 1], [0, 1]] == 1.0)
    e.close()


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
def test_pybind_kernel_type(native):
    """kernel_type= on fit_svm and cross_validate_svm: "linear" is the rows kernel's model (svm_cases.solve on K2 from
    get_rows_kernel_block_np), "rbf" and anything else raise ValueError, a call without the keyword is "fastsk"."""
    from fastsk_amd import FastSK
    c = cases.edge_case(90, C=10.0, n_test=9)
    n, N = 90, 99
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(ValueError, match="not built"):
        f.fit_svm(c["y"], kernel_type="rbf")
    f.compute_kernel(c["X"][:n], c["X"][n:])
    for call in (f.fit_svm, f.cross_validate_svm):
        with pytest.raises(ValueError, match="not built"):
            call(c["y"], kernel_type="rbf")
        with pytest.raises(ValueError):
            call(c["y"], kernel_type="nonsense")
    plain = f.fit_svm(c["y"], C=10.0)
    a_plain = f.get_dual_coef_np()
    named = f.fit_svm(c["y"], C=10.0, kernel_type="fastsk")
    assert np.array_equal(f.get_dual_coef_np(), a_plain) and named["iterations"] == plain["iterations"] and named["kernel_type"] == "fastsk"
    assert np.array_equal(np.abs(a_plain), cases.solve(f.get_train_kernel_np(), c["y"], 10.0, 1e-3)["alpha"])
    info = f.fit_svm(c["y"], C=10.0, kernel_type="linear")
    K2 = f.get_rows_kernel_block_np(0, N, 0, N)
    L = f.get_rows_kernel_block_np(0, N, 0, N, raw=True)
    wantL, wantK2, _ = rk.reference(np.vstack([f.get_train_kernel_np(), f.get_test_kernel_np()]), n)
    assert rk.same_bits(L, wantL) and rk.same_bits(K2, wantK2)
    want = cases.solve(K2[:n, :n], c["y"], 10.0, 1e-3)
    assert info["converged"] and info["iterations"] == want["iterations"] and info["objective"] == want["objective"] and info["kernel_type"] == "linear"
    assert np.array_equal(f.get_dual_coef_np(), want["alpha"] * c["y"]) and f.get_intercept() == -want["rho"]
    for which, rows in (("train", K2[:n, :n]), ("test", K2[n:, :n])):     # decision_function_* follow the model's kind
        ref, bound = cases.decision_reference(rows, c["y"], want["alpha"], want["rho"])
        assert np.all(np.abs(f.decision_function_np(which) - ref) <= bound), which
    cvr = f.cross_validate_svm(c["y"], Cs=(1.0, 10.0), folds=3, kernel_type="linear", refit=True)
    assert cvr["kernel_type"] == "linear" and cvr["refit"]["kernel_type"] == "linear" and len(cvr["problems"]) == 6
    import svm_cv_cases as cv
    wantcv = cv.expected(K2[:n, :n], c["y"], cvr["fold"], (1.0, 10.0), 1e-3)
    for got, w in zip(cvr["problems"], wantcv):
        assert got["iterations"] == w["iterations"] and got["rho"] == w["rho"] and got["objective"] == w["objective"]
    assert f.rows_kernel_info()["builds"] == 1


def test_pybind_skip_test_block(native):
    """skip_test_block False, True and "lazy" give identical bits, and nothing of the rows kernel asks for the lazy block."""
    from fastsk_amd import FastSK
    c = cases.edge_case(70, C=10.0, n_test=33)
    n, N = 70, 103
    got = []
    for skip in (False, True, "lazy"):
        f = FastSK(g=c["g"], m=c["m"], t=1, skip_test_block=skip)
        f.compute_kernel(c["X"][:n], c["X"][n:])
        f.fit_svm(c["y"], C=10.0, kernel_type="linear")
        got.append((f.get_rows_kernel_block_np(0, N, 0, N, raw=True), f.get_rows_kernel_block_np(0, N, 0, N), f.get_dual_coef_np(),
                    f.decision_function_np("test")))
        if skip == "lazy":
            assert f.stats()["test_block_computed"] is False
    for other in got[1:]:
        assert rk.same_bits(other[0], got[0][0]) and rk.same_bits(other[1], got[0][1])
        assert np.array_equal(other[2], got[0][2]) and np.array_equal(other[3], got[0][3])


def test_ep300_end_to_end(native):
    """EP300, g = 10, m = 6 exact, skip_test_block="lazy": fit_svm(C=100, kernel_type="linear") converges and reaches the
    reference CI's bar, test AUC >= 0.9 (the same model on the CPU: 0.9804; on the MI355X: 3864 iterations, 0.9804); the raw rows block equals float64 A @ A.T from
    get_train_kernel_np() to a relative 1e-12 (the one tolerance here: a BLAS sum order over 2000 terms stays far inside)."""
    from sklearn.metrics import roc_auc_score
    from fastsk_amd import FastSK
    tokens, offsets, ntr, nte, ytr, yte = load_tokens("EP300")
    f = FastSK(g=10, m=6, t=1, skip_test_block="lazy")
    f.compute_kernel_flat(tokens, offsets, ntr)
    info = f.fit_svm(np.where(np.asarray(ytr) > 0, 1, -1).astype(np.int32), C=100.0, kernel_type="linear")
    assert info["converged"], info
    auc = roc_auc_score(np.asarray(yte) > 0, f.decision_function_np("test"))
    print("EP300 rows-kernel SVM: iterations %d, test AUC %.4f" % (info["iterations"], auc))
    assert auc >= 0.9, auc
    A = f.get_train_kernel_np()
    want = A[:64] @ A[:64].T
    got = f.get_rows_kernel_block_np(0, 64, 0, 64, raw=True)
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-12
    assert f.stats()["test_block_computed"] is False
