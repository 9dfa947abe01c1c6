"""The SVM stage (fsk_svm_train / fsk_svm_decision, ``FastSK.fit_svm`` / ``decision_function_np``) on the MI355X: the product
library against the yardsticks of tests/svm_cases.py through the check functions of tests/test_emu_svm.py, at scale 1 — every
edge of both loops run to convergence, the 8192-row workgroup (the LDS budget), the pybind11 class, EP300 end to end."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_tokens

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402
from test_emu_svm import (check_automatic_switch, check_bounds, check_case, check_decision, check_duplicates, check_errors,  # noqa: E402
                          check_max_iter, check_no_candidate, check_result_kinds, check_tuning_keys, check_two_launch_edge, check_unbalanced,
                          check_workgroup_edge, computed, same_model)

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


@pytest.mark.parametrize("name", ["n96", "n300", "n300_C100", "n700", "all_at_bound"])
def test_table_cases(make, name):
    c = cases.table_cases()[name]
    want = check_case(make, c)
    assert want["converged"]
    if name == "all_at_bound":
        assert want["iterations"] == 32 and want["n_bsv"] == c["n_train"]
    if name == "n300_C100":
        assert want["n_bsv"] == 0


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 513])
def test_two_launch_edges(make, n):
    check_two_launch_edge(make, n)


@pytest.mark.parametrize("n", [2, 64, 1023, 1024, 1025])
def test_workgroup_edges(make, n):
    check_workgroup_edge(make, n)


def test_workgroup_of_8192_rows(make):
    """The only size at which the LDS budget can fail: 17 bytes a row and the reduction scratch, 156,160 bytes. 1500 steps
    against the restatement stopped there (the launch, the eight elements a thread and the write-back are what is new)."""
    c = cases.case(8192, 60, 8, 4)
    e = computed(make, c)
    K = e.get_train()
    want = cases.solve(K, c["y"], c["C"], c["eps"], 1500)
    info = e.svm_train(c["y"], c["C"], c["eps"], 1500)
    assert info["form"] == "workgroup" and info["launches"] == 1500 // 256 + 1
    alpha, rho, _ = same_model(e, want, "8192")
    assert any(i >= 7168 or j >= 7168 for i, j in want["pairs"])   # (a thread's eighth element)
    dec = e.svm_decision(8000, 8192)
    ref, bound = cases.decision_reference(K[8000:], c["y"], alpha, rho)
    assert np.all(np.abs(dec - ref) <= bound)
    e.close()


def test_automatic_switch(make):
    check_automatic_switch(make)


def test_all_and_none_at_the_bound(make):
    check_bounds(make)


def test_duplicate_sequences_with_opposite_labels(make):
    check_duplicates(make)


def test_one_positive_in_64(make):
    check_unbalanced(make)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "group"])
def test_result_kinds(make, kind):
    check_result_kinds(make, kind)


def test_max_iter(make):
    check_max_iter(make)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("n_test", [1, 63, 64, 65])
def test_decision_values(make, n_test, skip):
    check_decision(make, n_test, skip)


def test_errors_and_the_models_life(make):
    import torch

    def device_buffer(n):
        t = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        return t.data_ptr(), lambda: t.cpu().numpy()

    check_errors(make, device_buffer)


def test_no_j_candidate_ends_the_solve(make):
    check_no_candidate(make)


def test_tuning_keys(native):
    check_tuning_keys(native.library())


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True, "lazy"])
def test_pybind_fit_and_decision(native, skip):
    """fit_svm / get_dual_coef_np / get_intercept / decision_function_np / _dlpack: the ctypes view's model, and under
    skip_test_block=True and "lazy" no recompute of the test x test block."""
    import torch
    from fastsk_amd import FastSK
    c = cases.edge_case(90, n_test=65)
    n = c["n_train"]
    f = FastSK(g=c["g"], m=c["m"], t=1, skip_test_block=skip)
    f.compute_kernel(c["X"][:n], c["X"][n:])
    before = f.stats()["test_block_computed"]
    assert before == (skip != "lazy")   # (the key speaks of the lazy block alone: under True there is nothing to come)
    info = f.fit_svm(c["y"], C=c["C"], eps=c["eps"])
    Ktr, Kte = f.get_train_kernel_np(), f.get_test_kernel_np()
    want = cases.solve(Ktr, c["y"], c["C"], c["eps"])
    assert info["iterations"] == want["iterations"] and info["objective"] == want["objective"] and info["converged"]
    assert info["form"] == "workgroup" and info["n_sv"] == want["n_sv"] and info["n_bsv"] == want["n_bsv"] and info["ms"] > 0
    coef = f.get_dual_coef_np()
    assert np.array_equal(coef, want["alpha"] * c["y"]) and f.get_intercept() == -want["rho"]
    for which, K_rows in (("test", Kte), ("train", Ktr)):
        dec = f.decision_function_np(which)
        ref, bound = cases.decision_reference(K_rows, c["y"], want["alpha"], want["rho"])
        assert np.all(np.abs(dec - ref) <= bound), which
        on_gpu = torch.from_dlpack(f.decision_function_dlpack(which))
        assert on_gpu.is_cuda and on_gpu.dtype == torch.float64 and np.array_equal(on_gpu.cpu().numpy().reshape(-1), dec)
    assert np.array_equal(f.decision_function_np(), f.decision_function_np("test"))
    assert f.stats()["test_block_computed"] == before   # ("lazy": still false — nothing asked for a test x test cell)
    cases.certify(Ktr, c["y"], np.abs(coef), c["C"], c["eps"])
    with pytest.raises(NotImplementedError):   # (the reference's stubs stay what they were)
        f.fit()


def test_pybind_errors(native):
    from fastsk_amd import FastSK
    c = cases.edge_case(20, n_test=3)
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(RuntimeError):
        f.fit_svm(c["y"])                              # nothing computed
    f.compute_kernel(c["X"][:20], c["X"][20:])
    for call in (f.get_dual_coef_np, f.get_intercept, f.decision_function_np, lambda: f.decision_function_dlpack("test")):
        with pytest.raises(RuntimeError):
            call()                                     # no model yet
    bad = c["y"].copy()
    bad[3] = 0
    for labels, kw in ((c["y"][:19], {}), (bad, {}), (np.ones(20, dtype=np.int32), {}), (c["y"], {"C": 0.0}), (c["y"], {"C": float("nan")}),
                       (c["y"], {"eps": -1.0}), (c["y"], {"eps": float("inf")}), (c["y"].reshape(4, 5), {})):
        with pytest.raises(ValueError):
            f.fit_svm(labels, **kw)
    assert f.fit_svm(c["y"], max_iter=3)["converged"] is False
    assert f.fit_svm(c["y"])["converged"] is True
    with pytest.raises(ValueError):
        f.decision_function_np("both")
    assert f.decision_function_np("train").shape == (20,)
    f.compute_train(c["X"][:20])                       # a new result: the model is gone
    for call in (f.get_dual_coef_np, f.get_intercept, lambda: f.decision_function_np("train")):
        with pytest.raises(RuntimeError):
            call()


def test_ep300_end_to_end(native):
    """EP300, g = 10, m = 6 exact: fit_svm + decision_function_np("test") reach the bar test_run_check_style_auc sets for the
    LinearSVC pipeline, with nothing but three vectors leaving the device."""
    from sklearn.metrics import roc_auc_score
    from fastsk_amd import FastSK
    tokens, offsets, ntr, nte, ytr, yte = load_tokens("EP300")
    f = FastSK(g=10, m=6, t=1, skip_test_block="lazy")
    f.compute_kernel_flat(tokens, offsets, ntr)
    info = f.fit_svm(np.where(np.asarray(ytr) > 0, 1, -1).astype(np.int32), C=1.0, eps=1e-3)
    assert info["converged"] and info["form"] == "workgroup"
    auc = roc_auc_score(np.asarray(yte) > 0, f.decision_function_np("test"))
    assert auc >= 0.9, auc
    assert f.stats()["test_block_computed"] is False
