"""The epsilon-SVR stage (fsk_svr_train / fsk_svr_cv, ``FastSK.fit_svr`` / ``predict_np`` / ``cross_validate_svr``) on the MI355X:
the product library against the yardsticks of tests/svr_cases.py through the check functions of tests/test_emu_svr.py, at scale
1 — every edge of both twin-element loops run to convergence, the 4096-row workgroup (the LDS ceiling), the pybind11 class."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svr_cases as cases  # noqa: E402
from test_emu_svr import (check_all_at_bound, check_automatic_switch, check_both_twins, check_constant_targets, check_cv,  # noqa: E402
                          check_cv_errors, check_cv_kinds, check_decision, check_duplicates, check_errors, check_linear, check_max_iter,
                          check_result_kinds, check_two_launch_edge, check_wide_tube, check_workgroup_edge, computed, same_model)

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


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 513])
def test_two_launch_edges(make, n):
    check_two_launch_edge(make, n)


@pytest.mark.parametrize("n", [2, 32, 33, 511, 512, 513, 1024, 1025])
def test_workgroup_edges(make, n):
    check_workgroup_edge(make, n)


def test_workgroup_of_4096_rows(make):
    """The LDS ceiling: 8192 elements, 16 bytes each, and the reduction scratch — 147,968 bytes, four rows a thread. The launch
    must succeed; 1500 steps against the restatement stopped there, and a pair of the run touches a thread's fourth row."""
    c = cases.edge_case(4096)
    e = computed(make, c, tuning={"svm_wg_max": 8192})
    K = e.get_train()
    want = cases.solve_svr(K, c["z"], 1.0, 0.1, 1e-3, 1500)
    info = e.svr_train(c["z"], 1.0, 0.1, 1e-3, 1500)
    assert info["form"] == "workgroup" and info["launches"] == 1500 // 256 + 1
    _, coef, rho, _ = same_model(e, want, "4096")
    assert any(i % 4096 >= 3072 or j % 4096 >= 3072 for i, j in want["pairs"])   # (a thread's fourth row)
    dec = e.svm_decision(3900, 4096)
    ref, bound = cases.decision_reference(K[3900:], coef, rho)
    assert np.all(np.abs(dec - ref) <= bound)
    e.close()


def test_automatic_switch(make):
    check_automatic_switch(make)


def test_both_twins_positive_at_epsilon_zero(make):
    check_both_twins(make)


def test_tube_wider_than_the_targets(make):
    check_wide_tube(make)


def test_every_support_vector_at_the_bound(make):
    check_all_at_bound(make)


def test_constant_targets(make):
    check_constant_targets(make)


def test_identical_sequences_with_different_targets(make):
    check_duplicates(make)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "group"])
def test_result_kinds(make, kind):
    check_result_kinds(make, kind)


def test_rows_kernel(make):
    check_linear(make)


def test_max_iter(make):
    check_max_iter(make)


@pytest.mark.parametrize("skip", [False, True])
def test_predictions(make, skip):
    check_decision(make, skip)


def test_errors_and_the_model_slot(make):
    check_errors(make)


@pytest.mark.parametrize("form", ["workgroup", "two-launch"])
@pytest.mark.parametrize("grid", [((1.0,), (0.1,)), ((0.5, 1.0, 10.0), (0.0, 0.2))], ids=["1x1", "3x2"])
@pytest.mark.parametrize("n_folds", [2, 5])
@pytest.mark.parametrize("n", [60, 300])
def test_cv(make, n, n_folds, grid, form):
    # (300 rows: every problem stopped at 150 steps and compared with the restatement stopped there — the batch's edges are its
    # shapes, and thirty numpy solves to the end would take the test's time)
    check_cv(make, n, n_folds, grid, form, max_iter=-1 if n == 60 else 150)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "linear"])
def test_cv_result_kinds(make, kind):
    check_cv_kinds(make, kind)


def test_cv_errors(make):
    check_cv_errors(make)


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True, "lazy"])
def test_pybind_fit_and_predict(native, skip):
    """fit_svr / get_dual_coef_np / get_intercept / predict_np / predict_dlpack / decision_function_*: the ctypes view's model, and
    under skip_test_block=True and "lazy" no test x test cell is computed."""
    import torch
    from fastsk_amd import FastSK
    c = cases.edge_case(90, n_test=65)
    n = c["n_train"]
    f = FastSK(g=c["g"], m=c["m"], t=1, skip_test_block=skip)
    f.compute_kernel(c["X"][:n], c["X"][n:])
    before = f.stats()["test_block_computed"]
    assert before == (skip != "lazy")
    info = f.fit_svr(c["z"], C=2.0, epsilon=0.05)
    Ktr, Kte = f.get_train_kernel_np(), f.get_test_kernel_np()
    want = cases.solve_svr(Ktr, c["z"], 2.0, 0.05, 1e-3)
    assert info["iterations"] == want["iterations"] and info["objective"] == want["objective"] and info["converged"]
    assert info["form"] == "workgroup" and info["n_sv"] == want["n_sv"] and info["n_bsv"] == want["n_bsv"] and info["ms"] > 0
    assert info["epsilon"] == 0.05 and info["kernel_type"] == "fastsk"
    coef = f.get_dual_coef_np()
    assert np.array_equal(coef, want["coef"]) and f.get_intercept() == -want["rho"]
    for which, K_rows in (("test", Kte), ("train", Ktr)):
        pred = f.predict_np(which)
        ref, bound = cases.decision_reference(K_rows, want["coef"], want["rho"])
        assert np.all(np.abs(pred - ref) <= bound), which
        assert np.array_equal(f.decision_function_np(which), pred)
        for capsule in (f.predict_dlpack(which), f.decision_function_dlpack(which)):
            on_gpu = torch.from_dlpack(capsule)
            assert on_gpu.is_cuda and on_gpu.dtype == torch.float64 and np.array_equal(on_gpu.cpu().numpy().reshape(-1), pred)
    assert np.array_equal(f.predict_np(), f.predict_np("test"))
    assert f.stats()["test_block_computed"] == before
    cases.certify(Ktr, c["z"], coef, 2.0, 0.05, 1e-3)
    with pytest.raises(RuntimeError):
        f.predict_proba_np("train")                    # an SVR model has no probabilities
    # the one slot: a C-SVC replaces it, and the reverse
    f.fit_svm(c["y"])
    assert np.all(np.sign(f.get_dual_coef_np()) * c["y"] >= 0) and not np.array_equal(f.get_dual_coef_np(), coef)
    assert f.fit_svr(c["z"], C=2.0, epsilon=0.05, kernel_type="fastsk")["objective"] == want["objective"]
    assert np.array_equal(f.get_dual_coef_np(), coef)
    lin = f.fit_svr(c["z"], kernel_type="linear")
    assert lin["kernel_type"] == "linear" and lin["converged"] and f.predict_np("test").shape == (65,)


def test_pybind_errors(native):
    from fastsk_amd import FastSK
    c = cases.edge_case(20, n_test=3)
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(RuntimeError):
        f.fit_svr(c["z"])                               # nothing computed
    f.compute_kernel(c["X"][:20], c["X"][20:])
    with pytest.raises(RuntimeError):
        f.predict_np()                                 # no model yet
    bad = c["z"].copy()
    bad[3] = np.nan
    for z, kw in ((c["z"][:19], {}), (bad, {}), (c["z"], {"C": 0.0}), (c["z"], {"epsilon": -1.0}), (c["z"], {"eps": float("inf")}),
                  (c["z"].reshape(4, 5), {}), (c["z"], {"kernel_type": "rbf"})):
        with pytest.raises(ValueError):
            f.fit_svr(z, **kw)
    assert f.fit_svr(c["z"], max_iter=3)["converged"] is False
    assert f.fit_svr(c["z"])["converged"] is True
    f.compute_train(c["X"][:20])                       # a new result: the model is gone
    for call in (f.get_dual_coef_np, f.get_intercept, lambda: f.predict_np("train")):
        with pytest.raises(RuntimeError):
            call()


def test_pybind_cross_validate(native):
    """cross_validate_svr: the ctypes view's result, best_* by the smallest mse (the lowest index among equals), refit."""
    import fastsk_amd
    from fastsk_amd import FastSK
    c = cases.edge_case(60)
    f = FastSK(g=c["g"], m=c["m"], t=1)
    f.compute_train(c["X"])
    Cs, epsilons = [0.5, 1.0, 10.0], [0.0, 0.2]
    out = f.cross_validate_svr(c["z"], Cs=Cs, epsilons=epsilons, folds=5, seed=4, refit=True)
    fold = fastsk_amd.kfold(60, 5, seed=4)
    assert np.array_equal(out["fold"], fold) and out["oof"].shape == (3, 2, 60) and len(out["problems"]) == 30
    for k in ("mse", "mae", "r2", "r"):
        assert out[k].shape == (3, 2)
        for ci in range(3):
            for q in range(2):
                assert out[k][ci, q] == cases.scores(out["oof"][ci, q], c["z"])[k]
    best = int(np.argmin(out["mse"].reshape(-1)))      # (numpy's argmin: the first of equals)
    assert out["best_C"] == Cs[best // 2] and out["best_epsilon"] == epsilons[best % 2]
    assert out["info"]["form"] == "workgroup" and out["info"]["n_eps"] == 2 and out["info"]["n_folds"] == 5
    K = f.get_train_kernel_np()
    want = cases.solve_svr(K, c["z"], out["best_C"], out["best_epsilon"], 1e-3)
    assert out["refit"]["objective"] == want["objective"] and np.array_equal(f.get_dual_coef_np(), want["coef"])
    # equal scores: a grid that repeats a point keeps the lowest index; folds as an array; no refit
    twice = f.cross_validate_svr(c["z"], Cs=[out["best_C"], out["best_C"]], epsilons=[out["best_epsilon"]], folds=fold)
    assert twice["mse"][0, 0] == twice["mse"][1, 0] == out["mse"].reshape(-1)[best] and twice["refit"] is None
    assert twice["best_C"] == out["best_C"] and np.array_equal(twice["oof"][0], twice["oof"][1])
    with pytest.raises(ValueError):
        f.cross_validate_svr(c["z"], Cs=[1.0], epsilons=[-0.1])
    with pytest.raises(ValueError):
        f.cross_validate_svr(c["z"], folds=1)
