"""The class-weighted C-SVC and the Platt calibration (fsk_svm_set_class_weights, fsk_svm_calibrate, fsk_svm_proba;
``fit_svm(class_weight=, probability=)`` / ``predict_proba_np``) on the MI355X: the product library against the yardsticks of
tests/svm_weighted_cases.py through the check functions of tests/test_emu_svm_weighted.py, at scale 1 — every case run to
convergence, the planted-motif 300-row calibration, the pybind11 class against the ctypes path."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402
import svm_weighted_cases as wc  # noqa: E402
from test_emu_svm_weighted import (TABLE, check_branches_reached, check_calibration, check_cv_w, check_table_case,  # noqa: E402
                                   check_unit_weights_and_setter)

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


@pytest.mark.parametrize("name", TABLE)
def test_table_cases(make, name):
    check_table_case(make, name)


def test_case_set_reaches_the_weighted_branches(make):
    check_branches_reached(make)


def test_unit_weights_and_the_setter(make):
    check_unit_weights_and_setter(make)


def test_weighted_cross_validation(make):
    check_cv_w(make)


@pytest.mark.parametrize("skip", [False, True])
def test_calibration_of_the_planted_motif_case(make, skip):
    """300 rows, g = 10, m = 6, weights (4, 1): A < 0 — the decision values of the positives are the large ones."""
    info = check_calibration(make, cases.case(300, 80, 10, 6, n_test=65), (4.0, 1.0), planted=True, skip=skip)
    assert info["A"] < 0


def test_calibration_with_few_positives(make):
    y = -np.ones(64, dtype=np.int32)
    y[[1, 5, 12, 20, 29, 37, 44, 50, 58, 63]] = 1                   # ten positives: two a fold
    check_calibration(make, cases.case(64, 40, 6, 2, labels=y, seed=6403, n_test=3), "balanced")


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
def test_pybind_balanced_and_calibrated_fit(native):
    """fit_svm(class_weight="balanced", probability=True) and predict_proba_np against the ctypes path, to the bit."""
    import fastsk_amd
    from fastsk_amd import FastSK
    y = -np.ones(64, dtype=np.int32)
    y[[1, 5, 12, 20, 29, 37, 44, 50, 58, 63]] = 1
    c = cases.case(64, 40, 6, 2, labels=y, seed=6403, n_test=9)
    n = c["n_train"]
    f = FastSK(g=c["g"], m=c["m"], t=1)
    f.compute_kernel(c["X"][:n], c["X"][n:])
    with pytest.raises(RuntimeError):
        f.predict_proba_np()                                        # no model
    info = f.fit_svm(y)
    assert info["class_weight"] == (1.0, 1.0) and "platt" not in info
    with pytest.raises(RuntimeError):
        f.predict_proba_np()                                        # a model, no calibration
    info = f.fit_svm(y, class_weight="balanced", probability=True)
    w = fastsk_amd.class_weights(y, "balanced")
    assert info["class_weight"] == w == (64 / 20.0, 64 / 108.0)
    e = native.Engine(c["g"], c["m"])
    tok, off = native.flatten(c["X"])
    e.compute(tok, off, n, c["n_test"])
    e.svm_set_class_weights(*w)
    theirs = e.svm_train(y, 1.0, 1e-3)
    platt = e.svm_calibrate(fastsk_amd.stratified_folds(y, 5, seed=0), 5)
    for key in ("iterations", "objective", "n_sv", "n_bsv", "gap", "converged"):
        assert info[key] == theirs[key], key
    for key in ("A", "B", "iterations", "status", "n_folds", "form", "launches"):
        assert info["platt"][key] == platt[key], key
    want = wc.solve_w(e.get_train(), y, w[0], w[1], 1e-3)
    assert info["iterations"] == want["iterations"] and info["n_bsv"] == want["n_bsv"] and np.array_equal(f.get_dual_coef_np(), want["alpha"] * y)
    assert np.array_equal(f.predict_proba_np(), e.svm_proba(n, n + 9)) and np.array_equal(f.predict_proba_np("test"), f.predict_proba_np())
    assert np.array_equal(f.predict_proba_np("train"), e.svm_proba(0, n))
    assert np.array_equal(f.predict_proba_np("train"), wc.sigmoid_predict(f.decision_function_np("train"), platt["A"], platt["B"]))
    with pytest.raises(ValueError):
        f.predict_proba_np("both")
    other = f.fit_svm(y, class_weight={1: 2.0, -1: 0.5}, probability=True, calibration_folds=2, seed=3)
    assert other["class_weight"] == (2.0, 0.5) and other["platt"]["n_folds"] == 2
    e.svm_set_class_weights(2.0, 0.5)
    e.svm_train(y, 1.0, 1e-3)
    platt2 = e.svm_calibrate(fastsk_amd.stratified_folds(y, 2, seed=3), 2)
    assert (other["platt"]["A"], other["platt"]["B"]) == (platt2["A"], platt2["B"])
    for bad in ("auto", (1.0, 0.0), (1.0,), {3: 1.0}):
        with pytest.raises(ValueError):
            f.fit_svm(y, class_weight=bad)
    with pytest.raises(ValueError):
        f.fit_svm(y, probability=True, calibration_folds=1)
    with pytest.raises(NotImplementedError):   # (the reference's stubs stay what they were)
        f.fit()
    with pytest.raises(NotImplementedError):
        f.score()
    e.close()


def test_pybind_weighted_cross_validation_refit(native):
    """cross_validate_svm(class_weight=...) solves weighted problems, and refit=True leaves a weighted model."""
    from fastsk_amd import FastSK
    c = cases.edge_case(96)
    y, n = c["y"], 96
    f = FastSK(g=c["g"], m=c["m"], t=1)
    f.compute_train(c["X"])
    got = f.cross_validate_svm(y, Cs=[0.05, 1.0], folds=3, class_weight=(4.0, 1.0), refit=True)
    assert got["class_weight"] == (4.0, 1.0) and got["refit"]["class_weight"] == (4.0, 1.0)
    K = f.get_train_kernel_np()
    want = wc.expected_w(K, y, got["fold"], (0.05, 1.0), 4.0, 1.0, 1e-3)
    for q, w in zip(got["problems"], want):
        for key in ("iterations", "rho", "objective", "gap", "n_sv", "n_bsv"):
            assert q[key] == w[key], key
    model = wc.solve_w(K, y, got["best_C"] * 4.0, got["best_C"] * 1.0, 1e-3)
    assert got["refit"]["iterations"] == model["iterations"] and got["refit"]["n_bsv"] == model["n_bsv"]
    assert np.array_equal(f.get_dual_coef_np(), model["alpha"] * y) and f.get_intercept() == -model["rho"]
    plain = f.cross_validate_svm(y, Cs=[0.05, 1.0], folds=3)
    assert plain["class_weight"] == (1.0, 1.0)
    assert any(p["objective"] != q["objective"] for p, q in zip(plain["problems"], got["problems"]))
