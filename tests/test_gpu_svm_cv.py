"""The cross-validated SVM (fsk_svm_cv, ``Engine.svm_cv``, ``FastSK.cross_validate_svm``) on the MI355X: the product library
against the yardsticks of tests/svm_cv_cases.py through the check functions of tests/test_emu_svm_cv.py, at the sizes of the
batch kernels' edges and run to convergence — unequal problems in one launch, the thread and element edges of the workgroup
form, unequal workgroup counts in one two-launch grid, more problems than compute units, the 8192-row problem (the LDS
budget), the pybind11 class, EP300 end to end."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_tokens

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402
import svm_cv_cases as cv  # noqa: E402
from test_emu_svm import computed  # noqa: E402
from test_emu_svm_cv import (check_duplicates, check_errors, check_index_mapping, check_many_problems, check_metrics, check_oof,  # noqa: E402
                             check_result_kinds, check_stratified_folds, check_two_launch_edge, check_unequal, check_workgroup_edge,
                             same_problems)

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


@pytest.mark.parametrize("n,runs", [(1030, ((0, 1028), (1, 1), (2, 1))), (1088, ((0, 1024), (1, 63), (2, 1)))])
def test_unequal_problems_in_one_launch(make, n, runs):
    """n_p = 2 and twice 1029; n_p = 64, 1025 and 1087."""
    check_unequal(make, n, runs)


@pytest.mark.parametrize("n_p", [64, 65, 1023, 1024, 1025])
def test_workgroup_edges(make, n_p):
    check_workgroup_edge(make, n_p)


@pytest.mark.parametrize("n,runs", [(770, ((0, 257), (1, 513))), (258, ((0, 256), (1, 2)))])
def test_two_launch_edges(make, n, runs):
    """n_p = 513 and 257: 3 and 2 workgroups a problem in one grid; n_p = 2 and 256."""
    check_two_launch_edge(make, n, runs)


def test_more_problems_than_compute_units(make):
    """10 folds x 30 values of C: 300 problems on 256 compute units."""
    check_many_problems(make, 30)


def test_lds_ceiling(make):
    """n = 8200, fold 0 of 8 rows, fold 1 of 8192: problems of 8192 and of 8 rows in one launch, the only size at which the
    LDS budget can fail (156,160 bytes). 1500 steps against the restatement stopped there. One row fewer in svm_wg_max and the
    same call takes the two launches."""
    c = cases.case(8200, 60, 8, 4)
    fold = cv.blocks((0, 8), (1, 8192))
    e = computed(make, c)
    K, y = e.get_train(), c["y"]
    want = cv.expected(K, y, fold, (1.0,), c["eps"], 1500)
    assert [len(w["idx"]) for w in want] == [8192, 8] and want[0]["iterations"] == 1500
    got = e.svm_cv(y, fold, (1.0,), c["eps"], 1500)
    assert got["form"] == "workgroup" and got["launches"] == 1500 // 256 + 1
    same_problems(e, got, want, "8192")
    assert any(i >= 7168 or j >= 7168 for i, j in want[0]["pairs"])   # (a thread's eighth element)
    first = got["decision"]
    e.set_tuning("svm_wg_max", 8191)
    want = cv.expected(K, y, fold, (1.0,), c["eps"], 50)
    got = e.svm_cv(y, fold, (1.0,), c["eps"], 50)
    assert got["form"] == "two-launch"
    same_problems(e, got, want, "8191")
    assert first.shape == got["decision"].shape == (1, 8200)
    e.close()


def test_index_mapping(make):
    check_index_mapping(make)


def test_duplicate_pair_in_one_training_set_and_split(make):
    check_duplicates(make)


@pytest.mark.parametrize("kind", ["fp64", "mismatch"])
def test_result_kinds(make, kind):
    check_result_kinds(make, kind)


@pytest.mark.parametrize("n", [63, 64, 65, 66])
def test_out_of_fold_rows(make, n):
    check_oof(make, n)


def test_metrics(make):
    check_metrics(make)


def test_errors_and_the_results_life(make):
    check_errors(make)


def test_stratified_folds():
    check_stratified_folds()


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
def test_pybind_cross_validate(native):
    """An int ``folds`` is stratified_folds (restated here); an array of fold ids gives Engine.svm_cv's result; refit=True
    leaves fit_svm(C=best_C)'s model; best_C is the C of the highest AUC, the smallest of equals."""
    from fastsk_amd import FastSK
    c = cases.edge_case(90, n_test=5)
    n, y = c["n_train"], c["y"]
    Cs = (100.0, 0.05, 1.0)
    f = FastSK(g=c["g"], m=c["m"], t=1)
    f.compute_kernel(c["X"][:n], c["X"][n:])
    r = f.cross_validate_svm(y, Cs=Cs, folds=3, seed=4)
    fold = cv.stratified_folds_restated(y, 3, seed=4)
    assert np.array_equal(r["fold"], fold)
    e = computed(lambda g, m, **kw: native.Engine(g, m, **kw), c)
    want = e.svm_cv(y, fold, Cs)
    e.close()
    by_array = f.cross_validate_svm(y, Cs=Cs, folds=fold)
    for got in (r, by_array):
        assert np.array_equal(got["decision"], want["decision"]) and got["problems"] == want["problems"]
        assert np.array_equal(got["auc"], want["auc"]) and np.array_equal(got["accuracy"], want["accuracy"])
        assert got["form"] == want["form"] == "workgroup" and got["launches"] == want["launches"] and got["ms"] > 0
        best = max(range(3), key=lambda ci: (got["auc"][ci], -Cs[ci]))
        assert got["best_C"] == Cs[best]
    # equal values of C score equal AUCs: the tie goes to the smallest C, wherever it stands
    tie = f.cross_validate_svm(y, Cs=(2.0, 1.0, 1.0, 2.0), folds=fold)
    assert tie["auc"][0] == tie["auc"][3] and tie["auc"][1] == tie["auc"][2]
    assert tie["best_C"] == (1.0 if tie["auc"][1] >= tie["auc"][0] else 2.0)
    same = f.cross_validate_svm(y, Cs=(1.0, 1.0), folds=fold)
    assert same["best_C"] == 1.0
    with pytest.raises(RuntimeError):
        f.get_dual_coef_np()                           # no model: cross-validation alone trains none
    r = f.cross_validate_svm(y, Cs=Cs, folds=fold, refit=True)
    coef, b = f.get_dual_coef_np(), f.get_intercept()
    dec = f.decision_function_np("test")
    f.fit_svm(y, C=r["best_C"])
    assert np.array_equal(coef, f.get_dual_coef_np()) and b == f.get_intercept() and np.array_equal(dec, f.decision_function_np("test"))
    default = f.cross_validate_svm(y)
    assert default["decision"].shape == (1, n) and len(default["problems"]) == 5 and default["best_C"] == 1.0
    assert np.array_equal(default["fold"], cv.stratified_folds_restated(y, 5, seed=0))
    with pytest.raises(NotImplementedError):
        f.fit()


def test_pybind_errors(native):
    from fastsk_amd import FastSK
    c = cases.edge_case(20, n_test=3)
    y = c["y"]
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(RuntimeError):
        f.cross_validate_svm(y)                        # nothing computed
    f.compute_kernel(c["X"][:20], c["X"][20:])
    bad = y.copy()
    bad[3] = 0
    for labels, kw in ((y[:19], {}), (bad, {}), (y, {"Cs": (1.0, 0.0)}), (y, {"Cs": ()}), (y, {"eps": -1.0}), (y, {"folds": 1}),
                       (y, {"folds": np.zeros(20, dtype=np.int32)}), (y, {"folds": np.arange(19) % 2}),
                       (y, {"folds": np.arange(20) % 2}), (y.reshape(4, 5), {})):
        with pytest.raises(ValueError):
            f.cross_validate_svm(labels, **kw)
    r = f.cross_validate_svm(y, folds=2, max_iter=3)
    assert [q["converged"] for q in r["problems"]] == [False, False]
    assert all(q["converged"] for q in f.cross_validate_svm(y, folds=2)["problems"])


def test_ep300_end_to_end(native):
    """EP300, g = 10, m = 6 exact, 5 stratified folds x 3 values of C in one batch: every problem converges, the best
    out-of-fold AUC reaches the bar test_ep300_end_to_end sets, and no test x test cell is computed under "lazy"."""
    from fastsk_amd import FastSK
    tokens, offsets, ntr, nte, ytr, yte = load_tokens("EP300")
    f = FastSK(g=10, m=6, t=1, skip_test_block="lazy")
    f.compute_kernel_flat(tokens, offsets, ntr)
    y = np.where(np.asarray(ytr) > 0, 1, -1).astype(np.int32)
    r = f.cross_validate_svm(y, Cs=(0.1, 1.0, 10.0), folds=5)
    assert len(r["problems"]) == 15 and all(q["converged"] for q in r["problems"]) and r["form"] == "workgroup"
    assert r["decision"].shape == (3, ntr) and max(r["auc"]) >= 0.9, r["auc"]
    assert r["best_C"] in (0.1, 1.0, 10.0) and r["auc"][(0.1, 1.0, 10.0).index(r["best_C"])] == max(r["auc"])
    assert f.stats()["test_block_computed"] is False
