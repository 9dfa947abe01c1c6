"""The one-vs-one multi-class C-SVC (fsk_svm_train_multiclass, fsk_svm_multiclass_decision, fsk_svm_multiclass_cv;
``fit_svm_multiclass``, ``predict_class_np``, ``cross_validate_svm_multiclass``) on the MI355X: the product library against the
yardsticks of tests/svm_multiclass_cases.py through the check functions of tests/test_emu_svm_multiclass.py, at the sizes of
the kernels' edges and run to convergence — the lane and stride edges of the vote kernel, the 1024-thread edge of the
workgroup form against the two launches, 2016 problems with every vote lane in use, the pybind11 class, and the WebKB slice
of tests/golden/webkb_slice.npz against scikit-learn's recorded result."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_multiclass_cases as mc  # noqa: E402
from test_emu_svm import computed  # noqa: E402
from test_emu_svm_multiclass import (check_class_weights, check_cv, check_cv_errors, check_fit, check_forms, check_label_values,  # noqa: E402
                                     check_lane_edges, check_linear, check_many_classes, check_reader, check_state, check_tiny,
                                     check_vote_tie, cv_case)

pytestmark = pytest.mark.gpu
NAME = "multi-class C-SVC"


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


def test_tiny_pairs(make):
    check_tiny(make)


def test_lane_edges_and_a_foreign_row(make):
    check_lane_edges(make)


def test_both_forms_at_the_workgroup_edge(make):
    """(512, 513, 1): pairs of 1025, 513 and 514 rows — the 1024-thread edge of the workgroup form; with svm_wg_max = 512 the
    two launches with 5, 3 and 3 workgroups in one grid. Run to convergence; both give the same model."""
    check_forms(make, (512, 513, 1), 512, (5, 3, 3))


def test_sixty_four_classes(make):
    """2016 problems of 4 rows on 256 compute units, every vote lane in use, every row of the N-set; k = 65 is refused."""
    check_many_classes(make)


def test_label_values(make):
    check_label_values(make)


def test_vote_tie(make):
    check_vote_tie(make)


def test_class_weights(make):
    check_class_weights(make)


def test_linear_kernel(make):
    check_linear(make)


def test_cross_validation(make):
    check_cv(make)


def test_cross_validation_errors_and_life(make):
    check_cv_errors(make)


def test_model_slot(make):
    import torch

    def device_buffers(n_dec, n_pred):
        dec = torch.zeros(n_dec, dtype=torch.float64, device="cuda:0")
        pred = torch.zeros(n_pred, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        return dec.data_ptr(), pred.data_ptr(), lambda: (dec.cpu().numpy(), pred.cpu().numpy())

    check_state(make, device_buffers)


def test_reader_multiclass(tmp_path):
    check_reader(tmp_path)


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
def test_pybind_fit_predict(native):
    """fit_svm_multiclass / decision_function_np [rows, P] / predict_class_np give Engine.svm_train_multiclass's result; the
    binary accessors raise RuntimeError naming the model; fit_svm afterwards restores 1-D decisions; a second compute_kernel
    drops the model; class weights as a dict and "balanced"; kernel_type="linear"."""
    from fastsk_amd import FastSK
    c = mc.case((30, 6, 14), n_test=5, labels=(5, -3, 8))
    n, y = c["n_train"], c["y"]
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(RuntimeError):
        f.fit_svm_multiclass(y)                                # nothing computed
    f.compute_kernel(c["X"][:n], c["X"][n:])
    with pytest.raises(RuntimeError):
        f.predict_class_np()                                   # no model
    e = computed(lambda g, m, **kw: native.Engine(g, m, **kw), c)
    for cw in (None, {5: 0.5, 8: 3.0}, "balanced"):
        info = f.fit_svm_multiclass(y, C=2.0, class_weight=cw)
        want = e.svm_train_multiclass(y, 2.0, class_weight=cw)
        model = e.svm_multiclass_model()
        assert info["classes"].tolist() == [-3, 5, 8] and info["k"] == 3 and info["n_pairs"] == 3 and info["converged"]
        assert info["pairs"] == model["pairs"] and info["n_sv"] == want["n_sv"] and info["form"] == want["form"] == "workgroup"
        assert info["launches"] == want["launches"] and info["ms"] > 0 and info["kernel_type"] == "fastsk"
        if cw is None:
            assert info["class_weight"] is None
        else:
            assert np.array_equal(info["class_weight"], native.multiclass_weights(y, cw))
        for which, (r0, r1) in (("test", (n, n + 5)), ("train", (0, n))):
            dec, pred = e.svm_multiclass_decision(r0, r1)
            got = f.decision_function_np(which)
            assert got.shape == (r1 - r0, 3) and np.array_equal(got, dec)
            assert np.array_equal(f.predict_class_np(which), pred) and f.predict_class_np(which).dtype == np.int32
    assert np.array_equal(f.decision_function_np(), f.decision_function_np("test"))
    for call in (f.predict_proba_np, f.get_dual_coef_np, f.get_intercept, f.decision_function_dlpack):
        with pytest.raises(RuntimeError, match=NAME):
            call()
    for bad in ({"class_weight": {7: 1.0}}, {"class_weight": {5: -1.0}}, {"class_weight": "even"}, {"C": 0.0}, {"eps": -1.0},
                {"kernel_type": "rbf"}):
        with pytest.raises(ValueError):
            f.fit_svm_multiclass(y, **bad)
    for labels in (y[:-1], np.full(n, 5, dtype=np.int32), y.reshape(5, 10)):
        with pytest.raises(ValueError):
            f.fit_svm_multiclass(labels)
    assert f.decision_function_np().shape == (5, 3)              # a refused call keeps the model
    # the binary fit takes the slot back, and the reverse
    yb = np.where(y == 5, 1, -1).astype(np.int32)
    f.fit_svm(yb)
    assert f.decision_function_np().shape == (5,) and f.get_dual_coef_np().shape == (n,)
    with pytest.raises(RuntimeError, match=r"C-SVC \(fsk_svm_train\)"):
        f.predict_class_np()
    f.fit_svr(y.astype(np.float64))
    with pytest.raises(RuntimeError, match="epsilon-SVR"):
        f.predict_class_np()
    f.fit_svm_multiclass(y)
    with pytest.raises(RuntimeError, match=NAME):
        f.get_dual_coef_np()
    # the rows kernel
    lin = f.fit_svm_multiclass(y, kernel_type="linear")
    e.svm_set_kernel("linear")
    e.svm_train_multiclass(y)
    assert lin["kernel_type"] == "linear" and lin["pairs"] == e.svm_multiclass_model()["pairs"]
    assert np.array_equal(f.decision_function_np("train"), e.svm_multiclass_decision(0, n)[0])
    e.close()
    # a new kernel drops the model
    f.compute_kernel(c["X"][:n], c["X"][n:])
    with pytest.raises(RuntimeError):
        f.predict_class_np()
    with pytest.raises(RuntimeError):
        f.decision_function_np()


def test_pybind_cross_validate(native):
    """An int ``folds`` is stratified_folds on the integer labels; an array of fold ids gives Engine.svm_multiclass_cv's
    result; best_C is the C of the highest accuracy, the smallest of equals; refit=True leaves fit_svm_multiclass(C=best_C)'s
    model."""
    from fastsk_amd import FastSK, stratified_folds
    c, fold = cv_case()
    n, y = c["n_train"], c["y"]
    Cs = (2.0, 0.5)
    f = FastSK(g=c["g"], m=c["m"], t=1)
    with pytest.raises(RuntimeError):
        f.cross_validate_svm_multiclass(y)                     # nothing computed
    f.compute_kernel(c["X"][:n], c["X"][n:])
    e = computed(lambda g, m, **kw: native.Engine(g, m, **kw), c)
    want = e.svm_multiclass_cv(y, fold, Cs)
    got = f.cross_validate_svm_multiclass(y, Cs=Cs, folds=fold)
    assert np.array_equal(got["pred"], want["pred"]) and np.array_equal(got["accuracy"], want["accuracy"])
    assert got["problems"] == want["problems"] and len(got["problems"]) == 18 and got["k"] == 3
    assert got["form"] == want["form"] == "workgroup" and got["launches"] == want["launches"] and got["ms"] > 0
    best = max(range(2), key=lambda ci: (got["accuracy"][ci], -Cs[ci]))
    assert got["best_C"] == Cs[best] and got["class_weight"] is None and "refit" not in got
    with pytest.raises(RuntimeError):
        f.predict_class_np()                                   # cross-validation alone trains no model
    by_int = f.cross_validate_svm_multiclass(y, Cs=Cs, folds=3, seed=4)
    assert np.array_equal(by_int["fold"], stratified_folds(y, 3, seed=4))
    assert np.array_equal(by_int["pred"], e.svm_multiclass_cv(y, by_int["fold"], Cs)["pred"])
    # equal values of C score equal accuracies: the tie goes to the smallest C, wherever it stands
    tie = f.cross_validate_svm_multiclass(y, Cs=(2.0, 0.5, 0.5, 2.0), folds=fold)
    assert tie["accuracy"][0] == tie["accuracy"][3] and tie["accuracy"][1] == tie["accuracy"][2]
    assert tie["best_C"] == (0.5 if tie["accuracy"][1] >= tie["accuracy"][0] else 2.0)
    assert f.cross_validate_svm_multiclass(y, Cs=(2.0, 2.0), folds=fold)["best_C"] == 2.0
    # refit, with weights
    bal = mc.balanced(y)
    r = f.cross_validate_svm_multiclass(y, Cs=Cs, folds=fold, refit=True, class_weight="balanced")
    assert np.array_equal(r["pred"], e.svm_multiclass_cv(y, fold, Cs, class_weight=bal)["pred"])
    dec, pred = f.decision_function_np("test"), f.predict_class_np("test")
    info = f.fit_svm_multiclass(y, C=r["best_C"], class_weight=bal)
    assert info["pairs"] == r["refit"]["pairs"]
    assert np.array_equal(dec, f.decision_function_np("test")) and np.array_equal(pred, f.predict_class_np("test"))
    e.close()
    for kw in ({"Cs": (1.0, 0.0)}, {"Cs": ()}, {"eps": -1.0}, {"folds": 1}, {"folds": np.zeros(n, dtype=np.int32)},
               {"folds": fold[:-1]}, {"class_weight": {4: 0.0}}):
        with pytest.raises(ValueError):
            f.cross_validate_svm_multiclass(y, **kw)
    default = f.cross_validate_svm_multiclass(y)
    assert default["pred"].shape == (1, n) and len(default["problems"]) == 15 and default["best_C"] == 1.0


# ---- the WebKB slice ------------------------------------------------------------------------------------------------------------
def test_webkb_slice_against_scikit_learn(native):
    """240 + 80 documents of the reference's four-class WebKB data (tests/make_golden_webkb.py), g = 8, m = 4, C = 1.
    1. The engine's pairs, decision values and labels equal the restatement exactly.
    2. Its labels equal scikit-learn's recorded labels on every row whose recorded pair decisions all exceed 0.01 in magnitude
       (ten times the stopping tolerance; the restatement and scikit-learn differ by less than 1e-3 in any decision value on
       this slice); at most 10 % of the rows may be left out — a condition, not a measurement: on the CPU oracle 5 of the 80
       test rows and 12 of the 240 train rows fall under the margin. Accuracy 0.75 on the test rows."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "webkb_slice.npz"))
    n, N = int(z["n_train"]), len(z["offsets"]) - 1
    y = z["labels"][:n]
    e = native.Engine(int(z["g"]), int(z["m"]))
    e.compute(z["tokens"], z["offsets"], n, N - n)
    c = {"y": y, "C": 1.0, "eps": 1e-3}
    classes, want, dec, labels, _ = check_fit(None, c, forms=(("workgroup", 8192),), chunks=(256,), engine=e, ranges=False)
    e.close()
    assert classes.tolist() == [0, 1, 2, 3] and all(w["converged"] for w in want)
    for name, rows in (("test", slice(n, N)), ("train", slice(0, n))):
        sk_dec, sk_pred = z["sk_dec_" + name], z["sk_pred_" + name]
        sure = np.all(np.abs(sk_dec) > 0.01, axis=1)
        print(name, "rows under the margin:", int((~sure).sum()), "largest difference to scikit-learn:", float(np.abs(dec[rows] - sk_dec).max()))
        assert int((~sure).sum()) * 10 <= len(sure), (name, int((~sure).sum()))
        assert np.array_equal(labels[rows][sure], sk_pred[sure]), name
    assert float(int((labels[n:] == z["labels"][n:]).sum())) / float(N - n) == 0.75
