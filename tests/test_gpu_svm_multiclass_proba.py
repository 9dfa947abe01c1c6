"""The multi-class probabilities (fsk_svm_multiclass_calibrate, fsk_svm_multiclass_proba; ``fit_svm_multiclass(probability=True)``,
``predict_proba_np``, ``predict_proba_dlpack``, ``predict_class_np(rule="proba")``) on the MI355X: the product library against the
yardsticks of tests/svm_multiclass_proba_cases.py through the check functions of tests/test_emu_svm_multiclass_proba.py, run to
convergence and at the kernel's edges — every lane a class and 64,512 bytes of LDS at 64 classes, dead waves and row offsets,
fold lists past 1024 rows in both solver forms — then the pybind11 class and the WebKB slice of tests/golden/webkb_slice.npz."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_multiclass_cases as mc  # noqa: E402
import svm_multiclass_proba_cases as pc  # noqa: E402
from test_emu_svm import computed  # noqa: E402
from test_emu_svm_multiclass_proba import (check_calibrate_forms, check_calibrate_four_classes, check_calibrate_linear,  # noqa: E402
                                           check_calibrate_three_classes, check_calibrate_weighted, check_errors_and_life, check_exp,
                                           check_launch_edges, check_many_classes, check_sigmoids, check_special_sigmoids, mod_folds)

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


def test_exp_neg_bits_and_bound(native):
    """The product library's host export: the same bits as the restatement, within 2 ulp of math.exp."""
    check_exp(native.library())


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
def test_seeded_sigmoids(make, k):
    check_sigmoids(make, k)


def test_special_sigmoids(make):
    check_special_sigmoids(make)


def test_sixty_four_classes(make):
    """P = 2016 pairs run to convergence; the last ten training rows and both test rows (the restatement of a 64-class coupling
    in Python floats is what costs the time, not the launch)."""
    check_many_classes(make, span=(118, 130))


def test_launch_edges_and_null_outputs(make):
    import torch

    def device_buffers(n_prob, n_int):
        prob = torch.zeros(n_prob, dtype=torch.float64, device="cuda:0")
        ints = torch.zeros(n_int, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        return prob.data_ptr(), ints.data_ptr(), lambda: (prob.cpu().numpy(), ints.cpu().numpy())

    check_launch_edges(make, device_buffers)


def test_calibrate_three_classes(make):
    check_calibrate_three_classes(make)


def test_calibrate_four_classes_five_folds(make):
    check_calibrate_four_classes(make)


def test_calibrate_both_forms_past_1024_rows(make):
    """(775, 775, 6), 3 folds: the largest fold lists hold about 1035 rows — past the 1024 threads of the workgroup form — and
    with svm_wg_max = 512 the batch takes the two launches. Run to convergence; both forms give one calibration."""
    check_calibrate_forms(make, (775, 775, 6), 512)


def test_calibrate_class_weights(make):
    check_calibrate_weighted(make)


def test_calibrate_linear_kernel(make):
    check_calibrate_linear(make)


def test_errors_and_life(make):
    check_errors_and_life(make)


# ---- the pybind11 class ---------------------------------------------------------------------------------------------------------
def test_pybind_probabilities(native):
    """fit_svm_multiclass(probability=True) gives Engine.svm_multiclass_calibrate's fits on stratified_folds(labels, folds, seed);
    predict_proba_np is [rows, k] float64 in the order of ``classes`` with rows summing to 1 within 64 ulp; predict_class_np
    (rule="proba") is its argmax, rule="vote" stays the vote; predict_proba_dlpack is the same array on the device; uncalibrated
    it raises RuntimeError naming the model; a bad rule raises ValueError; cross_validate_svm_multiclass passes the keyword on."""
    import torch
    from fastsk_amd import FastSK, stratified_folds
    c = mc.case((30, 16, 24), n_test=7, labels=(5, -3, 8))
    n, y = c["n_train"], c["y"]
    f = FastSK(g=c["g"], m=c["m"], t=1)
    f.compute_kernel(c["X"][:n], c["X"][n:])
    plain = f.fit_svm_multiclass(y, C=2.0)
    assert "platt" not in plain
    with pytest.raises(RuntimeError, match=NAME):
        f.predict_proba_np()
    with pytest.raises(RuntimeError):
        f.predict_proba_dlpack()
    with pytest.raises(RuntimeError):
        f.predict_class_np("test", rule="proba")
    vote = f.predict_class_np("test")
    info = f.fit_svm_multiclass(y, C=2.0, probability=True, calibration_folds=3, seed=4)
    e = computed(lambda g, m, **kw: native.Engine(g, m, **kw), c)
    e.svm_train_multiclass(y, 2.0)
    fold = stratified_folds(y, 3, seed=4)
    fits = e.svm_multiclass_calibrate(fold, 3)
    assert info["launches"] == plain["launches"] and info["pairs"] == plain["pairs"]      # the fit is what it was
    assert [{key: q[key] for key in ("A", "B", "iterations", "status")} for q in fits] == info["platt"]["pairs"]
    assert info["platt"]["n_folds"] == 3 and info["platt"]["form"] == fits[0]["form"] == "workgroup"
    assert info["platt"]["launches"] == fits[0]["launches"] and info["platt"]["ms"] > 0
    for which, (r0, r1) in (("test", (n, n + 7)), ("train", (0, n))):
        prob, pred, _ = e.svm_multiclass_proba(r0, r1)
        got = f.predict_proba_np(which)
        assert got.shape == (r1 - r0, 3) and got.dtype == np.float64 and np.array_equal(got, prob)
        assert np.all(np.abs(got.sum(axis=1) - 1.0) <= 64 * 2.0 ** -52) and np.all((got >= 0) & (got <= 1))
        by_proba = f.predict_class_np(which, rule="proba")
        assert by_proba.dtype == np.int32 and np.array_equal(by_proba, pred)
        assert np.array_equal(by_proba, info["classes"][np.argmax(got, axis=1)])           # columns in the order of classes
        on_device = torch.from_dlpack(f.predict_proba_dlpack(which))
        assert on_device.is_cuda and on_device.shape == (r1 - r0, 3) and np.array_equal(on_device.cpu().numpy(), got)
    assert np.array_equal(f.predict_proba_np(), f.predict_proba_np("test"))
    assert np.array_equal(f.predict_class_np("test"), vote) and np.array_equal(f.predict_class_np("test", rule="vote"), vote)
    with pytest.raises(ValueError):
        f.predict_class_np("test", rule="mean")
    with pytest.raises(ValueError):
        f.fit_svm_multiclass(y, probability=True, calibration_folds=1)
    assert f.predict_proba_np().shape == (7, 3)                                              # a refused call keeps the calibration
    # the binary model's probabilities are what they were: the host sigmoid
    yb = np.where(y == 5, 1, -1).astype(np.int32)
    f.fit_svm(yb, probability=True, calibration_folds=3)
    assert f.predict_proba_np().shape == (7,)
    with pytest.raises(RuntimeError):
        f.predict_proba_dlpack()
    # the cross-validation's refit
    r = f.cross_validate_svm_multiclass(y, Cs=(2.0,), folds=3, seed=4, refit=True, probability=True, calibration_folds=3)
    assert r["refit"]["platt"]["pairs"] == info["platt"]["pairs"]
    assert np.array_equal(f.predict_proba_np("test"), e.svm_multiclass_proba(n, n + 7)[0])
    assert "platt" not in f.cross_validate_svm_multiclass(y, Cs=(2.0,), folds=3, refit=True)["refit"]
    e.close()


# ---- the WebKB slice ------------------------------------------------------------------------------------------------------------
def test_webkb_slice_probabilities(native):
    """240 + 80 documents of the four-class WebKB data, g = 8, m = 4, C = 1, probability=True (5 stratified folds): every
    probability lies in [0, 1], every row sums to 1 (within 64 ulp), every pair's fit ends with status 0. The accuracy of
    rule="proba" on the test rows is printed beside the vote's 0.75; nothing has set a threshold for it."""
    from fastsk_amd import FastSK
    z = np.load(os.path.join(ROOT, "tests", "golden", "webkb_slice.npz"))
    n, N = int(z["n_train"]), len(z["offsets"]) - 1
    y = z["labels"][:n]
    f = FastSK(g=int(z["g"]), m=int(z["m"]), t=1)
    f.compute_kernel_flat(np.ascontiguousarray(z["tokens"], dtype=np.int32), np.ascontiguousarray(z["offsets"], dtype=np.int64), n)
    info = f.fit_svm_multiclass(y, C=1.0, probability=True)
    assert info["classes"].tolist() == [0, 1, 2, 3] and len(info["platt"]["pairs"]) == 6 and info["platt"]["n_folds"] == 5
    assert all(q["status"] == 0 for q in info["platt"]["pairs"]), info["platt"]["pairs"]
    for which in ("train", "test"):
        prob = f.predict_proba_np(which)
        assert np.all((prob >= 0) & (prob <= 1)) and np.all(np.abs(prob.sum(axis=1) - 1.0) <= 64 * 2.0 ** -52), which
    by_proba, by_vote = f.predict_class_np("test", rule="proba"), f.predict_class_np("test")
    truth = z["labels"][n:]
    print("WebKB slice, test accuracy: rule='proba' %.4f, vote %.4f; the two rules differ on %d of %d rows"
          % (float((by_proba == truth).mean()), float((by_vote == truth).mean()), int((by_proba != by_vote).sum()), N - n))
    assert float(int((by_vote == truth).sum())) / float(N - n) == 0.75
