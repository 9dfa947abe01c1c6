"""The multi-class probabilities (fsk_exp_neg, fsk_svm_multiclass_calibrate / _get_calibration / _set_calibration,
fsk_svm_multiclass_proba(_device)) on the CPU: the engine's HIP source compiled against tests/emu/hip_emu.h. Every value —
the class probabilities, the argmax label, the coupling's iteration count, the out-of-fold pair decisions, A, B and the fits'
iterations and status — must equal the restatements of tests/svm_multiclass_proba_cases.py bit for bit, and the probabilities
must agree with LIBSVM's own arithmetic (``math.exp``) within 1e-9 where the iteration counts agree. The ``check_*`` functions
take an engine factory; tests/test_gpu_svm_multiclass_proba.py runs them on the MI355X. Reduced sizes here.

Measured on the CPU with the two restatements alone: no row of any case below differs in its iteration count between
fsk_exp_neg and ``math.exp`` (``agree`` allows 1 % of a case's rows)."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_multiclass_cases as mc  # noqa: E402
import svm_multiclass_proba_cases as pc  # noqa: E402
from test_emu_svm import computed, emu_lib, make  # noqa: E402,F401  (the fixtures: the emulator's library and engine factory)
from test_emu_svm_multiclass import code, host_is_device, kernel_rows  # noqa: E402

NAME = "multi-class C-SVC"


# ---- 1. the exponential (host only) ----------------------------------------------------------------------------------------
def check_exp(lib):
    """fsk_exp_neg equals its restatement bit for bit on the breakpoints, the n-boundaries to one ulp either side and 10^5
    seeded points, and is within 2 ulp of math.exp on [-708, 0] (measured: 1)."""
    worst, at = 0, None
    for x in pc.exp_points():
        got, want = lib.exp_neg(x), pc.exp_neg(x)
        if x != x:
            assert got != got and want != want
            continue
        assert pc.bits(got) == pc.bits(want), (x, got, want)
        if x < -708.0:
            assert got == 0.0, x
        elif x <= 0.0:
            u = pc.ulps(got, math.exp(x))
            if u > worst:
                worst, at = u, x
    print("fsk_exp_neg: largest distance to math.exp on [-708, 0]: %d ulp at %r" % (worst, at))
    assert worst <= 2, (worst, at)
    assert lib.exp_neg(0.0) == 1.0 and lib.exp_neg(-0.0) == 1.0 and lib.exp_neg(-708.0) > 2.0 ** -1022
    return worst


# ---- 2. chosen sigmoids on a fitted model ----------------------------------------------------------------------------------
def fitted(make, sizes, n_test, cap=None, **kw):
    c = mc.case(sizes, n_test=n_test, **kw)
    e = computed(make, c)
    e.svm_train_multiclass(c["y"], c["C"], c["eps"], -1 if cap is None else cap)
    return e, c


def same_proba(e, dec, A, B, span=None, name=""):
    """Rows ``span`` of the N-set under the installed sigmoids: prob, the argmax label and the iteration counts equal the
    restatement exactly; the restatement agrees with LIBSVM's own arithmetic. Returns the restatement (prob, top, iters)."""
    classes = e.svm_multiclass_model()["classes"]
    k = len(classes)
    s0, s1 = span or (0, e.N)
    want = pc.proba(dec[s0:s1], A, B, k)
    prob, pred, iters = e.svm_multiclass_proba(s0, s1)
    assert prob.shape == (s1 - s0, k) and prob.dtype == np.float64 and pred.dtype == np.int32 and iters.dtype == np.int32
    assert np.array_equal(prob, want[0]), (name, float(np.abs(prob - want[0]).max()))
    assert np.array_equal(pred, classes[want[1]]), name
    assert np.array_equal(iters, want[2]), (name, iters.tolist(), want[2].tolist())
    pc.agree(want, pc.proba_libm(dec[s0:s1], A, B, k), k, name)
    return want


def check_sigmoids(make, k, sizes=None, n_test=5, cap=None, span=None, seed=3):
    """k classes, seeded sigmoids: every row."""
    e, c = fitted(make, sizes or (4,) * k, n_test, cap, length=16)
    dec, _ = e.svm_multiclass_decision(0, e.N, predict=False)
    A, B = pc.seeded_sigmoids(k, seed + k)
    e.svm_multiclass_set_calibration(A, B)
    want = same_proba(e, dec, A, B, span, ("seeded", k))
    oof, fits = e.svm_multiclass_calibration()
    assert oof is None and [f["A"] for f in fits] == A.tolist() and [f["B"] for f in fits] == B.tolist()
    assert np.all(np.abs(want[0].sum(axis=1) - 1.0) <= 64 * 2.0 ** -52)
    if k == 2:
        assert np.all(want[2] == 0) and np.array_equal(want[0][:, 1], 1 - want[0][:, 0])
    e.close()
    return want


def check_special_sigmoids(make):
    """k = 4 and 8 on one model each: A = B = 0 (every r = 0.5: iteration 0, p = 1 / k exactly, the lowest class wins the tie);
    every pair clamped at 1 - 1e-7 in class order (1 iteration); the cyclic tournament (every pair clamped at one end or the
    other: 4 iterations at k = 4, 3 at k = 8); saturating sigmoids (fApB beyond +-708 on some rows: the zero branch of the
    exponential and both clamps); a NaN sigmoid (B = NaN: the pair becomes 1e-7)."""
    for k, cyclic_iters in ((4, 4), (8, 3)):
        e, c = fitted(make, (3,) * k, 6, length=16)
        classes = np.unique(c["y"])
        P = k * (k - 1) // 2
        dec, _ = e.svm_multiclass_decision(0, e.N, predict=False)
        # A = B = 0
        e.svm_multiclass_set_calibration(np.zeros(P), np.zeros(P))
        prob, pred, iters = e.svm_multiclass_proba(0, e.N)
        assert np.all(prob == 1.0 / k) and np.all(iters == 0) and np.all(pred == classes[0])
        same_proba(e, dec, np.zeros(P), np.zeros(P), name=("zero", k))
        # class order
        A, B = pc.constant_sigmoids(k, lambda a, b: True)
        e.svm_multiclass_set_calibration(A, B)
        want = same_proba(e, dec, A, B, name=("ordered", k))
        assert np.all(want[2] == 1) and np.all(want[1] == 0)
        # the cyclic tournament
        A, B = pc.constant_sigmoids(k, pc.cyclic(k))
        e.svm_multiclass_set_calibration(A, B)
        want = same_proba(e, dec, A, B, name=("cyclic", k))
        assert np.all(want[2] == cyclic_iters), want[2].tolist()
        # saturating
        A, B = pc.seeded_sigmoids(k, 50 + k)
        A = A * 4000.0 * np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
        f = dec * A[None, :] + B[None, :]
        assert (f > 708.0).any() and (f < -708.0).any() and (np.abs(f) < 708.0).any()
        e.svm_multiclass_set_calibration(A, B)
        want = same_proba(e, dec, A, B, name=("saturating", k))
        assert np.all((want[0] >= 0) & (want[0] <= 1))
        # a NaN sigmoid
        A, B = pc.seeded_sigmoids(k, 70 + k)
        B[1] = float("nan")
        e.svm_multiclass_set_calibration(A, B)
        want = same_proba(e, dec, A, B, name=("nan", k))
        assert pc.pair_prob(dec[0, 1], A[1], B[1]) == 1e-7 and not np.isnan(want[0]).any()
        assert code(lambda: e.svm_multiclass_set_calibration(np.where(np.arange(P) == 2, np.inf, A), B), "pair 2") == -1   # A must be finite
        assert code(lambda: e.svm_multiclass_set_calibration(np.where(np.arange(P) == 0, np.nan, A), B), "pair 0") == -1
        again = e.svm_multiclass_proba(0, e.N)                                       # a refused call keeps the sigmoids
        assert np.array_equal(again[0], want[0])
        e.close()


def check_many_classes(make, cap=None, span=None):
    """k = 64: P = 2016, every lane a class, 64,512 bytes of LDS a workgroup. k = 65 still raises."""
    e, c = fitted(make, (2,) * 64, 2, cap, length=16)
    s0, s1 = span or (0, e.N)
    dec = np.zeros((e.N, 2016))
    dec[s0:s1] = e.svm_multiclass_decision(s0, s1, predict=False)[0]
    A, B = pc.seeded_sigmoids(64, 64)
    e.svm_multiclass_set_calibration(A, B)
    want = same_proba(e, dec, A, B, span, "k = 64")
    assert want[0].shape[1] == 64
    e.close()
    c = mc.case((2,) * 65, length=16)
    e = computed(make, c)
    assert code(lambda: e.svm_train_multiclass(c["y"]), "65 classes") == -6
    e.close()


def check_launch_edges(make, device_buffers=host_is_device):
    """Row counts 1, 4 and 5, ranges with r0 > 0, the empty range, each output null in turn, and the _device form."""
    k = 3
    e, c = fitted(make, (7, 6, 8), 6, length=16)
    N, n = e.N, e.n_train
    dec, _ = e.svm_multiclass_decision(0, N, predict=False)
    A, B = pc.seeded_sigmoids(k, 11)
    e.svm_multiclass_set_calibration(A, B)
    want = same_proba(e, dec, A, B, name="edges")
    classes = e.svm_multiclass_model()["classes"]
    for r0, r1 in ((0, 1), (0, 4), (0, 5), (n, N), (n + 1, N), (3, 8), (N - 1, N), (2, 2)):
        prob, pred, iters = e.svm_multiclass_proba(r0, r1)
        assert prob.shape == (r1 - r0, k)
        assert np.array_equal(prob, want[0][r0:r1]) and np.array_equal(pred, classes[want[1][r0:r1]]) and np.array_equal(iters, want[2][r0:r1]), (r0, r1)
    for drop in ("proba", "predict", "iterations"):
        got = e.svm_multiclass_proba(1, N, **{drop: False})
        for name, g, w in zip(("proba", "predict", "iterations"), got, (want[0][1:], classes[want[1][1:]], want[2][1:])):
            assert (g is None) if name == drop else np.array_equal(g, w), (drop, name)
    L = e.lib.L
    assert L.fsk_svm_multiclass_proba(e.h, 0, N, None, None, None) == 0 and L.fsk_svm_multiclass_proba_device(e.h, 0, N, None, None, None) == 0
    assert L.fsk_svm_multiclass_get_calibration(e.h, None, None) == 0                 # every output may be null
    prob_ptr, pred_ptr, read = device_buffers(N * k, 2 * N)
    assert L.fsk_svm_multiclass_proba_device(e.h, 1, N, prob_ptr, pred_ptr, pred_ptr + 4 * N) == 0
    got = read()
    assert np.array_equal(got[0][:(N - 1) * k].reshape(N - 1, k), want[0][1:])
    assert np.array_equal(got[1][:N - 1], classes[want[1][1:]]) and np.array_equal(got[1][N:2 * N - 1], want[2][1:])
    assert L.fsk_svm_multiclass_proba_device(e.h, 0, N + 1, prob_ptr, pred_ptr, None) == -1
    for r0, r1 in ((-1, 2), (0, N + 1), (3, 2)):
        assert code(lambda: e.svm_multiclass_proba(r0, r1), "rows") == -1
    e.close()


# ---- 3. the calibration end to end -----------------------------------------------------------------------------------------
def same_fits(fits, want, name):
    for p, (g, w) in enumerate(zip(fits, want)):
        for key in ("A", "B", "iterations", "status"):
            assert g[key] == w[key], (name, p, key, g[key], w[key])
    assert len(fits) == len(want), name


def check_calibrate(make, c, fold, forms=(("workgroup", 8192),), max_iter=-1, class_weight=None, linear=False, list_sizes=None):
    """fsk_svm_multiclass_calibrate against the restatement in every form given: the out-of-fold pair decisions, the fits and
    the launches (those of the slowest fold problem); then the probabilities of every row under the fitted sigmoids. The
    decisions, labels and the fit's launches are what they are without a calibration."""
    e = computed(make, c)
    if linear:
        e.svm_set_kernel("linear")
        e.rows_build()
    Kr = kernel_rows(e, linear)
    y, C, eps, n = c["y"], c["C"], c["eps"], c["n_train"]
    F = int(fold.max()) + 1
    oof, fits, problems, classes = pc.calibration(Kr[:n], y, fold, C, eps, max_iter, class_weight)
    k = len(classes)
    P = k * (k - 1) // 2
    if list_sizes is not None:
        list_sizes(sorted(len(w["idx"]) for w in problems))
    slowest = max(w["iterations"] for w in problems)
    chunk = 256
    e.set_tuning("svm_chunk", chunk)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        info = e.svm_train_multiclass(y, C, eps, max_iter, class_weight=class_weight)
        before = e.svm_multiclass_decision(0, e.N)
        got = e.svm_multiclass_calibrate(fold, F)
        rounds = slowest // chunk + 1
        assert all(f["form"] == form and f["n_folds"] == F and f["ms"] > 0 for f in got), (form, got[0])
        assert got[0]["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, got[0]["launches"], slowest)
        same_fits(got, fits, form)
        got_oof, again = e.svm_multiclass_calibration()
        assert again == got and got_oof.shape == (n, P) and np.array_equal(got_oof, oof), form
        # the unchanged paths
        after = e.svm_multiclass_decision(0, e.N)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert e.svm_multiclass_model()["info"]["launches"] == info["launches"] == e.svm_train_multiclass(y, C, eps, max_iter, class_weight=class_weight)["launches"]
        assert code(lambda: e.svm_multiclass_proba(0, e.N), "no calibration") == -3      # the refit dropped it
        e.svm_multiclass_calibrate(fold, F)
    A, B = np.array([f["A"] for f in fits]), np.array([f["B"] for f in fits])
    want = same_proba(e, after[0], A, B, name="calibrated")
    assert np.all(np.abs(want[0].sum(axis=1) - 1.0) <= 64 * 2.0 ** -52)
    e.close()
    return fits, want


def mod_folds(n, F, shift=0):
    return ((np.arange(n) + shift) % F).astype(np.int32)


def check_calibrate_three_classes(make):
    """3 classes, 3 folds: fold lists of 63 .. 66 rows, either side of one lane stride."""
    c = mc.case((48, 47, 50), n_test=3)

    def sizes(s):
        assert s[0] <= 64 < s[-1] and any(v % 64 for v in s), s
    check_calibrate(make, c, mod_folds(c["n_train"], 3), list_sizes=sizes)


def check_calibrate_four_classes(make):
    """4 classes, 5 folds by an explicit array of unequal folds: fold lists from under 64 to over 128 rows."""
    c = mc.case((75, 90, 40, 30), n_test=2, labels=(7, -2, 3, 11))
    n = c["n_train"]
    fold = mod_folds(n, 5)
    fold[:9] = 4                                        # (unequal folds)

    def sizes(s):
        assert s[0] < 64 and s[-1] > 128 and any(64 < v < 128 for v in s), s
    fits, _ = check_calibrate(make, c, fold, list_sizes=sizes)
    assert all(f["status"] == 0 for f in fits)


def check_calibrate_forms(make, sizes, wg_max, cap=None):
    """Both solver forms give one calibration (svm_wg_max lowered below the largest fold list)."""
    c = mc.case(sizes, n_test=2)
    seen = []
    check_calibrate(make, c, mod_folds(c["n_train"], 3), forms=(("workgroup", 8192), ("two-launch", wg_max)),
                    max_iter=-1 if cap is None else cap, list_sizes=seen.extend)
    assert max(seen) > wg_max


def check_calibrate_weighted(make):
    c = mc.case((30, 9, 14), n_test=4, labels=(5, -3, 8))
    check_calibrate(make, c, mod_folds(c["n_train"], 3, 1), class_weight=mc.balanced(c["y"]))


def check_calibrate_linear(make):
    c = mc.case((40, 30, 26), n_test=5)
    check_calibrate(make, c, mod_folds(c["n_train"], 3), linear=True)


# ---- 4. errors and life ----------------------------------------------------------------------------------------------------
def check_errors_and_life(make):
    from fastsk_amd import _native
    c = mc.case((12, 9, 10), n_test=3)
    y, n, N = c["y"], c["n_train"], c["n_train"] + c["n_test"]
    tok, off = _native.flatten(c["X"])
    fold = mod_folds(n, 3)
    e = make(c["g"], c["m"])
    e.n_train, e.n_test, e.N = n, c["n_test"], N
    L = e.lib.L
    zeros = np.zeros(3)
    # before a kernel, before a model
    assert L.fsk_svm_multiclass_calibrate(e.h, fold.ctypes.data, 3) == -3 and L.fsk_svm_multiclass_proba(e.h, 0, 1, None, None, None) == -3
    e.compute(tok, off, n, c["n_test"])
    for call in (lambda: e.svm_multiclass_calibrate(fold), lambda: e.svm_multiclass_set_calibration(zeros, zeros),
                 lambda: e.svm_multiclass_proba(0, N), e.svm_multiclass_calibration):
        assert code(call, "no model") == -3
    assert L.fsk_svm_multiclass_get_calibration(e.h, None, None) == -3 and L.fsk_svm_multiclass_set_calibration(e.h, zeros.ctypes.data, zeros.ctypes.data) == -3
    # on a binary and on an SVR model: refused by name
    yb = np.where(y == 0, 1, -1).astype(np.int32)
    for train, name in ((lambda: e.svm_train(yb, 1.0), "C-SVC (fsk_svm_train)"), (lambda: e.svr_train(y.astype(np.float64)), "epsilon-SVR")):
        train()
        assert L.fsk_svm_multiclass_calibrate(e.h, fold.ctypes.data, 3) == -3
        assert name in e.lib.L.fsk_last_error(e.h).decode()
        assert L.fsk_svm_multiclass_proba(e.h, 0, N, None, None, None) == -3 and name in e.lib.L.fsk_last_error(e.h).decode()
        assert L.fsk_svm_multiclass_set_calibration(e.h, zeros.ctypes.data, zeros.ctypes.data) == -3
        assert L.fsk_svm_multiclass_get_calibration(e.h, None, None) == -3
    # the multi-class model, uncalibrated
    e.svm_train_multiclass(y)
    assert code(lambda: e.svm_multiclass_proba(0, N), "no calibration") == -3
    assert code(e.svm_multiclass_calibration, "no calibration") == -3
    for call in (lambda: e.svm_calibrate(fold), e.svm_calibration, lambda: e.svm_proba(0, N)):     # the binary calls stay the binary model's
        assert code(call, NAME) == -3
    # the refusals of the calibration
    bad = fold.copy()
    bad[5] = 3
    assert code(lambda: e.svm_multiclass_calibrate(bad, 3), "row 5") == -1
    emptied = fold.copy()
    emptied[y == 1] = 1
    assert code(lambda: e.svm_multiclass_calibrate(emptied, 3), "class 1", "fold 1") == -1
    assert code(lambda: e.svm_multiclass_calibrate(fold * 2, 5), "fold 1") == -1                  # an empty fold
    assert code(lambda: e.svm_multiclass_calibrate(np.zeros(n, dtype=np.int32)), "n_folds") == -1
    assert L.fsk_svm_multiclass_calibrate(e.h, None, 3) == -1
    assert L.fsk_svm_multiclass_set_calibration(e.h, None, zeros.ctypes.data) == -1
    with pytest.raises(ValueError):
        e.svm_multiclass_set_calibration(np.zeros(2), np.zeros(2))
    assert code(lambda: e.svm_multiclass_proba(0, N), "no calibration") == -3                     # a refused call leaves none
    # a calibration; a stored cross-validation is neither needed nor touched, and the reverse
    cv = e.svm_multiclass_cv(y, mod_folds(n, 2), (0.5, 2.0))
    fits = e.svm_multiclass_calibrate(fold)
    oof, _ = e.svm_multiclass_calibration()
    prob = e.svm_multiclass_proba(0, N)
    pred = np.empty((2, n), dtype=np.int32)
    assert L.fsk_svm_multiclass_cv_get(e.h, pred.ctypes.data, None, None, None) == 0 and np.array_equal(pred, cv["pred"])
    e.svm_multiclass_cv(y, mod_folds(n, 2), (0.5,))
    assert e.svm_multiclass_calibration()[1] == fits and np.array_equal(e.svm_multiclass_calibration()[0], oof)
    # refused calls keep it
    assert code(lambda: e.svm_multiclass_calibrate(emptied, 3), "class 1") == -1
    assert code(lambda: e.svm_multiclass_set_calibration(np.array([0.0, np.inf, 0.0]), zeros), "pair 1") == -1
    assert code(lambda: e.svm_train_multiclass(y, -1.0)) == -1
    again = e.svm_multiclass_proba(0, N)
    assert all(np.array_equal(a, b) for a, b in zip(prob, again)) and e.svm_multiclass_calibration()[1] == fits
    # installed sigmoids replace fitted ones and carry no out-of-fold values
    e.svm_multiclass_set_calibration(zeros, zeros)
    assert e.svm_multiclass_calibration()[0] is None
    assert L.fsk_svm_multiclass_get_calibration(e.h, np.empty(n * 3).ctypes.data, None) == -3
    assert np.all(e.svm_multiclass_proba(0, N)[0] == 1.0 / 3)
    # a refit, a binary model, an SVR drop it
    e.svm_multiclass_calibrate(fold)
    e.svm_train_multiclass(y)
    assert code(lambda: e.svm_multiclass_proba(0, N), "no calibration") == -3
    for train in (lambda: e.svm_train(yb, 1.0), lambda: e.svr_train(y.astype(np.float64))):
        e.svm_multiclass_calibrate(fold)
        train()
        e.svm_train_multiclass(y)
        assert code(lambda: e.svm_multiclass_proba(0, N), "no calibration") == -3
    # a new kernel drops the model and with it the calibration
    e.svm_multiclass_calibrate(fold)
    e.compute(tok, off, n, c["n_test"])
    assert code(lambda: e.svm_multiclass_proba(0, N), "no model") == -3
    e.close()


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
def test_exp_neg_bits_and_bound(emu_lib):
    check_exp(emu_lib)


def test_restatements_agree_on_skewed_matrices():
    """The two yardsticks alone, 300 random skewed matrices of k = 3 .. 8 as decisions under A = -1, B = 0: the counts differ
    on no row, and the coupling stays below its cap of max(100, k) iterations (no input that reaches the cap is known)."""
    rng = np.random.Generator(np.random.PCG64(99))
    for k in range(3, 9):
        P = k * (k - 1) // 2
        dec = rng.standard_normal((50, P)) * rng.choice([0.3, 3.0, 12.0], size=(50, 1))
        A, B = -np.ones(P), np.zeros(P)
        ours, libm = pc.proba(dec, A, B, k), pc.proba_libm(dec, A, B, k)
        print("k = %d: at most %d iterations" % (k, ours[2].max()))
        assert pc.agree(ours, libm, k, k) == 0 and ours[2].max() < 100, (k, ours[2].max())


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
def test_seeded_sigmoids(make, k):
    check_sigmoids(make, k)


def test_special_sigmoids(make):
    check_special_sigmoids(make)


def test_sixty_four_classes(make):
    check_many_classes(make, cap=3, span=(126, 130))


def test_launch_edges_and_null_outputs(make):
    check_launch_edges(make)


def test_calibrate_three_classes(make):
    check_calibrate_three_classes(make)


def test_calibrate_four_classes_five_folds(make):
    check_calibrate_four_classes(make)


def test_calibrate_both_forms(make):
    """(100, 95, 6) with svm_wg_max = 64: fold lists of up to 130 rows take the two launches; 24 iterations a problem."""
    check_calibrate_forms(make, (100, 95, 6), 64, cap=24)


def test_calibrate_class_weights(make):
    check_calibrate_weighted(make)


def test_calibrate_linear_kernel(make):
    check_calibrate_linear(make)


def test_errors_and_life(make):
    check_errors_and_life(make)
