"""The one-vs-one multi-class C-SVC (fsk_svm_train_multiclass / fsk_svm_multiclass_get_model / fsk_svm_multiclass_decision /
fsk_svm_multiclass_cv) on the CPU: the engine's HIP source compiled against tests/emu/hip_emu.h. Every pair of a fit must
reproduce, to the bit, the numpy restatement of tests/svm_cases.py on its own sub-matrix in both forms of the loop; the pairs'
decision values must equal the restatement of the wave's summation bit for bit, so the votes and labels are exact on every
row; the cross-validation must equal the same per problem, its out-of-fold labels and accuracies restated. The ``check_*``
functions take an engine factory and the sizes; tests/test_gpu_svm_multiclass.py runs them at the kernels' edges on the
MI355X. Reduced sizes here."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_multiclass_cases as mc  # noqa: E402
from test_emu_svm import computed, emu_lib, make  # noqa: E402,F401  (the fixtures: the emulator's library and engine factory)

FORMS = (("workgroup", 8192), ("two-launch", 0))
KEYS = ("iterations", "rho", "objective", "gap", "converged", "n_sv", "n_bsv", "class_a", "class_b")
TIE_SEED = 14   # of check_vote_tie: found by a search over seeds 1..29 on the CPU — two tied rows, votes (2, 0, 2, 2) and (0, 2, 2, 2)


def code(fn, *words):
    from fastsk_amd import _native
    with pytest.raises(_native.FskError) as err:
        fn()
    assert all(w in str(err.value) for w in words), str(err.value)
    return err.value.code


def kernel_rows(e, linear=False):
    """K(r, train) of every row r of the N-set, train rows first: what the engine's getters hand out."""
    n, N = e.n_train, e.N
    if linear:
        return e.rows_block(0, N, 0, n)
    return np.vstack([e.get_train(), e.get_test()]) if e.n_test else e.get_train()


def same_model(e, classes, want, name):
    got = e.svm_multiclass_model()
    k = len(classes)
    assert np.array_equal(got["classes"], classes) and got["classes"].dtype == np.int32, name
    assert got["info"]["k"] == k and got["info"]["n_pairs"] == len(want) == k * (k - 1) // 2 == len(got["pairs"]), name
    sv = np.zeros(e.n_train, dtype=bool)
    for p, (g, w) in enumerate(zip(got["pairs"], want)):
        for key in KEYS:
            assert g[key] == w[key], (name, p, key, g[key], w[key])
        assert g["n_rows"] == len(w["idx"]), (name, p)
        assert np.array_equal(got["alpha"][p], w["alpha"]), (name, p)
        sv[w["idx"][w["alpha"] > 0]] = True
    assert got["info"]["n_sv"] == int(sv.sum()), name
    return got


def check_decisions(e, c, classes, want, Kr, ranges=True, span=None):
    """Every row of the N-set (of ``span``): the pairs' decision values and the voted label equal the restatement exactly;
    then the sub-ranges, the empty range and either output alone."""
    N, n = e.N, e.n_train
    s0, s1 = span or (0, N)
    ref = mc.decisions(Kr, want)
    labels, v = mc.vote(ref, want, classes)
    dec, pred = e.svm_multiclass_decision(s0, s1)
    assert dec.shape == (s1 - s0, len(want)) and pred.shape == (s1 - s0,) and pred.dtype == np.int32
    assert np.array_equal(dec, ref[s0:s1]), float(np.nanmax(np.abs(dec - ref[s0:s1])))
    assert np.array_equal(pred, labels[s0:s1])
    if ranges:
        for r0, r1 in ((1, N - 1), (n, N), (0, n), (N - 1, N)):
            d, q = e.svm_multiclass_decision(r0, r1)
            assert np.array_equal(d, ref[r0:r1]) and np.array_equal(q, labels[r0:r1]), (r0, r1)
        d, q = e.svm_multiclass_decision(2, 2)
        assert d.shape == (0, len(want)) and q.shape == (0,)
        d, q = e.svm_multiclass_decision(0, N, predict=False)
        assert q is None and np.array_equal(d, ref)
        d, q = e.svm_multiclass_decision(0, N, decision=False)
        assert d is None and np.array_equal(q, labels)
    return ref, labels, v


def check_fit(make, c, forms=FORMS, chunks=(7, 256), max_iter=-1, class_weight=None, linear=False, engine=None, ranges=True,
              span=None):
    """Both forms and every chunk: the pairs equal the restatement, the launches are those of the slowest pair; the decision
    values and labels of every row equal the restated wave. Returns (classes, the restatement's pairs, decisions, labels,
    votes)."""
    e = engine or computed(make, c)
    if linear:
        e.svm_set_kernel("linear")
        e.rows_build()
    Kr = kernel_rows(e, linear)
    y, C, eps = c["y"], c["C"], c["eps"]
    classes, want = mc.expected(Kr[:e.n_train], y, C, eps, max_iter, class_weight)
    slowest = max(w["iterations"] for w in want)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            info = e.svm_train_multiclass(y, C, eps, max_iter, class_weight=class_weight)
            assert info["form"] == form, (info, form)
            same_model(e, classes, want, (form, chunk))
            rounds = slowest // chunk + 1
            assert info["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, info)
    ref, labels, v = check_decisions(e, c, classes, want, Kr, ranges, span)
    if engine is None:
        e.close()
    return classes, want, ref, labels, v


# ---- 1. the smallest pairs ------------------------------------------------------------------------------------------------------
def check_tiny(make):
    """Class sizes (1, 1, 2): pairs of 2, 3 and 3 rows."""
    c = mc.case((1, 1, 2), n_test=3, length=16)
    _, want, _, _, _ = check_fit(make, c)
    assert [len(w["idx"]) for w in want] == [2, 3, 3]


# ---- 2. the lane and second-stride edges of the decision kernel ----------------------------------------------------------------
def check_lane_edges(make):
    """(63, 1, 64, 65): pair lists of 64, 127, 128, 65, 66 and 129 rows; 5 test rows (not a multiple of the waves a workgroup),
    the last of which shares no g-mer with any training row: every decision value of it is -rho."""
    c = mc.foreign_test_row(mc.case((63, 1, 64, 65), n_test=5))
    _, want, ref, _, _ = check_fit(make, c, chunks=(256,))
    assert [len(w["idx"]) for w in want] == [64, 127, 128, 65, 66, 129]
    assert all(w["converged"] for w in want)
    assert np.array_equal(ref[-1], np.array([0.0 - w["rho"] for w in want]))


# ---- 3. both forms at the workgroup's edge ---------------------------------------------------------------------------------------
def check_forms(make, sizes, wg_max, n_wg, cap=None):
    """At the default every pair is one workgroup; with svm_wg_max = ``wg_max`` below the largest pair the batch takes the two
    launches, ``n_wg`` workgroups a pair in one grid. Both give the restatement's model — the same model."""
    c = mc.case(sizes, n_test=2)
    e = computed(make, c)
    max_iter = -1 if cap is None else cap
    _, want, _, _, _ = check_fit(make, c, forms=FORMS[:1], chunks=(256,), max_iter=max_iter, engine=e, ranges=False)
    first = e.svm_multiclass_model()
    assert [(len(w["idx"]) + 255) // 256 for w in want] == list(n_wg)
    e.set_tuning("svm_wg_max", wg_max)
    e.set_tuning("svm_chunk", 256)
    info = e.svm_train_multiclass(c["y"], c["C"], c["eps"], max_iter)
    assert info["form"] == "two-launch" and max(len(w["idx"]) for w in want) > wg_max
    second = same_model(e, np.unique(c["y"]), want, "two-launch")
    assert all(np.array_equal(a, b) for a, b in zip(first["alpha"], second["alpha"])) and first["pairs"] == second["pairs"]
    e.close()


# ---- 4. every vote lane ----------------------------------------------------------------------------------------------------------
def check_many_classes(make, cap=None, forms=FORMS, span=None):
    """k = 64 with 2 rows a class: 2016 problems of 4 rows, more than the compute units, every vote lane in use. k = 65 is
    refused and the handle stays usable."""
    c = mc.case((2,) * 64, n_test=2, length=16)
    e = computed(make, c)
    classes, want, _, labels, _ = check_fit(make, c, forms=forms, chunks=(256,), max_iter=-1 if cap is None else cap, engine=e,
                                           ranges=False, span=span)
    assert len(classes) == 64 and len(want) == 2016 and all(len(w["idx"]) == 4 for w in want)
    e.close()
    c = mc.case((2,) * 65, length=16)
    e = computed(make, c)
    assert code(lambda: e.svm_train_multiclass(c["y"]), "65 classes") == -6       # FSK_EUNSUPPORTED
    y = c["y"].copy()
    y[y == 64] = 63
    assert e.svm_train_multiclass(y, max_iter=-1 if cap is None else cap)["k"] == 64   # the handle stays usable
    e.close()


# ---- 5. label values -------------------------------------------------------------------------------------------------------------
def check_label_values(make):
    """Labels (2147483647, -7, 0) presented unsorted: the classes come back ascending, predictions are label values."""
    c = mc.case((9, 12, 7), n_test=6, labels=(2147483647, -7, 0))
    classes, want, _, labels, _ = check_fit(make, c, forms=FORMS[:1], chunks=(256,))
    assert classes.tolist() == [-7, 0, 2147483647] and (want[0]["class_a"], want[0]["class_b"]) == (-7, 0)
    assert set(labels.tolist()) <= {-7, 0, 2147483647}


# ---- 6. a vote tie ---------------------------------------------------------------------------------------------------------------
def tie_case(seed=TIE_SEED):
    return mc.case((5, 5, 5, 5), n_test=40, seed=seed)


def check_vote_tie(make):
    """At least one row whose two highest vote counts are equal — the restatement sees it, so it cannot quietly vanish —
    and the engine returns the lowest class of them (check_decisions compares every label)."""
    c = tie_case()
    classes, want, _, labels, v = check_fit(make, c, forms=FORMS[:1], chunks=(256,), ranges=False)
    tied = mc.tied_rows(v)
    assert len(tied) >= 1, "the tie is gone: search TIE_SEED again"
    for r in tied.tolist():
        top = np.flatnonzero(v[r] == v[r].max())
        assert len(top) >= 2 and labels[r] == classes[top[0]]


# ---- 7. class weights, the rows kernel ---------------------------------------------------------------------------------------------
def check_class_weights(make):
    from fastsk_amd import _native
    c = mc.case((30, 6, 14), n_test=4, labels=(5, -3, 8))
    by_dict = {5: 0.5, 8: 3.0}                   # (class -3 keeps 1)
    _, weighted, _, _, _ = check_fit(make, c, forms=FORMS[:1], chunks=(256,), class_weight=by_dict, ranges=False)
    _, plain, _, _, _ = check_fit(make, c, forms=FORMS[:1], chunks=(256,), ranges=False)
    assert any(not np.array_equal(a["alpha"], b["alpha"]) for a, b in zip(weighted, plain))
    bal = mc.balanced(c["y"])
    assert bal == {5: 50 / (3.0 * 30), -3: 50 / (3.0 * 6), 8: 50 / (3.0 * 14)}
    assert np.array_equal(_native.multiclass_weights(c["y"], "balanced"), [bal[-3], bal[5], bal[8]])
    assert np.array_equal(_native.multiclass_weights(c["y"], by_dict), [1.0, 0.5, 3.0])
    assert _native.multiclass_weights(c["y"], None) is None
    for bad in ({7: 1.0}, {5: 0.0}, {5: float("nan")}, "even", (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            _native.multiclass_weights(c["y"], bad)
    check_fit(make, c, forms=FORMS[:1], chunks=(256,), class_weight=bal, ranges=False)


def check_linear(make, sizes=(40, 30, 26)):
    """kernel_type="linear": the pairs solve on the rows kernel K2 and the decisions read it."""
    c = mc.case(sizes, n_test=5)
    check_fit(make, c, forms=FORMS[:1], chunks=(256,), linear=True, ranges=False)


# ---- 8. cross-validation ---------------------------------------------------------------------------------------------------------
def same_problems(got, want, name):
    assert len(got["problems"]) == len(want), name
    for p, (g, w) in enumerate(zip(got["problems"], want)):
        for key in KEYS + ("C", "fold"):
            assert g[key] == w[key], (name, p, key, g[key], w[key])
        assert g["n_rows"] == len(w["idx"]), (name, p)


def cv_case():
    """k = 3, 3 folds of unequal size (every fold keeps rows of every class in its training part)."""
    c = mc.case((20, 13, 17), n_test=2, labels=(4, 1, 9))
    n = c["n_train"]
    fold = np.zeros(n, dtype=np.int32)
    fold[n // 2:n // 2 + 15] = 1
    fold[n - 7:] = 2
    return c, fold


def check_cv(make, forms=FORMS, chunks=(7, 256)):
    """3 folds of unequal size x Cs (0.5, 2) x 3 pairs = 18 problems: every problem equals the restatement, the out-of-fold
    labels and the accuracies are restated, both forms and every chunk give the same arrays."""
    c, fold = cv_case()
    Cs = (0.5, 2.0)
    e = computed(make, c)
    K, y = e.get_train(), c["y"]
    classes, want = mc.expected_cv(K, y, fold, Cs, c["eps"])
    assert len(want) == 18 and sorted(set(np.bincount(fold).tolist())) == [7, 15, 28]
    pred, acc = mc.oof_labels(K, y, fold, classes, want, len(Cs))
    slowest = max(w["iterations"] for w in want)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            got = e.svm_multiclass_cv(y, fold, Cs, c["eps"])
            assert got["form"] == form and got["k"] == 3
            same_problems(got, want, (form, chunk))
            rounds = slowest // chunk + 1
            assert got["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, got["launches"])
            assert np.array_equal(got["pred"], pred) and got["pred"].dtype == np.int32
            assert np.array_equal(got["accuracy"], acc)
    e.close()


def check_cv_errors(make):
    """The refusals, and the two cross-validation results and the model that do not disturb each other."""
    from fastsk_amd import _native
    c, fold = cv_case()
    y = c["y"]
    e = computed(make, c)
    L = e.lib.L
    Cs = np.array([0.5, 2.0])
    assert L.fsk_svm_multiclass_cv_get(e.h, None, None, None, None) == -3        # none yet
    emptied = fold.copy()
    emptied[y == 1] = 1                                                           # fold 1 holds every row of class 1
    assert code(lambda: e.svm_multiclass_cv(y, emptied, Cs), "class 1", "fold 1") == -1
    assert code(lambda: e.svm_multiclass_cv(y, fold, np.ones(7282)), "problems") == -1   # 3 x 7282 x 3 = 65538 > 65535
    assert code(lambda: e.svm_multiclass_cv(y, fold * 2, Cs, n_folds=5), "fold 1") == -1  # an empty fold
    bad = fold.copy()
    bad[5] = 3
    assert code(lambda: e.svm_multiclass_cv(y, bad, Cs, n_folds=3), "row 5") == -1
    assert code(lambda: e.svm_multiclass_cv(y, np.zeros(len(y), dtype=np.int32), Cs), "n_folds") == -1
    assert code(lambda: e.svm_multiclass_cv(y, fold, np.zeros(0)), "n_C") == -1
    assert code(lambda: e.svm_multiclass_cv(y, fold, [1.0, -1.0]), "C 1") == -1
    assert code(lambda: e.svm_multiclass_cv(y, fold, Cs, eps=0.0), "eps") == -1
    assert code(lambda: e.svm_multiclass_cv(y[:-1], fold[:-1], Cs)) == -1
    assert code(lambda: e.svm_multiclass_cv(np.full(len(y), 4, dtype=np.int32), fold, Cs), "one class") == -1
    assert code(lambda: e.svm_multiclass_cv(y, fold, Cs, class_weight=[1.0, 0.0, 1.0]), "class 4") == -1
    assert L.fsk_svm_multiclass_cv_get(e.h, None, None, None, None) == -3        # a refused call leaves no result
    # beside the binary cross-validation and the model: nobody disturbs anybody
    yb = np.where(y == 4, 1, -1).astype(np.int32)
    binary = e.svm_cv(yb, fold, Cs)
    e.svm_train(yb, 1.0)
    dec0 = e.svm_decision(0, e.N)
    multi = e.svm_multiclass_cv(y, fold, Cs)
    again = e.svm_cv(yb, fold, Cs)
    assert np.array_equal(binary["decision"], again["decision"]) and binary["problems"] == again["problems"]
    assert np.array_equal(e.svm_cv_alpha(0), e.svm_cv_alpha(0)) and np.array_equal(dec0, e.svm_decision(0, e.N))
    assert code(lambda: e.svm_multiclass_cv(y, emptied, Cs), "class 1") == -1     # a refused call keeps the earlier result
    info = _native_cv_pred(e, len(Cs), len(y))
    assert np.array_equal(info, multi["pred"])
    e.svm_train_multiclass(y)
    assert np.array_equal(_native_cv_pred(e, len(Cs), len(y)), multi["pred"])
    few = e.svm_multiclass_cv(y, fold, Cs, max_iter=2)
    assert all(q["iterations"] <= 2 for q in few["problems"]) and not all(q["converged"] for q in few["problems"])
    # the result belongs to the kernel
    tok, off = _native.flatten(c["X"])
    e.compute(tok, off, c["n_train"], c["n_test"])
    assert L.fsk_svm_multiclass_cv_get(e.h, None, None, None, None) == -3
    e.close()


def _native_cv_pred(e, n_C, n):
    pred = np.empty((n_C, n), dtype=np.int32)
    assert e.lib.L.fsk_svm_multiclass_cv_get(e.h, pred.ctypes.data, None, None, None) == 0
    return pred


# ---- 9. the model slot -----------------------------------------------------------------------------------------------------------
def host_is_device(n_dec, n_pred):
    """The emulator's "device memory" is host memory: (address of n_dec doubles, address of n_pred int32, a function that
    reads both back)."""
    dec, pred = np.zeros(n_dec), np.zeros(n_pred, dtype=np.int32)
    return dec.ctypes.data, pred.ctypes.data, lambda: (dec, pred)


def check_state(make, device_buffers=host_is_device):
    """Every binary or SVR accessor is refused, naming the model, while the multi-class model holds the slot, and the
    reverse; a binary train restores 1-D decisions; a new compute drops the model; a refused call keeps the old one.
    ``device_buffers(n_dec, n_pred)`` gives DEVICE memory for fsk_svm_multiclass_decision_device and a function that copies it
    to the host."""
    from fastsk_amd import _native
    c = mc.case((8, 9, 7), n_test=3)
    tok, off = _native.flatten(c["X"])
    y, n, N = c["y"], c["n_train"], c["n_train"] + c["n_test"]
    yb = np.where(y == 0, 1, -1).astype(np.int32)
    e = make(c["g"], c["m"])
    e.n_train, e.n_test, e.N = n, c["n_test"], N
    assert code(lambda: e.svm_train_multiclass(y)) == -3                          # nothing computed
    assert code(lambda: e.svm_multiclass_model()) == -3
    e.compute(tok, off, n, c["n_test"])
    assert code(lambda: e.svm_multiclass_model()) == -3                           # no model yet
    assert code(lambda: e.svm_multiclass_decision(0, N)) == -3
    # refusals
    assert code(lambda: e.svm_train_multiclass(np.zeros(n, dtype=np.int32)), "one class") == -1
    assert code(lambda: e.svm_train_multiclass(y[:-1])) == -1
    assert code(lambda: e.svm_train_multiclass(y, class_weight=[1.0, -2.0, 1.0]), "class 1") == -1
    assert code(lambda: e.svm_train_multiclass(y, class_weight=[1.0, float("inf"), 1.0]), "class 1") == -1
    for C in (0.0, -1.0, float("nan")):
        assert code(lambda: e.svm_train_multiclass(y, C), "C must") == -1
    assert code(lambda: e.svm_train_multiclass(y, eps=0.0), "eps") == -1
    assert e.lib.L.fsk_svm_train_multiclass(e.h, None, n, 1.0, None, 1e-3, -1) == -1
    # a binary model, then the refusals once more: the model stays
    e.svm_train(yb, 2.0)
    alpha0, rho0, _ = e.svm_model()
    assert code(lambda: e.svm_multiclass_model(), "C-SVC (fsk_svm_train)") == -3
    assert code(lambda: e.svm_multiclass_decision(0, N), "C-SVC (fsk_svm_train)") == -3
    assert code(lambda: e.svm_train_multiclass(np.zeros(n, dtype=np.int32)), "one class") == -1
    alpha1, rho1, _ = e.svm_model()
    assert np.array_equal(alpha0, alpha1) and rho0 == rho1
    # the multi-class model takes the slot
    e.svm_set_class_weights(2.0, 0.5)                                           # (neither consulted nor changed)
    e.svm_train(yb, 2.0)
    e.svm_train_multiclass(y)
    assert e.svm_get_class_weights() == (2.0, 0.5)
    plain = make(c["g"], c["m"])
    plain.compute(tok, off, n, c["n_test"])
    plain.svm_train_multiclass(y)
    assert all(np.array_equal(a, b) for a, b in zip(e.svm_multiclass_model()["alpha"], plain.svm_multiclass_model()["alpha"]))
    plain.close()
    e.svm_set_class_weights(1.0, 1.0)                                           # (a change of weights drops any model)
    assert code(lambda: e.svm_multiclass_model()) == -3
    e.svm_train_multiclass(y)
    name = "multi-class C-SVC"
    fold = (np.arange(n) % 2).astype(np.int32)
    for call in (e.svm_model, lambda: e.svm_decision(0, N), lambda: e.svm_calibrate(fold), e.svm_calibration,
                 lambda: e.svm_proba(0, N), e.svr_model):
        assert code(call, name) == -3
    dec, pred = e.svm_multiclass_decision(0, N)
    assert dec.shape == (N, 3)
    L = e.lib.L
    dec_ptr, pred_ptr, read = device_buffers(N * 3, N)
    assert L.fsk_svm_multiclass_decision_device(e.h, 1, N, dec_ptr, pred_ptr) == 0
    on_dev = read()
    assert np.array_equal(on_dev[0][:(N - 1) * 3].reshape(N - 1, 3), dec[1:]) and np.array_equal(on_dev[1][:N - 1], pred[1:])
    assert L.fsk_svm_multiclass_decision_device(e.h, 0, N, None, pred_ptr) == 0 and np.array_equal(read()[1], pred)
    assert L.fsk_svm_multiclass_decision_device(e.h, 0, N, None, None) == 0 and L.fsk_svm_multiclass_decision(e.h, 0, N, None, None) == 0
    assert L.fsk_svm_multiclass_decision_device(e.h, 0, N + 1, dec_ptr, pred_ptr) == -1
    assert L.fsk_svm_multiclass_get_model(e.h, None, None, None, None) == 0            # every output may be null
    assert code(lambda: e.svm_multiclass_decision(-1, 2)) == -1 and code(lambda: e.svm_multiclass_decision(0, N + 1)) == -1
    assert code(lambda: e.svm_multiclass_decision(3, 2)) == -1
    # a refused multi-class call keeps the multi-class model
    assert code(lambda: e.svm_train_multiclass(y, -1.0)) == -1
    again = e.svm_multiclass_decision(0, N)
    assert np.array_equal(again[0], dec) and np.array_equal(again[1], pred)
    # an SVR, a C-SVC replace it
    e.svr_train(y.astype(np.float64))
    assert code(lambda: e.svm_multiclass_model(), "epsilon-SVR") == -3 and e.svm_decision(0, N).shape == (N,)
    e.svm_train_multiclass(y)
    e.svm_train(yb, 2.0)
    assert e.svm_decision(0, N).shape == (N,) and code(lambda: e.svm_multiclass_decision(0, N), "C-SVC") == -3
    # a new kernel drops it; a stale one hides it
    e.svm_train_multiclass(y)
    e.accumulate(np.arange(3, dtype=np.int32))
    assert code(lambda: e.svm_multiclass_decision(0, N)) == -3
    e.finalize()
    assert code(lambda: e.svm_multiclass_decision(0, N)) == -3
    e.svm_train_multiclass(y)
    e.compute(tok, off, n, c["n_test"])
    assert code(lambda: e.svm_multiclass_model()) == -3
    e.close()


# ---- 10. the reader --------------------------------------------------------------------------------------------------------------
def check_reader(tmp_path):
    from fastsk_amd.utils import FastaUtility, MalformedFasta
    path = tmp_path / "three.fasta"
    path.write_text(">3\nACGTAC\n>-2\nGGTACA\n>10\nTTGACC\n>3\nACCTGA\n")
    X, Y = FastaUtility().read_data(str(path), multiclass=True)
    assert Y == [3, -2, 10, 3] and all(isinstance(v, int) for v in Y)
    assert X[0] == [1, 2, 3, 4, 1, 2] and len(X) == 4
    with pytest.raises(MalformedFasta):
        FastaUtility().read_data(str(path))                 # the default call still wants -1 / 0 / 1
    bad = tmp_path / "bad.fasta"
    bad.write_text(">3\nACGT\n>2.5\nGGTA\n")
    with pytest.raises(MalformedFasta, match="2.5"):
        FastaUtility().read_data(str(bad), multiclass=True)
    ok = tmp_path / "binary.fasta"
    ok.write_text(">1\nACGT\n>-1\nGGTA\n")
    assert FastaUtility().read_data(str(ok))[1] == [1, -1] == FastaUtility().read_data(str(ok), multiclass=True)[1]


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
def test_tiny_pairs(make):
    check_tiny(make)


def test_lane_edges_and_a_foreign_row(make):
    check_lane_edges(make)


def test_both_forms_at_the_workgroup_edge(make):
    """(130, 131, 1) with svm_wg_max = 128: pairs of 261, 131 and 132 rows, 2, 1 and 1 workgroups in one grid."""
    check_forms(make, (130, 131, 1), 128, (2, 1, 1), cap=24)


def test_sixty_four_classes(make):
    check_many_classes(make, cap=3, forms=FORMS[:1], span=(126, 130))


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
    check_state(make)


def test_reader_multiclass(tmp_path):
    check_reader(tmp_path)
