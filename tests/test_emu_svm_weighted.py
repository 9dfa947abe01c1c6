"""The class-weighted C-SVC and the Platt calibration (fsk_svm_set_class_weights, fsk_svm_platt_fit, fsk_svm_calibrate,
fsk_svm_get_calibration, fsk_svm_proba) on the CPU: the engine's HIP source compiled against tests/emu/hip_emu.h must reproduce,
to the bit, the numpy restatement of tests/svm_weighted_cases.py (``solve_w``: tests/svm_cases.py's ``solve`` with the box of a
row chosen by its class) in both forms of the loop and for every svm_chunk, singly and in a cross-validation batch; Platt's fit
must equal LIBSVM's sigmoid_train restated on Python floats, bit for bit. The ``check_*`` functions take an engine factory;
tests/test_gpu_svm_weighted.py runs them at scale 1 on the MI355X. Every row of the table runs in both forms and at svm_chunk 1,
7 and 256, here as there; the one reduction here is that the 1025-row edge stops after ``cap`` iterations (compared with the
restatement stopped there). The 300-row calibration is the GPU's."""
import collections
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402
import svm_cv_cases as cv  # noqa: E402
import svm_weighted_cases as wc  # noqa: E402
from test_emu_svm import CHUNKS, FORMS, computed, emu_lib, make, same_model  # noqa: E402,F401  (the fixtures: the emulator's library and engine factory)
from test_emu_svm_cv import same_problems  # noqa: E402

TABLE = sorted(wc.table())
_RESTATED = {}   # (name, max_iter) -> (K, the restatement's result): computed once, shared, left unchanged


def kernel_of(e, c, kind):
    """The matrix the solver reads: the engine's own ``get_train``, or K2 of the rows kernel."""
    if kind == "linear":
        e.svm_set_kernel("linear")
        e.rows_build()
        return e.rows_block(0, c["n_train"], 0, c["n_train"])
    return e.get_train()


def restated(name, K, c, weights, max_iter):
    """``solve_w`` on K, once for every (case, max_iter) and matrix."""
    key = (name, max_iter)
    if key not in _RESTATED or not np.array_equal(_RESTATED[key][0], K):
        _, _, Cp, Cn = wc.boxes(c, weights)
        _RESTATED[key] = (K, wc.solve_w(K, c["y"], Cp, Cn, c["eps"], max_iter))
    return _RESTATED[key][1]


# ---- 1. every case -------------------------------------------------------------------------------------------------------------
def check_case_w(make, name, forms=FORMS, chunks=CHUNKS, max_iter=-1, sklearn=True):
    """Both forms and every chunk equal ``solve_w`` bit for bit (alpha, rho, objective, gap, iterations, n_sv, n_bsv) with the
    launches of the unweighted solve; a converged case passes the certificate with per-class boxes and lies within
    2 eps (Cp n_pos + Cn n_neg) of scikit-learn's objective; the train rows' decision values. Returns the restatement's result."""
    c, weights, engine_kw, kind = wc.table()[name]
    e = computed(make, c, **engine_kw)
    if engine_kw:
        assert len(e.get_stdevs()) > 0   # (the fp64 triangle of variance mode)
    K = kernel_of(e, c, kind)
    n, eps = c["n_train"], c["eps"]
    w_pos, w_neg, Cp, Cn = wc.boxes(c, weights)
    want = restated(name, K, c, weights, max_iter)
    e.svm_set_class_weights(w_pos, w_neg)
    assert e.svm_get_class_weights() == (w_pos, w_neg)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            info = e.svm_train(c["y"], c["C"], eps, max_iter)
            assert info["form"] == form
            alpha, rho, info = same_model(e, want, (name, form, chunk))
            rounds = want["iterations"] // chunk + 1
            assert info["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, info)
    if want["converged"]:
        cert = wc.certify_w(K, c["y"], alpha, Cp, Cn, eps)
        assert abs(cert["objective"] - info["objective"]) <= 1e-9 * max(1.0, abs(cert["objective"]))
        if sklearn:
            n_pos = int((c["y"] > 0).sum())
            theirs = wc.sklearn_objective_w(K, c["y"], c["C"], w_pos, w_neg, eps)
            assert abs(info["objective"] - theirs) <= 2.0 * eps * (Cp * n_pos + Cn * (n - n_pos)), (info["objective"], theirs)
    dec = e.svm_decision(0, n)
    ref, bound = cases.decision_reference(K, c["y"], alpha, rho)
    assert np.all(np.abs(dec - ref) <= bound), float(np.max(np.abs(dec - ref) - bound))
    e.close()
    return want


def check_table_case(make, name, cap=None):
    """One row of the issue's table — both forms and svm_chunk 1, 7 and 256 for every row — with what the row is there for.
    ``cap``: the iteration cap of the 1025-row case (the emulator's; None runs it to the end)."""
    if name == "edge1025":
        want = check_case_w(make, name, max_iter=-1 if cap is None else cap, sklearn=cap is None)
        assert want["iterations"] > 0 and (cap is not None or want["converged"])
        assert cap is not None or any(1024 in p for p in want["pairs"])            # (a thread's second element, the fifth workgroup)
    else:
        want = check_case_w(make, name)
        assert want["converged"]
    if name == "edge257":
        assert any(256 in p for p in want["pairs"])                                 # (the second workgroup's one row)
    c, weights, _, _ = wc.table()[name]
    _, _, Cp, Cn = wc.boxes(c, weights)
    if name.startswith("bound"):   # a whole class ends at its bound: the one with the small box
        small = c["y"] > 0 if Cp < Cn else c["y"] < 0
        assert np.all(want["alpha"][small] == min(Cp, Cn)) and want["n_bsv"] >= int(small.sum())
    if name == "duplicates":       # the TAU pair, with C_i != C_j
        assert want["tau_selected"] > 0 and want["branches"]["tau_mixed_weights"] > 0
    return want


# ---- 3. the case set reaches the new code ----------------------------------------------------------------------------------------
def check_branches_reached(make, cap=None):
    """The union of the restatement's branch counters over the table: each clip of the mixed step taken, and each of them
    with diff strictly between 0 and C_i - C_j, where the weighted code decides differently from the unweighted."""
    total = collections.Counter()
    for name in TABLE:
        c, weights, engine_kw, kind = wc.table()[name]
        max_iter = cap if (name == "edge1025" and cap is not None) else -1
        if (name, max_iter) not in _RESTATED:
            e = computed(make, c, **engine_kw)
            restated(name, kernel_of(e, c, kind), c, weights, max_iter)
            e.close()
        total.update(_RESTATED[(name, max_iter)][1]["branches"])
    for branch in wc.BRANCHES:
        assert total[branch] > 0, (branch, dict(total))
    return total


# ---- 4. weights (1, 1), and the setter -------------------------------------------------------------------------------------------
def check_unit_weights_and_setter(make):
    """Weights (1, 1) set explicitly: model and launch count of the unset handle. Setting the values in force keeps the model,
    the cross-validation result and the calibration; changing them drops all three; bad weights are FSK_EINVAL."""
    from fastsk_amd import _native
    c = cases.edge_case(96)
    y, fold = c["y"], cv.paired(96, 3)

    def code(fn):
        with pytest.raises(_native.FskError) as err:
            fn()
        return err.value.code

    plain, e = computed(make, c), computed(make, c)
    assert e.svm_get_class_weights() == (1.0, 1.0)
    e.svm_set_class_weights(1.0, 1.0)
    for form, wg_max in FORMS:
        for x in (plain, e):
            x.set_tuning("svm_wg_max", wg_max)
            x.set_tuning("svm_chunk", 7)
        a0, rho0, info0 = (plain.svm_train(y, c["C"], c["eps"]), plain.svm_model())[1]
        a1, rho1, info1 = (e.svm_train(y, c["C"], c["eps"]), e.svm_model())[1]
        for info in (info0, info1):
            info.pop("ms")
        assert np.array_equal(a0, a1) and rho0 == rho1 and info0 == info1 and info1["form"] == form
        want = cases.solve(e.get_train(), y, c["C"], c["eps"])
        same_model(e, want, form)
    plain.close()
    e.svm_cv(y, fold, (1.0,))
    e.svm_calibrate(fold)
    e.svm_set_class_weights(1.0, 1.0)                              # the values in force: nothing dropped
    assert np.array_equal(e.svm_model()[0], a1) and e.svm_cv_alpha(0).shape == (96,) and e.svm_calibration()[1]["status"] == 0
    e.svm_set_class_weights(2.0, 1.0)                              # a change: the model, the cross-validation, the calibration
    assert code(e.svm_model) == -3 and code(lambda: e.svm_cv_alpha(0)) == -3 and code(e.svm_calibration) == -3
    assert code(lambda: e.svm_proba(0, 1)) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    assert e.svm_get_class_weights() == (2.0, 1.0)
    for bad in ((0.0, 1.0), (1.0, 0.0), (-1.0, 1.0), (1.0, -2.0), (float("inf"), 1.0), (1.0, float("inf")), (float("nan"), 1.0),
                (1.0, float("nan"))):
        assert code(lambda: e.svm_set_class_weights(*bad)) == -1, bad
    assert e.svm_get_class_weights() == (2.0, 1.0)                  # a refused call changes nothing
    L = e.lib.L
    assert L.fsk_svm_set_class_weights(None, 1.0, 1.0) == -1 and L.fsk_svm_get_class_weights(e.h, None, None) == -1
    e.svm_train(y, c["C"], c["eps"])
    want = wc.solve_w(e.get_train(), y, 2.0 * c["C"], c["C"], c["eps"])   # the weights stay with the handle
    same_model(e, want, "after the change")
    tok, off = _native.flatten(c["X"])
    e.compute(tok, off, 96, 0)
    assert e.svm_get_class_weights() == (2.0, 1.0)                  # ... through a new result as well
    e.close()


# ---- 5. weighted cross-validation ------------------------------------------------------------------------------------------------
def check_cv_w(make, n=120, chunks=(7, 256)):
    """3 folds x C in {0.05, 1} with weights (4, 1): every problem equals ``solve_w`` on its sub-matrix, n_bsv included, in both
    forms; the out-of-fold values lie within numpy's bound of the problems' own models."""
    c = cases.edge_case(n)
    fold, Cs, (w_pos, w_neg) = cv.paired(n, 3), (0.05, 1.0), (4.0, 1.0)
    e = computed(make, c)
    K, y = e.get_train(), c["y"]
    want = wc.expected_w(K, y, fold, Cs, w_pos, w_neg, c["eps"])
    assert any(w["n_bsv"] > 0 for w in want) and sum((sum(w["branches"].values()) for w in want)) > 0
    unweighted = cv.expected(K, y, fold, Cs, c["eps"])
    assert any(not np.array_equal(w["alpha"], u["alpha"]) for w, u in zip(want, unweighted))   # (the weights are really on)
    e.svm_set_class_weights(w_pos, w_neg)
    slowest = max(w["iterations"] for w in want)
    for form, wg_max in FORMS:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            got = e.svm_cv(y, fold, Cs, c["eps"])
            assert got["form"] == form
            same_problems(e, got, want, (form, chunk))
            rounds = slowest // chunk + 1
            assert got["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, got["launches"])
    ref, bound = cv.oof_reference(K, y, fold, want, len(Cs))
    assert np.all(np.abs(got["decision"] - ref) <= bound)
    e.close()


# ---- 6. Platt's fit, host only ---------------------------------------------------------------------------------------------------
def check_platt_fit(lib):
    """A, B, iterations and status equal LIBSVM's sigmoid_train restated on Python floats, bit for bit."""
    seen = {}
    for name, (dec, y) in wc.platt_inputs().items():
        want, got = wc.platt_fit(dec, y), lib.platt_fit(dec, y)
        for key in ("A", "B", "iterations", "status"):
            assert got[key] == want[key], (name, key, got[key], want[key])
        seen[name] = want
    assert seen["all_equal"]["iterations"] == 0 and seen["all_equal"]["A"] == 0.0 and seen["all_equal"]["status"] == 0
    assert seen["anti_correlated"]["A"] > 0 and seen["overlapping"]["A"] < 0 and seen["far_apart"]["A"] < 0
    assert all(w["status"] == 0 and w["iterations"] > 0 for name, w in seen.items() if name != "all_equal")
    dec, y = wc.platt_inputs()["overlapping"]
    L = lib.L
    from fastsk_amd import _native
    out = _native.SvmPlattInfo()
    import ctypes
    y32, bad = np.ascontiguousarray(y, dtype=np.int32), np.ascontiguousarray(y, dtype=np.int32).copy()
    bad[3] = 0
    assert L.fsk_svm_platt_fit(dec.ctypes.data, y32.ctypes.data, len(dec), ctypes.byref(out)) == 0
    assert L.fsk_svm_platt_fit(None, y32.ctypes.data, len(dec), ctypes.byref(out)) == -1
    assert L.fsk_svm_platt_fit(dec.ctypes.data, None, len(dec), ctypes.byref(out)) == -1
    assert L.fsk_svm_platt_fit(dec.ctypes.data, y32.ctypes.data, len(dec), None) == -1
    assert L.fsk_svm_platt_fit(dec.ctypes.data, y32.ctypes.data, 0, ctypes.byref(out)) == -1
    assert L.fsk_svm_platt_fit(dec.ctypes.data, bad.ctypes.data, len(dec), ctypes.byref(out)) == -1
    for wrong, word in ((bad, "label 3"), (y32[:0], "at least one")):     # the wrapper names what is wrong
        with pytest.raises(ValueError) as err:
            lib.platt_fit(dec[:len(wrong)], wrong)
        assert word in str(err.value)
    with pytest.raises(ValueError):
        lib.platt_fit(dec[:5], y32)
    p = wc.sigmoid_predict(np.array([-20.0, -1.0, 0.0, 1.0, 20.0]), seen["overlapping"]["A"], seen["overlapping"]["B"])
    assert np.all(np.diff(p) > 0) and 0.0 < p[0] < p[-1] < 1.0     # (A < 0: larger decision values, larger P(+1))


# ---- 7. calibration --------------------------------------------------------------------------------------------------------------
def check_calibration(make, c, weights, planted=False, skip=False):
    """svm_train with weights, then svm_calibrate(fold, 5): the out-of-fold values against ``solve_w`` and numpy's sums per fold;
    (A, B) equal ``platt_fit(oof, y)`` and ``svm_proba`` equals ``sigmoid_predict(svm_decision)``, bit for bit, for train and
    test rows; a stored cross-validation is not touched and touches nothing; a new train drops the calibration."""
    from fastsk_amd import _native
    n, N, y, eps, C = c["n_train"], c["n_train"] + c["n_test"], c["y"], c["eps"], c["C"]
    w_pos, w_neg, Cp, Cn = wc.boxes(c, weights)
    fold = _native.stratified_folds(y, 5, seed=0)
    e = computed(make, c, skip_test_block=skip)
    K = e.get_train()

    def code(fn, *words):
        with pytest.raises(_native.FskError) as err:
            fn()
        assert all(w in str(err.value) for w in words), str(err.value)
        return err.value.code

    e.svm_set_class_weights(w_pos, w_neg)
    assert code(lambda: e.svm_calibrate(fold, 5)) == -3            # no model yet
    e.svm_train(y, C, eps)
    model = e.svm_model()
    assert code(lambda: e.svm_proba(0, 1)) == -3 and code(e.svm_calibration) == -3   # a model, no calibration yet
    stored = e.svm_cv(y, cv.paired(n, 2), (C,), eps)
    alpha_cv = [e.svm_cv_alpha(p) for p in range(2)]
    first = None
    for form, wg_max in FORMS:
        e.set_tuning("svm_wg_max", wg_max)
        info = e.svm_calibrate(fold, 5)
        oof, info2 = e.svm_calibration()
        assert info == info2 and info["form"] == form and info["n_folds"] == 5 and info["launches"] > 0 and info["ms"] > 0
        first = first if first is not None else (oof, info)
        assert np.array_equal(oof, first[0]) and (info["A"], info["B"]) == (first[1]["A"], first[1]["B"])
    want = wc.expected_w(K, y, fold, (C,), w_pos, w_neg, eps)
    slowest = max(w["iterations"] for w in want)
    assert info["launches"] == 2 * 256 * (slowest // 256 + 1)       # (the last calibration ran two launches an iteration)
    ref, bound = cv.oof_reference(K, y, fold, want, 1)
    assert np.all(np.abs(oof - ref[0]) <= bound[0]), float(np.max(np.abs(oof - ref[0]) - bound[0]))
    fit = wc.platt_fit(oof, y)
    for key in ("A", "B", "iterations", "status"):
        assert info[key] == fit[key], (key, info[key], fit[key])
    if planted:
        assert info["A"] < 0 and info["status"] == 0
    for r0, r1 in ((0, n), (n, N), (n - 1, min(n + 1, N)), (N, N)):
        proba = e.svm_proba(r0, r1)
        assert proba.shape == (r1 - r0,) and np.array_equal(proba, wc.sigmoid_predict(e.svm_decision(r0, r1), info["A"], info["B"])), (r0, r1)
        assert np.all((proba > 0.0) & (proba < 1.0))
    assert code(lambda: e.svm_proba(0, N + 1)) == -1 and e.lib.L.fsk_svm_proba(e.h, 0, 2, None) == -1
    assert e.lib.L.fsk_svm_get_calibration(e.h, None, None) == 0    # every output may be null
    # neither touches the other, nor the model
    again = e.svm_cv(y, cv.paired(n, 2), (C,), eps)
    assert all(np.array_equal(alpha_cv[p], e.svm_cv_alpha(p)) for p in range(2)) and np.array_equal(stored["decision"], again["decision"])
    oof2, info3 = e.svm_calibration()
    assert np.array_equal(oof, oof2) and (info3["A"], info3["B"]) == (info["A"], info["B"])
    alpha, rho, _ = e.svm_model()
    assert np.array_equal(alpha, model[0]) and rho == model[1]
    # what fsk_svm_cv refuses, with its messages; a refused call leaves the calibration
    assert code(lambda: e.svm_calibrate(np.where(y > 0, 0, 1).astype(np.int32), 2), "fold 0", "one class") == -1
    ff = fold.copy()
    ff[5] = 7
    assert code(lambda: e.svm_calibrate(ff, 5), "row 5") == -1
    assert code(lambda: e.svm_calibrate(np.where(fold == 1, 2, fold), 5), "fold 1") == -1
    assert code(lambda: e.svm_calibrate(np.zeros(n, dtype=np.int32)), "n_folds") == -1
    assert e.lib.L.fsk_svm_calibrate(e.h, None, 5) == -1 and e.lib.L.fsk_svm_calibrate(None, fold.ctypes.data, 5) == -1
    assert np.array_equal(e.svm_calibration()[0], oof)
    e.svm_train(y, C, eps)                                          # a new model: the calibration is gone
    assert code(lambda: e.svm_proba(0, 1)) == -3 and code(e.svm_calibration) == -3
    e.svm_calibrate(fold, 5)
    tok, off = _native.flatten(c["X"])
    e.compute(tok, off, n, c["n_test"])                             # a new result: the model and with it the calibration
    assert code(lambda: e.svm_proba(0, 1)) == -3 and code(e.svm_calibration) == -3
    e.close()
    return info


def check_class_weights_helper():
    import fastsk_amd
    y = np.array([1, -1, -1, -1, 1, -1, -1, -1], dtype=np.int32)
    assert fastsk_amd.class_weights(y, None) == (1.0, 1.0)
    assert fastsk_amd.class_weights(y, "balanced") == (8 / (2.0 * 2), 8 / (2.0 * 6))
    assert fastsk_amd.class_weights(y, (3, 0.5)) == (3.0, 0.5) and fastsk_amd.class_weights(y, [2.0, 4.0]) == (2.0, 4.0)
    assert fastsk_amd.class_weights(y, {1: 5.0, -1: 0.25}) == (5.0, 0.25) and fastsk_amd.class_weights(y, {-1: 2}) == (1.0, 2.0)
    for bad in ("auto", (1.0,), (1.0, 2.0, 3.0), (0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (float("inf"), 1.0), {0: 1.0}, {2: 1.0}):
        with pytest.raises(ValueError):
            fastsk_amd.class_weights(y, bad)
    with pytest.raises(ValueError):
        fastsk_amd.class_weights(np.ones(4, dtype=np.int32), "balanced")


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
def test_solve_w_with_equal_boxes_is_solve():
    """Host only: ``solve_w`` with Cp == Cn returns what ``svm_cases.solve`` returns."""
    rng = np.random.Generator(np.random.PCG64(9))
    Z = rng.normal(size=(48, 6))
    Z /= np.linalg.norm(Z, axis=1)[:, None]
    K = Z @ Z.T
    np.fill_diagonal(K, 1.0)
    y = np.where(rng.random(48) < 0.4, 1, -1).astype(np.int32)
    for C in (0.05, 1.0, 100.0):
        a, b = cases.solve(K, y, C, 1e-3), wc.solve_w(K, y, C, C, 1e-3)
        assert a["iterations"] > 0 and a["converged"]
        for key in ("rho", "objective", "iterations", "converged", "gap", "n_sv", "n_bsv", "tau_steps", "tau_selected", "pairs"):
            assert a[key] == b[key], (C, key)
        assert np.array_equal(a["alpha"], b["alpha"]) and np.array_equal(a["G"], b["G"])
        assert not any(b["branches"][k] for k in ("mixed_clip_i_between", "mixed_clip_j_between"))


@pytest.mark.parametrize("name", TABLE)
def test_table_cases(make, name):
    check_table_case(make, name, cap=24)


def test_case_set_reaches_the_weighted_branches(make):
    check_branches_reached(make, cap=24)


def test_unit_weights_and_the_setter(make):
    check_unit_weights_and_setter(make)


def test_weighted_cross_validation(make):
    check_cv_w(make)


def test_platt_fit_equals_sigmoid_train(emu_lib):
    check_platt_fit(emu_lib)


def test_platt_fit_of_the_product_library():
    """The same comparison on the hipcc build's host code (no device is touched)."""
    import __graft_entry__ as ge
    ge.build_engine()
    from fastsk_amd import _native
    check_platt_fit(_native.Library())


@pytest.mark.parametrize("skip", [False, True])
def test_calibration(make, skip):
    check_calibration(make, cases.case(96, 60, 8, 4, n_test=9), (4.0, 1.0), planted=True, skip=skip)


def test_calibration_with_few_positives(make):
    y = -np.ones(64, dtype=np.int32)
    y[[1, 5, 12, 20, 29, 37, 44, 50, 58, 63]] = 1                   # ten positives: two a fold
    check_calibration(make, cases.case(64, 40, 6, 2, labels=y, seed=6403, n_test=3), "balanced")


def test_class_weights_helper():
    check_class_weights_helper()
