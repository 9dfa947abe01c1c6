"""The cross-validated SVM (fsk_svm_cv / fsk_svm_cv_get / fsk_svm_cv_get_alpha) on the CPU: the engine's HIP source compiled
against tests/emu/hip_emu.h. Every problem of a batch must reproduce, to the bit, the numpy restatement of tests/svm_cases.py
on its own sub-matrix, in both forms of the loop and for every svm_chunk; the out-of-fold decision values must be those of
the problem that held the row out, within numpy's summation bound, and identical across forms and chunks; the metrics must
equal their formulas. The ``check_*`` functions take an engine factory and the sizes; tests/test_gpu_svm_cv.py runs them at
the sizes of the kernels' edges on the MI355X. Reduced sizes here, and the larger edges stop after ``cap`` iterations
(compared with the restatement stopped at the same count)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402
import svm_cv_cases as cv  # noqa: E402
from test_emu_svm import computed, emu_lib, make  # noqa: E402,F401  (the fixtures: the emulator's library and engine factory)

FORMS = (("workgroup", 8192), ("two-launch", 0))
CHUNKS = (1, 7, 256)
KEYS = ("iterations", "rho", "objective", "gap", "converged", "n_sv", "n_bsv")


def same_problems(e, got, want, name):
    """Every problem of the call equals the restatement: ``==`` on alpha, rho, objective, gap, iterations, n_sv and n_bsv."""
    assert len(got["problems"]) == len(want), name
    for p, (g, w) in enumerate(zip(got["problems"], want)):
        for key in KEYS:
            assert g[key] == w[key], (name, p, key, g[key], w[key])
        assert g["n_rows"] == len(w["idx"]) and g["C"] == w["C"] and g["fold"] == w["fold"], (name, p)
        assert np.array_equal(e.svm_cv_alpha(p), w["alpha_full"]), (name, p)


def check_cv(make, c, fold, Cs, forms=FORMS, chunks=CHUNKS, max_iter=-1, engine=None, decision=True):
    """Both forms and every chunk: the problems equal the restatement, the launches are those of the slowest problem, the
    decision values lie within numpy's bound and are the same array every time, the metrics equal their formulas. Returns
    (the restatement's problems, the last call's result)."""
    e = engine or computed(make, c)
    K, y, eps = e.get_train(), c["y"], c["eps"]
    want = cv.expected(K, y, fold, Cs, eps, max_iter)
    slowest = max(w["iterations"] for w in want)
    first = got = None
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            got = e.svm_cv(y, fold, Cs, eps, max_iter)
            assert got["form"] == form
            same_problems(e, got, want, (form, chunk))
            rounds = slowest // chunk + 1
            assert got["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, got["launches"])
            if first is None:
                first = got
            assert np.array_equal(got["decision"], first["decision"]), (form, chunk)
            assert np.array_equal(got["auc"], first["auc"]) and np.array_equal(got["accuracy"], first["accuracy"])
    dec = got["decision"]
    assert dec.shape == (len(Cs), c["n_train"])
    if decision:
        ref, bound = cv.oof_reference(K, y, fold, want, len(Cs))
        assert np.all(np.abs(dec - ref) <= bound), float(np.max(np.abs(dec - ref) - bound))
    for ci in range(len(Cs)):
        assert got["auc"][ci] == cv.auc_restated(dec[ci], y)[0] and got["accuracy"][ci] == cv.accuracy_restated(dec[ci], y)
    if engine is None:
        e.close()
    return want, got


# ---- 1. unequal problems in one launch -----------------------------------------------------------------------------------------
def check_unequal(make, n, runs, cap=None, chunks=(7, 256)):
    """Folds of very different sizes x Cs = (0.05, 100): problems of 2 and of a thousand rows in one launch, ending hundreds of
    iterations apart — one that finished early keeps its result through every later launch (chunk 7: many of them)."""
    c = cases.edge_case(n)
    fold = cv.blocks(*runs)
    assert len(fold) == n
    want, _ = check_cv(make, c, fold, (0.05, 100.0), forms=FORMS[:1], chunks=chunks, max_iter=-1 if cap is None else cap)
    its = [w["iterations"] for w in want]
    sizes = sorted({len(w["idx"]) for w in want})
    assert sizes == sorted({n - count for _, count in runs})
    if cap is None:
        assert all(w["converged"] for w in want) and max(its) - min(its) >= 14 and len(set(its)) > 2, its
    return want


# ---- 2. workgroup thread and element edges ---------------------------------------------------------------------------------------
def check_workgroup_edge(make, n_p, cap=None):
    """n_p rows as the larger of two problems (the other has the 2 rows that n_p holds out): min(1024, n_p rounded up to 64)
    threads, ceil(n_p / 1024) elements a thread; the near-duplicate last row is the last element and takes part in a step."""
    c = cases.edge_case(n_p + 2)
    fold = cv.blocks((1, 2), (0, n_p))
    want, _ = check_cv(make, c, fold, (1.0,), forms=FORMS[:1], chunks=(256,) if n_p != 1025 else (7, 256),
                       max_iter=-1 if cap is None else cap)
    big = want[1]
    assert len(big["idx"]) == n_p and len(want[0]["idx"]) == 2
    if cap is None:
        assert big["converged"] and any(n_p - 1 in pair for pair in big["pairs"])


# ---- 3. two-launch edges ---------------------------------------------------------------------------------------------------------
def check_two_launch_edge(make, n, runs, cap=None):
    """svm_wg_max = 0: problems of different workgroup counts in one grid; i and j in the same and in different workgroups."""
    c = cases.edge_case(n)
    fold = cv.blocks(*runs)
    assert len(fold) == n
    want, _ = check_cv(make, c, fold, (1.0,), forms=FORMS[1:], chunks=(7, 256) if n <= 258 else (256,), max_iter=-1 if cap is None else cap)
    assert sorted(len(w["idx"]) for w in want) == sorted(n - count for _, count in runs)
    if cap is None:
        assert all(w["converged"] for w in want)
        pairs = [pair for w in want if len(w["idx"]) > 256 for pair in w["pairs"]]
        if pairs:
            assert any(i // 256 == j // 256 for i, j in pairs) and any(i // 256 != j // 256 for i, j in pairs)
    return want


# ---- 4. more problems than CUs ---------------------------------------------------------------------------------------------------
def check_many_problems(make, n_C, forms=FORMS):
    c = cases.edge_case(40)
    Cs = np.logspace(-2.0, 2.0, n_C)
    want, got = check_cv(make, c, cv.paired(40, 10), Cs, forms=forms, chunks=(256,) if len(forms) == 1 else (7,))
    assert len(want) == 10 * n_C and all(w["converged"] for w in want)


# ---- 6. index mapping ------------------------------------------------------------------------------------------------------------
def check_index_mapping(make):
    """Held-out rows at the first and the last training row and in between, with test rows present and ignored."""
    c = cases.edge_case(90, n_test=65)
    fold = cv.paired(90, 3)
    assert fold[0] == 0 and fold[89] == 2
    check_cv(make, c, fold, (1.0, 100.0), chunks=(7,))


def check_duplicates(make):
    """Rows 0 and 1 identical with opposite labels: both in one training set (K = 1 there: TAU in the selection and in the
    step), and split across folds."""
    c = cases.duplicates_case()
    together = cv.blocks((0, 2), (1, 19), (2, 19))
    want, _ = check_cv(make, c, together, (1.0,), chunks=(7,))
    assert want[0]["tau_steps"] == 0 and all(w["tau_selected"] > 0 and w["tau_steps"] > 0 for w in want[1:])
    split = cv.blocks((0, 1), (1, 1), (0, 19), (1, 19))
    check_cv(make, c, split, (1.0,), chunks=(7,))


def check_result_kinds(make, kind):
    c = cases.edge_case(70)
    kw = {"fp64": dict(approx=True, t=1, max_iters=6, seed=5), "mismatch": dict(max_mismatches=1)}[kind]
    e = computed(make, c, **kw)
    assert (len(e.get_stdevs()) > 0) if kind == "fp64" else (e.mismatch_info()["n_levels"] == 2)
    check_cv(make, c, cv.paired(70, 3), (1.0,), chunks=(7,), engine=e)
    e.close()


# ---- 7. the out-of-fold kernel ---------------------------------------------------------------------------------------------------
def check_oof(make, n):
    """Rows a workgroup and a wave of k_svm_decision_oof: row t's value at C index c is that of problem c F + fold[t], and of no
    other problem of that C."""
    c = cases.edge_case(n)
    fold = cv.paired(n, 3)
    Cs = (0.5, 50.0)
    want, got = check_cv(make, c, fold, Cs, forms=FORMS[:1], chunks=(256,))
    e = computed(make, c)
    K = e.get_train()
    e.close()
    for ci in range(2):
        for f in range(3):
            w = want[ci * 3 + f]
            own, bound = cases.decision_reference(K, c["y"], w["alpha_full"], w["rho"])
            mine = fold == f
            assert np.all(np.abs(got["decision"][ci, mine] - own[mine]) <= bound[mine]), (ci, f)
            assert not np.all(np.abs(got["decision"][ci, ~mine] - own[~mine]) <= bound[~mine]), (ci, f)


# ---- 8. metrics ------------------------------------------------------------------------------------------------------------------
def check_metrics(make):
    """auc against its formula (check_cv) and scikit-learn's; tied decision values from duplicate sequences held out together."""
    from sklearn.metrics import roc_auc_score
    c = cases.duplicates_case()
    y = c["y"]
    fold = cv.blocks((0, 2), (1, 19), (2, 19))
    _, got = check_cv(make, c, fold, (0.05, 1.0), forms=FORMS[:1], chunks=(256,))
    for ci in range(2):
        dec = got["decision"][ci]
        assert dec[0] == dec[1] and y[0] == -y[1]          # the identical pair, held out together: one tie of a pos and a neg
        auc, level = cv.auc_restated(dec, y)
        assert level >= 1 and got["auc"][ci] == auc
        assert abs(got["auc"][ci] - roc_auc_score(y > 0, dec)) <= 1e-12
        assert got["accuracy"][ci] == cv.accuracy_restated(dec, y) and 0.0 < got["accuracy"][ci] <= 1.0


# ---- 9. errors and life ----------------------------------------------------------------------------------------------------------
def check_errors(make):
    from fastsk_amd import _native
    c = cases.edge_case(20, n_test=3)
    tok, off = _native.flatten(c["X"])
    e = make(c["g"], c["m"])
    L = e.lib.L
    y = np.ascontiguousarray(c["y"], dtype=np.int32)
    fold = cv.paired(20, 2)
    Cs = np.array([1.0, 10.0])

    def code(fn, *words):
        with pytest.raises(_native.FskError) as err:
            fn()
        assert all(w in str(err.value) for w in words), str(err.value)
        return err.value.code

    e.n_train = 20
    assert code(lambda: e.svm_cv(y, fold, Cs)) == -3                       # nothing computed
    assert code(lambda: e.svm_cv_alpha(0)) == -3
    e.load_sequences(tok, off, 20, 3)
    e.accumulate(np.arange(15, dtype=np.int32))
    assert code(lambda: e.svm_cv(y, fold, Cs)) == -3                       # accumulated, not finalized
    e.compute(tok, off, 20, 3)
    assert code(lambda: e.svm_cv_alpha(0)) == -3                           # finalized, no cross-validation yet
    assert L.fsk_svm_cv_get(e.h, None, None, None, None) == -3
    assert code(lambda: e.svm_cv(y[:19], fold[:19], Cs)) == -1             # n != n_train
    for bad in (0, 2, -2):
        yy = y.copy()
        yy[7] = bad
        assert code(lambda: e.svm_cv(yy, fold, Cs), "label 7") == -1
    for bad in (-1, 2):
        ff = fold.copy()
        ff[5] = bad
        assert code(lambda: e.svm_cv(y, ff, Cs, n_folds=2), "row 5") == -1  # a fold id out of range
    assert code(lambda: e.svm_cv(y, fold * 2, Cs), "fold 1") == -1         # folds 0 and 2: fold 1 is empty
    assert code(lambda: e.svm_cv(y, (np.arange(20) % 2).astype(np.int32), Cs), "fold 0", "one class") == -1
    assert code(lambda: e.svm_cv(y, np.zeros(20, dtype=np.int32), Cs), "n_folds") == -1      # n_folds = 1
    assert code(lambda: e.svm_cv(y, fold, Cs, n_folds=0), "n_folds") == -1
    assert code(lambda: e.svm_cv(y, fold, np.zeros(0)), "n_C") == -1
    for C in (0.0, -1.0, float("inf"), float("nan")):
        assert code(lambda: e.svm_cv(y, fold, [1.0, C]), "C 1") == -1
    for eps in (0.0, -1e-3, float("inf"), float("nan")):
        assert code(lambda: e.svm_cv(y, fold, Cs, eps), "eps") == -1
    assert code(lambda: e.svm_cv(y, fold, np.ones(32768)), "problems") == -1                 # 2 x 32768 > 65535
    assert L.fsk_svm_cv(None, y.ctypes.data, 20, fold.ctypes.data, 2, Cs.ctypes.data, 2, 1e-3, -1) == -1
    assert L.fsk_svm_cv(e.h, None, 20, fold.ctypes.data, 2, Cs.ctypes.data, 2, 1e-3, -1) == -1
    assert code(lambda: e.svm_cv_alpha(0)) == -3                           # a refused call leaves no result
    # the engine is usable after every error; the model of a prior train is not touched, nor the result by a later train
    e.svm_train(y, 3.0)
    alpha0, rho0, info0 = e.svm_model()
    dec0 = e.svm_decision(0, 23)
    got = e.svm_cv(y, fold, Cs)
    assert all(q["converged"] for q in got["problems"])
    alpha1, rho1, info1 = e.svm_model()
    assert np.array_equal(alpha0, alpha1) and rho0 == rho1 and info0 == info1 and np.array_equal(dec0, e.svm_decision(0, 23))
    a_before = [e.svm_cv_alpha(p) for p in range(4)]
    e.svm_train(y, 0.5)
    assert all(np.array_equal(a_before[p], e.svm_cv_alpha(p)) for p in range(4))
    assert L.fsk_svm_cv_get(e.h, None, None, None, None) == 0              # every output may be null
    assert code(lambda: e.svm_cv_alpha(4)) == -1 and code(lambda: e.svm_cv_alpha(-1)) == -1
    assert L.fsk_svm_cv_get_alpha(e.h, 0, None) == -1
    few = e.svm_cv(y, fold, Cs, max_iter=3)
    assert [q["converged"] for q in few["problems"]] == [False] * 4 and [q["iterations"] for q in few["problems"]] == [3] * 4
    # the result belongs to the kernel: a stale one hides it, a new one drops it
    e.accumulate(np.arange(3, dtype=np.int32))
    assert code(lambda: e.svm_cv_alpha(0)) == -3
    e.finalize()
    assert code(lambda: e.svm_cv_alpha(0)) == -3
    e.svm_cv(y, fold, Cs)
    e.compute(tok, off, 20, 3)
    assert code(lambda: e.svm_cv_alpha(0)) == -3 and L.fsk_svm_cv_get(e.h, None, None, None, None) == -3
    e.close()


# ---- 10. the fold helper ---------------------------------------------------------------------------------------------------------
def check_stratified_folds():
    import fastsk_amd
    rng = np.random.Generator(np.random.PCG64(3))
    y = np.where(rng.random(103) < 0.3, 1, -1).astype(np.int32)
    for k, seed in ((5, 0), (3, 11)):
        fold = fastsk_amd.stratified_folds(y, k, seed=seed)
        assert fold.dtype == np.int32 and np.array_equal(fold, cv.stratified_folds_restated(y, k, seed))
        for label in (1, -1):
            counts = np.bincount(fold[y == label], minlength=k)
            assert counts.max() - counts.min() <= 1
    assert not np.array_equal(fastsk_amd.stratified_folds(y, 5, seed=0), fastsk_amd.stratified_folds(y, 5, seed=1))
    for bad in (1, 0, 2.0, True):
        with pytest.raises(ValueError):
            fastsk_amd.stratified_folds(y, bad)


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("n,runs,cap", [(70, ((0, 68), (1, 1), (2, 1)), None), (132, ((0, 66), (1, 65), (2, 1)), None),
                                        (1030, ((0, 1028), (1, 1), (2, 1)), 12)])
def test_unequal_problems_in_one_launch(make, n, runs, cap):
    check_unequal(make, n, runs, cap=cap, chunks=(7, 256) if cap is None else (7,))


@pytest.mark.parametrize("n_p", [64, 65, 1025])
def test_workgroup_edges(make, n_p):
    check_workgroup_edge(make, n_p, cap=None if n_p <= 65 else 16)


@pytest.mark.parametrize("n,runs,cap", [(258, ((0, 256), (1, 2)), None), (770, ((0, 257), (1, 513)), 40)])
def test_two_launch_edges(make, n, runs, cap):
    check_two_launch_edge(make, n, runs, cap=cap)


def test_more_problems_than_compute_units(make):
    check_many_problems(make, 12, forms=FORMS[:1])
    check_many_problems(make, 2)


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
