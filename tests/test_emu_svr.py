"""The epsilon-SVR stage (fsk_svr_train / fsk_svr_get_model / fsk_svr_cv, the shared fsk_svm_decision) on the CPU: the engine's
HIP source compiled against tests/emu/hip_emu.h must reproduce, to the bit, the numpy restatement of tests/svr_cases.py in both
forms of the twin-element loop and for every svm_chunk; a converged solution must pass the certificate and reach scikit-learn's
objective; predictions must agree with numpy within the summation bound. The ``check_*`` functions take an engine factory;
tests/test_gpu_svr.py runs them at scale 1 on the MI355X. Here the larger edges stop after ``cap`` iterations (compared with the
restatement stopped there)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svr_cases as cases  # noqa: E402

FORMS = (("workgroup", 8192), ("two-launch", 0))
CHUNKS = (1, 7, 256)


@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


def computed(make, c, **kw):
    """An engine with the case's kernel resident."""
    from fastsk_amd import _native
    tok, off = _native.flatten(c["X"])
    args = dict(c["engine"])
    args.update(kw)
    seed = args.pop("seed", None)
    e = make(c["g"], c["m"], **args)
    if seed is not None:
        e.set_seed(seed)
    e.compute(tok, off, c["n_train"], c["n_test"])
    return e


def same_model(e, want, name):
    alpha2, coef, rho, info = e.svr_model()
    assert info["iterations"] == want["iterations"], (name, info["iterations"], want["iterations"])
    assert np.array_equal(alpha2, want["alpha2"]) and np.array_equal(coef, want["coef"]), name
    assert rho == want["rho"] and info["objective"] == want["objective"], (name, rho, want["rho"], info["objective"], want["objective"])
    assert info["converged"] == want["converged"] and info["gap"] == want["gap"], name
    assert info["n_sv"] == want["n_sv"] and info["n_bsv"] == want["n_bsv"], name
    return alpha2, coef, rho, info


def check_case(make, c, C=1.0, epsilon=0.1, eps=1e-3, forms=FORMS, chunks=CHUNKS, max_iter=-1, sklearn=True, engine=None, z=None):
    """1. both forms and every chunk equal the restatement bit for bit, launch counts included; 2. the certificate, and
    scikit-learn's objective within 2 eps C (2n); 3. the train rows' predictions. Returns the restatement's result."""
    e = engine or computed(make, c)
    K = e.get_train()
    z = c["z"] if z is None else z
    n = c["n_train"]
    want = cases.solve_svr(K, z, C, epsilon, eps, max_iter)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            info = e.svr_train(z, C, epsilon, eps, max_iter)
            assert info["form"] == form
            alpha2, coef, rho, info = same_model(e, want, (form, chunk))
            rounds = want["iterations"] // chunk + 1
            assert info["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, info)
    if want["converged"]:
        cert = cases.certify(K, z, coef, C, epsilon, eps)
        if not np.any((alpha2[:n] > 0) & (alpha2[n:] > 0)):   # (the objective from coef alone is the solver's only then)
            assert abs(cert["objective"] - info["objective"]) <= 1e-9 * max(1.0, abs(cert["objective"]))
        if sklearn:
            theirs = cases.sklearn_objective(K, z, C, epsilon, eps)
            assert abs(info["objective"] - theirs) <= 2.0 * eps * C * (2 * n), (info["objective"], theirs)
    dec = e.svm_decision(0, n)
    ref, bound = cases.decision_reference(K, coef, rho)
    assert np.all(np.abs(dec - ref) <= bound), float(np.max(np.abs(dec - ref) - bound))
    if engine is None:
        e.close()
    return want


# ---- the edges of each loop -----------------------------------------------------------------------------------------------------
def check_two_launch_edge(make, n, cap=None):
    """svm_wg_max = 0 at n rows: one row a thread, 256 rows a workgroup. Run to the end: the last row takes part in a step;
    from two workgroups on i and j fall into the same and into different ones; an element >= n is chosen as i and as j."""
    c = cases.edge_case(n)
    want = check_case(make, c, forms=FORMS[1:], chunks=(256,) if n != 257 else (7, 256), max_iter=-1 if cap is None else cap,
                      sklearn=cap is None)
    if cap is None:
        pairs = want["pairs"]
        assert want["converged"] and any(n - 1 in (i % n, j % n) for i, j in pairs)
        if n > 256:
            assert any(i >= n for i, _ in pairs) and any(j >= n for _, j in pairs)
            wg = [((i % n) // 256, (j % n) // 256) for i, j in pairs]
            assert any(a == b for a, b in wg) and any(a != b for a, b in wg)
    return want


def check_workgroup_edge(make, n, cap=None):
    """One workgroup at n rows: min(1024, n rounded up to 64) threads, ceil(n / 1024) rows a thread, both twins of each.
    512 / 513: the first row whose second twin lies beyond 1024 elements; 1024 / 1025: a thread's second row."""
    c = cases.edge_case(n)
    want = check_case(make, c, forms=FORMS[:1], chunks=(256,) if n != 1025 else (7, 256), max_iter=-1 if cap is None else cap,
                      sklearn=cap is None and n <= 1025)
    if cap is None:
        pairs = want["pairs"]
        assert want["converged"] and any(n - 1 in (i % n, j % n) for i, j in pairs)
        assert n < 32 or (any(i >= n for i, _ in pairs) and any(j >= n for _, j in pairs))
    return want


def check_automatic_switch(make, max_iter=-1):
    """svm_wg_max = 300: 2n is what is compared — 150 rows take the workgroup, 151 the two launches; the same arithmetic."""
    for n, form in ((150, "workgroup"), (151, "two-launch")):
        c = cases.edge_case(n)
        e = computed(make, c, tuning={"svm_wg_max": 300})
        want = cases.solve_svr(e.get_train(), c["z"], 1.0, 0.1, 1e-3, max_iter)
        assert e.svr_train(c["z"], 1.0, 0.1, 1e-3, max_iter)["form"] == form
        same_model(e, want, form)
        e.close()


def check_both_twins(make):
    """epsilon = 0 at C = 10: some row ends with alpha_e > 0 and alpha*_e > 0 together."""
    c = cases.edge_case(40)
    want = check_case(make, c, C=10.0, epsilon=0.0, chunks=(7,))
    a = want["alpha2"]
    assert want["converged"] and np.any((a[:40] > 0) & (a[40:] > 0))


def check_wide_tube(make):
    """epsilon larger than every |z|: 0 iterations, every coef zero, rho the midpoint of its bounds."""
    c = cases.edge_case(40)
    epsilon = 10.0
    assert epsilon > np.abs(c["z"]).max()
    want = check_case(make, c, epsilon=epsilon, chunks=(1, 256))
    assert want["iterations"] == 0 and want["converged"] and not want["coef"].any() and want["n_sv"] == 0
    z = c["z"]
    ub, lb = float((epsilon - z).min()), float((-(epsilon + z)).max())   # (alpha = 0: y = +1 bounds from above, y = -1 from below)
    assert want["rho"] == (ub + lb) / 2.0


def check_all_at_bound(make):
    """C = 0.05: every support vector at the bound."""
    c = cases.bound_case()
    want = check_case(make, c, C=0.05)
    assert want["n_sv"] == 64 and want["n_bsv"] == 64 and np.all(np.abs(want["coef"]) == 0.05)


def check_constant_targets(make):
    c = cases.edge_case(40)
    z = np.full(40, 0.75)
    want = check_case(make, c, z=z, chunks=(7,))
    assert want["iterations"] == 0 and abs(want["rho"] + 0.75) <= 2.0 ** -52    # (the prediction is the constant)
    want = check_case(make, c, z=z, epsilon=0.0, chunks=(7,))
    assert want["iterations"] == 0 and not want["coef"].any()


def check_duplicates(make):
    """Two identical sequences with different targets: TAU in the selection and in the step."""
    c = cases.duplicates_case()
    want = check_case(make, c, C=10.0, epsilon=0.0)
    assert want["tau_selected"] > 0 and want["tau_steps"] > 0


def check_result_kinds(make, kind):
    """The three triangles a result can be, and engine 0 of a group (chosen as test_emu_svm.check_result_kinds chooses them)."""
    from fastsk_amd import _native
    c = cases.edge_case(70)
    kw = {"fp64": dict(approx=True, t=1, max_iters=6, seed=5), "mismatch": dict(max_mismatches=1),
          "group": dict(devices=[0, 0], collective=_native.COLL_P2P)}[kind]
    e = computed(make, c, **kw)
    if kind == "group":
        assert e.multi_info()["ndev"] == 2
    if kind == "mismatch":
        assert e.mismatch_info()["n_levels"] == 2
    if kind == "fp64":
        assert len(e.get_stdevs()) > 0
    plain = computed(make, c)
    differs = not np.array_equal(plain.get_train(), e.get_train())
    plain.close()
    assert differs == (kind != "group")
    check_case(make, c, chunks=(7,), engine=e)
    e.close()


def check_linear(make):
    """kernel_type="linear": the same solver on the rows kernel K2."""
    c = cases.edge_case(70, n_test=5)
    e = computed(make, c)
    e.svm_set_kernel("linear")
    e.rows_build()
    K2 = e.rows_block(0, 75, 0, 70)
    want = cases.solve_svr(K2[:70], c["z"], 1.0, 0.1, 1e-3)
    for form, wg_max in FORMS:
        e.set_tuning("svm_wg_max", wg_max)
        assert e.svr_train(c["z"], 1.0, 0.1, 1e-3)["form"] == form
        _, coef, rho, _ = same_model(e, want, form)
    assert want["converged"] and not np.array_equal(K2[:70], e.get_train())
    ref, bound = cases.decision_reference(K2, coef, rho)
    assert np.all(np.abs(e.svm_decision(0, 75) - ref) <= bound)
    e.close()


def check_max_iter(make):
    """max_iter = 3: FSK_OK, converged = 0, the restatement stopped after three steps."""
    c = cases.edge_case(96)
    want = check_case(make, c, chunks=(1, 7), max_iter=3)
    assert want["iterations"] == 3 and not want["converged"] and want["gap"] > 1e-3


def check_decision(make, skip):
    """Predictions of train and test rows; with skip_test_block no test x test cell is there and none is read."""
    c = cases.edge_case(90, n_test=65)
    e = computed(make, c, skip_test_block=skip)
    n, N = 90, 155
    e.svr_train(c["z"])
    _, coef, rho, _ = e.svr_model()
    for r0, r1, K_rows in ((0, n, e.get_train()), (n, N, e.get_test()), (n - 1, n + 1, e.get_block(n - 1, n + 1, 0, n))):
        ref, bound = cases.decision_reference(K_rows, coef, rho)
        dec = e.svm_decision(r0, r1)
        assert dec.shape == (r1 - r0,) and np.all(np.abs(dec - ref) <= bound), (r0, r1)
    full = computed(make, c)
    full.svr_train(c["z"])
    assert np.array_equal(full.svm_decision(0, N), e.svm_decision(0, N))
    full.close()
    e.close()


def check_errors(make):
    """Every FSK_EINVAL / FSK_ESTATE of the header, and the one model slot's life."""
    from fastsk_amd import _native
    c = cases.edge_case(20, n_test=3)
    tok, off = _native.flatten(c["X"])
    e = make(c["g"], c["m"])
    L = e.lib.L
    z = np.ascontiguousarray(c["z"])
    y = np.ascontiguousarray(c["y"], dtype=np.int32)
    fold = (np.arange(20) % 2).astype(np.int32)

    def err(fn):
        with pytest.raises(_native.FskError) as x:
            fn()
        return x.value.code, str(x.value)

    def code(fn):
        return err(fn)[0]

    e.n_train = 20
    assert code(lambda: e.svr_train(z)) == -3 and code(e.svr_model) == -3          # nothing computed
    e.compute(tok, off, 20, 3)
    assert code(e.svr_model) == -3                                                   # no model yet
    e.svm_train(y)
    alpha_c, rho_c, _ = e.svm_model()
    # refused calls leave the earlier model, here the C-SVC
    assert code(lambda: e.svr_train(z[:19])) == -1 and code(lambda: e.svr_train(np.ones(23))) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        zz = z.copy()
        zz[7] = bad
        assert code(lambda: e.svr_train(zz)) == -1
    for C, epsilon, eps in ((0.0, 0.1, 1e-3), (-1.0, 0.1, 1e-3), (float("inf"), 0.1, 1e-3), (float("nan"), 0.1, 1e-3), (1.0, -0.1, 1e-3),
                            (1.0, float("inf"), 1e-3), (1.0, float("nan"), 1e-3), (1.0, 0.1, 0.0), (1.0, 0.1, -1e-3), (1.0, 0.1, float("inf")),
                            (1.0, 0.1, float("nan"))):
        assert code(lambda: e.svr_train(z, C, epsilon, eps)) == -1, (C, epsilon, eps)
    assert L.fsk_svr_train(e.h, None, 20, 1.0, 0.1, 1e-3, -1) == -1 and L.fsk_svr_train(None, z.ctypes.data, 20, 1.0, 0.1, 1e-3, -1) == -1
    again = e.svm_model()
    assert np.array_equal(again[0], alpha_c) and again[1] == rho_c
    c3, text = err(e.svr_model)                                                      # the slot holds a C-SVC
    assert c3 == -3 and "C-SVC" in text
    # an SVR model replaces it; the C-SVC's calls name the kind
    assert e.svr_train(z)["converged"]
    assert L.fsk_svr_get_model(e.h, None, None, None, None) == 0                     # every output may be null
    for fn in (e.svm_model, lambda: e.svm_calibrate(fold), lambda: e.svm_proba(0, 2), e.svm_calibration):
        c3, text = err(fn)
        assert c3 == -3 and "SVR" in text, text
    _, coef, rho, _ = e.svr_model()
    assert code(lambda: e.svr_train(z, C=-1.0)) == -1 and np.array_equal(e.svr_model()[1], coef)
    # ... and the reverse
    e.svm_train(y)
    assert code(e.svr_model) == -3 and np.array_equal(e.svm_model()[0], alpha_c)
    # n < 2
    e.compute(tok[:off[1]], off[:2], 1, 0)
    e.n_train = 1
    assert code(lambda: e.svr_train(z[:1])) == -1
    # the model belongs to the result: accumulate, reset, load, a second compute and a change of kernel kind drop it
    e.compute(tok, off, 20, 3)
    e.svr_train(z)
    e.accumulate(np.arange(3, dtype=np.int32))
    assert code(e.svr_model) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    e.finalize()
    assert code(e.svr_model) == -3
    e.svr_train(z)
    e.reset_counts()
    assert code(e.svr_model) == -3
    e.compute(tok, off, 20, 3)
    e.svr_train(z)
    e.load_sequences(tok, off, 20, 3)
    assert code(e.svr_model) == -3
    e.compute(tok, off, 20, 3)
    e.svr_train(z)
    e.compute(tok, off, 20, 3)
    assert code(e.svr_model) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    e.svr_train(z)
    e.svm_set_kernel("linear")
    assert code(e.svr_model) == -3
    e.close()


# ---- cross-validation -----------------------------------------------------------------------------------------------------------
def check_cv(make, n, n_folds, grid, form, max_iter=-1, engine=None, c=None, K=None):
    """Every problem bit-identical to solve_svr on its sub-matrix, oof within the summation bound, the scores the restated sums
    bit for bit."""
    from fastsk_amd import _native
    c = c or cases.edge_case(n)
    e = engine or computed(make, c)
    K = e.get_train() if K is None else K
    z = c["z"]
    Cs, epsilons = grid
    fold = _native.kfold(n, n_folds, seed=3)
    e.set_tuning("svm_wg_max", dict(FORMS)[form])
    e.set_tuning("svm_chunk", 64)
    out = e.svr_cv(z, fold, Cs, epsilons, 1e-3, max_iter)
    assert out["form"] == form and out["oof"].shape == (len(Cs), len(epsilons), n) and len(out["problems"]) == len(Cs) * len(epsilons) * n_folds
    ref = np.zeros_like(out["oof"])
    bound = np.zeros_like(out["oof"])
    most = 0
    for ci, C in enumerate(Cs):
        for q, epsilon in enumerate(epsilons):
            for f in range(n_folds):
                tr = np.flatnonzero(fold != f)
                te = np.flatnonzero(fold == f)
                want = cases.solve_svr(K[np.ix_(tr, tr)], z[tr], C, epsilon, 1e-3, max_iter)
                got = out["problems"][(ci * len(epsilons) + q) * n_folds + f]
                for k in ("iterations", "converged", "gap", "objective", "rho", "n_sv", "n_bsv"):
                    assert got[k] == want[k], (ci, q, f, k, got[k], want[k])
                assert got["n_rows"] == len(tr) and got["fold"] == f and got["C"] == C and got["epsilon"] == epsilon
                ref[ci, q, te], bound[ci, q, te] = cases.decision_reference(K[np.ix_(te, tr)], want["coef"], want["rho"])
                most = max(most, want["iterations"])
            want_scores = cases.scores(out["oof"][ci, q], z)
            for k, v in want_scores.items():
                assert out[k][ci, q] == v or (np.isnan(v) and np.isnan(out[k][ci, q])), (k, out[k][ci, q], v)
    assert np.all(np.abs(out["oof"] - ref) <= bound)
    rounds = most // 64 + 1
    assert out["launches"] == (rounds if form == "workgroup" else 2 * 64 * rounds)
    if engine is None:
        e.close()
    return out


def check_cv_kinds(make, kind):
    """Two result kinds and the rows kernel under the batch."""
    c = cases.edge_case(60)
    if kind == "linear":
        e = computed(make, c)
        e.svm_set_kernel("linear")
        e.rows_build()
        K = e.rows_block(0, 60, 0, 60)
    else:
        e = computed(make, c, **{"fp64": dict(approx=True, t=1, max_iters=6, seed=5), "mismatch": dict(max_mismatches=1)}[kind])
        K = None
    for form in ("workgroup", "two-launch"):
        check_cv(make, 60, 2, ((1.0,), (0.1,)), form, engine=e, c=c, K=K)
    e.close()


def check_cv_errors(make):
    """The refusals of fsk_svr_cv; a refused call leaves the earlier result."""
    from fastsk_amd import _native
    c = cases.edge_case(20)
    e = computed(make, c)
    z = c["z"]
    fold = _native.kfold(20, 4, seed=1)
    L = e.lib.L

    def code(fn):
        with pytest.raises(_native.FskError) as x:
            fn()
        return x.value.code

    assert L.fsk_svr_cv_get(e.h, None, None, None, None) == -3
    first = e.svr_cv(z, fold, [1.0, 2.0], [0.1])
    bad = fold.copy()
    bad[3] = 4
    neg = fold.copy()
    neg[3] = -1
    zz = z.copy()
    zz[5] = np.nan
    gap = np.where(fold == 2, 3, fold).astype(np.int32)      # fold 2 without rows
    for args, kw in (((z, bad, [1.0], [0.1]), dict(n_folds=4)), ((z, neg, [1.0], [0.1]), dict(n_folds=4)), ((z, gap, [1.0], [0.1]), dict(n_folds=4)),
                     ((z, np.zeros(20, dtype=np.int32), [1.0], [0.1]), dict(n_folds=1)), ((zz, fold, [1.0], [0.1]), {}),
                     ((z, fold, [0.0], [0.1]), {}), ((z, fold, [1.0], [-0.1]), {}), ((z, fold, [1.0], [np.inf]), {}), ((z, fold, [], [0.1]), {}),
                     ((z, fold, [1.0], []), {}), ((z, fold, [1.0], [0.1]), dict(eps=0.0)), ((z[:19], fold[:19], [1.0], [0.1]), {}),
                     ((z, fold, np.ones(128), np.zeros(128)), {})):           # 4 x 128 x 128 problems: over the limit
        assert code(lambda: e.svr_cv(*args, **kw)) == -1, (args[2:], kw)
    n_out = np.empty((2, 1, 20))
    assert L.fsk_svr_cv_get(e.h, n_out.ctypes.data, None, None, None) == 0 and np.array_equal(n_out, first["oof"])
    e.compute(*_native.flatten(c["X"]), 20, 0)
    assert L.fsk_svr_cv_get(e.h, None, None, None, None) == -3               # a new result drops it
    e.close()


def check_kfold():
    from fastsk_amd import _native
    import fastsk_amd
    assert fastsk_amd.kfold is _native.kfold and "kfold" in fastsk_amd.__all__
    f = _native.kfold(23, 5, seed=9)
    perm = np.random.Generator(np.random.PCG64(9)).permutation(23)
    assert f.dtype == np.int32 and np.array_equal(f[perm], np.arange(23) % 5)
    assert sorted(np.bincount(f).tolist()) == [4, 4, 5, 5, 5] and not np.array_equal(f, _native.kfold(23, 5, seed=10))
    for n, k in ((10, 1), (10, True), (-1, 2), (10, 2.5)):
        with pytest.raises(ValueError):
            _native.kfold(n, k)


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 513])
def test_two_launch_edges(make, n):
    check_two_launch_edge(make, n, cap=None if n <= 65 else 40)


@pytest.mark.parametrize("n", [2, 32, 33, 511, 512, 513, 1024, 1025])
def test_workgroup_edges(make, n):
    check_workgroup_edge(make, n, cap=None if n <= 33 else 24)


def test_automatic_switch(make):
    check_automatic_switch(make, max_iter=60)


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
def test_cv(make, n_folds, grid, form):
    check_cv(make, 60, n_folds, grid, form, max_iter=-1 if form == "workgroup" else 30)


@pytest.mark.parametrize("form", ["workgroup", "two-launch"])
def test_cv_300_rows(make, form):
    check_cv(make, 300, 2, ((1.0,), (0.1,)), form, max_iter=20)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "linear"])
def test_cv_result_kinds(make, kind):
    check_cv_kinds(make, kind)


def test_cv_errors(make):
    check_cv_errors(make)


def test_kfold():
    check_kfold()
