"""The SVM stage (fsk_svm_train / fsk_svm_get_model / fsk_svm_decision) on the CPU: the engine's HIP source compiled against
tests/emu/hip_emu.h must reproduce, to the bit, the numpy restatement of tests/svm_cases.py in both forms of the loop and for
every svm_chunk; a solution must pass the certificate and reach scikit-learn's objective; decision values must agree with
numpy within the summation bound. The ``check_*`` functions take an engine factory; tests/test_gpu_svm.py runs them at
scale 1 on the MI355X. Small scale here: the sizes whose kernel alone takes seconds on the emulator are the GPU's, and the
larger edges stop after ``cap`` iterations (compared with the restatement stopped there)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svm_cases as cases  # noqa: E402

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
    alpha, rho, info = e.svm_model()
    assert info["iterations"] == want["iterations"], (name, info["iterations"], want["iterations"])
    assert np.array_equal(alpha, want["alpha"]), name
    assert rho == want["rho"] and info["objective"] == want["objective"], (name, rho, want["rho"])
    assert info["converged"] == want["converged"] and info["gap"] == want["gap"], name
    assert info["n_sv"] == want["n_sv"] and info["n_bsv"] == want["n_bsv"], name
    return alpha, rho, info


def check_case(make, c, forms=FORMS, chunks=CHUNKS, max_iter=-1, sklearn=True, engine=None):
    """1. both forms and every chunk equal the restatement bit for bit; 2. the certificate, and scikit-learn's objective
    within 2 eps C n; 3. the train rows' decision values. Returns the restatement's result."""
    e = engine or computed(make, c)
    K = e.get_train()
    n, C, eps = c["n_train"], c["C"], c["eps"]
    want = cases.solve(K, c["y"], C, eps, max_iter)
    for form, wg_max in forms:
        e.set_tuning("svm_wg_max", wg_max)
        for chunk in chunks:
            e.set_tuning("svm_chunk", chunk)
            info = e.svm_train(c["y"], C, eps, max_iter)
            assert info["form"] == form
            alpha, rho, info = same_model(e, want, (form, chunk))
            # a launch takes `chunk` iterations (workgroup) / the host enqueues `chunk` pairs of launches (two-launch)
            rounds = want["iterations"] // chunk + 1
            assert info["launches"] == (rounds if form == "workgroup" else 2 * chunk * rounds), (form, chunk, info)
    if want["converged"]:
        cert = cases.certify(K, c["y"], alpha, C, eps)
        assert abs(cert["objective"] - info["objective"]) <= 1e-9 * max(1.0, abs(cert["objective"]))
        if sklearn:
            theirs = cases.sklearn_objective(K, c["y"], C, eps)
            assert abs(info["objective"] - theirs) <= 2.0 * eps * C * n, (info["objective"], theirs)
    dec = e.svm_decision(0, n)
    ref, bound = cases.decision_reference(K, c["y"], alpha, rho)
    assert np.all(np.abs(dec - ref) <= bound), float(np.max(np.abs(dec - ref) - bound))
    if engine is None:
        e.close()
    return want


# ---- the edges of each loop -----------------------------------------------------------------------------------------------------
def check_two_launch_edge(make, n, cap=None):
    """svm_wg_max = 0 at n rows: 256 rows a workgroup. Run to the end: the last row takes part in a step, and from two
    workgroups on i and j fall into the same and into different ones."""
    c = cases.edge_case(n)
    want = check_case(make, c, forms=FORMS[1:], chunks=(256,) if n != 257 else (7, 256), max_iter=-1 if cap is None else cap,
                      sklearn=cap is None)
    if cap is None:
        pairs = want["pairs"]
        assert want["converged"] and any(n - 1 in p for p in pairs)
        if n > 256:
            assert any(i // 256 == j // 256 for i, j in pairs) and any(i // 256 != j // 256 for i, j in pairs)
    return want


def check_workgroup_edge(make, n, cap=None, c=None):
    """One workgroup at n rows: min(1024, n rounded up to 64) threads, ceil(n / 1024) elements a thread."""
    c = c or cases.edge_case(n)
    want = check_case(make, c, forms=FORMS[:1], chunks=(256,) if n != 1025 else (7, 256), max_iter=-1 if cap is None else cap,
                      sklearn=cap is None and n <= 2048)
    if cap is None:
        assert want["converged"] and any(n - 1 in p for p in want["pairs"])
    return want


def check_automatic_switch(make, max_iter=-1):
    """svm_wg_max = 300: 300 rows take the workgroup, 301 the two launches; the same arithmetic either way."""
    for n, form in ((300, "workgroup"), (301, "two-launch")):
        c = cases.edge_case(n)
        e = computed(make, c, tuning={"svm_wg_max": 300})
        want = cases.solve(e.get_train(), c["y"], c["C"], c["eps"], max_iter)
        assert e.svm_train(c["y"], c["C"], c["eps"], max_iter)["form"] == form
        same_model(e, want, form)
        e.close()


def check_bounds(make):
    """C = 0.05: every alpha at C and rho from the midpoint of its bounds; C = 100: none at C."""
    c = cases.table_cases()["all_at_bound"]
    want = check_case(make, c)
    assert want["n_bsv"] == c["n_train"] and np.all(want["alpha"] == c["C"])
    c = cases.edge_case(96, C=100.0)
    want = check_case(make, c, chunks=(256,))
    assert want["n_bsv"] == 0 and want["n_sv"] > 0


def check_duplicates(make):
    """Identical sequences with opposite labels: K = 1, a_t = 0 — TAU in the selection and in the step."""
    c = cases.duplicates_case()
    want = check_case(make, c)
    assert want["tau_selected"] > 0 and want["tau_steps"] > 0


def check_unbalanced(make):
    check_case(make, cases.unbalanced_case())


def check_result_kinds(make, kind):
    """The three triangles a result can be, and engine 0 of a group."""
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
    assert differs == (kind != "group")   # (the mode is really on; a group's reduced triangle is the single engine's)
    check_case(make, c, chunks=(7,), engine=e)
    e.close()


def check_max_iter(make):
    """max_iter = 5: FSK_OK, converged = 0, the restatement stopped after five steps."""
    c = cases.edge_case(96)
    want = check_case(make, c, chunks=(1, 7), max_iter=5)
    assert want["iterations"] == 5 and not want["converged"] and want["gap"] > c["eps"]
    want0 = check_case(make, c, chunks=(7,), max_iter=0)
    assert want0["iterations"] == 0 and not np.any(want0["alpha"])


def check_decision(make, n_test, skip):
    """Test rows of 1, 63, 64 and 65: a wave a row, four rows a workgroup; with skip_test_block the test x test cells are not
    there and are not read."""
    c = cases.edge_case(90, n_test=n_test)
    e = computed(make, c, skip_test_block=skip)
    n, N = c["n_train"], c["n_train"] + n_test
    e.svm_train(c["y"], c["C"], c["eps"])
    alpha, rho, _ = e.svm_model()
    for r0, r1, K_rows in ((0, n, e.get_train()), (n, N, e.get_test()), (n - 1, n + 1, e.get_block(n - 1, n + 1, 0, n))):
        dec = e.svm_decision(r0, r1)
        ref, bound = cases.decision_reference(K_rows, c["y"], alpha, rho)
        assert dec.shape == (r1 - r0,) and np.all(np.abs(dec - ref) <= bound), (r0, r1)
    assert len(e.svm_decision(N, N)) == 0
    full = computed(make, c)
    full.svm_train(c["y"], c["C"], c["eps"])
    assert np.array_equal(full.svm_decision(0, N), e.svm_decision(0, N))
    full.close()
    e.close()


def host_is_device(n):
    """The emulator's "device memory" is host memory: (address of n doubles, a function that reads them back)."""
    out = np.zeros(n)
    return out.ctypes.data, lambda: out


def check_errors(make, device_buffer=host_is_device):
    """Every FSK_EINVAL / FSK_ESTATE of the header, and the model's life. ``device_buffer(n)`` gives n doubles of DEVICE memory
    for fsk_svm_decision_device and a function that copies them to the host."""
    from fastsk_amd import _native
    c = cases.edge_case(20, n_test=3)
    tok, off = _native.flatten(c["X"])
    e = make(c["g"], c["m"])
    L = e.lib.L
    y = np.ascontiguousarray(c["y"], dtype=np.int32)
    dev_ptr, dev_read = device_buffer(32)

    def code(fn):
        with pytest.raises(_native.FskError) as err:
            fn()
        return err.value.code

    e.n_train = 20
    assert code(lambda: e.svm_train(y)) == -3                      # nothing computed
    assert code(e.svm_model) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    e.load_sequences(tok, off, 20, 3)
    e.accumulate(np.arange(15, dtype=np.int32))
    assert code(lambda: e.svm_train(y)) == -3                      # accumulated, not finalized
    e.finalize()
    assert code(e.svm_model) == -3                                 # finalized, no model yet
    assert code(lambda: e.svm_train(y[:19])) == -1 and code(lambda: e.svm_train(np.ones(23, dtype=np.int32))) == -1
    for bad in (0, 2, -2):
        yy = y.copy()
        yy[7] = bad
        assert code(lambda: e.svm_train(yy)) == -1
    assert code(lambda: e.svm_train(np.ones(20, dtype=np.int32))) == -1     # one class
    assert code(lambda: e.svm_train(-np.ones(20, dtype=np.int32))) == -1
    for C, eps in ((0.0, 1e-3), (-1.0, 1e-3), (float("inf"), 1e-3), (float("nan"), 1e-3), (1.0, 0.0), (1.0, -1e-3),
                   (1.0, float("inf")), (1.0, float("nan"))):
        assert code(lambda: e.svm_train(y, C, eps)) == -1, (C, eps)
    assert L.fsk_svm_train(e.h, None, 20, 1.0, 1e-3, -1) == -1 and L.fsk_svm_train(None, y.ctypes.data, 20, 1.0, 1e-3, -1) == -1
    assert code(e.svm_model) == -3                                 # a refused call leaves no model
    assert e.svm_train(y)["converged"]
    assert L.fsk_svm_get_model(e.h, None, None, None) == 0          # every output may be null
    assert code(lambda: e.svm_decision(-1, 2)) == -1 and code(lambda: e.svm_decision(0, 24)) == -1
    assert code(lambda: e.svm_decision(3, 2)) == -1 and L.fsk_svm_decision(e.h, 0, 2, None) == -1
    assert L.fsk_svm_decision_device(e.h, 0, 23, dev_ptr) == 0 and np.array_equal(dev_read()[:23], e.svm_decision(0, 23))
    assert L.fsk_svm_decision_device(e.h, 0, 2, None) == -1
    # the model belongs to the result: accumulate, reset, load and a second compute drop it
    e.accumulate(np.arange(3, dtype=np.int32))
    assert code(e.svm_model) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    e.finalize()
    assert code(e.svm_model) == -3
    e.svm_train(y)
    e.reset_counts()
    assert code(e.svm_model) == -3
    e.compute(tok, off, 20, 3)
    e.svm_train(y)
    e.load_sequences(tok, off, 20, 3)
    assert code(e.svm_model) == -3
    e.compute(tok, off, 20, 3)
    e.svm_train(y)
    e.compute(tok, off, 20, 3)
    assert code(e.svm_model) == -3 and code(lambda: e.svm_decision(0, 1)) == -3
    e.close()


def check_no_candidate(make):
    """A finalized result with a zero diagonal (sequences loaded, nothing accumulated): every normalised cell is 0 / sqrt(0),
    no row can be a j candidate. Both forms end the solve at once — FSK_OK, not converged, no step, alpha = 0 — as LIBSVM's
    selection does when it finds no second index; the restatement agrees. Then the handle trains normally."""
    from fastsk_amd import _native
    for n in (40, 300):
        c = cases.edge_case(n)
        tok, off = _native.flatten(c["X"])
        e = make(c["g"], c["m"])
        e.load_sequences(tok, off, n, 0)
        e.finalize()
        K = e.get_train()
        assert np.isnan(K).all()
        with np.errstate(invalid="ignore"):
            want = cases.solve(K, c["y"], c["C"], c["eps"])
        assert want["iterations"] == 0 and not want["converged"]
        for form, wg_max in FORMS:
            for chunk in (1, 256):
                e.set_tuning("svm_wg_max", wg_max)
                e.set_tuning("svm_chunk", chunk)
                info = e.svm_train(c["y"], c["C"], c["eps"])
                alpha, rho, _ = e.svm_model()
                assert info["form"] == form and info["iterations"] == 0 and not info["converged"] and info["gap"] == 2.0
                assert not alpha.any() and rho == want["rho"] and info["n_sv"] == 0
        e.compute(tok, off, n, 0)
        assert e.svm_train(c["y"], c["C"], c["eps"])["converged"]
        e.close()


def check_tuning_keys(lib):
    keys = lib.tuning_keys()
    assert keys["svm_wg_max"][:3] == (8192, 0, 8192) and keys["svm_chunk"][:3] == (256, 1, 65536)


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("name", ["n96", "all_at_bound"])
def test_table_cases(make, name):
    want = check_case(make, cases.table_cases()[name])
    assert want["converged"]
    if name == "all_at_bound":
        assert want["iterations"] == 32   # (the count the restatement and LIBSVM both took on this problem)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 513])
def test_two_launch_edges(make, n):
    check_two_launch_edge(make, n, cap=None if n <= 257 else 60)


@pytest.mark.parametrize("n", [2, 64, 1025])
def test_workgroup_edges(make, n):
    check_workgroup_edge(make, n, cap=None if n <= 64 else 24)


def test_automatic_switch(make):
    check_automatic_switch(make, max_iter=80)


def test_all_and_none_at_the_bound(make):
    check_bounds(make)


def test_duplicate_sequences_with_opposite_labels(make):
    check_duplicates(make)


def test_one_positive_in_64(make):
    check_unbalanced(make)


@pytest.mark.parametrize("kind", ["fp64", "mismatch", "group"])
def test_result_kinds(make, kind):
    check_result_kinds(make, kind)


def test_max_iter(make):
    check_max_iter(make)


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("n_test", [1, 63, 64, 65])
def test_decision_values(make, n_test, skip):
    check_decision(make, n_test, skip)


def test_errors_and_the_models_life(make):
    check_errors(make)


def test_no_j_candidate_ends_the_solve(make):
    check_no_candidate(make)


def test_tuning_keys(emu_lib):
    check_tuning_keys(emu_lib)
