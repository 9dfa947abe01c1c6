"""What an engine owns goes with it: every scenario of tests/lifecycle_cases.py creates, runs and destroys engines inside
``with guard():`` and compares what they computed with a golden or a case value. On the emulator the guard reads the four live
counters of tests/emu/hip_emu.h — device allocations, pinned allocations, streams, events — before the scenario and asserts
that all four are back where they were after it. tests/test_gpu_lifecycle.py runs the check functions on the device, where the
guard has no counters and instead has a fresh engine compute a golden again after every destroy.

The second half states what a load resets: the per-load figures of fsk_stats start from their initial values after every
fsk_load_sequences."""
import contextlib
import ctypes
import gc
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lifecycle_cases as cases  # noqa: E402

COUNTERS = ("device allocations", "pinned allocations", "streams", "events")


def golden_engine(make, d, **kw):
    e = make(d["g"], d["m"], t=d["t"], approx=bool(d["approx"]), delta=d["delta"], max_iters=d["max_iters"],
             skip_variance=bool(d["skip_variance"]), **kw)
    if d["approx"]:
        e.set_combo_order(d["order"])
    return e


def compute(e, d):
    e.compute(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
    return e


def error_of(native, call):
    with pytest.raises(native.FskError) as err:
        call()
    return err.value


# ---- the scenarios -----------------------------------------------------------------------------------------------------------
def check_dense_exact(make, guard):
    d = cases.golden(cases.DENSE)
    with guard():
        e = compute(golden_engine(make, d, path=1), d)
        assert e.stats()["path_used"] == 1
        assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"])
        e.close()


def check_sparse_two_lanes(make, guard):
    """The batches of an exact accumulate in two lanes: the second lane's stream and the four events that order the lanes are
    made on the way (the emulator sees them alive before the destroy)."""
    d = cases.golden(cases.SPARSE)
    with guard() as g:
        e = compute(golden_engine(make, d, path=2, tuning=cases.lanes_tuning(d)), d)
        assert e.stats()["path_used"] == 2
        assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"])
        made = g.made()
        assert made is None or (made[2] == 2 and made[3] >= 2 + 4), made   # (the engine's stream and lane 1's; ev0, ev1, ev_lane[4])
        e.close()


def check_blocks_passes(make, guard):
    d = cases.golden(cases.SPARSE)
    with guard():
        e = compute(golden_engine(make, d, path=2, tuning=cases.BLOCKS_TUNING), d)
        st = e.stats()
        assert st["sparse_form"] == 2 and st["sparse_passes"] > 1, st
        assert np.array_equal(e.get_counts(), d["counts"])
        e.close()


def check_variance_mode(make, guard, path):
    """Variance mode: the chain stream, the pinned sums, three event arrays a call — and a dropped batch whose sequential sums
    may still run on the chain stream when the engine goes."""
    d = cases.golden(cases.VARIANCE)
    with guard():
        e = compute(golden_engine(make, d, path=path), d)
        assert np.array_equal(e.get_triangle(), d["tri"]) and np.array_equal(e.get_stdevs(), d["stdevs"])
        e.close()


def check_skip_variance(make, guard):
    d = cases.golden(cases.SKIPVAR)
    with guard():
        e = compute(golden_engine(make, d), d)
        assert np.array_equal(e.get_triangle(), d["tri"]) and np.array_equal(e.get_counts(), d["counts"])
        e.close()


def shift_inputs(port):
    import dense_shift_cases as shift
    from test_emu_dense_shift import positions
    from test_emu_dense_shift_lanes import oracle
    import dense_shift_packed_cases as packed
    pos = positions(port)
    ids = packed.span4(pos)
    seqs, tok, off, want = oracle(port, "lifecycle uniform", shift.uniform, ids)
    return ids, [pos[c] for c in ids], tok, off, len(seqs), want


def check_shift_packed_in_place(make, guard, port):
    """The shift classes with the key-major planes, updated in place (the launches are asserted by the case's own run)."""
    from test_emu_dense_shift import differ
    from test_emu_dense_shift_inplace import run
    ids, plist, tok, off, n, want = shift_inputs(port)
    with guard():
        got = run(make, 1, tok, off, n, ids, plist)
        assert not differ(got, want), differ(got, want)


def check_shift_plane_cap(make, guard, port):
    """dense_shift_plane_kb = 1: the planes do not fit and k_dense_shift_fix runs the corrections, three launches fewer — on
    an engine that never had the planes, and on one that holds them from an earlier call."""
    import dense_shift_cases as shift
    import dense_shift_inplace_cases as inplace
    import dense_shift_packed_cases as packed
    from test_emu_dense_shift import differ
    ids, plist, tok, off, n, want = shift_inputs(port)
    packed_launches = 1 + 1 + len({len(c) for c in packed.cut(shift.chains(plist))}) + 1 + 3
    with guard():
        e = make(shift.G, shift.M, path=1, tuning=dict(inplace.TUNING, dense_shift_inplace=1, dense_shift_plane_kb=1))
        e.load_sequences(tok, off, n, 0)
        for cap, launches in ((1, packed_launches - 3), (0, packed_launches), (1, packed_launches - 3)):
            e.set_tuning("dense_shift_plane_kb", cap)
            e.reset_counts()
            before = e.stats()["launches"]
            e.accumulate(np.asarray(ids, dtype=np.int32))
            assert e.stats()["launches"] - before == launches, (cap, e.stats()["launches"] - before, launches)
            e.finalize()
            assert not differ(e.get_counts(), want), (cap, differ(e.get_counts(), want))
        e.close()


def check_modes_in_one_load(make, guard, port, path):
    """Reverse complement, wildcards and centre weights in one load: the complement ranks, the validity bitmap, the window map
    and the profile are all on the device."""
    import center_weight_cases as cw
    import revcomp_cases
    from test_emu_center_weights import run
    case = cw.wildcard_case()
    comp = revcomp_cases.DNA
    want = cw.brute(port, case["seqs"], case["profile"], case["g"], case["m"], case["combos"], comp, set(case["wild"]))
    with guard():
        e = run(make, case, path, comp=comp)
        assert np.array_equal(e.get_counts(), want)
        e.close()


def check_mismatch_levels(make, guard, port):
    """Mismatch-weighted mode: one load and one raw triangle a level, folded through mm_scratch."""
    import mismatch_cases
    from fastsk_amd import _native
    case = mismatch_cases.definition_case()
    weights = mismatch_cases.DEFINITION_WEIGHTS[1]
    want = mismatch_cases.levels_reference(port, case["seqs"], case["g"], weights)[0]
    tok, off = _native.flatten(case["seqs"])
    with guard():
        e = make(case["g"], case["m"], weights=weights)
        e.compute(tok, off, len(case["seqs"]), 0)
        assert len(e.mismatch_info()["levels"]) > 1
        assert np.array_equal(e.get_counts(), want)
        e.close()


def check_svm_and_rows(make, guard):
    """svm_train, svm_cv, svm_calibrate and rows_build on one result: the solver's state, the two fold batches and the rows
    kernel all live until the engine goes."""
    import svm_cases
    from fastsk_amd import _native
    c = svm_cases.edge_case(40, n_test=4)
    tok, off = _native.flatten(c["X"])
    n, y = c["n_train"], c["y"]
    with guard():
        e = make(c["g"], c["m"])
        e.compute(tok, off, n, c["n_test"])
        K = e.get_train()
        want = svm_cases.solve(K, y, c["C"], c["eps"])
        e.svm_train(y, c["C"], c["eps"])
        alpha, rho, _ = e.svm_model()
        assert np.array_equal(alpha, want["alpha"]) and rho == want["rho"]
        fold = _native.stratified_folds(y, 3, seed=0)
        cv = e.svm_cv(y, fold, (0.5, 1.0), c["eps"])
        assert len(cv["problems"]) == 6 and all(p["converged"] for p in cv["problems"])
        assert e.svm_calibrate(fold, 3)["n_folds"] == 3
        assert e.rows_build()["builds"] == 1
        L = e.rows_block(0, n, 0, n, raw=True)
        assert np.allclose(L, K @ K.T, rtol=1e-12, atol=0)
        e.svm_set_kernel("linear")   # the next solve reads the rows kernel
        e.svm_train(y, c["C"], c["eps"])
        assert e.svm_model()[2]["converged"]
        e.close()


def check_profile_pending(make, guard):
    """profile = 2 records event pairs and harvests them later: the engine goes with intervals still pending (nothing asked
    for its statistics)."""
    d = cases.golden(cases.SPARSE)
    with guard() as g:
        e = compute(golden_engine(make, d, path=2, profile=2), d)
        assert np.array_equal(e.get_counts(), d["counts"])
        made = g.made()
        assert made is None or made[3] > 2 + 2, made   # (more events than ev0, ev1 and one interval)
        e.close()


def check_group(make, guard, collective, devices):
    """A group of two engines: the whole pass against the golden, then a second group destroyed right after its accumulate,
    with no synchronize — the exchange may still be in flight."""
    d = cases.golden(cases.GROUP)
    combos = np.asarray(d["combos"], dtype=np.int32)
    with guard():
        e = make(d["g"], d["m"], devices=devices, collective=collective, bands=2)
        compute(e, d)
        assert e.multi_info()["ndev"] == 2
        assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"])
        e.close()
        e = make(d["g"], d["m"], devices=devices, collective=collective, bands=2)
        e.load_sequences(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
        e.accumulate(combos)
        e.close()


def check_bound_counts(make, guard, device_buffer):
    """``device_buffer(cells)`` -> (address of that many u64 cells of device memory, a function that reads them back): the
    engine never frees a buffer it was given, and the counts are still there when the engine is gone."""
    d = cases.golden(cases.DENSE)
    N = d["n_train"] + d["n_test"]
    ptr, read, keep = device_buffer(N * (N + 1) // 2)
    with guard():
        e = make(d["g"], d["m"])
        e.load_sequences(d["tokens"], d["offsets"], d["n_train"], d["n_test"])   # the engine's own triangle: freed at the bind
        e.bind_counts(ptr, N * (N + 1) // 2, keepalive=keep)
        e.reset_counts()
        e.accumulate(np.asarray(d["combos"], dtype=np.int32))
        e.finalize()
        assert e.counts_device_ptr() == ptr and np.array_equal(e.get_triangle(), d["tri"])
        e.close()
    assert np.array_equal(read(), d["counts"])


def check_two_loads(make, guard):
    """Two loads of different N on one engine: every buffer sized by the sequences grows, and the old blocks go."""
    for path, name, n0 in cases.TWO_LOADS:
        d = cases.golden(name)
        tok0, off0, want0 = cases.prefix(d, n0)
        with guard():
            e = make(d["g"], d["m"], path=path)
            e.compute(tok0, off0, n0, 0)
            assert np.array_equal(e.get_counts(), want0), path
            compute(e, d)
            assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"]), path
            e.compute(tok0, off0, n0, 0)
            assert np.array_equal(e.get_counts(), want0), path
            e.close()


def check_error_paths(native, make, guard, monkeypatch, lib=None):
    """A call that fails leaves nothing behind and says why."""
    last = lambda: ((lib or native.library()).L.fsk_last_error(None) or b"").decode()
    d = cases.golden(cases.DENSE)
    with guard() as g:
        monkeypatch.setenv("FSK_TUNING", "no_such_key=1")
        err = error_of(native, lambda: make(5, 2))
        monkeypatch.delenv("FSK_TUNING")
        assert err.code == -1 and "FSK_TUNING" in str(err) and "FSK_TUNING" in last()
        assert g.made() in (None, (0, 0, 0, 0))
        err = error_of(native, lambda: make(5, 2, devices=[0, 99]))   # engine 0 exists when device 99 is refused
        assert err.code == -1 and "device 99" in str(err) and "device 99" in last()
        assert g.made() in (None, (0, 0, 0, 0))
        e = make(d["g"], d["m"])
        before = g.made()
        err = error_of(native, lambda: e.load_sequences(d["tokens"], d["offsets"], 0, d["n_train"] + d["n_test"]))
        assert err.code == -1 and "n_train" in str(err)
        assert g.made() == before
        compute(e, d)   # the handle is as good as before
        assert np.array_equal(e.get_counts(), d["counts"])
        e.close()


# ---- what a load resets ---------------------------------------------------------------------------------------------------------
def per_load(e):
    st = e.stats()
    return {k: st[k] for k in cases.PER_LOAD_STATS}


def check_reload_resets_stats(make, guard):
    """The blocks form in several passes, then the same sequences again: the second run's figures are the first run's, not
    their sum."""
    d = cases.golden(cases.SPARSE)
    with guard():
        e = compute(golden_engine(make, d, path=2, tuning=cases.BLOCKS_TUNING), d)
        first = per_load(e)
        assert first["sparse_passes"] > 1 and first["sparse_form"] == 2, first
        compute(e, d)
        assert np.array_equal(e.get_counts(), d["counts"])
        assert per_load(e) == first, (per_load(e), first)
        e.close()


def check_dense_load_in_between(make, guard):
    """... and a set that takes the dense dataflow in between starts from the initial values: no pass, no form taken."""
    d, dense = cases.golden(cases.SPARSE), cases.golden(cases.DENSE)
    assert (d["g"], d["m"]) == (dense["g"], dense["m"])
    with guard():
        e = compute(golden_engine(make, d, tuning=cases.BLOCKS_TUNING), d)
        first = per_load(e)
        assert e.stats()["path_used"] == 2 and first["sparse_passes"] > 1, first
        compute(e, dense)
        assert e.stats()["path_used"] == 1 and np.array_equal(e.get_counts(), dense["counts"])
        assert per_load(e) == cases.INITIAL_STATS, per_load(e)
        compute(e, d)
        assert np.array_equal(e.get_counts(), d["counts"]) and per_load(e) == first, (per_load(e), first)
        e.close()


# ---- the emulator runs ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


class LiveCounters:
    """``with guard() as g``: the four counters are read on entry; ``g.made()`` is what has been made and not freed since;
    on exit everything is back."""

    def __init__(self, lib):
        self.lib = lib

    def live(self):
        out = (ctypes.c_int64 * 4)()
        self.lib.L.emu_live_counts(out)
        return tuple(out)

    def made(self):
        return tuple(a - b for a, b in zip(self.live(), self.start))

    @contextlib.contextmanager
    def __call__(self):
        gc.collect()
        self.start = self.live()
        yield self
        gc.collect()
        left = {name: n for name, n in zip(COUNTERS, self.made()) if n}
        assert not left, "still alive after the destroy: %s" % left


@pytest.fixture(scope="module")
def guard(emu_lib):
    return LiveCounters(emu_lib)


def host_is_device(cells):
    """The emulator's "device memory" is host memory."""
    buf = np.full(cells, 7, dtype=np.uint64)
    return buf.ctypes.data, lambda: buf, buf


def test_emu_dense_exact(make, guard):
    check_dense_exact(make, guard)


def test_emu_sparse_two_lanes(make, guard):
    check_sparse_two_lanes(make, guard)


def test_emu_blocks_form_in_passes(make, guard):
    check_blocks_passes(make, guard)


@pytest.mark.parametrize("path", [1, 2])
def test_emu_variance_mode(make, guard, path):
    check_variance_mode(make, guard, path)


def test_emu_skip_variance(make, guard):
    check_skip_variance(make, guard)


def test_emu_shift_packed_in_place(make, guard, port):
    check_shift_packed_in_place(make, guard, port)


def test_emu_shift_plane_cap(make, guard, port):
    check_shift_plane_cap(make, guard, port)


@pytest.mark.parametrize("path", [1, 2])
def test_emu_revcomp_wildcards_center_weights(make, guard, port, path):
    check_modes_in_one_load(make, guard, port, path)


def test_emu_mismatch_levels(make, guard, port):
    check_mismatch_levels(make, guard, port)


def test_emu_svm_and_rows(make, guard):
    check_svm_and_rows(make, guard)


def test_emu_profile_2_with_pending_intervals(make, guard):
    check_profile_pending(make, guard)


@pytest.mark.parametrize("collective", ["p2p", "rccl"])
def test_emu_group_destroyed_without_synchronize(make, guard, collective):
    from fastsk_amd import _native
    check_group(make, guard, _native.COLL_RCCL if collective == "rccl" else _native.COLL_P2P, [0, 1])


def test_emu_bound_counts_outlive_the_engine(make, guard):
    check_bound_counts(make, guard, host_is_device)


def test_emu_two_loads_of_different_size(make, guard):
    check_two_loads(make, guard)


def test_emu_error_paths(make, guard, monkeypatch, emu_lib):
    from fastsk_amd import _native
    check_error_paths(_native, make, guard, monkeypatch, emu_lib)


def test_emu_reload_resets_the_per_load_stats(make, guard):
    check_reload_resets_stats(make, guard)


def test_emu_dense_load_in_between_starts_from_nothing(make, guard):
    check_dense_load_in_between(make, guard)
