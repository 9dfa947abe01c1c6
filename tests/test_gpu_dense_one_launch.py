"""The one base launch over all chain-length groups on the MI355X: the product library through the C ABI, the check functions
of tests/test_emu_dense_one_launch.py (which state the contract) over all 495 combinations of (g = 12, m = 8) and the lists of
100 — the 64-bit stores of the first flush and the 64-bit atomic adds of the later ones onto the same cells, the flushes under
direct-to-LDS loads in flight and the stage wait behind them, which the emulator replaces with plain stores, adds and copies.
Every case is N = 130 with dense_shift_one_launch = 1 and = -1; the last runs the benchmark's generator at N = 32,000, the size
at which the launch runs by the default rule, against the committed digest."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_one_launch_cases as one  # noqa: E402
import dense_shift_cases as cases  # noqa: E402
from test_emu_dense_one_launch import (check_list, check_nine_groups, check_planted, check_ragged, check_row_bands,  # noqa: E402
                                       check_twice, check_uneven_steps)
from test_emu_dense_shift import positions  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = np.arange(cases.N_COMBOS, dtype=np.int32)


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


def test_all_combinations_nine_groups_of_step_one(make, port):
    check_nine_groups(make, port, ALL)


def test_uneven_weight_steps(make, port):
    check_uneven_steps(make, port, cases.small_list(positions(port)))


@pytest.mark.parametrize("name", ["gap", "repeated", "subset", "shuffled", "one"])
def test_lists(make, port, name):
    check_list(make, port, name)


@pytest.mark.parametrize("which", ["rows", "cols", "both"])
def test_counts_above_15(make, port, which):
    check_planted(make, port, which, ALL)


def test_ragged(make, port):
    check_ragged(make, port, ALL)


def test_two_calls_without_a_reset(make, port):
    check_twice(make, port, ALL)


def test_row_bands(make, port):
    check_row_bands(make, port, ALL)


def test_default_rule_at_32000_sequences(make):
    """Default tuning at 31,375 tiles: the shift path runs by its own rule and its base products in one launch. The digest of the
    counts equals the committed one of this workload, and the same engine's with the key at -1; the launches are eight apart."""
    import time
    want = json.load(open(os.path.join(ROOT, "profiles", "k_digests.json")))[one.BIG_KEY]
    tok, off = one.bench_sequences()
    e = make(cases.G, cases.M, path=1)
    e.load_sequences(tok, off, one.BIG_N, 0)
    seen = {}
    for key in (0, -1):
        e.set_tuning("dense_shift_one_launch", key)
        e.reset_counts()
        before = e.stats()
        t0 = time.perf_counter()
        e.accumulate(ALL)
        e.synchronize()
        dt = time.perf_counter() - t0
        st = e.stats()
        seen[key] = (e.counts_digest(), {k: st[k] - before[k] for k in ("dense_macs", "n_tile_launches", "launches")})
        print("key %d: %.3f s, %s" % (key, dt, seen[key][1]))
        assert st["path_used"] == 1 and dt < 1.0
    e.close()
    assert seen[0][1]["n_tile_launches"] == seen[-1][1]["n_tile_launches"] == 1
    assert seen[0][1]["dense_macs"] == seen[-1][1]["dense_macs"] == cases.expected_macs(one.BIG_TILES, 165)
    assert seen[-1][1]["launches"] - seen[0][1]["launches"] == 8
    assert seen[0][0] == seen[-1][0] == (int(want["sum"], 16), int(want["xor"], 16))
