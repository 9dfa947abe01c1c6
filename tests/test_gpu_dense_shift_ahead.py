"""The ahead schedule of the packed shift corrections on the MI355X: the product library through the C ABI, the check functions
of tests/test_emu_dense_shift_ahead.py (which state the contract). What only the device can show is the timing of the prefetch:
direct-to-LDS loads that stay in flight across the barriers of a chain's steps (raw s_barrier behind lgkmcnt(0) only), the wait
and the barrier at the chain's end that order every later read after them, and the barrier that orders the overwrite of the idle
buffer and ring half after the previous chain's last read. The emulator lands a load when it is issued and sees none of this;
here every cell of every tile is compared with the CPU oracle, under dense_shift_ahead = 1 and = 0, and that is the race check.
All 495 combinations of (g = 12, m = 8): 120 chains with steps, every chain length, the run of 36 chains of one step, a last chain
without a successor. The last case runs the benchmark's generator at N = 32,000, the size from which the shift path runs by its
default rule, against the committed digest."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import dense_one_launch_cases as one  # noqa: E402
import dense_shift_ahead_cases as ahead  # noqa: E402
import dense_shift_batch_cases as batch  # noqa: E402
import dense_shift_cases as cases  # noqa: E402
import dense_shift_inplace_cases as inplace  # noqa: E402
from test_emu_dense_shift import positions  # noqa: E402
from test_emu_dense_shift_ahead import check_cut, check_list, check_mixed, check_placed, check_small_keys  # noqa: E402

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


def test_all_combinations(make, port):
    check_mixed(make, port, ALL, "all 495")


def test_one_chain(make, port):
    check_list(make, port, ahead.one_chain_list(positions(port)), "one chain", lengths=[9])


def test_one_chain_of_one_step(make, port):
    check_list(make, port, batch.one_step_list(positions(port)), "one step", lengths=[2])


def test_a_class_with_a_gap(make, port):
    check_list(make, port, cases.lists(positions(port))["gap"], "gap", lengths=[4, 4])


def test_a_rank_of_a_sharded_run(make, port):
    check_list(make, port, batch.rank_list(1, 3), "rank 1 of 3")


def test_chain_cut(make, port):
    check_cut(make, port)


@pytest.mark.parametrize("m", (9, 10))
def test_fewer_than_256_keys(make, port, m):
    check_small_keys(make, port, m)


@pytest.mark.parametrize("place", sorted(ahead.PLACES))
def test_flagged_step_loses_the_prefetch(make, port, place):
    check_placed(make, port, place)


def test_flagged_steps_among_all_combinations(make, port):
    check_placed(make, port, "middle", ids=ALL)


def test_two_calls_without_a_reset(make, port):
    check_mixed(make, port, ALL, "all 495", calls=2)


def test_two_row_bands(make, port):
    check_mixed(make, port, ALL, "all 495", bands=((0, 128), (128, inplace.NIBBLES_N)))


def test_key_is_ignored_without_the_in_place_form(make, port):
    check_mixed(make, port, ALL, "all 495", inplace_form=0)


def test_default_rule_at_32000_sequences(make):
    """Default tuning at 31,375 tiles: the shift path runs by its own rule, its corrections by the ahead schedule. The digest of
    the counts equals the committed one of this workload, and the same engine's with the key at 0."""
    want = json.load(open(os.path.join(ROOT, "profiles", "k_digests.json")))[one.BIG_KEY]
    tok, off = one.bench_sequences()
    e = make(cases.G, cases.M, path=1)
    e.load_sequences(tok, off, one.BIG_N, 0)
    seen = {}
    for key in ahead.AHEAD:
        e.set_tuning("dense_shift_ahead", key)
        e.reset_counts()
        before = e.stats()
        e.accumulate(ALL)
        e.synchronize()
        st = e.stats()
        seen[key] = (e.counts_digest(), {k: st[k] - before[k] for k in ("dense_macs", "n_tile_launches", "launches")})
        assert st["path_used"] == 1
    e.close()
    assert seen[1][1] == seen[0][1] and seen[1][1]["dense_macs"] == cases.expected_macs(one.BIG_TILES, 165)
    assert seen[1][0] == seen[0][0] == (int(want["sum"], 16), int(want["xor"], 16))
