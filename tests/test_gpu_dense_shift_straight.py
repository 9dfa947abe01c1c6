"""The straight chains of the packed shift corrections on the MI355X: the product library through the C ABI, the check functions
of tests/test_emu_dense_shift_straight.py (which state the contract). What only the device can show is the timing: a straight
chain's barriers are raw s_barrier behind lgkmcnt(0) with the next chain's prefetch in flight across all of them, the chain's
closing wait and barrier order every later read, and a flagged chain between two straight ones stages over a prefetch a
straight chain's successor must not miss. The emulator lands a load when it is issued and sees none of this; here every cell of
every tile is compared with the CPU oracle, under dense_shift_straight = 1 and = 0, and that is the race check. All 495
combinations of (g = 12, m = 8): 120 chains with steps — more than the 64 descriptors a refill holds — every chain length, the run
of 36 chains of one step, a last chain without a successor. The last case runs the benchmark's generator at N = 32,000, the size
from which the shift path runs by its default rule, against the committed digest."""
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
import dense_shift_straight_cases as straight  # noqa: E402
from test_emu_dense_shift import positions  # noqa: E402
from test_emu_dense_shift_straight import check_cut, check_list, check_mixed, check_one_side, check_placed  # noqa: E402

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
    """120 chains with steps: the descriptors are refilled once."""
    check_mixed(make, port, ALL, "all 495")


def test_one_chain_of_one_step(make, port):
    check_list(make, port, batch.one_step_list(positions(port)), "one step", lengths=[2])


def test_one_chain_of_two_steps(make, port):
    check_list(make, port, straight.two_step_list(positions(port)), "two steps", lengths=[3])


def test_one_chain_of_nine_members(make, port):
    check_list(make, port, ahead.one_chain_list(positions(port)), "one chain", lengths=[9])


def test_one_step_chains_behind_a_long_one(make, port):
    check_list(make, port, straight.long_one_one(positions(port)), "long one one", lengths=[9, 2, 2])


def test_a_rank_of_a_sharded_run(make, port):
    check_list(make, port, batch.rank_list(1, 3), "rank 1 of 3")


def test_a_class_with_a_gap(make, port):
    check_list(make, port, cases.lists(positions(port))["gap"], "gap", lengths=[4, 4])


def test_chain_cut(make, port):
    check_cut(make, port)


@pytest.mark.parametrize("where", straight.WHERE)
@pytest.mark.parametrize("place", sorted(straight.PLACES))
def test_flagged_chain_among_straight_ones(make, port, place, where):
    check_placed(make, port, place, where)


def test_flagged_steps_among_all_combinations(make, port):
    check_placed(make, port, "middle", "first_in_call", ids=ALL)


def test_flag_on_one_side_only(make, port):
    check_one_side(make, port)


def test_two_calls_without_a_reset(make, port):
    check_mixed(make, port, ALL, "all 495", calls=2)


def test_two_row_bands(make, port):
    check_mixed(make, port, ALL, "all 495", bands=((0, 128), (128, inplace.NIBBLES_N)))


@pytest.mark.parametrize("off", ("dense_shift_inplace", "dense_shift_ahead"))
def test_key_is_ignored_without_the_ahead_schedule(make, port, off):
    check_mixed(make, port, ALL, "all 495", **{off: 0})


def test_default_rule_at_32000_sequences(make):
    """Default tuning at 31,375 tiles: the shift path runs by its own rule, its corrections by the straight chains. The digest of
    the counts equals the committed one of this workload, and the same engine's with the key at 0."""
    want = json.load(open(os.path.join(ROOT, "profiles", "k_digests.json")))[one.BIG_KEY]
    tok, off = one.bench_sequences()
    e = make(cases.G, cases.M, path=1)
    e.load_sequences(tok, off, one.BIG_N, 0)
    seen = {}
    for key in straight.STRAIGHT:
        e.set_tuning("dense_shift_straight", key)
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
