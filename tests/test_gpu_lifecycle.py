"""Engine lifecycle on the MI355X: the check functions of tests/test_emu_lifecycle.py on the product library, for the scenarios
whose teardown differs on real hardware — streams that still hold work when the engine goes (variance mode's chain stream, a
group's exchange), events recorded and never waited for (profile = 2), a second lane's stream, a counts buffer the engine was
only lent, the key-major planes that do not fit. The product library has no counters: the guard asserts instead that a fresh
engine created AFTER each scenario's destroy computes a golden again, in the same process, on both dataflows."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import lifecycle_cases as cases  # noqa: E402
from test_emu_lifecycle import (check_bound_counts, check_group, check_profile_pending, check_shift_plane_cap,  # noqa: E402
                                check_sparse_two_lanes, check_variance_mode, compute, golden_engine)

pytestmark = pytest.mark.gpu


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


class FreshEngineAfter:
    """``with guard() as g``: no counters here (``g.made()`` is None); after the scenario's engines are gone, new ones compute
    the goldens of both dataflows."""

    def __init__(self, make):
        self.make = make

    def made(self):
        return None

    @contextlib.contextmanager
    def __call__(self):
        yield self
        for name, path in ((cases.DENSE, 1), (cases.SPARSE, 2)):
            d = cases.golden(name)
            e = compute(golden_engine(self.make, d, path=path), d)
            assert e.stats()["path_used"] == path
            assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"]), name
            e.close()


@pytest.fixture(scope="module")
def guard(make):
    return FreshEngineAfter(make)


@pytest.mark.parametrize("path", [1, 2])
def test_variance_mode(make, guard, path):
    check_variance_mode(make, guard, path)


def test_profile_2_with_pending_intervals(make, guard):
    check_profile_pending(make, guard)


def test_sparse_two_lanes(make, guard):
    check_sparse_two_lanes(make, guard)


def test_group_destroyed_without_synchronize(native, make, guard):
    """Two engines on device 0 (a device listed twice runs over the peer-to-peer exchange)."""
    check_group(make, guard, native.COLL_P2P, [0, 0])


def test_bound_counts_outlive_the_engine(make, guard):
    import torch

    def device_buffer(cells):
        t = torch.full((cells,), 7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        return t.data_ptr(), lambda: t.cpu().numpy().view(np.uint64), t

    check_bound_counts(make, guard, device_buffer)


def test_shift_plane_cap(make, guard, port):
    check_shift_plane_cap(make, guard, port)
