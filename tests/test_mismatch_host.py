"""The host side of the mismatch-weighted kernels: the level solver (fsk_mismatch_levels) against Python integers, the argument
checks of both Python surfaces, the header and the ctypes view. No device: the product library loads without one."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

import mismatch_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def product_lib():
    import __graft_entry__ as ge
    ge.build_engine()
    from fastsk_amd import _native
    return _native.Library()


def levels_raw(lib, g, c):
    """fsk_mismatch_levels as it is: (return code, coefficients)."""
    import ctypes as C
    arr = np.array([int(x) for x in c], dtype=np.uint64)
    a = np.zeros(len(arr) + 1, dtype=np.int64)
    n = C.c_int32(-1)
    rc = lib.L.fsk_mismatch_levels(g, arr.ctypes.data, len(arr), a.ctypes.data, C.byref(n))
    return rc, [int(v) for v in a[:max(n.value, 0)]]


def test_solver_against_python_integers(product_lib):
    """Every g <= 14, every m < g: the gkm weights, their truncations, and seeded weight vectors with zeros inside and at the end."""
    rng = np.random.Generator(np.random.PCG64(1407))
    checked = 0
    for g in range(1, 15):
        for m in range(g):
            vectors = [cases.gkm_weights(g, m)] + [cases.gkm_weights(g, m, d) for d in range(m)]
            for _ in range(4):
                c = [int(v) for v in rng.integers(0, 1000, size=m + 1)]
                c[0] = max(c[0], 1)
                for z in rng.integers(0, m + 1, size=int(rng.integers(0, 3))):
                    if z:
                        c[int(z)] = 0
                vectors.append(c)
            tail = [int(rng.integers(1, 50))] + [int(v) for v in rng.integers(0, 9, size=m)]
            tail[(m + 1) // 2 + 1:] = [0] * (m - (m + 1) // 2)   # trailing zeros: trimmed, d < m
            vectors.append(tail)
            vectors.append([int(rng.integers(1, 2 ** 40))] + [int(v) for v in rng.integers(0, 2 ** 20, size=m)])
            for c in vectors:
                want = cases.solve_levels(g, c)
                if not all(-2 ** 63 <= v < 2 ** 63 for v in want):
                    continue
                rc, got = levels_raw(product_lib, g, c)
                assert rc == 0 and got == want, (g, m, c)
                assert product_lib.mismatch_levels(g, c) == want
                checked += 1
    assert checked > 700


def test_gkm_weights_are_the_plain_kernel(product_lib):
    for g, m in ((6, 3), (11, 4), (14, 13), (8, 0), (12, 7)):
        assert product_lib.mismatch_levels(g, cases.gkm_weights(g, m)) == [0] * m + [1]


def test_the_issue_example_and_the_package_level_helper(product_lib):
    assert product_lib.mismatch_levels(4, [6, 3, 0]) == [-6, 3]
    import fastsk_amd
    from fastsk_amd import _native
    assert fastsk_amd.mismatch_levels(4, [6, 3, 0]) == _native.mismatch_levels(4, [6, 3, 0]) == [-6, 3]
    assert _native.solve_mismatch_levels(4, [6, 3, 0]) == [-6, 3]
    # LS-GKM's default: l = 11, k = 7, d = 3
    assert product_lib.mismatch_levels(11, cases.gkm_weights(11, 4, 3)) == cases.solve_levels(11, cases.gkm_weights(11, 4, 3))
    assert len(product_lib.mismatch_levels(11, cases.gkm_weights(11, 4, 3))) == 4


def test_coefficients_beyond_int64_and_bad_weights_are_einval(product_lib):
    for g, c in ((14, [1, 2 ** 63]),                 # a_1 = 2^63
                 (14, [1, 2 ** 62]),                 # a_0 = 1 - 14 * 2^62 < -2^63
                 (14, [2 ** 64 - 1, 0, 0]),          # a_0 = c_0 itself
                 (14, [1, 1, 2 ** 60, 2 ** 62])):    # a product of two large numbers on the way
        want = cases.solve_levels(g, c)
        assert not all(-2 ** 63 <= v < 2 ** 63 for v in want)
        rc, _ = levels_raw(product_lib, g, c)
        assert rc == -1, (g, c)
    assert levels_raw(product_lib, 14, [2 ** 63 - 1, 0])[0] == 0   # (the largest c_0 that is a coefficient)
    for g, c in ((6, [0, 1, 1]), (6, [0]), (4, [1, 1, 1, 1, 1]), (4, []), (0, [1]), (300, [1, 1])):   # c_0 = 0; wrong lengths; bad g
        assert levels_raw(product_lib, g, c)[0] == -1, (g, c)
    from fastsk_amd import _native
    with pytest.raises(_native.FskError) as ei:
        product_lib.mismatch_levels(6, [0, 1, 1])
    assert ei.value.code == -1 and "c[0]" in str(ei.value)


BAD_KEYWORDS = [dict(weights=[1, 1, 1, 1], max_mismatches=2),       # both
                dict(weights=[1, 1, 1]), dict(weights=[1, 1, 1, 1, 1]), dict(weights=[]),   # not m + 1 of them
                dict(weights=[0, 1, 1, 1]),                         # c_0 = 0
                dict(weights=[1, -1, 1, 1]), dict(weights=[1, 2 ** 64, 1, 1]), dict(weights=[1, 1.5, 1, 1]), dict(weights=[1, True, 1, 1]),
                dict(weights="1111"), dict(weights=7),
                dict(weights=[1, 2 ** 62, 0, 0]),                   # a coefficient beyond int64
                dict(max_mismatches=-1), dict(max_mismatches=4), dict(max_mismatches=1.0), dict(max_mismatches="2"), dict(max_mismatches=True)]


@pytest.mark.parametrize("kw", BAD_KEYWORDS, ids=lambda kw: ",".join("%s=%r" % i for i in kw.items())[:50])
def test_python_argument_errors_come_before_any_device_call(product_lib, kw):
    """g = 6, m = 3 on both surfaces: ValueError — there is no device here, a device call would fail differently."""
    from fastsk_amd import _native
    with pytest.raises(ValueError):
        _native.mismatch_weights(6, 3, **kw)
    with pytest.raises(ValueError):
        _native.Engine(6, 3, lib=product_lib, **kw)
    import __graft_entry__ as ge
    ge.build_bindings()
    from fastsk_amd import _fastsk
    with pytest.raises(ValueError):
        _fastsk.FastSK(6, 3, **kw)


def test_python_keyword_forms_and_unsupported_combinations(product_lib):
    from fastsk_amd import _native
    assert _native.mismatch_weights(6, 3) is None
    assert _native.mismatch_weights(11, 4, max_mismatches=3) == [330, 120, 36, 8, 0] == cases.gkm_weights(11, 4, 3)
    assert _native.mismatch_weights(6, 3, max_mismatches=3) == cases.gkm_weights(6, 3)
    assert _native.mismatch_weights(6, 3, weights=(np.int64(5), 3, 0, 0)) == [5, 3, 0, 0]
    for extra, word in ((dict(approx=True), "approx"), (dict(devices=[0, 0]), "devices")):
        with pytest.raises(ValueError) as ei:
            _native.Engine(6, 3, lib=product_lib, max_mismatches=2, **extra)
        assert word in str(ei.value)
    import __graft_entry__ as ge
    ge.build_bindings()
    from fastsk_amd import _fastsk
    for extra, word in ((dict(approx=True), "approx"), (dict(devices=[0, 0]), "devices")):
        with pytest.raises(ValueError) as ei:
            _fastsk.FastSK(6, 3, weights=[1, 1, 0, 0], **extra)
        assert word in str(ei.value)
    assert _fastsk.mismatch_levels(4, [6, 3, 0]) == [-6, 3]
    with pytest.raises(ValueError):
        _fastsk.mismatch_levels(4, [0, 3, 0])
    doc = _fastsk.FastSK.__init__.__doc__
    assert re.search(r"weights: [^,]*= None", doc) and re.search(r"max_mismatches: [^,)]*= None", doc)


def test_header_and_ctypes_view_agree(product_lib):
    from fastsk_amd import _native
    src = open(os.path.join(ROOT, "include", "fastsk_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fsk_[a-z0-9_]+)\s*\(", src))
    new = {"fsk_set_mismatch_weights", "fsk_mismatch_levels", "fsk_get_mismatch_info", "fsk_get_mismatch_times"}
    assert new <= declared and new <= set(_native.SYMBOLS) and declared == set(_native.SYMBOLS)
    for name in new:
        assert hasattr(product_lib.L, name)
    assert product_lib.L.fsk_abi_version() == 5
    assert "mismatch_order" in product_lib.tuning_keys()
