"""The load plan (fastsk_amd/csrc/fsk_load_plan.cpp: lengths, window census, alphabet, packed words) without an engine:
tests/host/load_plan_check.cpp links that one unit, is built with the host sanitizers (address + undefined; thread for the
team case) and runs one case a child process. Every field of the plan it writes is compared with the numpy restatement of
the definitions in tests/load_plan_cases.py. No GPU, no library of the package."""
import os
import subprocess

import numpy as np
import pytest

import load_plan_cases as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "load_plan_check.cpp"), os.path.join(ROOT, "fastsk_amd", "csrc", "fsk_load_plan.cpp")]
CASES = lp.cases()
SCALARS = "N nfeat longest shortest most_valid sigma bits V key_symbits total_sym total n_words rc_on wild_on cw_on".split()
VECTORS = "len32 fstart wstart nvalid vstart vbits fwin comp_rank sym_freq distinct staging".split()


def _build(out, sanitize):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] + SOURCES + ["-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "cannot build %s:\n%s" % (out, r.stderr)
    return out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("load_plan"))


@pytest.fixture(scope="module")
def asan_program(workdir):
    return _build(os.path.join(workdir, "load_plan_check_asan"), "address,undefined")


@pytest.fixture(scope="module")
def tsan_program(workdir):
    return _build(os.path.join(workdir, "load_plan_check_tsan"), "thread")


def _run(program, workdir, name, case):
    """One case through the program: a non-zero exit or anything on stderr (a sanitizer's report) fails."""
    src, dst = os.path.join(workdir, name + ".case"), os.path.join(workdir, name + "." + os.path.basename(program) + ".plan")
    lp.write_case(src, case)
    r = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, "%s on %s: exit %d\n%s" % (os.path.basename(program), name, r.returncode, r.stderr)
    return lp.read_plan(dst)


def _compare(got, want, expect):
    assert (got["code"], got["msg"]) == (want["code"], want["msg"])
    for key, value in expect.items():
        if key == "n_words_each":
            assert np.diff(np.append(got["wstart"], got["n_words"])).tolist() == value
        elif key in ("code", "msg") or key in SCALARS:
            assert got[key] == value, key
        else:
            assert got[key].tolist() == value, key
    if want["code"]:
        return
    for key in SCALARS:
        assert got[key] == want[key], key
    for key in VECTORS:
        assert np.array_equal(got[key], want[key]), key


def _team_or_skip(name):
    if name == lp.TEAM and (os.cpu_count() or 1) < 2:
        pytest.skip("one hardware thread: the load plan's team is a single thread here")


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_matches_the_definitions(name, asan_program, workdir):
    _team_or_skip(name)
    case = CASES[name]
    got = _run(asan_program, workdir, name, case)
    _compare(got, lp.reference_plan(case), case.get("expect", {}))
    if "same_as" in case:   # offsets[0] > 0: the same sequences inside a longer token buffer give the same plan
        twin = _run(asan_program, workdir, case["same_as"], CASES[case["same_as"]])
        assert sorted(got) == sorted(twin)
        for key in got:
            assert np.array_equal(got[key], twin[key]), key


def test_team_under_the_thread_sanitizer(tsan_program, workdir):
    _team_or_skip(lp.TEAM)
    case = CASES[lp.TEAM]
    _compare(_run(tsan_program, workdir, lp.TEAM, case), lp.reference_plan(case), case["expect"])
