"""Centre-weighted mode (fsk_set_center_weights, ``center_weights=``) on the CPU: the engine's HIP source compiled against
tests/emu/hip_emu.h must reproduce, to the bit, the yardsticks of tests/center_weight_cases.py — the brute force over
weighted windows, the CPU oracle folded over single windows and over the level rows of a non-increasing profile. The
``check_*`` functions take an engine factory and a scale; tests/test_gpu_center_weights.py runs them at scale 1 on the MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import center_weight_cases as cases  # noqa: E402
import revcomp_cases  # noqa: E402

SCALE = 0.3
_FOLDS = {}


@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


def fold_once(port, key, case, comp=None):
    """The layer fold of a case (non-increasing profile), computed once per session and shared: read-only."""
    key = (key, None if comp is None else tuple(sorted(comp.items())))
    if key not in _FOLDS:
        want = cases.layer_fold(port, case["seqs"], case["profile"], case["g"], case["m"], case["combos"], comp)
        want.setflags(write=False)
        _FOLDS[key] = want
    return _FOLDS[key]


def run(make, case, path, tuning=None, comp=None, n_train=None, profile="case", **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(case["seqs"])
    n = len(case["seqs"])
    ntr = n if n_train is None else n_train
    e = make(case["g"], case["m"], path=path, tuning=dict(tuning or {}), revcomp=comp,
             center_weights=case["profile"] if profile == "case" else profile, wildcards=case.get("wild"), **kw)
    e.load_sequences(tok, off, ntr, n - ntr)
    e.accumulate(case["combos"])
    e.finalize()
    return e


def stats_of(case, comp=None):
    return cases.expected_stats(case["seqs"], case["g"], case["profile"], set(case.get("wild") or ()), comp)


# ---- 1. the definition --------------------------------------------------------------------------------------------------------
def check_definition(make, port, path, comp=None):
    """brute and window_fold agree with each other before the engine is asked; then counts, statistics and every getter."""
    case = cases.definition_case()
    seqs, g, m, prof, ntr = case["seqs"], case["g"], case["m"], case["profile"], case["n_train"]
    n = len(seqs)
    want = cases.brute(port, seqs, prof, g, m, case["combos"], comp)
    assert np.array_equal(want, cases.window_fold(port, seqs, prof, g, m, case["combos"], comp))
    e = run(make, case, path, comp=comp, n_train=ntr)
    st = e.stats()
    nfeat, maxw = stats_of(case, comp)
    assert st["center_weights"] == prof and st["n_feat"] == nfeat and st["max_windows"] == maxw
    assert path == 0 or st["path_used"] == path
    assert np.array_equal(e.get_counts(), want)
    tri = port.normalise(want.astype(np.float64), n)
    assert np.array_equal(e.get_triangle(), tri)
    sq = tri_to_square(tri, n)
    assert np.array_equal(e.get_train(), sq[:ntr, :ntr]) and np.array_equal(e.get_test(), sq[ntr:, :ntr])
    e.close()


# ---- 2. identities ----------------------------------------------------------------------------------------------------------------
def check_ones_is_off(make, port, path, comp=None):
    """All ones, and a profile whose entries other than 1 no window reaches: counts, statistics and the launches of the mode
    off."""
    from fastsk_amd import _native
    case = cases.definition_case()
    tok, off = _native.flatten(case["seqs"])
    reach = max(int(cases.distances(len(s), case["g"]).max()) for s in case["seqs"])
    out = []
    for prof in (None, [1], [1] * 9, [1] * (reach + 1) + [7, 0]):
        e = make(case["g"], case["m"], path=path, center_weights=prof, revcomp=comp)
        e.compute(tok, off, len(case["seqs"]), 0)
        st = e.stats()
        out.append((e.get_counts(), st["n_feat"], st["launches"], st["max_windows"], st["count_launches"], st["sort_records"]))
        e.close()
    plain = port.raw_counts(tok, off, case["g"], case["m"], case["combos"], threads=cases.THREADS)[0]
    if comp is None:
        assert np.array_equal(out[0][0], plain)
    for o in out[1:]:
        assert np.array_equal(out[0][0], o[0]) and out[0][1:] == o[1:]


def check_constant(make, port, path, c=3):
    """[c]: c^2 K, n_feat and max_windows c-fold."""
    from fastsk_amd import _native
    case = cases.definition_case()
    tok, off = _native.flatten(case["seqs"])
    plain = port.raw_counts(tok, off, case["g"], case["m"], case["combos"], threads=cases.THREADS)[0]
    e = make(case["g"], case["m"], path=path, center_weights=[c])
    e.compute(tok, off, len(case["seqs"]), 0)
    assert np.array_equal(e.get_counts(), plain * np.uint64(c * c))
    assert e.stats()["n_feat"] == c * sum(len(s) - case["g"] + 1 for s in case["seqs"])
    e.close()


def check_plateau(make, port, path, scale, comp=None):
    """[1] * P + [0]: the plain kernel of the trimmed sequences, by the oracle itself at a full regime size."""
    from fastsk_amd import _native
    from oracle import loader
    case = cases.regime_case(300, 8, scale)
    plateau = 40
    cut = cases.trimmed(case["seqs"], case["g"], plateau)
    tok0, off0 = loader.flatten(cut + [[cases.DNA[t] for t in reversed(s)] for s in cut] if comp else cut)
    want = port.raw_counts(tok0, off0, case["g"], case["m"], case["combos"], threads=cases.THREADS)[0]
    if comp:
        import wildcard_cases
        want = wildcard_cases.fold_rows(want, list(range(len(cut))) * 2, len(cut))
    e = run(make, case, path, comp=comp, profile=[1] * plateau + [0])
    st = e.stats()
    s = 2 if comp else 1
    assert st["n_feat"] == s * sum(len(c) - case["g"] + 1 for c in cut) and st["max_windows"] == s * max(len(c) - case["g"] + 1 for c in cut)
    assert max(len(c) - case["g"] + 1 for c in cut) == 2 * plateau   # (an even number of windows: two of them at d = 0)
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 3. one panel ---------------------------------------------------------------------------------------------------------------------
def check_panel(make, port, path, comp=None):
    case = cases.panel_case()
    want = cases.brute(port, case["seqs"], case["profile"], case["g"], case["m"], case["combos"], comp)
    e = run(make, case, path, comp=comp)
    assert e.stats()["n_feat"] == stats_of(case, comp)[0]
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 4. the dense staging regimes ---------------------------------------------------------------------------------------------------
# (longest sequence, m at g = 12, tuning, strands) -> planned (chunked staging, sweeps > 1, window-key cache)
REGIMES = [("resident", 300, 8, {}, 1, (False, False, False)),
           ("two chunks", 1025, 8, {}, 1, (True, False, False)),
           ("tiny chunks", 300, 8, {"dense_chunk": 7}, 1, (True, False, False)),
           ("many sweeps", 1000, 5, {}, 1, (False, True, False)),
           ("many sweeps, key cache", 500, 5, {}, 1, (False, True, True)),
           ("both strands resident", 300, 8, {}, 2, (False, False, False)),
           ("both strands chunked", 1025, 8, {}, 2, (True, False, False))]


def check_regime(make, port, name, lmax, m, tun, strands, planned, scale):
    """k_dense_count<., ., ., ., WGT> where accumulate_dense puts it (center_weight_cases.dense_plan restates the plan and
    the plan is asserted): symbols resident, chunked staging (the chunk's base enters the distance), a seven-window chunk,
    many histogram sweeps replaying the window-key cache, and the strand loop of reverse complement, resident and
    re-staged. path = 2: the sparse dataflow on the same sequences (repeated records)."""
    comp = cases.DNA if strands == 2 else None
    case = cases.regime_case(lmax, m, scale)
    ch, sweeps, resident, cache = cases.dense_plan(lmax, case["g"], case["keys"], False, strands, len(case["profile"]), False,
                                                   tun.get("dense_chunk", 0))
    assert (ch < lmax - case["g"] + 1, sweeps > 1, cache) == planned, (ch, sweeps, resident, cache)
    assert max(len(s) for s in case["seqs"]) == lmax
    want = fold_once(port, ("regime", lmax, m, scale), case, comp)
    nfeat, maxw = stats_of(case, comp)
    for path, t in ((1, tun), (2, {})):
        e = run(make, case, path, t, comp)
        st = e.stats()
        assert st["path_used"] == path and st["n_feat"] == nfeat and st["max_windows"] == maxw and st["key_space"] == case["keys"]
        assert np.array_equal(e.get_counts(), want), (name, path)
        e.close()


def check_rare_symbol(make, port, scale):
    """A rare fifth symbol (m = 7: 5^5 keys): key compaction with the marking pass over every window (compact_rare asked for
    or not: the places-of-rare-symbols form is not taken in this mode) and without compaction."""
    case = cases.regime_case(300, 7, scale, rare=True)
    assert case["keys"] == 3125
    want = fold_once(port, ("rare", scale), case)
    for tun, compacted in (({"compact": 1, "compact_rare": 0}, True), ({"compact": 1, "compact_rare": 1}, True), ({"compact": 0}, False)):
        e = run(make, case, 1, tun)
        st = e.stats()
        assert st["path_used"] == 1 and st["alphabet"] == 5 and (st["compact_keys_avg"] > 0) == compacted, tun
        assert np.array_equal(e.get_counts(), want), tun
        e.close()


def check_zero_weights_in_a_regime(make, port, name, lmax, m, tun, strands, scale):
    """Zeros inside the profile: the validity words and the weights together (k_dense_count<., ., ., true, true>)."""
    comp = cases.DNA if strands == 2 else None
    case = dict(cases.regime_case(lmax, m, scale))
    case["profile"] = [5, 0, 3, 3, 0, 0, 2] + [1] * 30 + [0] * 25 + [2]
    want = cases.brute(port, case["seqs"], case["profile"], case["g"], case["m"], case["combos"], comp)
    nfeat, maxw = stats_of(case, comp)
    for path, t in ((1, tun), (2, {})):
        e = run(make, case, path, t, comp)
        st = e.stats()
        assert st["path_used"] == path and st["n_feat"] == nfeat and st["max_windows"] == maxw
        assert np.array_equal(e.get_counts(), want), (name, path)
        e.close()


# ---- 5. planes ------------------------------------------------------------------------------------------------------------------------
def check_poly_a(make, port, windows, path, scale):
    """Counts above 15 (the hi plane) and above 255 (the overflow flag, the batch recounted by the sparse dataflow) that the
    weights alone produce."""
    case = cases.poly_a_case(windows, scale)
    assert (case["top"] > 15, case["top"] > 255, windows > 15) == ((True, False, False) if windows == 10 else (True, True, True))
    want = fold_once(port, ("poly", windows, scale), case)
    assert want.max() >= 10 * case["top"] ** 2
    e = run(make, case, path)
    st = e.stats()
    assert np.array_equal(e.get_counts(), want)
    if path == 1:
        assert st["path_used"] == 1 and (st["sort_records"] > 0) == (case["top"] > 255)
    e.close()


# ---- 6. weighted sums past 65,535 -----------------------------------------------------------------------------------------------------
def check_heavy(make, port, scale):
    """max_windows = 76,500 from 300 windows: the dense path refused by name and not chosen, unpacked entries and wide cells
    on the sparse dataflow in every form, variance mode refused with the bound named and the engine usable after."""
    from fastsk_amd import _native
    case = cases.heavy_case(scale)
    want = cases.brute(port, case["seqs"], case["profile"], case["g"], case["m"], case["combos"])
    assert int(want.max()) > 2 ** 32 and case["max_windows"] ** 2 > 2 ** 32
    tok, off = _native.flatten(case["seqs"])
    n = len(case["seqs"])
    e = make(case["g"], case["m"], path=1, center_weights=case["profile"])
    with pytest.raises(_native.FskError) as err:
        e.load_sequences(tok, off, n, 0)
    assert err.value.code == -6
    e.close()
    forms = [("auto", {})] + [(name, tun) for name, tun, _ in revcomp_cases.SPARSE_FORMS]
    for name, tun in forms:
        e = run(make, case, 2 if tun else 0, tun)
        st = e.stats()
        assert st["path_used"] == 2 and st["max_windows"] == case["max_windows"], name
        assert np.array_equal(e.get_counts(), want), name
        e.close()
    e = make(case["g"], case["m"], t=1, approx=True, max_iters=4, center_weights=case["profile"])
    with pytest.raises(_native.FskError) as err:
        e.compute(tok, off, n, 0)
    assert err.value.code == -6 and "2^32" in str(err.value)
    e.set_center_weights(None)   # the handle stays usable
    e.compute(tok, off, n, 0)
    assert len(e.get_stdevs()) > 0
    e.close()


# ---- 7. sparse forms ------------------------------------------------------------------------------------------------------------------
def check_sparse_forms(make, port, scale):
    case = cases.low_complexity_case(scale)
    want = fold_once(port, ("lowc", scale), case)
    digests = set()
    forms = revcomp_cases.SPARSE_FORMS + [revcomp_cases.SMALL_BLOCKS,
                                          ("pairs", {"sparse_pairs": 1}, None), ("no pairs", {"sparse_pairs": 0}, None)]
    for name, tun, form in forms:
        e = run(make, case, 2, tun)
        st = e.stats()
        assert st["path_used"] == 2 and (form is None or st["sparse_form"] == form), name
        assert st["n_feat"] == stats_of(case)[0]
        assert np.array_equal(e.get_counts(), want), name
        digests.add(e.counts_digest())
        e.close()
    assert len(digests) == 1


def check_shared_prefix(make, port, scale):
    """sparse_share forced on a batch of more than 16 slots."""
    case = dict(cases.low_complexity_case(scale))
    case["combos"] = np.arange(0, 126, 6 if scale >= 1.0 else 7, dtype=np.int32)
    assert len(case["combos"]) > 16
    want = fold_once(port, ("share", scale), case)
    e = run(make, case, 2, {"sparse_share": 2})
    assert e.stats()["share_positions"] > 0
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 8. with the other modes ------------------------------------------------------------------------------------------------------------
def check_wildcards(make, port, path, comp=None):
    """The weights apply to the valid windows; a sequence whose valid windows all weigh 0 fails the load, named."""
    from fastsk_amd import _native
    case = cases.wildcard_case()
    seqs, g, m, prof, wild = case["seqs"], case["g"], case["m"], case["profile"], set(case["wild"])
    want = cases.brute(port, seqs, prof, g, m, case["combos"], comp, wild)
    assert np.array_equal(want, cases.window_fold(port, seqs, prof, g, m, case["combos"], comp, wild))
    e = run(make, case, path, comp=comp)
    nfeat, maxw = stats_of(case, comp)
    st = e.stats()
    assert st["n_feat"] == nfeat and st["max_windows"] == maxw and st["alphabet"] == 4
    assert np.array_equal(e.get_counts(), want)
    tok, off = _native.flatten(seqs[:4] + [case["dead"]] + seqs[4:])
    with pytest.raises(_native.FskError) as err:
        e.compute(tok, off, len(seqs) + 1, 0)
    assert err.value.code == -2 and "sequence 4 " in str(err.value)
    e.set_center_weights(None)   # without the weights the sequence has two windows left
    e.compute(tok, off, len(seqs) + 1, 0)
    e.close()


def check_mismatch(make, port, path, comp, max_mismatches=2):
    from fastsk_amd import _native
    import mismatch_cases
    case = cases.mismatch_case()
    g, m = case["g"], case["m"]
    c = mismatch_cases.gkm_weights(g, m, max_mismatches)
    want = cases.brute_mismatch(case["seqs"], case["profile"], g, c, comp)
    tok, off = _native.flatten(case["seqs"])
    e = make(g, m, path=path, revcomp=comp, max_mismatches=max_mismatches, center_weights=case["profile"])
    e.compute(tok, off, len(case["seqs"]), 0)
    assert np.array_equal(e.get_counts(), want)
    e.close()


def check_skip_variance(make, port, lib, path):
    """approx + skip_variance, t = 3, seed: brute over exactly the combos the seeded order draws."""
    from fastsk_amd import _native
    case = dict(cases.definition_case())
    g, m = case["g"], case["m"]
    tok, off = _native.flatten(case["seqs"])
    e = make(g, m, t=3, approx=True, skip_variance=True, max_iters=2, path=path, center_weights=case["profile"])
    e.set_seed(7)
    e.compute(tok, off, len(case["seqs"]), 0)
    done = int(e.stats()["combos_done"])
    order = lib.seed_order(7, port.num_combos(g, m))
    assert 0 < done <= 6
    want = cases.brute(port, case["seqs"], case["profile"], g, m, np.sort(order[:done]))
    assert np.array_equal(e.get_counts(), want)
    e.close()


def check_variance(make, port, lib):
    """Variance mode, t = 1, seeded. Under the case's profile: triangle and stdevs equal, to the bit, the reference's Welford
    chain restated on the host over ``brute``'s per-combination triangles in the seeded order
    (center_weight_cases.brute_variance, which is first held against the oracle's own approx mode with all weights 1), on
    both dataflows. Then: the mode is
    really on (they differ from the unweighted run), and under [c] — c^2 K for every combination, so every Welford quantity
    scales by an exact power of two at c = 2 — the normalised triangle is the oracle's own and the stdevs 4-fold (from the
    second iteration on)."""
    from fastsk_amd import _native
    from oracle import loader
    case = cases.definition_case()
    g, m, n = case["g"], case["m"], len(case["seqs"])
    tok, off = _native.flatten(case["seqs"])
    outs = {}
    for prof in ("case", None, [2]):
        for path in (1, 2):
            e = make(g, m, t=1, approx=True, max_iters=8, path=path, center_weights=case["profile"] if prof == "case" else prof)
            e.set_seed(11)
            e.compute(tok, off, n, 0)
            outs[(str(prof), path)] = (e.get_triangle(), np.asarray(e.get_stdevs()))
            e.close()
    for prof in ("case", "None", "[2]"):
        assert np.array_equal(outs[(prof, 1)][0], outs[(prof, 2)][0]) and np.array_equal(outs[(prof, 1)][1], outs[(prof, 2)][1])
    assert not np.array_equal(outs[("case", 1)][0], outs[("None", 1)][0])
    order = lib.seed_order(11, port.num_combos(g, m))
    tok0, off0 = loader.flatten(case["seqs"])
    tri, sds, _ = port.compute(tok0, off0, n, 0, g, m, t=1, approx=True, max_iters=8, order=order)
    tri1, sds1 = cases.brute_variance(port, case["seqs"], [1], g, m, order, n, max_iters=8)   # the restatement is the oracle's
    assert np.array_equal(tri1, tri) and np.array_equal(sds1, np.asarray(sds))
    want_tri, want_sds = cases.brute_variance(port, case["seqs"], case["profile"], g, m, order, n, max_iters=8)
    assert len(want_sds) >= 2 and not np.array_equal(want_tri, tri)
    for path in (1, 2):
        assert np.array_equal(outs[("case", path)][0], want_tri), path
        assert np.array_equal(outs[("case", path)][1], want_sds), path
    assert np.array_equal(outs[("None", 1)][0], tri)
    assert np.array_equal(outs[("[2]", 1)][0], tri)
    got, ref = outs[("[2]", 1)][1], np.asarray(sds)
    assert len(got) == len(ref) and got[0] == ref[0]   # (the first iteration has no variance yet: the reference's constant)
    assert np.array_equal(got[1:], 4.0 * ref[1:])


def check_staged(make, port, path, scale):
    """load + accumulate in two calls, a row band (fsk_accumulate_rows), reset_counts, the handle reused at another N, the
    profile switched on -> off -> on."""
    from fastsk_amd import _native
    case = cases.regime_case(150, 8, scale)
    n = len(case["seqs"])
    want = fold_once(port, ("staged", scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], path=path, center_weights=case["profile"])
    e.load_sequences(tok, off, n, 0)
    e.accumulate(case["combos"][:1])
    e.accumulate(case["combos"][1:])
    e.finalize()
    assert np.array_equal(e.get_counts(), want)
    e.reset_counts()
    lo, hi = (128, 256) if n >= 256 else (0, min(n, 128))
    e.set_center_weights([2] * 4096)   # takes effect from the next load: the loaded sequences keep their weights
    e.accumulate_rows(case["combos"], lo, hi)
    e.synchronize()
    band = e.get_counts()
    a, _ = np.tril_indices(n)
    inside = (a >= lo) & (a < hi)
    assert np.array_equal(band[inside], want[inside]) and not band[~inside].any()
    small = {"seqs": case["seqs"][:n // 2 + 1], "g": case["g"], "m": case["m"], "profile": case["profile"], "combos": case["combos"]}
    tok2, off2 = _native.flatten(small["seqs"])
    e.set_center_weights(None)
    e.load_sequences(tok2, off2, len(small["seqs"]), 0)
    e.accumulate(case["combos"])
    e.finalize()
    plain, _, _ = port.raw_counts(tok2, off2, case["g"], case["m"], case["combos"], threads=cases.THREADS)
    assert e.stats()["center_weights"] is None and np.array_equal(e.get_counts(), plain)
    e.set_center_weights(case["profile"])
    e.load_sequences(tok2, off2, len(small["seqs"]), 0)
    e.accumulate(case["combos"])
    e.finalize()
    assert np.array_equal(e.get_counts(), cases.layer_fold(port, small["seqs"], case["profile"], case["g"], case["m"], case["combos"]))
    e.close()


def check_skip_test_block(make, port, path, scale):
    """Cells that may be left at zero are zero or whole; every cell with a train column, and the diagonal, is whole."""
    case = cases.regime_case(150, 8, scale)
    n = len(case["seqs"])
    ntr = (2 * n) // 3
    want = fold_once(port, ("staged", scale), case)
    e = run(make, case, path, n_train=ntr, skip_test_block=True)
    got = e.get_counts()
    a, b = np.tril_indices(n)
    keep = (b < ntr) | (a == b)
    assert np.array_equal(got[keep], want[keep])
    rest = got[~keep]
    assert ((rest == 0) | (rest == want[~keep])).all()
    e.close()


def check_group(make, port, scale):
    """A group handle (devices=[0, 0], the P2P collective) sets the profile on every engine: the single engine's triangle."""
    from fastsk_amd import _native
    case = cases.regime_case(150, 8, scale)
    n = len(case["seqs"])
    want = fold_once(port, ("staged", scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], devices=[0, 0], collective=_native.COLL_P2P, center_weights=case["profile"])
    e.load_sequences(tok, off, n, 0)
    e.accumulate(case["combos"])
    e.finalize()
    assert e.multi_info()["ndev"] == 2 and np.array_equal(e.get_counts(), want)
    assert e.stats()["n_feat"] == stats_of(case)[0]
    e.close()


# ---- 9. errors at the C ABI -------------------------------------------------------------------------------------------------------------
def check_errors(make, port):
    from fastsk_amd import _native
    g, m = 5, 2
    good = [[1, 2, 3, 4, 1, 2, 3], [2, 2, 3, 1, 4, 4, 1, 2]]
    tok, off = _native.flatten(good)
    plain = port.raw_counts(tok, off, g, m, np.arange(10, dtype=np.int32))[0]
    e = make(g, m)
    L = e.lib.L
    for arr, why in ((np.zeros(4097, dtype=np.uint32) + 1, "4096"), (np.array([1, 256], dtype=np.uint32), "255"),
                     (np.array([0, 1], dtype=np.uint32), "first")):
        with pytest.raises(_native.FskError) as err:
            e.set_center_weight_array(arr)
        assert err.value.code == -1 and why in str(err.value)
    assert L.fsk_set_center_weights(e.h, None, 2) == -1 and L.fsk_set_center_weights(e.h, None, -1) == -1
    assert L.fsk_set_center_weights(None, None, 0) == -1
    e.compute(tok, off, 2, 0)   # a refused profile leaves the mode as it was: off
    assert np.array_equal(e.get_counts(), plain)
    e.set_center_weight_array(np.ones(4096, dtype=np.uint32) * 2)   # the longest profile there is
    e.compute(tok, off, 2, 0)
    assert np.array_equal(e.get_counts(), plain * np.uint64(4))
    e.set_center_weight_array(np.zeros(0, dtype=np.uint32))   # n = 0 switches the mode off
    e.compute(tok, off, 2, 0)
    assert e.stats()["center_weights"] is None and np.array_equal(e.get_counts(), plain)
    e.close()


def check_too_many_features(make):
    """The weighted n_feat is what the sort records and feature offsets hold: refused at 2^31, on sequences whose plain
    windows are far below it."""
    from fastsk_amd import _native
    n, L, g = 900, 10000, 8
    tokens = np.ones(n * L, dtype=np.int32)
    offsets = np.arange(n + 1, dtype=np.int64) * L
    assert n * (L - g + 1) < 2 ** 31 <= 255 * n * (L - g + 1)
    e = make(g, 3, path=2, center_weights=[255])
    with pytest.raises(_native.FskError) as err:
        e.load_sequences(tokens, offsets, n, 0)
    assert err.value.code == -6 and "2^31" in str(err.value)
    e.close()


# ---- 10. golden ---------------------------------------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(os.path.join(GOLD, "center_weights.npz"))
    return {k: z[k] for k in z.files}


def check_golden(make, path):
    """The layer fold of the COMPILED reference on rows of EP300 (tests/make_golden_center_weights.py)."""
    d = load_golden()
    assert str(d["reference"]) == "compiled"
    g, m, n = int(d["g"]), int(d["m"]), len(d["offsets"]) - 1
    e = make(g, m, path=path, center_weights=[int(v) for v in d["profile"]])
    e.compute(d["tokens"], d["offsets"], int(d["n_train"]), n - int(d["n_train"]))
    st = e.stats()
    assert st["n_feat"] == int(d["n_feat"]) and st["max_windows"] == int(d["max_windows"])
    assert np.array_equal(e.get_counts(), d["counts"])
    assert np.array_equal(e.get_triangle(), d["tri"])
    e.close()


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_definition(make, port, path, comp):
    check_definition(make, port, path, comp)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_ones_and_unreached_entries_are_the_mode_off(make, port, path, comp):
    check_ones_is_off(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_constant_profile_scales_by_its_square(make, port, path):
    check_constant(make, port, path)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_plateau_is_the_trimmed_kernel(make, port, path, comp):
    check_plateau(make, port, path, SCALE, comp)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_one_panel_every_centre(make, port, path, comp):
    check_panel(make, port, path, comp)


@pytest.mark.parametrize("name,lmax,m,tun,strands,planned", REGIMES, ids=[r[0] for r in REGIMES])
def test_dense_regimes(make, port, name, lmax, m, tun, strands, planned):
    check_regime(make, port, name, lmax, m, tun, strands, planned, SCALE)


@pytest.mark.parametrize("name,lmax,m,tun,strands", [r[:5] for r in REGIMES if r[0] in ("tiny chunks", "both strands resident", "both strands chunked")],
                         ids=["tiny chunks", "both strands resident", "both strands chunked"])
def test_zero_weights_in_a_dense_regime(make, port, name, lmax, m, tun, strands):
    check_zero_weights_in_a_regime(make, port, name, lmax, m, tun, strands, SCALE)


def test_rare_symbol_compaction(make, port):
    check_rare_symbol(make, port, SCALE)


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("windows", [10, 40])
def test_poly_a_crosses_the_planes_by_weight(make, port, windows, path):
    check_poly_a(make, port, windows, path, SCALE)


def test_weighted_sums_past_65535(make, port):
    check_heavy(make, port, SCALE)


def test_sparse_forms(make, port):
    check_sparse_forms(make, port, 0.1)


def test_shared_prefix_batches(make, port):
    check_shared_prefix(make, port, 0.1)


@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_with_wildcards(make, port, path, comp):
    check_wildcards(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
def test_with_mismatch_weights(make, port, path, comp):
    check_mismatch(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_variance(make, port, emu_lib, path):
    check_skip_variance(make, port, emu_lib, path)


def test_variance_mode(make, port, emu_lib):
    check_variance(make, port, emu_lib)


@pytest.mark.parametrize("path", [1, 2])
def test_staged_calls_and_state(make, port, path):
    check_staged(make, port, path, SCALE)


@pytest.mark.parametrize("path", [1, 2])
def test_skip_test_block(make, port, path):
    check_skip_test_block(make, port, path, SCALE)


def test_group_handle(make, port):
    check_group(make, port, SCALE)


def test_errors(make, port):
    check_errors(make, port)


def test_weighted_features_past_2_31_are_refused(make):
    check_too_many_features(make)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(make, path):
    check_golden(make, path)
