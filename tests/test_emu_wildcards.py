"""Wildcard mode (fsk_set_wildcards, ``wildcards=``) on the CPU: the engine's HIP source compiled against tests/emu/hip_emu.h
must reproduce, to the bit, the two yardsticks of tests/wildcard_cases.py — the brute force over valid windows and the CPU
oracle folded over the fragments. The ``check_*`` functions take an engine factory and a scale; tests/test_gpu_wildcards.py
runs them at scale 1 on the MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import revcomp_cases  # noqa: E402
import wildcard_cases as cases  # noqa: E402

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
    """The fragment fold of a case, computed once per session and shared: read-only."""
    key = (key, None if comp is None else tuple(sorted(comp.items())))
    if key not in _FOLDS:
        want = cases.fragment_fold(port, case["seqs"], set(case["wild"]), case["g"], case["m"], case["combos"], comp)
        want.setflags(write=False)
        _FOLDS[key] = want
    return _FOLDS[key]


def run(make, case, path, tuning=None, comp=None, n_train=None, **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(case["seqs"])
    n = len(case["seqs"])
    ntr = n if n_train is None else n_train
    e = make(case["g"], case["m"], path=path, tuning=dict(tuning or {}), wildcards=case["wild"], revcomp=comp, **kw)
    e.load_sequences(tok, off, ntr, n - ntr)
    e.accumulate(case["combos"])
    e.finalize()
    return e


def expected_stats(case, comp=None):
    v = cases.valid_counts(case["seqs"], set(case["wild"]), case["g"])
    s = 2 if comp is not None else 1
    return s * sum(v), s * max(v)


# ---- 1. the definition --------------------------------------------------------------------------------------------------------
def check_definition(make, port, path, comp=None):
    """The two yardsticks agree with each other before the engine is asked; then counts, statistics and every getter."""
    case = cases.definition_case()
    seqs, g, m, wild, ntr = case["seqs"], case["g"], case["m"], set(case["wild"]), case["n_train"]
    n = len(seqs)
    want = cases.brute_counts(port, seqs, wild, g, m, case["combos"], comp)
    assert np.array_equal(want, cases.fragment_fold(port, seqs, wild, g, m, case["combos"], comp))
    e = run(make, case, path, comp=comp, n_train=ntr)
    st = e.stats()
    nfeat, maxw = expected_stats(case, comp)
    assert st["wildcards"] == [5, 6] and st["n_feat"] == nfeat and st["max_windows"] == maxw
    assert st["alphabet"] == 4 and st["key_space"] == 4 ** (g - m) and st["bits_per_symbol"] == 2
    assert path == 0 or st["path_used"] == path
    assert np.array_equal(e.get_counts(), want)
    tri = port.normalise(want.astype(np.float64), n)
    assert np.array_equal(e.get_triangle(), tri)
    sq = tri_to_square(tri, n)
    assert np.array_equal(e.get_train(), sq[:ntr, :ntr]) and np.array_equal(e.get_test(), sq[ntr:, :ntr])
    e.close()


def check_absent_wildcard(make, port, path):
    """The mode on with a token that does not occur: counts, n_feat, alphabet and launches are a plain engine's."""
    from fastsk_amd import _native
    case = cases.definition_case()
    tok, off = _native.flatten(case["seqs"])
    out = []
    for wild in (None, [77]):
        e = make(case["g"], case["m"], path=path, wildcards=wild)
        e.compute(tok, off, len(case["seqs"]), 0)
        st = e.stats()
        out.append((e.get_counts(), st["n_feat"], st["alphabet"], st["launches"], st["max_windows"], st["key_space"]))
        e.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]
    assert out[0][2] == 6   # n and the other wildcard are letters like any other there


# ---- 2. one panel, every place ----------------------------------------------------------------------------------------------------
def check_panel(make, port, ragged_lengths, path):
    case = cases.panel_case(ragged_lengths)
    want = fold_once(port, ("panel", ragged_lengths), case)
    if not ragged_lengths:   # a hole at every position of the window trip: 43 distinct places, 21 of them twice
        assert sorted({s.index(cases.N_) for s in case["seqs"]}) == list(range(43))
    e = run(make, case, path)
    assert e.stats()["n_feat"] == expected_stats(case)[0]
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 3. the dense staging regimes ---------------------------------------------------------------------------------------------------
# (longest sequence, m at g = 12, tuning, strands) -> planned (chunked staging, sweeps > 1, window-key cache)
REGIMES = [("resident", 300, 8, {}, 1, (False, False, False)),
           ("two chunks", 1025, 8, {}, 1, (True, False, False)),
           ("tiny chunks", 300, 8, {"dense_chunk": 7}, 1, (True, False, False)),
           ("many sweeps", 1000, 5, {}, 1, (False, True, False)),
           ("many sweeps, key cache", 500, 5, {}, 1, (False, True, True)),
           ("both strands resident", 300, 8, {}, 2, (False, False, False)),
           ("both strands chunked", 1025, 8, {}, 2, (True, False, False))]


def check_regime(make, port, name, lmax, m, tun, strands, planned, scale):
    """k_dense_count<., ., ., WILD> where accumulate_dense puts it (wildcard_cases.dense_plan restates the plan and the plan is
    asserted): symbols resident, chunked staging with wildcards in the overlap rows a chunk shares with the next, a
    seven-window chunk, many histogram sweeps replaying the window-key cache, and the strand loop of reverse complement.
    path = 2: the sparse dataflow on the same sequences."""
    comp = cases.DNA if strands == 2 else None
    case = cases.regime_case(lmax, m, scale, strands=strands)
    ch, sweeps, resident, cache = cases.dense_plan(lmax, case["g"], case["keys"], False, strands, tun.get("dense_chunk", 0))
    assert (ch < lmax - case["g"] + 1, sweeps > 1, cache) == planned, (ch, sweeps, resident, cache)
    if name.endswith("chunks") and not tun:   # wildcards really sit in the overlap rows
        assert any(s[p] == cases.N_ for s in case["seqs"] if len(s) > ch + case["g"] - 2 for p in (ch - 1, ch, ch + case["g"] - 2))
    assert max(len(s) for s in case["seqs"]) == lmax
    want = fold_once(port, ("regime", lmax, m, strands, scale), case, comp)
    nfeat, maxw = expected_stats(case, comp)
    for path, t in ((1, tun), (2, {})):
        e = run(make, case, path, t, comp)
        st = e.stats()
        assert st["path_used"] == path and st["n_feat"] == nfeat and st["max_windows"] == maxw and st["key_space"] == case["keys"]
        assert np.array_equal(e.get_counts(), want), (name, path)
        e.close()


def check_rare_symbol(make, port, scale):
    """A rare real symbol r beside the wildcard n (m = 7: 5^5 keys): key compaction with the marking pass over every window
    (compact_rare asked for or not: the places-of-rare-symbols form is not taken in this mode) and without compaction."""
    case = cases.regime_case(300, 7, scale, rare=True)
    assert case["keys"] == 3125
    near = sum(1 for s in case["seqs"] for p, t in enumerate(s) if t == cases.R_ and cases.N_ in s[max(0, p - 11):p + 12])
    assert near >= 3
    want = fold_once(port, ("rare", scale), case)
    for tun, compacted in (({"compact": 1, "compact_rare": 0}, True), ({"compact": 1, "compact_rare": 1}, True), ({"compact": 0}, False)):
        e = run(make, case, 1, tun)
        st = e.stats()
        assert st["path_used"] == 1 and st["alphabet"] == 5 and (st["compact_keys_avg"] > 0) == compacted, tun
        assert np.array_equal(e.get_counts(), want), tun
        e.close()
    e = run(make, case, 2)
    assert np.array_equal(e.get_counts(), want)
    e.close()


def check_poly_a(make, port, period, length, path, scale):
    """Counts above 15 (the hi plane) and above 255 (the overflow flag, the batch recounted by the sparse dataflow) that valid
    windows alone produce: without the mode the n would cut nothing and the counts would differ."""
    case = cases.poly_a_case(period, length, scale)
    assert (case["top"] > 15, case["top"] > 255) == ((True, False) if period == 20 else (True, True))
    want = fold_once(port, ("poly", period, scale), case)
    e = run(make, case, path)
    st = e.stats()
    assert np.array_equal(e.get_counts(), want)
    if path == 1:
        assert (st["sort_records"] > 0) == (case["top"] > 255)
    e.close()


# ---- 4. sparse forms --------------------------------------------------------------------------------------------------------------
def check_sparse_forms(make, port, scale):
    case = cases.low_complexity_case(scale)
    want = fold_once(port, ("lowc", scale), case)
    digests = set()
    forms = revcomp_cases.SPARSE_FORMS + [revcomp_cases.SMALL_BLOCKS,
                                          ("pairs", {"sparse_pairs": 1}, None), ("no pairs", {"sparse_pairs": 0}, None),
                                          ("one slot a workgroup", {"extract_slots": 1}, None), ("four slots", {"extract_slots": 4}, None)]
    for name, tun, form in forms:
        e = run(make, case, 2, tun)
        st = e.stats()
        assert st["path_used"] == 2 and (form is None or st["sparse_form"] == form), name
        if "sparse_desc" in tun:
            assert st["sparse_desc"] == (1 if tun["sparse_desc"] > 0 else 0), name
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


def check_wide_windows(make, port, path, scale):
    """g x bits > 128: no window array, k_sx_extract<., ., WILD> gathers the symbols of the window its map names."""
    case = cases.wide_window_case(port, scale)
    want = fold_once(port, ("widewin", scale), case)
    e = run(make, case, path)
    st = e.stats()
    assert st["alphabet"] == 20 and st["bits_per_symbol"] == 8 and st["path_used"] == 2
    assert np.array_equal(e.get_counts(), want)
    e.close()


def check_wide_keys(make, port):
    case = cases.wide_key_case()
    want = fold_once(port, "widekey", case)
    e = run(make, case, 0)
    st = e.stats()
    assert st["alphabet"] == 65 and st["path_used"] == 2
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 5. reverse complement ----------------------------------------------------------------------------------------------------------
def check_revcomp_errors(make):
    """A wildcard listed in the complement map must have a wildcard for a complement."""
    from fastsk_amd import _native
    case = cases.definition_case()
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], wildcards=[5, 6], revcomp={1: 4, 4: 1, 2: 3, 3: 2, 5: 7, 7: 5, 6: 6})
    with pytest.raises(_native.FskError) as err:
        e.compute(tok, off, len(case["seqs"]), 0)
    assert err.value.code == -1 and "5" in str(err.value) and "wildcard" in str(err.value)
    e.set_complement({1: 4, 4: 1, 2: 3, 3: 2, 5: 6, 6: 5})   # n <-> the other wildcard: fine
    e.compute(tok, off, len(case["seqs"]), 0)
    e.close()


# ---- 6. mismatch weights ------------------------------------------------------------------------------------------------------------
def check_mismatch(make, port, path, comp, weights=None, max_mismatches=None):
    from fastsk_amd import _native
    import mismatch_cases
    case = cases.mismatch_case()
    g, m = case["g"], case["m"]
    c = weights if weights is not None else mismatch_cases.gkm_weights(g, m, max_mismatches)
    want = cases.brute_weighted(case["seqs"], set(case["wild"]), g, c, comp)
    tok, off = _native.flatten(case["seqs"])
    e = make(g, m, path=path, wildcards=case["wild"], revcomp=comp, weights=weights, max_mismatches=max_mismatches)
    e.compute(tok, off, len(case["seqs"]), 0)
    assert np.array_equal(e.get_counts(), want)
    if weights is not None and weights[0] >= 2 ** 40:
        assert int(want.max()) >= 2 ** 32
    e.close()


# ---- 7. approx modes ----------------------------------------------------------------------------------------------------------------
def check_skip_variance(make, port, emu_lib_or_native, path):
    """approx + skip_variance, t = 3, seed: the fold over exactly the combos the seeded order draws."""
    from fastsk_amd import _native
    case = dict(cases.definition_case())
    g, m = case["g"], case["m"]
    tok, off = _native.flatten(case["seqs"])
    e = make(g, m, t=3, approx=True, skip_variance=True, max_iters=2, path=path, wildcards=case["wild"])
    e.set_seed(7)
    e.compute(tok, off, len(case["seqs"]), 0)
    done = int(e.stats()["combos_done"])
    order = emu_lib_or_native.seed_order(7, port.num_combos(g, m))
    assert 0 < done <= 6
    case["combos"] = np.sort(order[:done])
    want = cases.fragment_fold(port, case["seqs"], set(case["wild"]), g, m, case["combos"])
    assert np.array_equal(e.get_counts(), want)
    e.close()


def check_variance_padding(make, port, lib, path):
    """Variance mode, t = 1, seeded: sequences padded with 0 .. 15 n at either end give the triangle and the stdevs of the
    trimmed sequences, bit for bit — the oracle's own approx mode on the trimmed ones with the same order."""
    from fastsk_amd import _native
    from oracle import loader
    case = cases.padded_case()
    g, m, n = case["g"], case["m"], len(case["seqs"])
    order = lib.seed_order(11, port.num_combos(g, m))
    tok0, off0 = loader.flatten(case["core"])
    tri, sds, _ = port.compute(tok0, off0, n, 0, g, m, t=1, approx=True, max_iters=12, order=order)
    tok, off = _native.flatten(case["seqs"])
    e = make(g, m, t=1, approx=True, max_iters=12, path=path, wildcards=case["wild"])
    e.set_seed(11)
    e.compute(tok, off, n, 0)
    assert np.array_equal(e.get_triangle(), tri)
    assert np.array_equal(np.asarray(e.get_stdevs()), np.asarray(sds)[:len(e.get_stdevs())]) and len(e.get_stdevs()) == len(sds)
    e.close()


def check_padding_exact(make, port, path, comp=None):
    """The padding consequence in exact mode (with and without reverse complement): the plain kernel of the trimmed ones."""
    from fastsk_amd import _native
    case = cases.padded_case()
    g, m, n = case["g"], case["m"], len(case["seqs"])
    outs = []
    for seqs, wild in ((case["core"], None), (case["seqs"], case["wild"])):
        tok, off = _native.flatten(seqs)
        e = make(g, m, path=path, wildcards=wild, revcomp=comp)
        e.compute(tok, off, n, 0)
        outs.append((e.get_counts(), e.stats()["n_feat"], e.stats()["max_windows"]))
        e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


# ---- 8. staged calls and state ------------------------------------------------------------------------------------------------------
def check_staged(make, port, path, scale):
    """load + accumulate in two calls, a row band, reset_counts, the handle reused at another N, the set switched on -> off -> on."""
    from fastsk_amd import _native
    case = cases.regime_case(150, 8, scale)
    n = len(case["seqs"])
    want = fold_once(port, ("staged", scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], path=path, wildcards=case["wild"])
    e.load_sequences(tok, off, n, 0)
    e.accumulate(case["combos"][:1])
    e.accumulate(case["combos"][1:])
    e.finalize()
    assert np.array_equal(e.get_counts(), want)
    e.reset_counts()
    lo, hi = (128, 256) if n >= 256 else (0, min(n, 128))
    e.accumulate_rows(case["combos"], lo, hi)
    e.synchronize()
    band = e.get_counts()
    a, _ = np.tril_indices(n)
    inside = (a >= lo) & (a < hi)
    assert np.array_equal(band[inside], want[inside]) and not band[~inside].any()
    # another N on the same handle, the set off (n is then a letter: the plain oracle), and on again
    small = {"seqs": case["seqs"][:n // 2 + 1], "g": case["g"], "m": case["m"], "wild": case["wild"], "combos": case["combos"]}
    tok2, off2 = _native.flatten(small["seqs"])
    e.set_wildcards(None)
    e.load_sequences(tok2, off2, len(small["seqs"]), 0)
    e.accumulate(case["combos"])
    e.finalize()
    plain, _, _ = port.raw_counts(tok2, off2, case["g"], case["m"], case["combos"], threads=cases.THREADS)
    assert e.stats()["alphabet"] == 5 and np.array_equal(e.get_counts(), plain)
    e.set_wildcards(case["wild"])
    e.load_sequences(tok2, off2, len(small["seqs"]), 0)
    e.accumulate(case["combos"])
    e.finalize()
    want2 = cases.fragment_fold(port, small["seqs"], set(case["wild"]), case["g"], case["m"], case["combos"])
    assert e.stats()["alphabet"] == 4 and np.array_equal(e.get_counts(), want2)
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
    """A group handle (devices=[0, 0], the P2P collective) sets the wildcards on every engine: the single engine's triangle."""
    from fastsk_amd import _native
    case = cases.regime_case(150, 8, scale)
    n = len(case["seqs"])
    want = fold_once(port, ("staged", scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], devices=[0, 0], collective=_native.COLL_P2P, wildcards=case["wild"])
    e.load_sequences(tok, off, n, 0)
    e.accumulate(case["combos"])
    e.finalize()
    assert e.multi_info()["ndev"] == 2 and np.array_equal(e.get_counts(), want)
    e.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------
def check_errors(make, port):
    from fastsk_amd import _native
    g, m = 5, 2
    good = [[1, 2, 3, 4, 1, 2, 3], [2, 2, 3, 1, 4, 4, 1, 2]]
    only = [5] * 9                                 # nothing but wildcards
    every = [1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2]   # length >= g, every window holds one
    e = make(g, m, wildcards=[5])
    for bad in (only, every):
        tok, off = _native.flatten(good + [bad] + good)
        with pytest.raises(_native.FskError) as err:
            e.compute(tok, off, 5, 0)
        assert err.value.code == -2 and "sequence 2 " in str(err.value) and "wildcard" in str(err.value)
        tok, off = _native.flatten(good + good)   # the handle stays usable
        e.compute(tok, off, 4, 0)
        assert np.array_equal(e.get_counts(), port.raw_counts(tok, off, g, m, np.arange(10, dtype=np.int32))[0])
    with pytest.raises(_native.FskError) as err:
        e.set_wildcard_array(np.array([5, 6, 5], dtype=np.int32))
    assert err.value.code == -1 and "twice" in str(err.value)
    assert e.lib.L.fsk_set_wildcards(e.h, None, 2) == -1 and e.lib.L.fsk_set_wildcards(e.h, None, -1) == -1
    # n = 0 switches the mode off: the sequence of wildcards alone is then an ordinary one
    e.set_wildcard_array(np.zeros(0, dtype=np.int32))
    tok, off = _native.flatten(good + [only])
    e.compute(tok, off, 3, 0)
    assert e.stats()["wildcards"] == [] and np.array_equal(e.get_counts(), port.raw_counts(tok, off, g, m, np.arange(10, dtype=np.int32))[0])
    e.close()


# ---- 10. real data ------------------------------------------------------------------------------------------------------------------------
def load_wildcard_golden():
    z = np.load(os.path.join(GOLD, "wildcards_ep47848_60.npz"))
    return {k: z[k] for k in z.files}


def check_golden(make, path):
    """60 rows of EP300_47848 (the five that hold n among them), g = 10, m = 6: the fragment fold of the compiled reference."""
    d = load_wildcard_golden()
    g, m, n = int(d["g"]), int(d["m"]), len(d["offsets"]) - 1
    e = make(g, m, path=path, wildcards=[int(d["wildcard"])])
    e.compute(d["tokens"], d["offsets"], int(d["n_train"]), n - int(d["n_train"]))
    st = e.stats()
    assert st["alphabet"] == 4 and st["n_feat"] == int(d["n_feat"])
    assert np.array_equal(e.get_counts(), d["counts"])
    assert np.array_equal(e.get_triangle(), d["tri"])
    e.close()


# =============================================================================================================================
# the emulator's share
# =============================================================================================================================
@pytest.mark.parametrize("comp", [None, cases.DNA, cases.DNA_N], ids=["one strand", "revcomp", "revcomp, n listed"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_definition(make, port, path, comp):
    check_definition(make, port, path, comp)


@pytest.mark.parametrize("path", [1, 2])
def test_absent_wildcard_changes_nothing(make, port, path):
    check_absent_wildcard(make, port, path)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("ragged_lengths", [False, True])
def test_one_panel_every_place(make, port, ragged_lengths, path):
    check_panel(make, port, ragged_lengths, path)


@pytest.mark.parametrize("name,lmax,m,tun,strands,planned", REGIMES, ids=[r[0] for r in REGIMES])
def test_dense_regimes(make, port, name, lmax, m, tun, strands, planned):
    check_regime(make, port, name, lmax, m, tun, strands, planned, SCALE)


def test_rare_symbol_beside_the_wildcard(make, port):
    check_rare_symbol(make, port, SCALE)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("period,length", [(20, 200), (300, 900)])
def test_poly_a_cut_by_wildcards(make, port, period, length, path):
    check_poly_a(make, port, period, length, path, SCALE)


def test_sparse_forms(make, port):
    check_sparse_forms(make, port, 0.1)


def test_shared_prefix_batches(make, port):
    check_shared_prefix(make, port, 0.1)


@pytest.mark.parametrize("path", [0, 2])
def test_windows_wider_than_128_bits(make, port, path):
    check_wide_windows(make, port, path, 0.1)


def test_keys_beyond_62_bits(make, port):
    check_wide_keys(make, port)


def test_wildcard_in_the_complement_map(make):
    check_revcomp_errors(make)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("comp", [None, cases.DNA], ids=["one strand", "revcomp"])
def test_mismatch_weights(make, port, path, comp):
    check_mismatch(make, port, path, comp, max_mismatches=2)


def test_mismatch_weights_beyond_32_bits(make, port):
    check_mismatch(make, port, 0, None, weights=[2 ** 40, 1, 0, 0])


@pytest.mark.parametrize("path", [1, 2])
def test_skip_variance(make, port, emu_lib, path):
    check_skip_variance(make, port, emu_lib, path)


@pytest.mark.parametrize("path", [1, 2])
def test_variance_mode_on_padded_sequences(make, port, emu_lib, path):
    check_variance_padding(make, port, emu_lib, path)


@pytest.mark.parametrize("comp", [None, cases.DNA_N], ids=["one strand", "revcomp"])
@pytest.mark.parametrize("path", [1, 2])
def test_padding_is_the_trimmed_kernel(make, port, path, comp):
    check_padding_exact(make, port, path, comp)


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


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(make, path):
    check_golden(make, path)
