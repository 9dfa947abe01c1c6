"""The front end of the sparse dataflow (path=2) at the edges of its digits, tiles and record types: the record extraction and
its first-digit histogram, the LSD radix sort (k_sx_hist, k_sx_scan_slot, k_sx_scatter<RecT, NB>, sx_sort) and the segment kernels
(k_sx_seg_count, k_sx_seg_scan, k_sx_seg_write). tests/sort_edges_cases.py holds the cases, the restated plan and the numpy
reference; the check functions here state the contract and tests/test_gpu_sort_edges.py runs them at the same sizes on the
device. ``make(g, m, **kw)`` creates an engine; no expected value comes from an engine.

The contract: get_counts() equals counts_by_definition_wide bit for bit in every case (under skip_test_block: the diagonal and
every cell with a train column exact, test x test cells off the diagonal zero); the stats show the sparse dataflow, the planned
``n_feat``, ``sort_passes``, ``key_space`` and slots x nfeat ``sort_records`` an accumulate, and the forced ``sparse_form`` /
``sparse_desc`` / ``share_positions``. Before a check calls the engine it asserts from the plan and the reference alone that its
case is where it is meant to be (digit widths, record bytes, tiles, the segment-tile feature of group H): a case that drifts off
its edge fails.

Groups (sort_edges_cases.py): A digit widths in 32-bit records, B in 64-bit records, C 128-bit records with bit-field keys, D
mixed-radix keys, E either side of 32 | 33 and 64 | 65 record bits, F tile tails and slot alignment, G buckets across tiles with
every update form, H segment-tile edges, I shared leading positions across the presort's record width.

On the emulator groups A and B are thinned (every digit width 1..8 and every pass count 1..8 stay); the device file runs the
whole sweeps."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, set_tuning_env

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sort_edges_cases as cases  # noqa: E402


# ---- the checks, shared with tests/test_gpu_sort_edges.py -------------------------------------------------------------------
def run(make, monkeypatch, c, tuning=None, form=None, desc=None, share=None, skip=False, triangle=None, port=None):
    """One engine over the case: load, one accumulate of the case's combinations, finalize -> the stats asserted against the
    plan, the counts against the reference (``skip``: the contract of skip_test_block). ``triangle``: get_triangle() against
    the oracle's normalisation of the reference as well."""
    from fastsk_amd import _native
    plan, N, nfeat, ntr = c["plan"], c["N"], c["nfeat"], c["n_train"]
    if tuning:
        set_tuning_env(monkeypatch, **tuning)
    tok, off = _native.flatten(c["X"])
    e = make(c["g"], c["m"], path=2, skip_test_block=skip)
    e.load_sequences(tok, off, ntr, N - ntr)
    before = e.stats()
    e.accumulate(c["combos"])
    e.finalize()
    st = e.stats()
    got = e.get_counts()
    tri = e.get_triangle() if triangle else None
    e.close()
    print("sigma=%d k=%d g=%d N=%d nfeat=%d: keybits %d + sb %d = %d record bits (%d bytes), passes %s, tps %d tpg %d, win_words %d; "
          "stats: sort_passes %d form %d desc %d share %d" % (c["sigma"], c["k"], c["g"], N, nfeat, plan["keybits"], plan["sb"], plan["recbits"],
                                                             plan["rec_bytes"], plan["widths"], plan["tps"], plan["tpg"], plan["win_words"],
                                                             st["sort_passes"], st["sparse_form"], st["sparse_desc"], st["share_positions"]))
    assert st["path_used"] == 2
    assert st["n_feat"] == nfeat and st["n_seq"] == N
    assert st["key_space"] == plan["V"] or plan["V"] >= 1 << 62   # (from 2^62 on the stat says "at least": no number to pin)
    assert st["alphabet"] == c["sigma"] and st["bits_per_symbol"] == plan["bits"]
    assert st["sort_records"] - before["sort_records"] == len(c["combos"]) * nfeat
    if share is None:
        assert st["sort_passes"] == plan["passes"]
        assert len(c["combos"]) <= 16 or st["share_positions"] == 0
    else:
        assert st["share_positions"] == share
        assert st["sort_passes"] == (c["k"] - share + 7) // 8   # (sigma = 2: a kept position is a key bit)
    assert form is None or st["sparse_form"] == form, st["sparse_form"]
    assert desc is None or st["sparse_desc"] == desc, st["sparse_desc"]
    want = c["want"]
    a, b = np.tril_indices(N)
    keep = (b < ntr) | (a == b) if skip else np.ones(len(want), dtype=bool)
    bad = np.flatnonzero((got != want) & keep)
    assert bad.size == 0, "%d cells differ, the first at %d: %d against %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]])
    if skip and N - ntr >= 2:   # (test x test cells off the diagonal exist: left at zero, their updates never issued)
        assert not got[~keep].any() and want[~keep].any()
        assert st["cell_updates"] - before["cell_updates"] < c["U"]
    else:
        assert st["cell_updates"] - before["cell_updates"] == c["U"]
    if triangle:
        assert np.array_equal(tri, port.normalise(want.astype(np.float64), N))
    return st


def shares_kmers(c):
    """At least one off-diagonal cell of the reference is non-zero: rows share k-mers, the update stage has pairs to emit."""
    a, b = np.tril_indices(c["N"])
    assert c["want"][a != b].any(), "no off-diagonal cell"


def check_widths(make, monkeypatch, port, c, rec_bytes, passes, triangle=False, win_words=None):
    """Groups A to E: the plan is the one the case is for, then the engine."""
    plan = c["plan"]
    assert plan["rec_bytes"] == rec_bytes and plan["passes"] == passes, (plan["recbits"], plan["widths"])
    assert win_words is None or plan["win_words"] == win_words
    shares_kmers(c)
    run(make, monkeypatch, c, triangle=triangle, port=port)


def check_a(make, monkeypatch, port, k):
    c = cases.group_a(k)
    plan = c["plan"]
    assert plan["keybits"] == k and plan["sb"] == 2 and plan["tps"] == 5 and plan["tpg"] == 9
    assert c["nfeat"] % cases.SX_TILE == 1 and c["nfeat"] % cases.SG_TILE == 1   # (one record in the last tile of either kind)
    assert plan["widths"] == cases.pass_widths(k) and sum(plan["widths"]) == k and max(plan["widths"]) - min(plan["widths"]) <= 1
    assert plan["small"] == (k <= 24)
    check_widths(make, monkeypatch, port, c, 4, (k + 7) // 8, triangle=True, win_words=2 if k <= 31 else 4)


def check_b(make, monkeypatch, port, k, m=1):
    c = cases.group_b(k, m)
    plan = c["plan"]
    assert plan["keybits"] == k and plan["recbits"] == k + 2 and plan["tps"] == 2 and not plan["symbits"]
    check_widths(make, monkeypatch, port, c, 8, (k + 7) // 8, win_words=0 if (k + m) * 2 > 128 else 4 if (k + m) * 2 > 64 else 2)


def check_c(make, monkeypatch, port, sigma, k):
    c = cases.group_c(sigma, k)
    plan = c["plan"]
    want = {(20, 15): (5, 75, 10, 4), (20, 19): (5, 95, 12, 0), (65, 13): (7, 91, 12, 4)}[sigma, k]
    assert (plan["symbits"], plan["keybits"], plan["passes"], plan["win_words"]) == want and plan["keybits"] <= 96 and plan["V"] == 1 << 62
    check_widths(make, monkeypatch, port, c, 16, want[2])


def check_d(make, monkeypatch, port, sigma, k):
    c = cases.group_d(sigma, k)
    plan = c["plan"]
    want = {(3, 5): [8], (3, 6): [5, 5], (5, 7): [6, 6, 5], (20, 4): [6, 6, 6], (20, 6): [7, 7, 6, 6]}[sigma, k]
    assert plan["widths"] == want and plan["V"] == sigma ** k and not plan["symbits"] and plan["sb"] == 6
    assert plan["small"] == ((sigma, k) != (20, 6))   # (20^6 > 2^24: beyond the 24-bit fast path, still 32-bit records)
    check_widths(make, monkeypatch, port, c, 4, len(want))


def check_e(make, monkeypatch, port, sigma, k, N, nfeat):
    c = cases.group_e(sigma, k, N, nfeat)
    plan = c["plan"]
    keybits = {2: 24, 4: 56}[sigma]
    assert plan["keybits"] == keybits and plan["sb"] == (8 if N <= 256 else 9) and plan["recbits"] == keybits + plan["sb"]
    assert plan["recbits"] == {(2, 255): 32, (2, 256): 32, (2, 257): 33, (4, 255): 64, (4, 256): 64, (4, 257): 65}[sigma, N]
    # (N = 256, 257: sequence 255 and 256 — the highest bit of the id field set, at bit 7 and bit 8 of the record)
    rec_bytes = {32: 4, 33: 8, 64: 8, 65: 16}[plan["recbits"]]
    check_widths(make, monkeypatch, port, c, rec_bytes, (keybits + 7) // 8, triangle=True)


def check_f(make, monkeypatch, port, N, nfeat, extract_slots):
    """Four slots of u32 records, two passes: the tails of the sort and segment tiles, the alignment of a slot's first record."""
    c = cases.group_f(N, nfeat)
    plan = c["plan"]
    assert plan["rec_bytes"] == 4 and plan["widths"] == [6, 6] and len(c["combos"]) == 4 and plan["win_words"] == 2
    assert plan["tps"] == (nfeat + 4095) // 4096 and plan["tpg"] == (nfeat + 2047) // 2048
    if nfeat >= cases.SX_TILE:   # (the 16-byte path of k_sx_hist: nfeat mod 4 over four slots gives these heads)
        assert cases.hist_heads(nfeat, 4) == {0: {0}, 1: {0, 1, 2, 3}, 2: {0, 2}, 3: {0, 1, 2, 3}}[nfeat % 4]
    if N > 1:
        shares_kmers(c)
    run(make, monkeypatch, c, tuning={"extract_slots": extract_slots})


def check_g(make, monkeypatch, port, form, skip):
    """Few keys, multiplicities in the hundreds: a digit bucket spans several sort tiles and all four waves of a tile, an entry
    many records; stable passes keep a key's sequences in order across them."""
    c = cases.group_g()
    plan = c["plan"]
    tuning, sform, sdesc = cases.FORMS[form]
    assert plan["widths"] == [5, 4] and plan["rec_bytes"] == 4 and plan["tps"] >= 3 and c["top"] > 255
    for combo in c["combos"]:   # (few keys; in both passes a digit's records come from three source tiles and more, and from
        keys = cases.slot_keys(c["X"], c["g"], combo, c["m"])   # all four waves of one of them)
        assert len(np.unique(keys)) < 100
        assert all(tiles >= 3 and quarters for tiles, quarters in cases.digit_spread(keys, plan["widths"]))
    st = run(make, monkeypatch, c, tuning=tuning, form=sform, desc=sdesc, skip=skip, triangle=not skip, port=port)
    assert st["max_windows"] > 255


def check_h_homopolymers(make, monkeypatch, port, n_train, form, skip):
    """One entry of 5000 records spans three segment tiles: a tile with no entry, a tile with entries and no run head."""
    c = cases.group_h_homopolymers(n_train)
    tuning, sform, sdesc = cases.FORMS[form]
    assert skip is False or n_train < c["N"]
    rec, sb = cases.sorted_records(c["X"], c["g"], 0, c["m"])
    tiles = cases.segment_tiles(rec, sb, n_train if skip else None)
    assert len(tiles) == c["plan"]["tpg"] == 6
    assert tiles[0][:2] == (1, 0) and tiles[1][0] == 0 and tiles[4][0] == 0     # (lrh == 0; no entry at all)
    assert tiles[2][0] > 0 and tiles[2][1] == -1 and tiles[3][0] > 0 and tiles[3][1] == -1   # (entries, no run head)
    if skip and n_train == 1:
        assert tiles[2][2] == 0   # (sequence 1, the first test entry of run 0, is tile 2's first entry)
    run(make, monkeypatch, c, tuning=tuning, form=sform, desc=sdesc, skip=skip)


def k1_preconditions(c):
    """The feature a case of group H (ii) was built for, from the reference's own sorted records of combination 0."""
    spec, ntr = c["spec"], c["n_train"]
    rec, sb = cases.sorted_records(c["X"], c["g"], 0, c["m"])
    tiles = cases.segment_tiles(rec, sb, ntr)
    key, seq = rec >> sb, rec & ((1 << sb) - 1)
    if "head_at" in spec:
        j = spec["head_at"]
        assert key[j] != key[j - 1] and (key[:j] == key[0]).all()
        if j == 2047:   # (the last record of tile 0 is its last entry and heads a run)
            assert tiles[0][1] == tiles[0][0] - 1
        if j == 2049:   # (record 2048 continues an entry of tile 0: the run head is tile 1's first entry)
            assert rec[2048] == rec[2047]
    if "test_at" in spec:
        j = spec["test_at"]
        assert key[j] == key[0] and seq[j] >= ntr and seq[j - 1] < ntr
        if j == 2047:
            assert tiles[0][2] == tiles[0][0] - 1
    if "tile" in spec:
        t = tiles[spec["tile"]]
        assert t[0] > 0
        assert "lrh" not in spec or t[1] == spec["lrh"]
        assert "lth" not in spec or t[2] == spec["lth"]


def check_h_k1(make, monkeypatch, port, name, skip):
    """k = 1 over two symbols: the sorted slot of combination 0 is the windows that start with 1, by sequence, then those that
    start with 2 — a run head or a test head is put on a chosen record."""
    c = cases.group_h_k1(name)
    k1_preconditions(c)
    run(make, monkeypatch, c, skip=skip)


def check_i(make, monkeypatch, port, share):
    """25 slots in one batch sort their first ``share`` kept positions once per group: presort records (top << wb) | window of
    share + 14 bits — 32 at share = 18 (u32 records), 33 at 19 (u64)."""
    c = cases.group_i()
    plan = c["plan"]
    wb = max(cases.bits_below(c["nfeat"]), 1)
    assert wb == 14 and share + wb == {18: 32, 19: 33}[share] and plan["rec_bytes"] == 4 and plan["win_words"] == 2 and len(c["combos"]) == 25 > 16
    shares_kmers(c)
    run(make, monkeypatch, c, tuning={"sparse_share": share}, share=share)


# ---- the yardsticks themselves ---------------------------------------------------------------------------------------------
REFERENCE_CASES = {"A": lambda: cases.group_a(11), "B": lambda: cases.group_b(33), "C": lambda: cases.group_c(20, 15),
                   "D": lambda: cases.group_d(5, 7), "E": lambda: cases.group_e(2, 24, 257, 8195), "F": lambda: cases.group_f(16, 4097),
                   "G": cases.group_g, "H1": lambda: cases.group_h_homopolymers(3), "H2": lambda: cases.group_h_k1("test_head_2048"),
                   "I": cases.group_i}


@pytest.mark.parametrize("group", sorted(REFERENCE_CASES))
def test_reference_is_the_oracle(port, group):
    """counts_by_definition_wide against ``port.raw_counts``, one combination at a time, on one case of every group: two
    references agree before an engine is asked."""
    c = REFERENCE_CASES[group]()
    cases.check_reference(port, dict(c, combos=c["combos"][:3]))


def test_sort_plan_table():
    """The restated plan at the shapes the groups name."""
    p = cases.sort_plan
    assert cases.pass_widths(19) == [7, 6, 6] and cases.pass_widths(17) == [6, 6, 5] and cases.pass_widths(62) == [8, 8, 8, 8, 8, 8, 7, 7]
    assert [len(cases.pass_widths(b)) for b in (8, 9, 16, 17, 24, 25, 30, 56)] == [1, 2, 2, 3, 3, 4, 4, 7]
    # every digit width 1..8 and every NB 4..8 over group A alone
    assert {w for k in cases.A_KS for w in cases.pass_widths(k)} == set(range(1, 9))
    assert {nb for k in cases.A_KS for nb in p(2, k, k + 1, 4, 16385)["NB"]} == {4, 5, 6, 7, 8}
    assert {len(cases.pass_widths(b)) for b in cases.A_KS + cases.B_KS + [75, 95, 91]} == set(range(1, 9)) | {10, 12}
    assert p(2, 30, 31, 4, 16385)["recbits"] == 32 and p(2, 31, 32, 4, 4097)["rec_bytes"] == 8 and p(2, 62, 63, 4, 4097)["recbits"] == 64
    assert p(2, 62, 63, 4, 4097)["V"] == 1 << 62 and not p(2, 62, 63, 4, 4097)["symbits"]
    assert p(20, 15, 16, 40, 4097)["symbits"] == 5 and p(65, 13, 14, 40, 4097)["keybits"] == 91
    assert p(20, 6, 7, 64, 8193)["keybits"] == 26 and p(20, 6, 7, 64, 8193)["recbits"] == 32
    assert [p(2, 12, 13, 16, n)["tps"] for n in (16, 4096, 4097, 8192, 8193, 12289, 16384, 16385)] == [1, 1, 2, 2, 3, 4, 4, 5]
    assert p(2, 1, 2, 1, 1)["sb"] == 1 and p(2, 1, 2, 2, 2)["sb"] == 1 and p(2, 1, 2, 256, 300)["sb"] == 8 and p(2, 1, 2, 257, 300)["sb"] == 9
    assert set().union(*(cases.hist_heads(n, 4) for n in (8193, 8194, 8195))) == {0, 1, 2, 3}


def test_segment_tiles_by_hand():
    """Three records a key of two sequences, 2048 + 3 records: counted by hand."""
    sb = 2
    rec = np.array([(0 << sb) | 0] * 2046 + [(0 << sb) | 1, (1 << sb) | 0] + [(1 << sb) | 0, (1 << sb) | 2, (2 << sb) | 2], dtype=np.int64)
    assert cases.segment_tiles(rec, sb) == [(3, 2, -1), (2, 1, -1)]          # tile 0: entries at 0, 2046, 2047 (a run head)
    assert cases.segment_tiles(rec, sb, 1) == [(3, 2, 1), (2, 1, 1)]         # test heads: 2046; 2049 and 2050 (a run of its own)
    assert cases.segment_tiles(rec, sb, 2) == [(3, 2, -1), (2, 1, 1)]
    assert cases.segment_tiles(np.zeros(5000, dtype=np.int64), sb) == [(1, 0, -1), (0, -1, -1), (0, -1, -1)]


def test_a_case_off_its_edge_fails_at_the_precondition():
    """One window fewer among the ones and the run head of ``run_head_2048`` is no longer tile 1's first record; one more among
    the train sequences and the test head of ``test_head_2048`` is not: the precondition fails before any engine is asked."""
    c = cases.group_h_k1("run_head_2048")
    k1_preconditions(c)
    with pytest.raises(AssertionError):
        k1_preconditions(dict(c, X=cases.k1_sequences([1000, 700, 347, 0, 0], c["spec"]["twos"])))
    c = cases.group_h_k1("test_head_2048")
    with pytest.raises(AssertionError):
        k1_preconditions(dict(c, X=cases.k1_sequences([1000, 1049, 500, 200, 1500], c["spec"]["twos"])))


# ---- the emulator runs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


# (thinned for time: digit widths 1..8 in one pass, then both sides of every pass count and the 32-bit record's top bit)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 24, 25, 30])
def test_widths_in_32_bit_records(make_emu, monkeypatch, port, k):
    check_a(make_emu, monkeypatch, port, k)


@pytest.mark.parametrize("k,m", [(31, 1), (33, 1), (41, 1), (49, 1), (57, 1), (62, 1), (62, 3)])
def test_widths_in_64_bit_records(make_emu, monkeypatch, port, k, m):
    check_b(make_emu, monkeypatch, port, k, m)


@pytest.mark.parametrize("sigma,k", cases.C_CASES)
def test_widths_in_128_bit_records(make_emu, monkeypatch, port, sigma, k):
    check_c(make_emu, monkeypatch, port, sigma, k)


@pytest.mark.parametrize("sigma,k", cases.D_CASES)
def test_mixed_radix_keys(make_emu, monkeypatch, port, sigma, k):
    check_d(make_emu, monkeypatch, port, sigma, k)


@pytest.mark.parametrize("sigma,k,N,nfeat", cases.E_CASES)
def test_record_type_boundaries(make_emu, monkeypatch, port, sigma, k, N, nfeat):
    check_e(make_emu, monkeypatch, port, sigma, k, N, nfeat)


@pytest.mark.parametrize("extract_slots", [1, 4])
@pytest.mark.parametrize("N,nfeat", [(16, n) for n in cases.F_NFEAT] + [(1, 1), (1, 2)])
def test_tile_tails_and_slot_alignment(make_emu, monkeypatch, port, N, nfeat, extract_slots):
    check_f(make_emu, monkeypatch, port, N, nfeat, extract_slots)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip_test_block"])
@pytest.mark.parametrize("form", sorted(cases.FORMS))
def test_buckets_across_tiles(make_emu, monkeypatch, port, form, skip):
    check_g(make_emu, monkeypatch, port, form, skip)


H1_CASES = [(n, f, s) for n in cases.H1_TRAIN for f in ("default", "desc", "blocks", "atomics") for s in ((False, True) if n < 6 else (False,))]


@pytest.mark.parametrize("n_train,form,skip", H1_CASES)
def test_entry_across_three_segment_tiles(make_emu, monkeypatch, port, n_train, form, skip):
    check_h_homopolymers(make_emu, monkeypatch, port, n_train, form, skip)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip_test_block"])
@pytest.mark.parametrize("name", sorted(cases.K1_CASES))
def test_heads_on_segment_tile_edges(make_emu, monkeypatch, port, name, skip):
    check_h_k1(make_emu, monkeypatch, port, name, skip)


@pytest.mark.parametrize("share", [18, 19])
def test_shared_positions_across_presort_width(make_emu, monkeypatch, port, share):
    check_i(make_emu, monkeypatch, port, share)
