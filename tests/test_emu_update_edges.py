"""The update stage of the sparse dataflow (path=2) at the edges of its slots, bands, parts and sub-bands: k_sx_seg_write's
classes, k_sx_ucol_*, k_sx_emit, k_sx_parts, k_sx_consume with sx_expand_descriptors, the by-slot stores of variance mode and
k_sxb_count / scan / scatter / drecords / consume. tests/update_edges_cases.py holds the inputs, the restated plan and the model;
the check functions here state the contract and tests/test_gpu_update_edges.py runs them at the same sizes on the device.
``make(g, m, **kw)`` creates an engine; no expected value comes from an engine.

The contract: get_counts() equals the reference cell for cell over the whole triangle and stats()["cell_updates"] equals U (under
skip_test_block: the diagonal and every cell with a train column exact, test x test cells off the diagonal zero, fewer updates);
stats()["sparse_form"] / ["sparse_desc"] / ["sparse_passes"] are what the restated plan says. Variance mode (group F): the
triangle and the stdevs equal port.compute(..., approx=True) bit for bit. No tolerance anywhere.

Before a check asks the engine it asserts FROM THE MODEL that the case sits on the edge it is named after — an entry of exactly
48 partners, a tile of exactly 11,800 short words, a part whose first word lies at a given residue —: a case that drifts off its
edge fails at that assertion. The model is never compared with an engine.

Groups: A band plan boundaries, B entry classes of k_sx_emit, C slot capacity, D runs across tile edges, E parts and streams of
k_sx_consume and its descriptors, F by-slot stores, G two-level blocks.

Size rule of this file (the emulator runs a workgroup's threads one after the other): a case of group A with N >= 4095 runs on
the device only — ``EMU_MAX_N``; every other case of every group runs here in full."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, set_tuning_env

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sort_edges_cases as sec  # noqa: E402
import update_edges_cases as cases  # noqa: E402
from update_edges_cases import EM_CAP, EM_SLOTS, SX_SHORT, tri  # noqa: E402

EMU_MAX_N = 4094   # group A only: the largest N the emulator file runs

# the update forms: (name in sort_edges_cases.FORMS, sparse_pairs, skip_test_block). sparse_pairs only changes the owner bands.
VARIANTS = [(f, p, s) for f in ("default", "desc", "nodesc") for p in (1, 0) for s in (False, True)] + \
           [(f, 1, s) for f in ("blocks", "atomics") for s in (False, True)]


def vid(v):
    return "%s-pairs%d-%s" % (v[0], v[1], "skip" if v[2] else "whole")


def tuning_of(variant, **more):
    """The variant's tuning. Descriptors are cut into about 64 parts unless a check says otherwise: the default, 2048 workgroups of
    1024 threads a batch, is two seconds a test on the emulator (test_entry_classes_descriptor_threshold keeps the default)."""
    tun = dict(sec.FORMS[variant[0]][0], sparse_pairs=variant[1], **more)
    if variant[0] == "desc":
        tun.setdefault("sparse_desc_parts", 64)
    return tun


def model_of(c, variant, **more):
    """The model of the case under the variant's tuning: the owner bands — or, for the blocks form, the first pass."""
    tun = tuning_of(variant, **more)
    skip, ntr = variant[2], c["n_train"]
    if variant[0] == "blocks":
        first = cases.blocks_pass_plan(c["N"], 0, c["N"], tun)
        assert first is not None
        return cases.update_model(c["X"], ntr, skip, tun, bands=first)
    if variant[0] == "atomics":   # (k_sx_emit<DIRECT>: no pairs, no descriptors; short and long entries as in the bands)
        tun = dict(tun, sparse_pairs=0)
    return cases.update_model(c["X"], ntr, skip, tun)


# ---- the checks, shared with tests/test_gpu_update_edges.py -------------------------------------------------------------------
def run(make, monkeypatch, c, variant, form=None, desc=None, passes=None, **more):
    """One engine over the case under the variant: load, one accumulate, finalize -> the stats against the plan, the counts
    against the reference cell for cell, U (the contract of skip_test_block under ``skip``)."""
    from fastsk_amd import _native
    fname, pairs, skip = variant
    tun = tuning_of(variant, **more)
    set_tuning_env(monkeypatch, **tun)
    N, ntr = c["N"], c["n_train"]
    tok, off = _native.flatten(c["X"])
    e = make(c["g"], c["m"], path=2, skip_test_block=skip)
    e.load_sequences(tok, off, ntr, N - ntr)
    e.accumulate(c["combos"])
    e.finalize()
    st = e.stats()
    got = e.get_counts()
    e.close()
    print("N=%d %s: form %d desc %d passes %d updates %d (U %d)" % (N, vid(variant), st["sparse_form"], st["sparse_desc"], st["sparse_passes"],
                                                                  st["cell_updates"], c["U"]))
    assert st["path_used"] == 2 and st["n_seq"] == N and st["max_windows"] == c["top"]
    want_form = sec.FORMS[fname][1] if form is None else form
    if "sparse_form" in more or fname != "default":
        assert st["sparse_form"] == cases.choose_form(cases.band_plan(N, pairs), tun, desc_now=tun.get("sparse_desc", 0) == 1)
    assert st["sparse_form"] == want_form, st["sparse_form"]
    want_desc = sec.FORMS[fname][2] if desc is None else desc
    assert want_desc is None or st["sparse_desc"] == want_desc, st["sparse_desc"]
    assert passes is None or st["sparse_passes"] == passes, st["sparse_passes"]
    want = c["want"]
    a, b = np.tril_indices(N)
    keep = (b < ntr) | (a == b) if skip else np.ones(len(want), dtype=bool)
    bad = np.flatnonzero((got != want) & keep)
    assert bad.size == 0, "%d cells differ, the first at %d (row %d, column %d): %d against %d" % (bad.size, bad[0], a[bad[0]], b[bad[0]],
                                                                                                got[bad[0]], want[bad[0]])
    if skip and N - ntr >= 2:
        assert not got[~keep].any() and want[~keep].any()
        if "U_skip" not in c:   # (by definition from the windows, once a case)
            c["U_skip"] = cases.updates_by_definition(c["X"], ntr, c["g"], c["m"], c["combos"])
        assert st["cell_updates"] == c["U_skip"] < c["U"]
    else:
        assert st["cell_updates"] == c["U"]
    return st


def model_updates(c, model, skip):
    """The model's own U against the reference's (under skip: against the definition's count for the kept cells)."""
    if "ra" not in model["bands"]:
        assert model["U"] == (cases.updates_by_definition(c["X"], c["n_train"], c["g"], c["m"], c["combos"]) if skip else c["U"])


def entries_where(model, **eq):
    ent = model["ent"]
    sel = np.ones(model["n"], dtype=bool)
    for k, v in eq.items():
        sel &= ent[k] == v
    return np.flatnonzero(sel)


# ---- A: the band plan -------------------------------------------------------------------------------------------------------
A_N = [1, 2, 3, 180, 181, 4095, 4096, 4097, 8191, 8192]
A_PLAN = {1: (14, 1, 1, True), 2: (14, 1, 1, True), 3: (14, 1, 1, True), 180: (14, 1, 1, True), 181: (14, 2, 1, True), 4095: (14, 512, 1, True),
          4096: (15, 257, 2, False), 4097: (15, 257, 2, False), 8191: (16, 512, 4, False), 8192: (17, 257, 7, False)}   # t, bands, rounds, pairs


def a_case(N, port):
    """Sequences of g .. g + 3 symbols (g = 2: one to four windows) over three keys: row i holds key i mod 3 once and, every
    fifth row, key 0 twice more; plus, N >= 4096, the rows whose cells lie at offset cap - 1, cap and ncell - 1 of band 1 paired
    with the columns there (a key each)."""
    def build():
        keys = [{}, {}, {}]
        for i in range(N):
            keys[i % 3][i] = 1
            if i % 5 == 0:
                keys[0][i] = keys[0].get(i, 0) + 2
        keys = [k for k in keys if k]
        plan = cases.band_plan(N)
        if plan["rounds"] > 1:
            for x in a_round_cells(plan):
                keys.append(cases.run(sorted(set(x))))
        return cases.key_rows(N, keys)
    return cases.case(("A", N), build, n_train=N - 4 if N >= 180 else N, oracle=N > 2000, port=port)   # (rows N - 4 and N - 1 share a key: a test x test cell)


def a_round_cells(plan):
    """(column, row) of the cells at offset cap - 1, cap and ncell - 1 of band 1 (ncell > cap: the band takes two rounds)."""
    r_lo, r_hi = plan["r0"][1], plan["r0"][2]
    ncell, out = tri(r_hi) - tri(r_lo), []
    assert ncell > plan["cap"]
    for off in (plan["cap"] - 1, plan["cap"], ncell - 1):
        i = r_lo
        while tri(i + 1) - tri(r_lo) <= off:
            i += 1
        j = off - (tri(i) - tri(r_lo))
        assert r_lo <= i < r_hi and 0 <= j <= i
        out.append((j, i))
    return out


def check_a(make, monkeypatch, port, N, variant, sparse_form=0):
    c = a_case(N, port)
    plan = cases.band_plan(N, variant[1])
    assert (plan["t"], plan["n_owners"], plan["rounds"], plan["pairs"]) == A_PLAN[N][:3] + (A_PLAN[N][3] and bool(variant[1]),)
    assert plan["lists"] and plan["n_owners"] <= cases.SX_MAX_OWNERS
    if N == 181:
        # (16,471 cells are two bands, but row 180 still begins below 2^14: the second band holds no row)
        assert plan["r0"] == [0, 181, 181] and cases.band_plan(180)["r0"] == [0, 180]
    if plan["rounds"] > 1:   # (cells either side of the first round's end, and the band's last)
        for j, i in a_round_cells(plan):
            assert c["want"][tri(i) + j] > 0 or i == j
    more = {"sparse_form": sparse_form} if sparse_form else {}
    form = cases.choose_form(plan, tuning_of(variant, **more), desc_now=variant[0] == "desc")
    if variant[0] == "default":
        assert form == (2 if N == 8192 and not sparse_form else 0)
    run(make, monkeypatch, c, variant, form=form, **more)


# ---- B: the entry classes ---------------------------------------------------------------------------------------------------
def check_b_partners(make, monkeypatch, port, variant, desc_min=None):
    """Partners 1, 32, 33, 48, 49; 47 + own cell = 48 and 48 + own cell = 49; a run clean up to its third entry."""
    X, ntr = cases.b_partners()
    c = cases.case("B-partners", lambda: X, n_train=ntr)
    more = {} if desc_min is None else {"sparse_desc_min": desc_min, "sparse_desc_parts": 2048}
    m = model_of(c, variant, **more)
    ent = m["ent"]
    model_updates(c, m, variant[2])
    assert len(m["tiles"]) == 1 and m["cmax"] >= 2
    short = lambda e: ent["cls"][e] in (1, 4)   # noqa: E731
    s = m["short_max"]
    assert s == (min(desc_min or 16, SX_SHORT) if m["desc"] else SX_SHORT)
    for T in (1, 32, 33, 48, 49):   # (key 0: multiplicity 1, T partners)
        e = entries_where(m, T=T, c=1, np=T)
        assert len(e) >= 1 and all(short(x) == (T <= s) for x in e), T
        assert all(ent["cls"][x] == (5 if m["desc"] else 2) for x in e if T > s)
    for T in (47, 48):              # (key 1: the own cell takes the word count to 48 and 49)
        e = entries_where(m, T=T, c=2)
        assert len(e) == 1 and ent["np"][e[0]] == T + 1 and short(e[0]) == (T + 1 <= s)
    if m["desc"]:                   # (entries of exactly s and s + 1 partners: the last binned one, the first descriptor)
        assert any(short(x) for x in entries_where(m, np=s)) and all(ent["cls"][x] == 5 for x in entries_where(m, np=s + 1))
    assert 3 not in ent["cls"]      # (class 3 needs more than short_max and at most 32 partners: not reachable while SX_SHORT >= 32)
    if m["pairs"] and not variant[2]:   # (key 0: every entry with partners a unit; key 2: units up to the entry of multiplicity 2)
        k0 = entries_where(m, head=0)
        assert ent["unit"][k0][1:s + 1].all() and not ent["unit"][k0][s + 1:].any()
        assert ent["cls"][k0][s] == 4   # (a UNIT entry of exactly short_max partners)
        k2 = entries_where(m, head=int(entries_where(m, c=2, T=3)[0]) - 3)
        assert list(ent["unit"][k2][:5]) == [False, True, 2 <= s, False, False] and list(ent["c"][k2][:5]) == [1, 1, 1, 2, 1]
    run(make, monkeypatch, c, variant, **more)


def check_b_cmax(make, monkeypatch, port, variant):
    """Multiplicity exactly cmax (one word a pair) and cmax + 1 (two)."""
    X, ntr = cases.b_cmax()
    c = cases.case("B-cmax", lambda: X, n_train=ntr)
    m = model_of(c, variant)
    ent = m["ent"]
    model_updates(c, m, variant[2])
    assert m["maxW"] == 257
    if m["pairs"]:
        assert m["cmax"] == 255
        (a,), (b,) = entries_where(m, c=255), entries_where(m, c=256)
        assert ent["wpp"][a] == 1 and ent["cls"][a] == 1 and ent["wpp"][b] == 2 and ent["cls"][b] == (5 if m["desc"] == 1 else 2)
        assert ent["wpp"][entries_where(m, c=257)[0]] == 2
    run(make, monkeypatch, c, variant)


def check_b_skip(make, monkeypatch, port, variant):
    """skip_test_block: test rows with 0, 1, 48 and 49 train partners."""
    assert variant[2]
    X, ntr = cases.b_skip()
    c = cases.case("B-skip", lambda: X, n_train=ntr)
    m = model_of(c, variant)
    ent = m["ent"]
    test = ent["row"] >= ntr
    assert sorted(set(ent["T"][test].tolist())) == [0, 1, 48, 49]
    s = m["short_max"]
    for T in (1, 48, 49):
        e = np.flatnonzero(test & (ent["T"] == T))
        assert len(e) == 2 and all(ent["cls"][x] == ((4 if ent["unit"][x] else 1) if T <= s else 5 if m["desc"] else 2) for x in e)
        assert ent["P"][e[1]] == T + 2   # (the second test row: its rank counts the test row before it, its partners do not)
    assert not ent["np"][test & (ent["T"] == 0)].any()
    run(make, monkeypatch, c, variant)


# ---- C: the slot array ------------------------------------------------------------------------------------------------------
C_CASES = {"exactly_EM_SLOTS": (EM_SLOTS, None), "EM_SLOTS_plus_1": (EM_SLOTS + 1, None), "pass_ends_at_EM_CAP": (None, EM_CAP),
           "pass_ends_at_EM_CAP_plus_47": (None, EM_CAP + SX_SHORT - 1)}


def check_c(make, monkeypatch, port, name, variant):
    """A tile whose short entries take exactly EM_SLOTS words (one straight-line pass) and EM_SLOTS + 1 (several); a first pass
    that ends with exactly EM_CAP and EM_CAP + 47 words. Under pairs: bands with no, one, an odd and an even number of unit cells."""
    total, first_pass = C_CASES[name]
    skip = variant[2]
    tail = 2 if skip else 3   # (the test rows' words, behind everything else)
    if total is not None:
        front, full = total - tail - 10 * tri(48), 10
    elif first_pass == EM_CAP:   # (nine full runs, then the entries of 0..47 partners of the tenth: the sum reaches EM_CAP exactly)
        front, full = EM_CAP - 9 * tri(48) - tri(47), 12
    else:                        # (one word less in front: the sum stands at EM_CAP - 1 and the entry of 48 partners ends the pass)
        front, full = EM_CAP - 1 - 9 * tri(48) - tri(47), 12
    X, ntr = cases.c_slots(front, full)
    c = cases.case(("C", name, skip), lambda: X, n_train=ntr)
    m = model_of(c, variant)
    model_updates(c, m, skip)
    assert len(m["tiles"]) == 1
    tl = m["tiles"][0]
    if m["desc"] == 0 and variant[0] != "blocks":
        assert tl["short_words"] == cases.c_total(front, full, skip)
        if total is not None:
            assert tl["short_words"] == total and tl["one_pass"] == (total <= EM_SLOTS) and (len(tl["passes"]) > 1) == (total > EM_SLOTS)
        else:
            assert not tl["one_pass"] and tl["passes"][0][2] == first_pass and len(tl["passes"]) == tl["short_words"] // EM_CAP + 1
            last = m["ent"]["np"][tl["passes"][0][1] - 1]   # (the entry that ends the first pass)
            assert last == (SX_SHORT if first_pass != EM_CAP else SX_SHORT - 1)
        if m["pairs"]:
            cells = m["tile_cells"][0]
            assert cells[0] > 1000 and cells[1] == 1 and cells[2] == 3 and cells[3] == 6 and cells[4] == 0   # (many, one, odd, even, none)
            assert m["band_stream"][4] == 0 and len(cells) == 6
        e0 = m["ent"]
        assert e0["cls"][0] == 1 and e0["np"][0] == 1 and e0["c"][0] == 2   # (entry 0: binned, one word)
    run(make, monkeypatch, c, variant)


def check_c_fullest(make, monkeypatch, port, variant):
    """skip_test_block: tile 1 is 2048 entries of exactly 48 partners — EM_MAX_PASS passes."""
    X, ntr = cases.c_fullest()
    c = cases.case("C-fullest", lambda: X, n_train=ntr)
    m = model_of(c, variant)
    model_updates(c, m, variant[2])
    if variant[2] and m["desc"] == 0 and variant[0] != "blocks":
        t1 = m["tiles"][1]
        assert t1["n"] == sec.SG_TILE and t1["short_words"] == sec.SG_TILE * SX_SHORT and len(t1["passes"]) == cases.EM_MAX_PASS
        assert (m["ent"]["np"][t1["e0"]:] == SX_SHORT).all() and (m["ent"]["before"][t1["e0"]:] >= SX_SHORT).all()
    run(make, monkeypatch, c, variant)


# ---- D: runs across tile edges ----------------------------------------------------------------------------------------------
D_STRADDLE = {"first_entry_1_partner": (2047, 2, 1), "first_entry_48_partners": (2000, 60, 48), "run_begins_49_before": (1999, 60, 49)}


def check_d_straddle(make, monkeypatch, port, name, variant):
    """The entry at tile-local index 0 of tile 1 with 1 and 48 partners, all of them before the tile (the LDS copy of the 48
    entries in front of a tile); a run that begins 49 entries before the tile (global reads of partners)."""
    pad, d, T = D_STRADDLE[name]
    X, ntr = cases.d_straddle(pad, d)
    c = cases.case(("D", name), lambda: X, n_train=ntr)
    m = model_of(c, variant)
    model_updates(c, m, variant[2])
    ent, t1 = m["ent"], m["tiles"][1]
    e = t1["e0"]
    assert len(m["tiles"]) == 2 and ent["el"][e] == 0 and ent["T"][e] == T and ent["before"][e] == T and ent["first"][e] == sec.SG_TILE
    if variant[0] != "blocks":
        assert ent["cls"][e] == ((4 if ent["unit"][e] else 1) if T <= m["short_max"] else 5 if m["desc"] else 2)
    if T >= SX_SHORT:   # (the entries behind it: long, their runs begin 48 / 49 before the tile)
        assert (ent["before"][e:e + d - T] == T).all() and (ent["T"][e + 1:e + d - T] > SX_SHORT).all()
    run(make, monkeypatch, c, variant)


def check_d_e0(make, monkeypatch, port, e0, variant):
    """Tiles in front of which lie exactly 1, 47 and 48 entries: the guard of the copy of the entries in front of a tile."""
    X, ntr = cases.d_e0(e0)
    c = cases.case(("D-e0", e0), lambda: X, n_train=ntr)
    m = model_of(c, variant)
    model_updates(c, m, variant[2])
    ent, t1 = m["ent"], m["tiles"][1]
    e = t1["e0"]
    assert e == e0 and m["tiles"][0]["n"] == e0 and ent["T"][e] == e0 and ent["before"][e] == e0 and ent["c"][:e0].sum() == sec.SG_TILE
    assert ent["wpp"].max() == 1 or e0 == 1
    run(make, monkeypatch, c, variant)


def check_d_far(make, monkeypatch, port, variant, **more):
    """A run that began more than 2048 entries before the tile: tile 2's entries read 4096 partners and more from global memory
    (as descriptors: on the owner bands, two LDS rounds a band)."""
    X, ntr = cases.d_far()
    c = cases.case("D-far", lambda: X, n_train=ntr, oracle=True, port=port)
    E = cases.entries_of(c["X"])
    assert len(E["row"]) == 4200 and (E["first"] == np.arange(4200)).all() and E["P"][4096] == 4097 and (E["head"] == 0).all()
    run(make, monkeypatch, c, variant, form=cases.choose_form(cases.band_plan(4200, variant[1]), tuning_of(variant, **more), desc_now=variant[0] == "desc"), **more)


# ---- E: parts and streams ---------------------------------------------------------------------------------------------------
def check_e_parts(make, monkeypatch, port, pairs, target):
    """Bands of 1, 2 and 5 parts side by side (plain read-modify-write beside atomics); over the targets 65, 66, 67 and 68 a
    part's first word lies at every residue mod 4."""
    variant = ("default", pairs, False)
    unit = 2 if pairs else 1   # (under pairs two unit cells share a container)
    X, ntr = cases.e_words(300, [55 * unit, 105 * unit, 276 * unit])
    c = cases.case(("E-parts", pairs), lambda: X, n_train=ntr)
    m = model_of(c, variant, sparse_parts_target=target)
    model_updates(c, m, False)
    nparts = [sum(1 for p in m["parts"] if p["band"] == o) for o in range(3)]
    assert m["target"] == target and nparts == [1, 2, 5], (nparts, m["band_stream"])
    # (band 0's 55 words, band 1's 105 from word 55 and band 2's 276 from word 160, cut every ``target`` words)
    assert [p["a"] for p in m["parts"]] == [0, 55, 55 + target, 160, 160 + target, 160 + 2 * target, 160 + 3 * target, 160 + 4 * target]
    assert all(p["b"] - p["a"] >= 4 for p in m["parts"]) and {p["a"] % 4 for p in m["parts"]} == E_RESIDUES[target]
    run(make, monkeypatch, c, variant, sparse_parts_target=target)


E_TARGETS = [65, 66, 67, 68]
E_RESIDUES = {65: {0, 1, 2, 3}, 66: {0, 1, 2, 3}, 67: {0, 1, 2, 3}, 68: {0, 3}}   # (first words mod 4: 68 keeps band 2's parts aligned)


def check_e_streams(make, monkeypatch, port, pairs):
    """Streams of 0, 1, 3, 4, 7 and 8 words in neighbouring bands: either side of the split into 16-byte pieces."""
    variant = ("default", pairs, False)
    unit = 2 if pairs else 1
    X, ntr = cases.e_words(450, [w * unit for w in (0, 1, 3, 4, 7, 8, 0)])
    c = cases.case(("E-streams", pairs), lambda: X, n_train=ntr)
    m = model_of(c, variant)
    model_updates(c, m, False)
    assert list(m["band_stream"]) == [0, 1, 3, 4, 7, 8, 0] and [p["b"] - p["a"] for p in m["parts"]] == [1, 3, 4, 7, 8]
    # (the streams start at words 0, 1, 4, 8 and 15: the 4 and 7 words from 4 and 8 are whole pieces with a tail, the 8 from 15 a
    # head of one word, one piece and a tail of three; 1 and 3 words are no piece at all)
    assert [p["a"] for p in m["parts"]] == [0, 1, 4, 8, 15]
    assert [((p["a"] + 3) & ~3) < (p["b"] & ~3) for p in m["parts"]] == [False, False, True, True, True]
    run(make, monkeypatch, c, variant)


def check_e_long_part(make, monkeypatch, port, words):
    """One part of 16,383 / 16,384 / 16,385 words: the last trip of the four-piece loop of k_sx_consume."""
    variant = ("default", 0, False)
    X, ntr = cases.e_words(181, [words, 0])
    c = cases.case(("E-long", words), lambda: X, n_train=ntr)
    m = model_of(c, variant, sparse_parts_target=1 << 20)
    model_updates(c, m, False)
    assert [(p["a"], p["b"]) for p in m["parts"]] == [(0, words)]
    n4 = (words & ~3) >> 2
    assert (n4 > 3 * cases.CS_THREADS + cases.CS_THREADS - 1) == (words >= 16384)   # (thread 1023 takes the unrolled trip from 16,384 on)
    run(make, monkeypatch, c, variant, sparse_parts_target=1 << 20)


def partner_format(cols, unpacked, N):
    """sx_expand_descriptors' FMT as sx_segment / k_sx_consume choose it: 0 packed entries, 1 8-byte entries, 2 two-byte columns,
    3 four-byte columns."""
    packed = not unpacked and N < 65535
    have_cols = cols >= 2 or (cols == 1 and not packed)
    return (2 if cols == 3 and N < 32768 else 3) if have_cols else (0 if packed else 1)


E_FORMATS = [(cols, unpacked) for cols in (0, 1, 2, 3) for unpacked in (0, 1)]


def check_e_desc(make, monkeypatch, port, cols, unpacked, desc_parts, variant=("desc", 1, False)):
    """Descriptors of 1, CHUNK - 1, CHUNK and CHUNK + 1 partners whose first partner lies at every residue of the 16-byte load, in
    each of the four partner formats; a partner of multiplicity above 1 (in a 2-byte column: one that does not fit and is read
    again from the entry), an entry of multiplicity above 1 (its own cell); few and many parts."""
    X, ntr = cases.e_desc(big=256)
    c = cases.case("E-desc", lambda: X, n_train=ntr)
    fmt = partner_format(cols, unpacked, c["N"])
    assert {partner_format(a, b, c["N"]) for a, b in E_FORMATS} == {0, 1, 2, 3}
    more = dict(sparse_desc_min=1, sparse_desc_cols=cols, sparse_unpacked=unpacked, sparse_desc_parts=desc_parts, sparse_parts_target=1)
    m = model_of(c, variant, **more)
    model_updates(c, m, variant[2])
    ent = m["ent"]
    d5 = np.flatnonzero(ent["cls"] == 5)
    per, chunk = cases.DESC_PER[fmt], cases.DESC_GROUP[1] * cases.DESC_PER[fmt]
    assert {int(ent["head"][e]) % per for e in d5} == set(range(per))
    for r in range(per):   # (at every residue: T = 1 and either side of a whole chunk; a last partner alone at the head of a piece)
        Ts = {int(ent["T"][e]) for e in d5 if ent["head"][e] % per == r}
        assert Ts >= {1, chunk - 1, chunk, chunk + 1}, (r, sorted(Ts))
    assert any((ent["head"][e] + ent["T"][e] - 1) % per == 0 for e in d5)
    e1 = [e for e in d5 if ent["T"][e] == 1]
    assert all(ent["c"][e] == 2 for e in e1)   # (T = 1 is a descriptor only through its own cell: np = 2 > desc_min = 1)
    colbits = max(1, sec.bits_below(c["N"]))
    assert colbits == 8 and (256 >> (16 - colbits)) != 0 and (255 >> (16 - colbits)) == 0   # (256 does not fit a 2-byte column's multiplicity field)
    nd = [p["nd"] for p in m["parts"]]
    if desc_parts == 1:
        assert len(m["parts"]) == 1 and nd[0] == len(d5)
    else:   # (more parts than descriptors would need: every part takes every nparts-th descriptor, the last ones may take none)
        assert len(m["parts"]) >= 32 and sum(nd) == len(d5) and max(nd) >= 2
    run(make, monkeypatch, c, variant, **more)


def check_e_desc_bands(make, monkeypatch, port, variant=("desc", 1, False)):
    """A band with descriptors and no words beside a band with words and no descriptors and a band with neither; fewer
    descriptors than parts."""
    N = 300
    (a0, _), (a1, _), _ = cases.band_rows(N)
    more = dict(sparse_desc_min=48, sparse_parts_target=1, sparse_desc_parts=64)
    keys = [cases.run(range(a0, a0 + 3)), {**{i: 1 for i in range(0, 49)}, a1 + 1: 1, a1 + 2: 1}]
    X2 = cases.key_rows(N, keys)
    c = cases.case("E-desc-bands-2", lambda: X2)
    m = model_of(c, variant, **more)
    # band 1: two entries of 49 and 50 partners — descriptors — and no word; band 2: nothing
    assert m["band_desc"][1] == 2 and m["band_stream"][1] == 0 and m["band_stream"][0] > 0 and m["band_desc"][2] == 0 and m["band_stream"][2] == 0
    mine = [p for p in m["parts"] if p["band"] == 1]
    assert len(mine) > 2 and sum(p["nd"] for p in mine) == 2 and all(p["a"] == p["b"] for p in mine)   # (fewer descriptors than parts)
    run(make, monkeypatch, c, variant, **more)


def check_e_two_rounds(make, monkeypatch, port):
    """Descriptors in a band of two LDS rounds: N = 4096, the owner bands forced (with descriptors the default is the blocks)."""
    variant = ("desc", 1, False)
    c = a_case(4096, port)
    plan = cases.band_plan(4096)
    assert plan["rounds"] == 2 and cases.choose_form(plan, tuning_of(variant), desc_now=True) == 2
    assert cases.choose_form(plan, tuning_of(variant, sparse_form=1), desc_now=True) == 0
    run(make, monkeypatch, c, variant, form=0, sparse_form=1)


# ---- F: the by-slot stores of variance mode ---------------------------------------------------------------------------------
def f_sequences(N, top):
    """Variance mode runs both combinations of (g, m) = (2, 1); every sequence closes with its own first symbol, so both see the
    same keys. ``top`` = 0: row i holds key i mod 3 once or twice. Else rows 0 and 1 are equal: 65535 — key 1 255 times and 510
    keys once (255^2 + 510 = 65535: cell (1, 0) and both diagonal cells, the largest a u16 slot triangle holds; 255 * 257 as ONE
    product is not reachable, a row of 257 windows of one key has a diagonal of 257^2) — or 65536: key 1 256 times (256 * 256)."""
    X = [[1 + i % 3] * (1 + i % 2) for i in range(N)]
    if top == 65535:
        X[0] = X[1] = [1] * 255 + list(range(4, 514))
    elif top == 65536:
        X[0] = X[1] = [1] * 256
    return [s + [s[0]] for s in X]


F_N = [1, 2, 3, 181, 830]


def f_residues(N, slots16):
    """Where the bands' first cells lie in the two slot triangles of a batch, modulo the cells of a 16-byte store (8 u16 or 4
    u32); the triangles are a multiple of 4 cells apart (fsk_engine_variance.hip:48-51)."""
    plan = cases.band_plan(N)
    ps = (tri(N) + 3) & ~3
    per = 8 if slots16 else 4
    return {(s * ps + tri(r)) % per for s in (0, 1) for r in plan["r0"][:-1]}, plan


def check_f(make, monkeypatch, port, N, slots16, t, top=0):
    """Triangle and stdevs of variance mode against port.compute, bit for bit; batches_redone: 0 while every sum fits u16, 1 when
    one reaches 65,536."""
    from fastsk_amd import _native
    X = f_sequences(N, top)
    res, plan = f_residues(N, slots16)
    if N <= 3:   # (spans shorter than the head of a 16-byte store; no whole store at all)
        assert plan["largest"] == tri(N) <= 6 and plan["n_owners"] == 1
    if N == 830:   # (22 bands: their first cells lie at every residue of a 16-byte store in one or the other slot triangle)
        assert res == set(range(8 if slots16 else 4)) and plan["n_owners"] == 22, res
    if top:
        K, _, _ = sec.counts_by_definition_wide(X, 2, 1, [0])
        assert int(K[tri(1)]) == top and int(K.max()) == top   # (cell (1, 0); nothing larger)
    tok, off = _native.flatten(X)
    want_tri, want_sd, _ = port.compute(tok, off, N, 0, 2, 1, t=t, approx=True, max_iters=2, order=np.array([0, 1], dtype=np.int32))
    set_tuning_env(monkeypatch, var_slots16=slots16)
    e = make(2, 1, t=t, approx=True, max_iters=2, path=2)
    e.set_combo_order(np.array([0, 1], dtype=np.int32))
    e.compute(tok, off, N, 0)
    st = e.stats()
    sd, got = e.get_stdevs(), e.get_triangle()
    e.close()
    print("N=%d slots16=%d t=%d top=%d: redone %d, form %d" % (N, slots16, t, top, st["batches_redone"], st["sparse_form"]))
    assert st["path_used"] == 2
    assert st["batches_redone"] == (1 if top == 65536 and slots16 else 0)
    assert np.array_equal(sd, want_sd) and np.array_equal(got, want_tri)


# ---- G: the two-level blocks ------------------------------------------------------------------------------------------------
def g_case(name):
    """N = 128, one band. ``crossing``: rows 100..127 share keys with columns chosen against the sub-bands of 16 cells — a list
    that crosses after its first partner, before its last, between every two partners, and one wholly inside a sub-band."""
    N = 128
    if name == "crossing":
        keys = []
        for i, cols in G_LISTS:
            keys.append({**cases.run(cols + [i]), **({i: 2} if i == G_LISTS[0][0] else {})})   # (the first list's row: multiplicity 2)
        return cases.key_rows(N, keys)
    if name.startswith("records"):
        return cases.key_rows(N, [cases.run(range(d)) for d in g_record_runs(int(name[7:]))])
    words = int(name)
    return cases.key_rows(N, [cases.run(range(d)) for d in cases.triangular_runs(words, N)])


def _g_lists(sub_shift=4):
    """(row, columns): tri(row) mod 16 decides where the sub-band edges fall among the row's columns."""
    out = []
    for i in range(100, 128):
        edge = (-tri(i)) % 16   # (the first column of the row that starts a new sub-band)
        if edge in (0, 15) or len(out) >= 5:
            continue
        if len(out) == 3 and 1 + -(-(i - edge) // 16) != (i >> sub_shift) + 2:   # (the fifth list: a row whose columns touch as
            continue                                                              # many sub-bands as it has records reserved)
        kind = len(out)
        cols = {0: [edge - 1, edge, edge + 1, edge + 2],          # crosses after its first partner
                1: [edge + 13, edge + 14, edge + 15, edge + 16],  # crosses before its last
                2: [edge + 16 * q for q in range(5)],             # between every two partners
                3: [edge, edge + 1, edge + 2, edge + 15]}[kind]   # wholly inside one sub-band
        out.append((i, cols))
        if kind == 3:
            out.append((i, [0] + list(range(edge, i, 16))))          # one partner in every sub-band the row touches
    assert len(out) == 5
    return out


def g_record_runs(records, sub_shift=6, N=128):
    """Run lengths over rows 0..d-1 whose descriptor entries (two partners and more: sparse_desc_min = 1) reserve ``records``
    records in all: (row >> 6) + 2 each — 316 a run of all 128 rows."""
    per = lambda d: sum((i >> sub_shift) + 2 for i in range(2, d))   # noqa: E731
    full, rest = divmod(records, per(N))
    for d1 in range(2, N + 1):
        for d2 in range(2, 8):
            if per(d1) + per(d2) == rest:
                return [N] * full + [d1, d2]
    raise AssertionError(records)


G_LISTS = _g_lists()
G_TUNING = {4: dict(blocks_sub_shift=4, blocks_max_bands=2, blocks_band_shift_max=14), 6: dict(blocks_sub_shift=6, blocks_max_bands=2, blocks_band_shift_max=14)}


def check_g_crossing(make, monkeypatch, port, sub_shift, desc, skip):
    """Partner lists against the sub-band edges; with descriptors a row's reserved records all used and all but one empty."""
    variant = ("blocks", 1, skip)
    c = cases.case("G-crossing", lambda: g_case("crossing"))
    tun = dict(G_TUNING[sub_shift], **({"sparse_desc": 1, "sparse_desc_min": 1} if desc else {}))
    P = cases.blocks_pass_plan(c["N"], 0, c["N"], dict(sec.FORMS["blocks"][0], **tun))
    assert P is not None and P["r0"][1] == c["N"] and P["t"] == 13 and P["sub_shift"] == sub_shift   # (every row in band 0)
    m = cases.update_model(c["X"], c["n_train"], skip, dict(sec.FORMS["blocks"][0], **tun), bands=P)
    ent = m["ent"]
    kinds = []
    for i, cols in G_LISTS:
        (e,) = [x for x in entries_where(m, row=i) if ent["T"][x] == len(cols)]
        sub = cases.partner_cells(m, e) >> sub_shift
        kinds.append(list(sub - sub[0]))
        if desc:
            assert ent["cls"][e] == 5
    if sub_shift == 4:
        assert kinds[0] == [0, 1, 1, 1] and kinds[1] == [0, 0, 0, 1] and kinds[2] == [0, 1, 2, 3, 4] and kinds[3] == [0, 0, 0, 0], kinds
        i5 = G_LISTS[4][0]   # (every reserved record of the row used; list 3 leaves all but one empty)
        assert kinds[4] == list(range((i5 >> 4) + 2)) and len(set(kinds[3])) == 1
    else:
        assert kinds[3] == [0, 0, 0, 0] and any(len(set(k)) > 1 for k in kinds)
    (own,) = [x for x in entries_where(m, row=G_LISTS[0][0]) if ent["c"][x] == 2]
    assert ent["np"][own] == ent["T"][own] + 1 and (not desc or (ent["cls"][own] == 5 and m["band_words"][0] >= 1))   # (its own cell: a word)
    if desc:   # (entries of two partners and more are records: only the one-partner entries and the own cells are words)
        assert m["band_desc"][0] > m["band_words"][0]
        words, recs = cases.sub_band_counts(m)
        assert sum(words.values()) == m["band_words"].sum() and len(recs) > 0
        assert any(k not in words for k in recs)      # (a sub-band with records and no words)
        assert any(k in words for k in recs) and any(k not in recs for k in words)   # (and with both, and with words alone)
    passes = cases.blocks_passes(c["N"], lambda plan: 1, dict(sec.FORMS["blocks"][0], **tun))
    assert len(passes) == 1
    run(make, monkeypatch, c, variant, form=2, desc=1 if desc else None, passes=1, **tun)


def check_g_tile(make, monkeypatch, port, words):
    """A band of 8191 / 8192 / 8193 words: the tile of k_sxb_scatter; one pass of one band."""
    variant = ("blocks", 1, False)
    c = cases.case(("G", words), lambda: g_case(str(words)))
    tun = dict(sec.FORMS["blocks"][0], **G_TUNING[6])
    P = cases.blocks_pass_plan(c["N"], 0, c["N"], tun)
    m = cases.update_model(c["X"], bands=P, tuning=tun)
    assert P["r0"][1] == c["N"] and list(m["band_stream"]) == [words, 0] and cases.SXB_TILE == 8192
    run(make, monkeypatch, c, variant, form=2, passes=1, **G_TUNING[6])


def check_g_records(make, monkeypatch, port, records):
    """8191 / 8192 / 8193 descriptor records in one band: the piece of k_sxb_drecords."""
    variant = ("blocks", 1, False)
    c = cases.case(("G-records", records), lambda: g_case("records%d" % records))
    tun = dict(sec.FORMS["blocks"][0], sparse_desc=1, sparse_desc_min=1, **G_TUNING[6])
    P = cases.blocks_pass_plan(c["N"], 0, c["N"], tun)
    m = cases.update_model(c["X"], bands=P, tuning=tun)
    assert m["desc"] == 2 and P["r0"][1] == c["N"] and list(m["band_desc"]) == [records, 0] and cases.SXD_PIECE == 8192
    run(make, monkeypatch, c, variant, form=2, desc=1, passes=1, sparse_desc=1, sparse_desc_min=1, **G_TUNING[6])


def check_g_passes(make, monkeypatch, port, pass_words):
    """Passes of at most two bands of 2^5 cells: every row from 13 on is a pass of its own. blocks_pass_words = 30 halves the
    pass of rows 8..10, whose 30 words reach it. stats()["sparse_passes"] against the restated loop."""
    variant = ("blocks", 1, False)
    c = cases.case("G-passes", lambda: cases.key_rows(40, [cases.run(range(40)), cases.run(range(0, 40, 3))]))
    tun = dict(sec.FORMS["blocks"][0], blocks_sub_shift=4, blocks_max_bands=2, blocks_band_shift_max=5, blocks_pass_words=pass_words)
    nrec = sum(len(s) - 1 for s in c["X"])

    def words_of(P):
        return int(cases.update_model(c["X"], bands=P, tuning=tun)["band_stream"].sum())
    plain = cases.blocks_passes(c["N"], words_of, dict(tun, blocks_pass_words=0), nrec)
    passes = cases.blocks_passes(c["N"], words_of, tun, nrec)
    assert any(p["rb"] - p["ra"] == 1 for p in passes) and any(p["rb"] - p["ra"] > 1 for p in passes)   # (a pass of one row)
    assert sum(p["words"] for p in passes) == sum(p["words"] for p in plain) == c["U"] - 40 - 14   # (every pair but the entries' own)
    assert len(plain) == 31 and (8, 11, 30) in [(p["ra"], p["rb"], p["words"]) for p in plain]
    if pass_words:
        assert pass_words == 30 and len(passes) == 32 and [(p["ra"], p["rb"]) for p in passes][2:4] == [(8, 10), (10, 11)]
    run(make, monkeypatch, c, variant, form=2, passes=len(passes), **{k: v for k, v in tun.items() if k != "sparse_form"})


# ---- the yardsticks themselves ------------------------------------------------------------------------------------------------
def test_constants_match_the_sources():
    """Every constant the model restates, found in the engine's sources as written there: the model cannot drift unnoticed."""
    for fname, text in cases.SOURCE_CONSTANTS:
        with open(os.path.join(ROOT, "fastsk_amd", "csrc", fname)) as f:
            assert text in f.read(), (fname, text)
    assert cases.EM_CAP == 11752 and cases.EM_MAX_PASS == 9


def test_band_plan_table():
    """The restated plans at the shapes group A names."""
    for N, (t, bands, rounds, pairs) in A_PLAN.items():
        p = cases.band_plan(N)
        assert (p["t"], p["n_owners"], p["rounds"], p["pairs"]) == (t, bands, rounds, pairs), N
        assert p["r0"][0] == 0 and p["r0"][-1] == N and p["cap"] == min(cases.SX_CAP, p["largest"])
    assert cases.choose_form(cases.band_plan(8191)) == 0 and cases.choose_form(cases.band_plan(8192)) == 2
    assert cases.choose_form(cases.band_plan(8192), {"sparse_form": 1}) == 0
    P = cases.blocks_pass_plan(128, 0, 128, G_TUNING[4])
    assert (P["t"], P["n_owners"], P["r0"], P["pb"], P["submax"]) == (13, 2, [0, 128, 128], 18, 8256 // 16 + 1)   # (8256 cells: a second, empty band)
    assert cases.blocks_pass_plan(400, 0, 400, dict(blocks_sub_shift=4, blocks_max_bands=2, blocks_band_shift_max=7)) is None


def test_model_by_hand():
    """Three keys over five rows, counted by hand."""
    X = cases.key_rows(5, [cases.run([0, 1, 2]), {1: 3, 4: 1}, cases.run([3])])
    m = cases.update_model(X)
    ent = m["ent"]
    assert list(ent["row"]) == [0, 1, 2, 1, 4, 3] and list(ent["c"]) == [1, 1, 1, 3, 1, 1] and list(ent["P"]) == [1, 2, 3, 1, 2, 1]
    assert list(ent["np"]) == [0, 1, 2, 1, 1, 0] and list(ent["unit"]) == [False, True, True, False, False, False]
    assert list(ent["cls"]) == [0, 4, 4, 1, 1, 0] and m["U"] == 6 + 3 + 1
    assert m["tiles"][0]["short_words"] == 5 and list(m["band_stream"]) == [2 + 2]   # (3 unit cells: 2 containers; 2 words)
    assert list(cases.update_model(X, tuning={"sparse_pairs": 0})["band_stream"]) == [5]


def test_a_case_off_its_edge_fails_at_the_precondition():
    """One word more in front and the tile of ``exactly_EM_SLOTS`` is no longer one pass: the model says so before an engine runs."""
    X, ntr = cases.c_slots(EM_SLOTS - 3 - 10 * tri(48), 10)
    assert cases.update_model(X, ntr)["tiles"][0]["one_pass"]
    X, ntr = cases.c_slots(EM_SLOTS - 3 - 10 * tri(48) + 1, 10)
    assert not cases.update_model(X, ntr)["tiles"][0]["one_pass"]


REFERENCE_CASES = {"B": lambda: cases.case("B-partners", lambda: cases.b_partners()[0], n_train=cases.b_partners()[1]),
                   "C": lambda: cases.case(("C", "exactly_EM_SLOTS", False), lambda: cases.c_slots(EM_SLOTS - 3 - 10 * tri(48), 10)[0],
                                           n_train=cases.c_slots(EM_SLOTS - 3 - 10 * tri(48), 10)[1]),
                   "E": lambda: cases.case("E-desc", lambda: cases.e_desc(big=256)[0]),
                   "G": lambda: cases.case("G-crossing", lambda: g_case("crossing"))}


@pytest.mark.parametrize("group", sorted(REFERENCE_CASES))
def test_reference_is_the_oracle(port, group):
    """counts_by_definition_wide against port.raw_counts on one case of the groups it serves: two references agree before an
    engine is asked (group A's large N and D-far take the oracle itself; group F port.compute)."""
    c = REFERENCE_CASES[group]()
    sec.check_reference(port, c)


# ---- the emulator runs --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    from fastsk_amd import _native
    return lambda g, m, **kw: _native.Engine(g, m, lib=emu_lib, **kw)


A_RUNS = [(N, v, 0) for N in A_N for v in (("default", 1, False), ("default", 0, False), ("default", 1, True), ("desc", 1, False), ("blocks", 1, False),
                                            ("atomics", 1, False))] + [(8192, ("default", 1, False), 1), (8192, ("desc", 1, False), 1)]
A_RUNS = [r for r in A_RUNS if not (r[0] <= 3 and r[1][2])]   # (skip_test_block needs test rows beside train rows: the N >= 180 cases have them)


@pytest.mark.parametrize("N,variant,sparse_form", [r for r in A_RUNS if r[0] <= EMU_MAX_N], ids=lambda v: vid(v) if isinstance(v, tuple) else str(v))
def test_band_plan_boundaries(make_emu, monkeypatch, port, N, variant, sparse_form):
    check_a(make_emu, monkeypatch, port, N, variant, sparse_form)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_entry_classes(make_emu, monkeypatch, port, variant):
    check_b_partners(make_emu, monkeypatch, port, variant)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip"])
@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("desc_min", [1, 16, 48])
def test_entry_classes_descriptor_threshold(make_emu, monkeypatch, port, desc_min, pairs, skip):
    check_b_partners(make_emu, monkeypatch, port, ("desc", pairs, skip), desc_min)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_multiplicity_at_cmax(make_emu, monkeypatch, port, variant):
    check_b_cmax(make_emu, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v[2]], ids=vid)
def test_test_rows_of_0_1_48_49_train_partners(make_emu, monkeypatch, port, variant):
    check_b_skip(make_emu, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("name", sorted(C_CASES))
def test_slot_capacity(make_emu, monkeypatch, port, name, variant):
    check_c(make_emu, monkeypatch, port, name, variant)


@pytest.mark.parametrize("variant", [("default", 1, True), ("default", 0, True), ("default", 1, False), ("desc", 1, True), ("blocks", 1, True),
                                     ("atomics", 1, True)], ids=vid)
def test_fullest_tile(make_emu, monkeypatch, port, variant):
    check_c_fullest(make_emu, monkeypatch, port, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("name", sorted(D_STRADDLE))
def test_runs_across_a_tile_edge(make_emu, monkeypatch, port, name, variant):
    check_d_straddle(make_emu, monkeypatch, port, name, variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("e0", [1, 47, 48])
def test_entries_in_front_of_a_tile(make_emu, monkeypatch, port, e0, variant):
    check_d_e0(make_emu, monkeypatch, port, e0, variant)


D_FAR = [("default", 1, False), ("desc", 1, False), ("blocks", 1, False), ("atomics", 1, False)]


@pytest.mark.parametrize("variant", D_FAR, ids=vid)
def test_run_that_began_two_tiles_back(make_emu, monkeypatch, port, variant):
    check_d_far(make_emu, monkeypatch, port, variant, **({"sparse_form": 1} if variant[0] == "desc" else {}))


@pytest.mark.parametrize("target", E_TARGETS)
@pytest.mark.parametrize("pairs", [1, 0])
def test_parts_side_by_side(make_emu, monkeypatch, port, pairs, target):
    check_e_parts(make_emu, monkeypatch, port, pairs, target)


@pytest.mark.parametrize("pairs", [1, 0])
def test_streams_of_a_few_words(make_emu, monkeypatch, port, pairs):
    check_e_streams(make_emu, monkeypatch, port, pairs)


@pytest.mark.parametrize("words", [16383, 16384, 16385])
def test_part_of_16384_words(make_emu, monkeypatch, port, words):
    check_e_long_part(make_emu, monkeypatch, port, words)


@pytest.mark.parametrize("desc_parts", [1, 64])
@pytest.mark.parametrize("cols,unpacked", E_FORMATS)
def test_descriptor_partner_formats(make_emu, monkeypatch, port, cols, unpacked, desc_parts):
    check_e_desc(make_emu, monkeypatch, port, cols, unpacked, desc_parts)


def test_descriptor_bands_without_words(make_emu, monkeypatch, port):
    check_e_desc_bands(make_emu, monkeypatch, port)


def test_descriptors_in_two_lds_rounds(make_emu, monkeypatch, port):
    check_e_two_rounds(make_emu, monkeypatch, port)


F_RUNS = [(N, s, t, 0) for N in F_N for s in (1, 0) for t in (1, 2)] + [(181, s, t, top) for top in (65535, 65536) for s in (1, 0) for t in (1, 2)]


@pytest.mark.parametrize("N,slots16,t,top", F_RUNS)
def test_by_slot_stores(make_emu, monkeypatch, port, N, slots16, t, top):
    check_f(make_emu, monkeypatch, port, N, slots16, t, top)


@pytest.mark.parametrize("skip", [False, True], ids=["whole", "skip"])
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("sub_shift", [4, 6])
def test_lists_across_sub_bands(make_emu, monkeypatch, port, sub_shift, desc, skip):
    check_g_crossing(make_emu, monkeypatch, port, sub_shift, desc, skip)


@pytest.mark.parametrize("words", [8191, 8192, 8193])
def test_scatter_tile(make_emu, monkeypatch, port, words):
    check_g_tile(make_emu, monkeypatch, port, words)


@pytest.mark.parametrize("records", [8191, 8192, 8193])
def test_descriptor_record_piece(make_emu, monkeypatch, port, records):
    check_g_records(make_emu, monkeypatch, port, records)


@pytest.mark.parametrize("pass_words", [0, 30])
def test_blocks_passes(make_emu, monkeypatch, port, pass_words):
    check_g_passes(make_emu, monkeypatch, port, pass_words)
