"""Inputs and the numpy statement of the batched unpack of the packed shift corrections (fsk_kernels_dense_shift.h:
k_dense_shift_packed; fsk_engine_dense_shift.hip: dense_shift_unpack_flags; tuning dense_shift_batch), shared by
tests/test_emu_dense_shift_batch.py and tests/test_gpu_dense_shift_batch.py. Nothing here touches an engine.
tests/dense_shift_packed_cases.py has the arithmetic this one replaces, tests/dense_shift_cases.py the identity.

The kernel no longer adds the bytes of every step's prefix sum to its int32 sums. It adds bytes to bytes for a batch of steps
and unpacks once a batch:

    D'    = lo(sigma) + (~lo(delta) & 15)           per term and cell = the difference + 15, in [0, 30]: a byte, no borrow
    R_r   = sum_{u <= r} D'_u                        inside a chain, in [0, 30 (r + 1)]; restarts at a chain base
    Q    += R_r                                      every step, row term and column term; does NOT restart at a chain base
    acc  += Q, Q = 0                                 where the step table carries the flag (bit 8 of the weight word)
    acc  += 16 w (hi(sigma) - hi(delta))             the counts above 15, at the step's weight w, every step, directly
    K    += acc - 30 x the sum of all weights

The flags come from the bound alone (``unpack_flags``): the step at chain position r (0-based) counts 30 (r + 1) against a
byte's 255, the table is walked in the plan's order, the flag stands on the step before the one that would pass 255 and on the
last step. ``batched_sum`` evaluates exactly this in the plan's step order, asserts that no byte of Q passes 255, and reports
what every batch reached against what the walk allowed it."""
import numpy as np

import dense_shift_cases as cases
import dense_shift_inplace_cases as inplace
import dense_shift_lanes_cases as lanes
import dense_shift_packed_cases as packed

TILE = cases.TILE
TUNING = dict(inplace.TUNING)     # {"tile_splits": 1, "dense_shift": 1, "dense_shift_packed": 0}
BATCH = (1, 0)                    # dense_shift_batch: by the bound, and after every step (the schedule before)
UNIT, BYTE = 30, 255              # a step at chain position r adds at most UNIT (r + 1) to a byte of Q


def plan_chains(plist):
    """The chains of a call in the engine's order: shapes in lexicographic order, a class cut after nine members, then the
    longest chains first (a stable sort). -> lists of places in the call."""
    shapes = {}
    for q, pos in enumerate(plist):
        shapes.setdefault(tuple(p - pos[0] for p in pos), []).append((pos[0], q))
    out = []
    for shape in sorted(shapes):
        members = sorted(shapes[shape], key=lambda sq: sq[0])
        run = []
        for i, (shift, q) in enumerate(members):
            if i == 0 or shift != members[i - 1][0] + 1 or len(run[-1]) >= packed.MAX_CHAIN:
                run.append([])
            run[-1].append(q)
        out += run
    out.sort(key=lambda ch: -len(ch))
    assert sorted(map(len, out)) == sorted(map(len, packed.cut(cases.chains(plist))))
    return out


def unpack_flags(lengths, batch=1, unit=UNIT):
    """The walk. ``lengths``: the chains' members in plan order. -> per derived step (chain, position r, flag)."""
    steps = [(c, r) for c, n in enumerate(lengths) for r in range(n - 1)]
    flags = [False] * len(steps)
    bound = 0
    for s, (c, r) in enumerate(steps):
        add = unit * (r + 1)
        assert add <= BYTE, "one step alone passes the byte: chains are cut at nine members"
        if s > 0 and (not batch or bound + add > BYTE):
            flags[s - 1] = True
            bound = 0
        bound += add
    if steps:
        flags[-1] = True
    return [(c, r, f) for (c, r), f in zip(steps, flags)]


def batches(lengths, batch=1):
    """-> the batches of the walk: lists of (chain, r), and the bound of each."""
    out, cur = [], []
    for c, r, f in unpack_flags(lengths, batch):
        cur.append((c, r))
        if f:
            out.append(cur)
            cur = []
    assert not cur, "the last step carries a flag"
    return out, [sum(UNIT * (r + 1) for c, r in b) for b in out]


# the 495 combinations of (g = 12, m = 8): 125 unpack points for 330 steps; the lower bound is ceil(792 units / 8 a byte) = 99
CONFIG5_LENGTHS = [n for n in sorted(cases.CLASS_SIZES, reverse=True) for _ in range(cases.CLASS_SIZES[n])]
assert sum(n - 1 for n in CONFIG5_LENGTHS) == 330 and sum(r + 1 for n in CONFIG5_LENGTHS for r in range(n - 1)) == 792
assert sum(f for c, r, f in unpack_flags(CONFIG5_LENGTHS)) == 125 and all(b <= BYTE for b in batches(CONFIG5_LENGTHS)[1])
assert all(f for c, r, f in unpack_flags(CONFIG5_LENGTHS, batch=0))
# nine units of 30 do not fit a byte: the walk with the bound one unit too high would let a batch reach 270
assert max(sum(UNIT * (r + 1) for c, r in b) for b in batches([2] * 9)[0]) == 240 and 9 * UNIT > BYTE


def batched_sum(seqs, positions, g=cases.G, batch=1):
    """The kernel's arithmetic in the plan's step order (every sequence has a window). Returns (the sum over ``positions``,
    seen): seen["batches"] = per batch {"steps": [(chain, r)], "bound", "top": {"row", "col"}, "low": {"row", "col"}} with the
    largest and the smallest byte of Q at the unpack, seen["flagged_steps"] the steps with a count above 15 as (batch, place in
    the batch), seen["top_cells"] / ["zero_cells"] = per term the (i, j), j <= i, whose byte of Q was at its batch's bound / at 0
    when a batch of more than one step was unpacked."""
    n = len(seqs)
    chains = plan_chains(positions)
    lengths = [len(c) for c in chains]
    flags = unpack_flags(lengths, batch)
    total = np.zeros((n, n), dtype=np.int64)
    acc = np.zeros((n, n), dtype=np.int64)
    q = {"row": np.zeros((n, n), dtype=np.int64), "col": np.zeros((n, n), dtype=np.int64)}
    lower = np.tril(np.ones((n, n), dtype=bool))
    seen = {"batches": [], "flagged_steps": [], "top_cells": {"row": set(), "col": set()}, "zero_cells": {"row": set(), "col": set()}}
    cur, wsum, s = [], 0, 0
    for ci, chain in enumerate(chains):
        length = len(chain)
        c_lo = packed.counts(seqs, positions[chain[0]], g)
        total += length * (c_lo @ c_lo.T)
        r_sum = {"row": np.zeros((n, n), dtype=np.int64), "col": np.zeros((n, n), dtype=np.int64)}   # R restarts at a chain base; Q does not
        for u in range(length - 1):
            assert flags[s][:2] == (ci, u)
            delta, sigma = packed.edge_keys(seqs, positions[chain[u]], positions[chain[u + 1]], g)
            c_up = packed.counts(seqs, positions[chain[u + 1]], g)
            if c_lo.max() > 15 or c_up.max() > 15:
                seen["flagged_steps"].append((len(seen["batches"]), len(cur)))
            d = {"row": (c_up & 15)[:, sigma] + (~(c_up & 15)[:, delta] & 15),          # [i, j]: row i's counts at column j's keys
                 "col": ((c_lo & 15)[:, sigma] + (~(c_lo & 15)[:, delta] & 15)).T}      # [i, j]: column j's counts at row i's keys
            for name in ("row", "col"):
                assert d[name].min() >= 0 and d[name].max() <= UNIT
                r_sum[name] += d[name]
                assert r_sum[name].max() <= UNIT * (u + 1) <= BYTE, "a prefix sum leaves its byte"
                q[name] += r_sum[name]
                assert q[name].max() <= BYTE, "a byte of Q wraps inside a batch"
            w = length - 1 - u
            wsum += w
            hi = ((c_up >> 4)[:, sigma] - (c_up >> 4)[:, delta]) + ((c_lo >> 4)[:, sigma] - (c_lo >> 4)[:, delta]).T
            acc = (acc + 16 * w * hi) & 0xffffffff
            cur.append((ci, u))
            if flags[s][2]:
                bound = sum(UNIT * (r + 1) for c, r in cur)
                assert bound <= BYTE
                seen["batches"].append({"steps": cur, "bound": bound, "top": {k: int(v.max()) for k, v in q.items()},
                                        "low": {k: int(v.min()) for k, v in q.items()}})
                for name in ("row", "col"):
                    if len(cur) > 1:
                        seen["top_cells"][name] |= set(zip(*np.nonzero((q[name] == bound) & lower)))
                        seen["zero_cells"][name] |= set(zip(*np.nonzero((q[name] == 0) & lower)))
                    acc = (acc + q[name]) & 0xffffffff
                    q[name][:] = 0
                cur = []
            s += 1
            c_lo = c_up
    assert s == len(flags) and not cur and all(v.max() == 0 for v in q.values())
    assert (2 * max(len(x) - g + 1 for x in seqs) + 32) * wsum < 2 ** 31   # the host's bound (now slightly conservative)
    v = (acc - UNIT * wsum) & 0xffffffff
    total += np.where(v >= 2 ** 31, v - 2 ** 32, v)
    return total, seen


# ---- lists ------------------------------------------------------------------------------------------------------------------------
def mixed_list(positions):
    """What the emulator affords and still has every feature of the walk: the class of nine shifts, a class of eight, a class of
    four and fourteen classes of two. Chains of 9, 8, 4 and fourteen of 2 members: 32 steps. The batches: three steps and five
    single ones of the first chain (the last, 240 of 255, ends exactly at the chain's end), three and three single ones of the
    second, whose last step shares its batch with the third chain's first, the third chain's other two steps with three
    one-step chains (a batch that spans four chains), eight one-step chains (8 x 30 = 240), and a partial last batch of three."""
    shape = lambda pos: tuple(p - pos[0] for p in pos)
    by = {}
    for c, pos in enumerate(positions):
        by.setdefault(shape(pos), []).append(c)
    ids = by[(0, 1, 2, 3)] + by[(0, 1, 2, 4)] + by[(0, 1, 2, 8)]
    twos = [v for k, v in sorted(by.items()) if len(v) == 2][:14]
    assert len(by[(0, 1, 2, 3)]) == 9 and len(by[(0, 1, 2, 4)]) == 8 and len(by[(0, 1, 2, 8)]) == 4 and len(twos) == 14
    ids = np.array(ids + [c for v in twos for c in v], dtype=np.int32)
    lengths = [len(c) for c in plan_chains([positions[c] for c in ids])]
    assert lengths == [9, 8, 4] + [2] * 14
    got, bounds = batches(lengths)
    assert [len(b) for b in got] == [3, 1, 1, 1, 1, 1, 3, 1, 1, 1, 2, 5, 8, 3], [len(b) for b in got]
    assert got[5] == [(0, 7)] and got[10] == [(1, 6), (2, 0)] and got[11] == [(2, 1), (2, 2), (3, 0), (4, 0), (5, 0)]
    assert bounds[10:] == [240, 240, 240, 90]
    return ids


def rank_list(rank, ranks):
    """The combinations of one rank of a combo-sharded run: every ``ranks``-th id."""
    return np.arange(cases.N_COMBOS, dtype=np.int32)[rank::ranks]


def one_step_list(positions):
    """Two neighbouring shifts of the class of nine: one chain of one step. The flag on the last step is the only one."""
    ids = packed.span4(positions)[3:5]
    assert [f for c, r, f in unpack_flags([len(c) for c in plan_chains([positions[c] for c in ids])])] == [True]
    return ids


def cut_flags(port):
    """g = 14, m = 10 (packed.cut_list): chains of 9, 9, 2 and three of 1. A batch ends in the middle of a chain (behind position
    2 .. 6 of either long chain) and one ends exactly at a chain's last step (position 7, 240 of 255: nothing else fits)."""
    ids, plist = packed.cut_list(port)
    lengths = [len(c) for c in plan_chains(plist)]
    assert lengths == [9, 9, 2, 1, 1, 1]
    flags = unpack_flags(lengths)
    assert [(c, r) for c, r, f in flags if f] == [(0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (2, 0)]
    return ids, plist


# ---- RUN / PLUS / MINUS at every in-tile position -----------------------------------------------------------------------------------
# (tests/dense_shift_packed_cases.py) Against RUN a term of PLUS is + 15 at every step of the class of nine shifts: D' = 30 at
# every step, R_r = 30 (r + 1), and a byte of Q is AT the bound of every one of its batches {0, 1, 2}, {3}, {4}, {5}, {6}, {7}:
# 180, 120, 150, 180, 210, 240 — the largest byte of Q over the run is 240. A term of MINUS is - 15: D' = 0 and Q stays 0.
# lanes.everywhere puts the three types at every in-tile position, as a row and as a column.
#
# Over all 495 combinations the same inputs hold the first six batches (the chain of nine comes first in the plan) at these
# values. The other 119 of the 125 batches belong to other shapes, under which PLUS against RUN is no longer + 15 at every step,
# and stay short of what the walk permits them: the batches of the three classes of eight shifts by 3 to 4 % (116 of 120, 145 of
# 150, 174 of 180, 232 of 240), and the shortest the batches of eight one-step chains (batches 120 .. 122 of the plan): 184 of
# 240, 23 a step where 30 are allowed. No input here takes those to their bound — a term of + 15 under eight different shapes at
# once would need a sequence built for each — so the full byte is shown on the chain of nine only; ``shortfall`` lists every
# batch with what it reached, the device test prints it, and the walk is the same bound for all of them.
SPAN4_BOUNDS = [180, 120, 150, 180, 210, 240]


def extremes_facts(seen):
    """From batched_sum's report over lanes.everywhere: the leading batches reach their bound and 0 in both terms; the cells that
    do so in a batch of several steps sit at even and at odd nibbles of the dword the term reads (the row's for the row term,
    the column's for the column term)."""
    head = seen["batches"][:len(SPAN4_BOUNDS)]
    assert [b["bound"] for b in head] == SPAN4_BOUNDS and [len(b["steps"]) for b in head] == [3, 1, 1, 1, 1, 1]
    for b in head:
        assert b["top"] == {"row": b["bound"], "col": b["bound"]} and b["low"] == {"row": 0, "col": 0}, b
    for name, side in (("row", 0), ("col", 1)):
        for cells in (seen["top_cells"][name], seen["zero_cells"][name]):
            assert {lanes.nibble(int(c[side]) % TILE) & 1 for c in cells} == {0, 1}
    return max(max(b["top"].values()) for b in seen["batches"])


def shortfall(seen):
    """Per batch behind the leading six: (bound, the largest byte of Q reached) where the two differ."""
    return [(i, b["bound"], max(b["top"].values())) for i, b in enumerate(seen["batches"]) if max(b["top"].values()) != b["bound"]]
