"""Inputs and numpy preconditions for the straight chains of the packed shift corrections (fsk_kernels_dense_shift.h:
k_dense_shift_packed<true, true, true>; tuning dense_shift_straight), shared by tests/test_emu_dense_shift_straight.py and
tests/test_gpu_dense_shift_straight.py. Nothing here touches an engine. tests/dense_shift_ahead_cases.py has the schedule this
is a form of and the planted count of 12 .. 16 .. 12 (PEAK16).

The kernel's loop runs over chains. A chain none of whose steps meets a count above 15 in the tile takes the straight path: the
prefetch at its head, then lookups and, between steps, barrier - update - barrier, carrying a step counter, the ring position
and the unpack bits; every other chain runs the step loop of the ahead schedule, and both end in the same hand-over. What it
can get wrong: the test that picks the path (it must see every step of the chain, on both sides of the tile), what the straight
path carries (the unpack bit of step r, the update between steps, the prefix sums' restart), and the hand-over between the two
paths in either direction (the buffer, the ring half, the prefetch a flagged chain lost).

The plan orders chains longest first (a stable sort), so a chain of one step can never stand between two longer ones; the
nearest lists there are: a long chain, a one-step chain and a further one-step chain (``long_one_one``), and the same with the
flagged chain in front."""
import numpy as np

import dense_shift_ahead_cases as ahead
import dense_shift_batch_cases as batch
import dense_shift_cases as cases
import dense_shift_inplace_cases as inplace
import dense_shift_packed_cases as packed

TILE = cases.TILE
TUNING = dict(ahead.TUNING)       # {"tile_splits": 1, "dense_shift": 1, "dense_shift_packed": 0}
STRAIGHT = (1, 0)                 # dense_shift_straight: clean chains straight, and every chain by the ahead schedule's step loop
PEAK16 = ahead.PEAK16             # AAAA counts 12 .. 16 .. 12 under the nine shifts of (0, 1, 2, 3): only shift 4 is above 15

# place -> (the members of the class of nine shifts the list takes, the steps of that chain that must be flagged). A sub-list
# [a, b) of the class has the steps u: shift a + u -> a + u + 1, and the flagged ones are those that touch shift 4.
PLACES = {
    "first": (slice(4, 9), [0]),        # four steps, the first flagged
    "middle": (slice(1, 8), [2, 3]),    # six steps, the third and the fourth flagged
    "last": (slice(0, 5), [3]),         # four steps, the last flagged
}
WHERE = ("between", "first_in_call", "last_in_call")


def n_members(place):
    return len(range(*PLACES[place][0].indices(9)))


def placed_list(positions, place, where):
    """The flagged chain of ``place`` (part of the class of nine shifts) with clean chains around it:
    "between": a class of eight in front (longer: it comes first in the plan), a class of four and two classes of two behind it:
               straight -> generic -> straight, and the chains behind must find their planes and offsets;
    "first_in_call": without the class of eight: the call's first chain is the flagged one;
    "last_in_call": the class of eight in front and nothing behind: the flagged chain has no successor.
    -> (ids, the flagged chain's place in the plan)."""
    by = ahead.by_shape(positions)
    part = list(packed.span4(positions)[PLACES[place][0]])
    twos = [v for k, v in sorted(by.items()) if len(v) == 2][:2]
    behind = by[(0, 1, 2, 8)] + [c for v in twos for c in v]
    front = by[(0, 1, 2, 4)]
    ids = {"between": front + part + behind, "first_in_call": part + behind, "last_in_call": front + part}[where]
    ids = np.array(ids, dtype=np.int32)
    lengths = [len(c) for c in batch.plan_chains([positions[c] for c in ids])]
    n = n_members(place)
    assert 4 < n < 8
    want = {"between": [8, n, 4, 2, 2], "first_in_call": [n, 4, 2, 2], "last_in_call": [8, n]}[where]
    assert lengths == want, lengths
    return ids, (0 if where == "first_in_call" else 1)


def two_step_list(positions):
    """Three neighbouring shifts of the class of nine: one chain of two steps (one update, one barrier pair)."""
    return packed.span4(positions)[5:8]


def long_one_one(positions):
    """The class of nine shifts and two classes of two: a chain of eight steps, then two chains of one step (head, lookups and
    tail with nothing in between), the second without a successor."""
    by = ahead.by_shape(positions)
    twos = [v for k, v in sorted(by.items()) if len(v) == 2][:2]
    ids = np.array(list(packed.span4(positions)) + [c for v in twos for c in v], dtype=np.int32)
    assert [len(c) for c in batch.plan_chains([positions[c] for c in ids])] == [9, 2, 2]
    return ids


def one_side(which, n=inplace.CROSSING_N, seed=45):
    """PEAK16 planted in tile row 1 only (the places of inplace.CROSSING_AT that lie there), four tile rows: tile (1, 0) is
    flagged on its ROW side only, tiles (2, 1) and (3, 1) on their COLUMN side only, tile (1, 1) on both, every other tile on
    neither. -> (sequences, the planted places)."""
    at = [x for x in inplace.CROSSING_AT if x // TILE == 1]
    assert len(at) == 2 and n == 4 * TILE - 126
    seqs = cases.uniform(n, 40, seed)
    for x in at:
        seqs[x] = list(which)
    return seqs, at


def flagged_by_tile_row(seqs, plist):
    """Per tile row, the (chain, step) of the plan at which one of its sequences has a count above 15."""
    rows = (len(seqs) + TILE - 1) // TILE
    return [ahead.flagged_steps(seqs[t * TILE:(t + 1) * TILE], plist) for t in range(rows)]
