"""Inputs and numpy preconditions for the ahead schedule of the packed shift corrections (fsk_kernels_dense_shift.h:
k_dense_shift_packed<true, true>; fsk_engine_dense_shift.hip: dense_shift_chain_table; tuning dense_shift_ahead), shared by
tests/test_emu_dense_shift_ahead.py and tests/test_gpu_dense_shift_ahead.py. Nothing here touches an engine.
tests/dense_shift_inplace_cases.py has the in-place form this is a schedule of, tests/dense_shift_batch_cases.py the plan's
chain order and the unpack flags.

At a chain's first step the kernel stages the NEXT chain's first planes into the idle stage buffer and the next chain's key
offsets into the idle half of an offsets ring, and makes every step's slots, weight and flags from a chain table. What it can
get wrong: the chain table (a chain's length, the slots and the weight of step r, the unpack flags), which chain is the next and
that the last has none, the ring half a chain reads, the hand-over when a chain has one step (its first step is its last), and
the prefetch that a flagged step overwrites: a step that meets a count above 15 in its tile, and the step behind it, are staged
as before — into the buffer that holds the prefetch — and the chain's end must then stage the next chain's start the old way.
``flagged_steps`` states in numpy where an input's flagged steps fall in the plan."""
import numpy as np

import dense_shift_batch_cases as batch
import dense_shift_cases as cases
import dense_shift_inplace_cases as inplace
import dense_shift_lanes_cases as lanes
import dense_shift_packed_cases as packed

TILE = cases.TILE
TUNING = dict(inplace.TUNING)     # {"tile_splits": 1, "dense_shift": 1, "dense_shift_packed": 0}
AHEAD = (1, 0)                    # dense_shift_ahead: the ahead schedule, and the schedule before (every chain start one step ahead)

# packed.CROSSING with ten A instead of twelve in front: AAAA counts 12 .. 16 .. 12 under the nine shifts of (0, 1, 2, 3): only
# the slot of shift 4 holds a count above 15, so of the class's eight steps exactly steps 3 (its upper slot) and 4 (its lower
# slot) are flagged, and a sub-list of the class puts the flagged step where a case wants it.
PEAK16 = [4] * 4 + [1] * 10 + [4] * 2 + [2, 3, 4, 2] * 7 + [1] * 12 + [4] * 4
PEAK16_COUNTS = [12, 13, 14, 15, 16, 15, 14, 13, 12]
assert len(PEAK16) == 60

# place -> (the members of the class of nine shifts the list takes, (chain, step) of the plan that must be flagged in the tiles
# of the planted sequences, what the case is about)
PLACES = {
    # the chain of five comes first: its first step is flagged, nothing is prefetched, step 1 is staged as before
    "first": (slice(4, 9), [(0, 0)]),
    # the whole class first: the prefetch is issued at step 0, steps 1 and 2 are made in place, step 2 stages step 3 over the
    # prefetch, steps 3 and 4 run the hi pass, step 5 is staged, 6 and 7 are made in place again, the end stages the next start
    "middle": (slice(0, 9), [(0, 3), (0, 4)]),
    # the chain of five first: steps 0 and 1 in place under the prefetch, step 2 stages the flagged last step over it
    "last": (slice(0, 5), [(0, 3)]),
    # a class of eight first, then the chain of five whose FIRST step is flagged: the prefetch stages a flagged step's planes
    "next_first": (slice(4, 9), [(1, 0)]),
}


def by_shape(positions):
    out = {}
    for c, pos in enumerate(positions):
        out.setdefault(tuple(p - pos[0] for p in pos), []).append(c)
    return out


def placed_list(positions, place):
    """The list of a PLACES case: part of the class of nine shifts, a class of four and a class of two behind it (the chain that
    lost its prefetch is followed by chains that must find their planes and offsets), and for "next_first" a class of eight in
    front."""
    by = by_shape(positions)
    part, _ = PLACES[place]
    twos = [v for k, v in sorted(by.items()) if len(v) == 2][:2]
    ids = list(packed.span4(positions)[part]) + by[(0, 1, 2, 8)] + [c for v in twos for c in v]
    if place == "next_first":
        ids = by[(0, 1, 2, 4)] + ids
    ids = np.array(ids, dtype=np.int32)
    lengths = [len(c) for c in batch.plan_chains([positions[c] for c in ids])]
    n_part = len(range(*part.indices(9)))
    assert lengths == ([8] if place == "next_first" else []) + sorted([n_part, 4], reverse=True) + [2, 2], lengths
    return ids


def flagged_steps(seqs, plist, g=cases.G):
    """(chain, step) of the plan (batch.plan_chains order) at which some sequence of ``seqs`` has a count above 15 under the
    step's lower or upper combination."""
    out = []
    for ci, chain in enumerate(batch.plan_chains(plist)):
        tops = [int(packed.counts(seqs, plist[q], g).max()) for q in chain]
        out += [(ci, u) for u in range(len(chain) - 1) if max(tops[u], tops[u + 1]) > 15]
    return out


def one_chain_list(positions):
    """The class of nine shifts alone: one chain of eight steps, the first and the last chain at once."""
    return packed.span4(positions)


def small_keys(port, g, m, take=None):
    """(ids, kept positions) of the combinations of (g, m) with k = g - m < 4: fewer than 256 keys, a stage of one load a side.
    ``take``: the first classes only, whole (what the emulator affords)."""
    k = g - m
    n = int(round(np.prod([(g - i) / (i + 1) for i in range(k)])))
    pos = [tuple(int(p) for p in port.combo_positions(g, k, c)) for c in range(n)]
    ids = list(range(n))
    if take is not None:
        by = by_shape(pos)
        ids = [c for shape in sorted(by)[:take] for c in by[shape]]
    return np.array(ids, dtype=np.int32), [pos[c] for c in ids]


def vq8(k):
    """dword rows of a count panel: 4^k keys, eight a dword."""
    return (4 ** k + 7) // 8


def expected_macs(n, n_chains, k=cases.K):
    return 8 * TILE * TILE * cases.n_tiles(n) * vq8(k) * n_chains
