"""Inputs and numpy preconditions of the one base launch over all chain-length groups (fsk_tile_kernel_dma.inc with
FSK_DMA_SHIFT 2: k_dense_tile_shift_all; tuning dense_shift_one_launch), shared by tests/test_emu_dense_one_launch.py and
tests/test_gpu_dense_one_launch.py. Nothing here touches an engine. tests/dense_shift_cases.py has the sequences, the lists and
the plan's chains; tests/dense_shift_packed_cases.py the cut of a chain at nine members.

The launch runs the plan's groups in descending chain length n_1 > n_2 > ... and does not clear its sums between them: after
group g they leave multiplied by the weight step d_g = n_g - n_(g+1) (n past the last group = 0), so a base of chain length n
has left sum_{h >= g} d_h = n times at the end. ``groups`` states that table from the chains alone. The first flush of a call
after reset_counts stores every cell (zeros too), every later one adds its non-zero cells: ``stored_zeros`` counts, in numpy,
the cells that are zero under the first group's bases and are added to by a later group — on sequences of 40 letters many
are, so the data itself exercises the stored zero and the add onto it."""
import numpy as np

import dense_shift_cases as cases
import dense_shift_packed_cases as packed

KEYS = (1, -1)   # dense_shift_one_launch: one launch whenever the shift path runs; one launch a group (the parent's)
TUNING = dict(cases.TUNING)

BIG_N, BIG_L, BIG_SEED = 32000, 300, 20201214   # the benchmark's generator at the size where the default rule applies
BIG_KEY = "config5:n_seq=32000,seq_len=300,g=12,m=8,combos=495"
BIG_TILES = 250 * 251 // 2


def plan_chains(plist):
    """The chains of a call as the engine plans them under the packed corrections: cut after nine members."""
    return packed.cut(cases.chains(plist))


def groups(plist):
    """[(end slot, weight step)] of the one launch: bases sorted by chain length, longest first."""
    lengths = sorted((len(c) for c in plan_chains(plist)), reverse=True)
    distinct = sorted(set(lengths), reverse=True)
    out, end = [], 0
    for g, n in enumerate(distinct):
        end += lengths.count(n)
        out.append((end, n - (distinct[g + 1] if g + 1 < len(distinct) else 0)))
    assert end == len(lengths) and sum(d for _, d in out) == distinct[0]
    return out


def one_chain_of_each_length(positions):
    """45 combinations: from the class of nine shifts, eight shifts of the next class, seven of the next ... one of the ninth —
    nine chains of lengths 9 .. 1, so nine groups of one base each and every weight step 1: the full list's group structure
    at a size the emulator affords."""
    shapes = {}
    for c, pos in enumerate(positions):
        shapes.setdefault(tuple(p - pos[0] for p in pos), []).append((pos[0], c))
    full = sorted(shapes.items())
    nine = [s for s, v in full if len(v) == 9]
    eight = [s for s, v in full if len(v) == 8]
    rest = [s for s, v in full if len(v) == 7]
    pick = nine[:1] + eight[:3] + rest[:5]
    assert len(pick) == 9
    ids = []
    for n, shape in zip(range(9, 0, -1), pick):
        members = sorted(shapes[shape])
        ids += [c for _, c in members[:n]]
    assert len(ids) == 45
    return np.array(ids, dtype=np.int32)


def stored_zeros(seqs, plist):
    """(cells j <= i that are zero under the first group's bases, how many of those a later group adds to)."""
    ch = sorted(plan_chains(plist), key=len, reverse=True)
    top = len(ch[0])
    n = len(seqs)
    first = np.zeros((n, n), dtype=np.int64)
    later = np.zeros((n, n), dtype=np.int64)
    for c in ch:
        C = packed.counts(seqs, plist[c[0]], cases.G)
        (first if len(c) == top else later)[...] += C @ C.T
    tri = np.tril(np.ones((n, n), dtype=bool))
    zero = tri & (first == 0)
    return int(zero.sum()), int((zero & (later != 0)).sum())


def bench_sequences():
    """bench.py's config-5 generator: (tokens, offsets)."""
    rng = np.random.Generator(np.random.PCG64(BIG_SEED))
    X = rng.integers(1, 5, size=(BIG_N, BIG_L), dtype=np.int32)
    return X.reshape(-1), np.arange(BIG_N + 1, dtype=np.int64) * BIG_L
