"""Inputs and numpy yardsticks of the dense dataflow by shift classes (fsk_engine_dense_shift.hip: dense_shift_plan,
k_dense_edge_keys, k_dense_tile_shift, k_dense_shift_fix), shared by tests/test_emu_dense_shift.py and
tests/test_gpu_dense_shift.py. Nothing here touches an engine.

The identity. Kept-position sets that differ only by a translation t of all kept positions form a class. The k-mer that
window w shows under shift t is the k-mer at absolute start w + t under shift 0, so from shift t to t + 1 a sequence's count
vector loses the key of its first window under t (delta) and gains the key of its last window under t + 1 (sigma):

    c_{t+1} = c_t + d_t,   d_t = e(sigma_t) - e(delta_t)
    G_{t+1}(i, j) = G_t(i, j) + [c_{t+1,i}(sigma_j) - c_{t+1,i}(delta_j)] + [c_{t,j}(sigma_i) - c_{t,j}(delta_i)]
    sum_{t = t0..t1} G_t = n G_{t0} + sum_{u = t0}^{t1 - 1} (t1 - u) (G_{u+1} - G_u),   n = t1 - t0 + 1

``identity_sum`` evaluates the right-hand sides in numpy, chain by chain (one Gram product a chain, four count lookups a cell
and further shift); ``direct_sum`` is the sum over every combination. tests/test_emu_dense_shift.py holds them against each
other and against the CPU oracle on ragged lengths. The engine's counts are compared bit for bit with ``port.raw_counts``.

``chains`` is the plan: combinations grouped by shape (kept positions minus the first), sorted by shift inside a shape, cut
into runs of consecutive shifts. ``expected_macs``: 8 * 128^2 * tiles * Vq8 * slots multiplied — with the number of chain
bases on the shift path, with every combination of the call on the old one."""
import numpy as np

SIGMA, G, M, K = 4, 12, 8, 4
N = 130                      # three tiles, the last with two real rows
V, VQ8, TILE, PANEL = 256, 32, 128, 64
N_COMBOS = 495
TUNING = {"tile_splits": 1, "dense_shift": 1}
CLASS_SIZES = {9: 1, 8: 3, 7: 6, 6: 10, 5: 15, 4: 21, 3: 28, 2: 36, 1: 45}   # shifts of a class: classes


def all_positions(port):
    return [tuple(int(p) for p in port.combo_positions(G, K, c)) for c in range(N_COMBOS)]


def chains(positions):
    """positions: the kept positions of a call's combinations, in call order -> chains of places in the call."""
    shapes = {}
    for q, pos in enumerate(positions):
        shapes.setdefault(tuple(p - pos[0] for p in pos), []).append((pos[0], q))
    out = []
    for members in shapes.values():
        members.sort(key=lambda sq: sq[0])   # (stable: a repeated id keeps its call order)
        for i, (shift, q) in enumerate(members):
            if i == 0 or shift != members[i - 1][0] + 1:
                out.append([])
            out[-1].append(q)
    return out


def expected_macs(n_tiles, slots):
    return 8 * TILE * TILE * n_tiles * VQ8 * slots


def n_tiles(n=N):
    t = (n + TILE - 1) // TILE
    return t * (t + 1) // 2


# ---- the numpy yardstick of the identity ----------------------------------------------------------------------------------------
def _key(x, start, pos):
    key = 0
    for p in pos:
        key = key * SIGMA + int(x[start + p]) - 1
    return key


def count_vector(x, pos):
    c = np.zeros(V, dtype=np.int64)
    for w in range(len(x) - G + 1):
        c[_key(x, w, pos)] += 1
    return c


def direct_sum(seqs, positions):
    total = np.zeros((len(seqs), len(seqs)), dtype=np.int64)
    for pos in positions:
        C = np.stack([count_vector(x, pos) for x in seqs])
        total += C @ C.T
    return total


def identity_sum(seqs, positions):
    """One Gram product a chain; every further shift from the two edge keys of every sequence."""
    n = len(seqs)
    total = np.zeros((n, n), dtype=np.int64)
    rows = np.arange(n)
    for chain in chains(positions):
        length = len(chain)
        C = np.stack([count_vector(x, positions[chain[0]]) for x in seqs])
        total += length * (C @ C.T)
        for u in range(length - 1):
            lower, upper = positions[chain[u]], positions[chain[u + 1]]
            has = np.array([len(x) >= G for x in seqs])
            delta = np.array([_key(x, 0, lower) if len(x) >= G else 0 for x in seqs])
            sigma = np.array([_key(x, len(x) - G, upper) if len(x) >= G else 0 for x in seqs])
            Cn = C.copy()
            Cn[rows[has], delta[has]] -= 1
            Cn[rows[has], sigma[has]] += 1
            assert all(np.array_equal(Cn[i], count_vector(seqs[i], upper)) for i in (0, n - 1))
            # (a sequence without a window: delta = sigma = 0, which contributes nothing)
            D = (Cn[:, sigma] - Cn[:, delta]) + (C[:, sigma] - C[:, delta]).T
            total += (length - 1 - u) * D
            C = Cn
    return total


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def uniform(n=N, L=40, seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [row.tolist() for row in rng.integers(1, SIGMA + 1, size=(n, L), dtype=np.int32)]


RAGGED = (12, 13, 14, 19, 20, 40)   # one window .. nine windows (the edges overlap), plenty; the engine refuses L < g


def ragged(n=N, seed=6):
    """Every length of RAGGED in every tile row (sequences 0.., 57.., 64.., 121..) and in the last tile's two rows."""
    seqs = uniform(n, 40, seed)
    at = {}
    for base in (0, 57, 64, 121):
        for i, L in enumerate(RAGGED):
            at[base + i] = L
    at[n - 2], at[n - 1] = 13, 12
    at[n - 3] = 19
    for i, L in at.items():
        seqs[i] = seqs[i][:L]
    return seqs


PLANTS = {   # which tile sides of tile (1, 0) hold counts above 15: its rows are sequences 128 and 129, its columns 0 .. 127
    "rows": {128: [1], 129: [2, 3]},
    "cols": {5: [4], 70: [1, 2]},
    "both": {128: [1], 129: [2, 3], 5: [4], 70: [1, 2]},
}


def planted(which, n=N, L=90, seed=7):
    """Homopolymers and period-2 sequences of 79 windows among uniform ones."""
    seqs = uniform(n, L, seed)
    for i, period in PLANTS[which].items():
        seqs[i] = (period * L)[:L]
    return seqs


def high_panels(seqs, positions):
    """The panels (64 sequences) in which some sequence counts a key above 15 under some combination; the largest count."""
    out, top = set(), 0
    for i, x in enumerate(seqs):
        m = max(int(count_vector(x, pos).max()) for pos in positions)
        top = max(top, m)
        if m > 15:
            out.add(i // PANEL)
    return out, top


def long_homopolymer(n=N, seed=8):
    """One sequence of 289 windows of one key: a count above 255 sends the batch to the sparse dataflow."""
    seqs = uniform(n, 40, seed)
    seqs[77] = [3] * 300
    return seqs


def lists(positions, seed=9):
    """The combination lists of a call: name -> ids."""
    rng = np.random.Generator(np.random.PCG64(seed))
    subset = np.sort(rng.choice(N_COMBOS, size=100, replace=False)).astype(np.int32)
    shuffled = subset.copy()
    rng.shuffle(shuffled)
    span4 = [c for c, pos in enumerate(positions) if tuple(p - pos[0] for p in pos) == (0, 1, 2, 3)]   # the class of nine shifts
    assert len(span4) == 9
    return {
        "subset": subset,
        "shuffled": shuffled,
        "one": np.array([123], dtype=np.int32),
        "gap": np.array(span4[:4] + span4[5:], dtype=np.int32),
        "repeated": np.array(span4[:3] + [span4[1]] + span4[3:6], dtype=np.int32),
    }


def small_list(positions):
    """Three whole classes (nine, eight and eight shifts) and two lone combinations: what the emulator affords on three tiles."""
    want = {(0, 1, 2, 3), (0, 1, 2, 4), (0, 2, 3, 4)}
    ids = [c for c, pos in enumerate(positions) if tuple(p - pos[0] for p in pos) in want]
    assert len(ids) == 25
    return np.array(ids + [200, 400], dtype=np.int32)
