"""Inputs and numpy yardsticks of the dense tile kernels' loop edges (fsk_tile_kernel_dma.inc: k_dense_tile_dma, _compact,
k_dense_tile_small, _small_compact), shared by tests/test_emu_tile_edges.py and tests/test_gpu_tile_edges.py. Nothing here
touches an engine.

Three yardsticks:
  the counts          ``port.raw_counts`` over the case's combinations (the CPU oracle), compared bit for bit;
  the flagged rows    ``flagged_rows``: every sequence's count of every key, in numpy, with the key formula of count_windows /
                      k_dense_count (symbols ranked 0..sigma-1, the first kept position most significant, dword row = key >> 3,
                      panels of 64 sequences) -> for every (panel, combination) the dword rows where a count exceeds 15;
  dense_macs          ``expected_macs``: 8 * 128^2 * (tiles * Vq8 * combos + 3 * sum over (tile, combo) of the flagged rows of
                      the tile's four panels OR-ed), what accumulate_dense and k_dense_remainder_rows state.

``geometry`` mirrors the launch arithmetic of accumulate_dense and of the kernel (Vq8, nst, chunk_slots, slots_per_split);
``assert_edges`` proves from the flagged rows alone that a case reaches the loop edges it names."""
from math import comb

import numpy as np

PANEL, TILE, STAGE_KQ, DMA_ROWS, MAXF = 64, 128, 32, 16, 4

FORMS = {   # tuning of the tile launch; "store": one workgroup a tile after reset_counts() (the storing flush)
    "one": {"tile_splits": 1, "dense_small": 0},
    "atomics": {"tile_splits": 2, "dense_small": 0},
    "staged": {"tile_splits": 2, "dense_small": 1},
    "store": {"tile_splits": 1, "dense_small": 0},
}

# name: sigma, g, m, L, compact, planted low-complexity sequences (index modulo N, so that -1 is the last sequence; period),
# places of the rare fifth symbol (sequence, position), the edges the case must reach, the forms whose split must cross a chunk
CASES = {
    # 256 keys, 32 rows, nst 1, 1820 combinations against chunk_slots 1024
    "A": dict(sigma=4, g=16, m=12, L=40, compact=0, plant=[(5, [1]), (40, [2]), (-1, [4])],
              edges=("row_lo16", "row_hi16", "last_row"), cross=("one", "store")),
    # 4096 keys, 512 rows, nst 16, 84 combinations against 64
    "B": dict(sigma=4, g=9, m=3, L=40, compact=0, plant=[(5, [1]), (40, [2]), (200, [3]), (-1, [4])],
              edges=("row_lo16", "row_hi16", "word_above_0", "last_row"), cross=("one", "store")),
    # 16,384 keys, 2048 rows, nst 64 (k_dense_count's srowmask[64] exactly full), 36 combinations against 16, 18 a split
    "C": dict(sigma=4, g=9, m=2, L=40, compact=0, plant=[(5, [1]), (40, [2]), (-1, [4])],
              edges=("row_lo16", "row_hi16", "word_above_0", "last_row", "word_63"), cross=("one", "atomics", "staged", "store")),
    # 243 keys, 31 rows: the second stage of every combination has 15 rows (the clamped load, an odd trip count)
    "D": dict(sigma=3, g=9, m=4, L=40, compact=0, plant=[(5, [1]), (40, [2]), (-1, [3])],
              edges=("stage_tail", "last_row"), cross=()),
    # four letters and a rare fifth, 625 keys, nst 3: chunk_slots = min(960 / 6, 64) = 64, the ROW_SLOTS cap, 70 combinations.
    # Tile (1, 0): poly-1 only among its rows (128), poly-2 only among its columns (5), poly-4 on both sides (129 and 70)
    "E": dict(sigma=5, g=8, m=4, L=40, compact=1, plant=[(128, [1]), (5, [2]), (129, [4]), (70, [4])],
              rare=[(20, 7), (90, 30), (100, 0), (127, 39)], edges=("sides",), cross=("one",)),
    # the same alphabet at k = 5: V = 3125 <= 4096 keys, 391 rows, nst 13: chunk_slots = 960 / 26 = 36, below the cap;
    # 126 combinations, 63 a split
    "F": dict(sigma=5, g=9, m=4, L=40, compact=1, plant=[(5, [1]), (40, [2]), (-1, [4])],
              rare=[(20, 7), (60, 30), (-2, 0)], edges=(), cross=("one", "atomics", "staged")),
    # 256 keys, the periodic patterns of test_emu_many_flagged_rows_in_one_stage: two and three hi-plane rounds of MAXF = 4
    "G": dict(sigma=4, g=8, m=4, L=90, compact=0,
              plant=[(3, [1]), (16, [2]), (29, [3]), (42, [4]), (55, [1, 2]), (68, [3, 4]), (81, [1, 3]), (94, [2, 4]),
                     (107, [1, 2, 3]), (120, [4, 3, 2, 1]), (-1, [2, 1, 1]), (-2, [1, 1, 2, 2])],
              edges=("row_lo16", "row_hi16", "rounds2", "rounds3"), cross=()),
    # 1024 keys, 128 rows, nst 4, six combinations: flagged rows in mask words above 0 at a size the emulator's profile mode affords
    "H": dict(sigma=4, g=6, m=1, L=40, compact=0, plant=[(5, [1]), (40, [2]), (-1, [4])],
              edges=("row_lo16", "row_hi16", "word_above_0", "last_row"), cross=()),
}


def geometry(sigma, k, n_combos, tile_splits, compact):
    """Vq8, nst, chunk_slots, n_splits and slots_per_split as accumulate_dense and the tile kernel compute them."""
    V = sigma ** k
    Vq = (V + 3) // 4
    Vq8 = (Vq + 1) // 2
    nst = (Vq8 + STAGE_KQ - 1) // STAGE_KQ
    chunk_slots = min(max(960 // (2 * nst), 1), 64) if compact else max(1024 // nst, 1)
    n_splits = min(n_combos, tile_splits, 4096)
    slots_per_split = (n_combos + n_splits - 1) // n_splits
    n_splits = (n_combos + slots_per_split - 1) // slots_per_split
    return dict(V=V, Vq8=Vq8, nst=nst, chunk_slots=chunk_slots, n_splits=n_splits, slots_per_split=slots_per_split)


def sequences(sigma, N, L, plant, rare=(), seed=0, low_complexity=True):
    """(N, L) tokens: uniform over the common letters (1..4, or 1..sigma when there is no rare symbol), the planted periodic
    sequences, the rare symbol ``sigma`` at its places."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.integers(1, (sigma - 1 if rare else sigma) + 1, size=(N, L), dtype=np.int32)
    if low_complexity:
        for idx, period in plant:
            X[idx % N] = (period * L)[:L]
    for s, p in rare:
        if not any(s % N == idx % N for idx, _ in plant):
            X[s % N, p] = sigma
    assert set(np.unique(X).tolist()) == set(range(1, sigma + 1))   # (the engine ranks the tokens that occur: token t is rank t - 1)
    return X


def flagged_rows(X, sigma, g, positions):
    """bool [panels padded to an even number][combination][Vq8]: some sequence of the panel counts a key of the dword row more
    than 15 times. ValueError where a count exceeds 255 (that batch would be handed to the sparse dataflow)."""
    N, L = X.shape
    k = len(positions[0])
    V = sigma ** k
    Vq8 = ((V + 3) // 4 + 1) // 2
    panels = (((N + PANEL - 1) // PANEL) + 1) & ~1
    win = np.lib.stride_tricks.sliding_window_view(X.astype(np.int64) - 1, g, axis=1)   # (N, W, g) ranks
    out = np.zeros((panels, len(positions), Vq8), dtype=bool)
    base = np.arange(N, dtype=np.int64)[:, None] * V
    for c, pos in enumerate(positions):
        key = np.zeros(win.shape[:2], dtype=np.int64)
        for p in pos:
            key = key * sigma + win[:, :, int(p)]
        counts = np.bincount((base + key).ravel(), minlength=N * V).reshape(N, V)
        if counts.max() > 255:
            raise ValueError("a count of %d: the batch leaves the dense dataflow" % counts.max())
        high = np.zeros((panels * PANEL, Vq8 * 8), dtype=bool)
        high[:N, :V] = counts > 15
        out[:, c, :] = high.reshape(panels, PANEL, Vq8, 8).any(axis=(1, 3))
    return out


def tiles_of(N, first_test_tile=None):
    """The (ti, tj) of the launch: the lower triangle of 128 x 128 tiles; skip_test_block keeps tj < first_test_tile or tj == ti."""
    T = (N + TILE - 1) // TILE
    return [(ti, tj) for ti in range(T) for tj in range(ti + 1) if first_test_tile is None or tj < first_test_tile or tj == ti]


def tile_flags(F, tiles, side=None):
    """[tile][combination][row]: the flagged rows of the tile's four panels OR-ed (side "A": its two row panels, "B": columns)."""
    a = np.stack([F[2 * ti] | F[2 * ti + 1] for ti, _ in tiles])
    b = np.stack([F[2 * tj] | F[2 * tj + 1] for _, tj in tiles])
    return a if side == "A" else b if side == "B" else a | b


def expected_macs(F, tiles, remainder=True):
    """``remainder``: with the flagged rows' three extra products a row (counted in profile mode only)."""
    n_combos, Vq8 = F.shape[1], F.shape[2]
    return 8 * TILE * TILE * (len(tiles) * Vq8 * n_combos + (3 * int(tile_flags(F, tiles).sum()) if remainder else 0))


def build(port, name, N=130, low_complexity=True):
    """The case at N sequences: tokens, combinations, the oracle's counts, the flagged rows."""
    from oracle import loader
    spec = CASES[name]
    sigma, g, m = spec["sigma"], spec["g"], spec["m"]
    k = g - m
    n_combos = port.num_combos(g, m)
    assert n_combos == comb(g, m)
    X = sequences(sigma, N, spec["L"], spec["plant"], spec.get("rare", ()), seed=sum(map(ord, name)) * 1000 + N, low_complexity=low_complexity)
    tok, off = loader.flatten([row.tolist() for row in X])
    combos = np.arange(n_combos, dtype=np.int32)
    positions = [port.combo_positions(g, k, int(c)) for c in combos]
    F = flagged_rows(X, sigma, g, positions)
    want = port.raw_counts(tok, off, g, m, combos, threads=4)[0]
    for a in (F, want, tok, off):
        a.setflags(write=False)
    return dict(spec, name=name, N=N, k=k, X=X, tok=tok, off=off, combos=combos, positions=positions, F=F, want=want)


def assert_edges(case, geo, form, tiles):
    """From the yardstick's flagged rows alone: the case, launched in this form, reaches every loop edge it names."""
    F, Vq8, cs, sps = case["F"], geo["Vq8"], geo["chunk_slots"], geo["slots_per_split"]
    n_combos = F.shape[1]
    assert F.shape[2] == Vq8
    tf = tile_flags(F, tiles)
    assert tf.any(), "no flagged row at all"
    # ---- chunk crossing: every workgroup (tile, split) whose range is longer than a chunk has a flagged row in the last
    # slot of its first chunk, in the first slot of its second (in that slot's first 16-row stage for some tile: the stage
    # loaded from cold) and in its last chunk
    assert (sps > cs) == (form in case["cross"]), "slots_per_split %d against chunk_slots %d" % (sps, cs)
    if form in case["cross"]:
        restart = False
        for s0 in range(0, n_combos, sps):
            s1 = min(s0 + sps, n_combos)
            if s1 - s0 <= cs:
                continue   # (a shorter last split)
            last0 = s0 + (s1 - s0 - 1) // cs * cs
            for t in range(len(tiles)):
                assert tf[t, s0 + cs - 1].any(), "no flagged row in the last slot of chunk 0"
                assert tf[t, s0 + cs].any(), "no flagged row in the first slot of chunk 1"
                assert tf[t, last0:s1].any(), "no flagged row in the last chunk"
                restart = restart or tf[t, s0 + cs, :DMA_ROWS].any()
        assert restart, "no flagged row in the first stage after a chunk restart"
    rows = np.flatnonzero(tf.any(axis=(0, 1)))
    edges = case["edges"]
    if "row_lo16" in edges:
        assert (rows % 32 < 16).any()
    if "row_hi16" in edges:
        assert (rows % 32 >= 16).any()
    if "word_above_0" in edges:
        assert ((rows >= 32) & (rows % 32 < 16)).any() and ((rows >= 32) & (rows % 32 >= 16)).any()
    if "last_row" in edges:
        assert Vq8 - 1 in rows
    if "word_63" in edges:
        assert geo["nst"] == 64 and Vq8 == 2048 and 2047 in rows
    if "stage_tail" in edges:
        tail0 = Vq8 // DMA_ROWS * DMA_ROWS
        assert 0 < Vq8 - tail0 < DMA_ROWS and (Vq8 - tail0) % 2 == 1 and (rows >= tail0).any()
    if "rounds2" in edges or "rounds3" in edges:
        pad = np.zeros(tf.shape[:2] + ((Vq8 + DMA_ROWS - 1) // DMA_ROWS * DMA_ROWS,), dtype=bool)
        pad[:, :, :Vq8] = tf
        per_stage = pad.reshape(tf.shape[0], n_combos, -1, DMA_ROWS).sum(axis=3)
        assert ((per_stage > MAXF) & (per_stage <= 2 * MAXF)).any(), "no stage of 5..8 flagged rows"
        assert (per_stage > 2 * MAXF).any(), "no stage of 9 or more flagged rows"
    if "sides" in edges:
        t = tiles.index((1, 0))
        a, b = tile_flags(F, tiles, "A")[t], tile_flags(F, tiles, "B")[t]
        assert (a & ~b).any() and (b & ~a).any() and (a & b).any()
