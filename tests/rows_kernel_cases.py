"""Inputs and the numpy yardstick of the rows kernel (fsk_rows_build / fsk_rows_get_block, ``kernel_type="linear"``), shared by
tests/test_emu_rows_kernel.py (CPU emulation) and tests/test_gpu_rows_kernel.py (MI355X). Nothing here touches an engine.

``reference``  L and K2 of include/fastsk_amd.h restated on A = the engine's own ``get_block(0, N, 0, n_train)``: one
               accumulator a cell, ``acc = acc + A[:, i, None] * A[None, :, i]`` for ascending i (vectorised over the cells,
               sequential in i; numpy's elementwise multiply and add are single IEEE operations), then the three operations
               of normalised_cell. Compared bit for bit.
``EDGE_*``     the tile and panel edges as expressions in T and P, which the tests read from the library (tuning keys rows_tile,
               rows_panel)."""
import numpy as np


def sequences(n, seed, lo=20, hi=40):
    """n sequences of lo..hi tokens 1..4 (PCG64), the lengths drawn too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(1, 5, size=int(rng.integers(lo, hi + 1)), dtype=np.int32) for _ in range(n)]


def case(n_train, n_test, seed=None, **engine):
    """Sequences of 20-40 symbols, g = 6, m = 2: a case costs milliseconds."""
    return {"X": sequences(n_train + n_test, 9100 + 7 * n_train + n_test if seed is None else seed), "n_train": n_train, "n_test": n_test,
            "g": 6, "m": 2, "engine": engine}


# The tile and panel edges, as expressions in the tile edge T and the panel depth P the library reports: a lone diagonal tile,
# panels in all three load regimes, a short last panel, a short last tile row, column blocks cut by n_train.
EDGE_N_TRAIN = ("1", "2", "P-1", "P", "P+1", "T-1", "T", "T+1", "2*T+1", "3*T+P+1")
EDGE_N_TEST = ("0", "1", "T+1")


def size_of(expr, T, P):
    return int(eval(expr, {"__builtins__": {}}, {"T": T, "P": P}))


def reference(A, n):
    """A: float64 [N, n], the normalised cells with a train column. -> (L [N, N], K2 [N, N], diag L [N]); the test x test
    off-diagonal cells of L are never computed and read 0.0."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    N = A.shape[0]
    assert A.shape == (N, n) and 1 <= n <= N
    with np.errstate(all="ignore"):
        acc = A[:, 0, None] * A[None, :n, 0]          # cells (r, c < n)
        d = A[:, 0] * A[:, 0]                         # cells (r, r)
        for i in range(1, n):
            acc = acc + A[:, i, None] * A[None, :n, i]
            d = d + A[:, i] * A[:, i]
        L = np.zeros((N, N))
        L[:, :n] = acc
        L[:n, :] = acc.T
        L[np.arange(N), np.arange(N)] = d
        K2 = L / np.sqrt(d[:, None] * d[None, :])
        K2[np.arange(N), np.arange(N)] = d / np.sqrt(d * d)
    assert np.array_equal(acc[np.arange(n), np.arange(n)].view(np.uint64), d[:n].view(np.uint64))
    return L, K2, d


def reference_rows(A_rows, A_train, n):
    """The yardstick on a few rows only (the case past 2^32 cells): A_rows [R, n] are the rows asked for, A_train [n, n] the
    train rows. -> (L(rows, 0..n-1) [R, n], L(row, row) [R])."""
    with np.errstate(all="ignore"):
        acc = A_rows[:, 0, None] * A_train[None, :n, 0]
        d = A_rows[:, 0] * A_rows[:, 0]
        for i in range(1, n):
            acc = acc + A_rows[:, i, None] * A_train[None, :n, i]
            d = d + A_rows[:, i] * A_rows[:, i]
    return acc, d


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
