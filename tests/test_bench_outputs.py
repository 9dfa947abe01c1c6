"""bench.py's --dump-outputs helpers (no GPU needed): the sampled cells are the same from run to run, lie in the
triangle and map back to their (row, col); the top-left block is the symmetric square of the triangle's first cells."""
import os

import numpy as np
import pytest

from conftest import tri_to_square


@pytest.fixture
def bench(monkeypatch):
    # (importing bench sets HSA_ENABLE_IPC_MODE_LEGACY for its own process: keep it out of this one)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    return bench


@pytest.mark.parametrize("N", [1, 7, 1000, 1500, 100000])
def test_sample_cells_are_fixed_and_in_the_triangle(bench, N):
    pairs = N * (N + 1) // 2
    cells, rows, cols = bench.sample_cells(pairs)
    again = bench.sample_cells(pairs)
    assert all(np.array_equal(a, b) for a, b in zip((cells, rows, cols), again))
    assert len(cells) == min(pairs, bench.DUMP_CELLS)
    if pairs <= bench.DUMP_CELLS:
        assert np.array_equal(cells, np.arange(pairs))
    assert (np.diff(cells) > 0).all() and cells[0] >= 0 and cells[-1] < pairs
    assert (cols >= 0).all() and (cols <= rows).all() and (rows < N).all()
    assert np.array_equal(rows * (rows + 1) // 2 + cols, cells)


def test_tri_head_square(bench):
    rng = np.random.Generator(np.random.PCG64(7))
    tri = rng.random(50 * 51 // 2)
    nb = 20
    assert np.array_equal(bench.tri_head_square(tri[:nb * (nb + 1) // 2], nb), tri_to_square(tri, 50)[:nb, :nb])
