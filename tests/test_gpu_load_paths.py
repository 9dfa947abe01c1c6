"""fsk_load_sequences with token ids beyond the byte table on the GPU: the general packing regime fills the same pinned
staging as the byte-table one and goes up by the same asynchronous copies, so a second load right behind the first has to
wait for the first one's upload (stage_in_flight) before it refills the staging. The integer counts must be the oracle's
for the same sequences rank-remapped to ids 0 .. sigma - 1 (the remap preserves equality: the same kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, M = 6, 2
FIVE_IDS = [1, 7, 300, 70000, 2 ** 20 + 5]      # distinct values by sort, ranks by binary search
MANY_IDS = list(range(44, 301))                 # 257 ids up to 300: the seen-table and the direct table, 16 bits a symbol


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build_engine()    # no-op when fastsk_amd/lib/libfastsk_amd.so is current
    ge.build_bindings()
    from fastsk_amd import _native
    _native.library()    # raises if the HIP library is missing: no fallback
    return _native


def ragged_set(ids, seed, n=24):
    """n sequences of 12 .. 40 tokens in which every id occurs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = rng.integers(12, 41, size=n)
    lens[:2] = (12, 40)
    tokens = rng.choice(ids, size=int(lens.sum()))
    assert len(tokens) >= len(ids)
    tokens[rng.permutation(len(tokens))[:len(ids)]] = ids
    return tokens.astype(np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("ids", [FIVE_IDS, MANY_IDS], ids=["five_wide_ids", "257_ids_to_300"])
def test_general_regime_load_behind_a_load(native, port, ids, path):
    first, second = ragged_set(ids, 1), ragged_set(ids, 2)
    assert not np.array_equal(first[0][:100], second[0][:100])
    combos = np.arange(port.num_combos(G, M), dtype=np.int32)
    ranks = np.searchsorted(ids, second[0]).astype(np.int32)
    assert np.array_equal(np.asarray(ids)[ranks], second[0]) and len(np.unique(ranks)) == len(ids)
    want = port.raw_counts(ranks, second[1], G, M, combos, threads=8)[0]
    e = native.Engine(G, M, path=path)
    e.load_sequences(first[0], first[1], 16, 8)
    e.load_sequences(second[0], second[1], 16, 8)   # at once: the first upload may still read the staging
    e.accumulate(combos)
    e.finalize()
    st = e.stats()
    assert st["alphabet"] == len(ids) and st["bits_per_symbol"] == (4 if len(ids) == 5 else 16)
    assert np.array_equal(e.get_counts(), want)
    e.close()
