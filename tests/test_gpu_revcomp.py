"""Reverse-complement mode (fsk_set_complement, ``FastSK(revcomp=...)``) on the MI355X: the product library against the CPU
oracle run on [X ; rc(X)] with the four blocks of its raw counts added (tests/test_emu_revcomp.py states the contract)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_tokens, reference_fasta, synthetic_dna, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests"))

import revcomp_cases as cases  # noqa: E402
from test_emu_revcomp import (check_dense_regime, check_long_sequence, check_narrowing, check_planes, check_products,  # noqa: E402
                              check_update_stages, check_wide_windows)

pytestmark = pytest.mark.gpu

ACGT = {1: 4, 4: 1, 2: 3, 3: 2}   # synthetic_dna: tokens 1..4


@pytest.fixture(scope="module")
def native():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build_engine()    # no-op when fastsk_amd/lib/libfastsk_amd.so is current
    ge.build_bindings()
    from fastsk_amd import _native
    lib = _native.library()  # raises if the HIP library is missing: no fallback
    assert lib.device_count() >= 1
    return _native


THREADS = min(32, os.cpu_count() or 8)


def folded_oracle(port, seqs, comp, g, m, combos, threads=THREADS):
    """``port.raw_counts`` on [X ; rc(X)], the four blocks added -> uint64 lower triangle."""
    from oracle import loader
    n = len(seqs)
    both = [list(s) for s in seqs] + [[comp[int(t)] for t in reversed(list(s))] for s in seqs]
    tok, off = loader.flatten(both)
    tri2, _, _ = port.raw_counts(tok, off, g, m, combos, threads=threads)
    sq = tri_to_square(tri2, 2 * n)
    f = sq[:n, :n] + sq[:n, n:] + sq[n:, :n] + sq[n:, n:]
    return f[np.tril_indices(n)]


def subset_against_fold(port, e, X, idx, comp, g, m, combos):
    """The fold of the oracle on just the sequences ``idx`` == the scattered cells (idx[a], idx[b]) of the big triangle."""
    want = folded_oracle(port, [X[i] for i in idx], comp, g, m, combos)
    a, b = np.tril_indices(len(idx))
    assert np.array_equal(e.get_counts_cells(idx[a], idx[b]), want)
    return want


# ---- 11 -----------------------------------------------------------------------------------------------------------------
def test_dense_and_sparse_equal_the_fold_on_seeded_dna(native, port):
    tokens, offsets = synthetic_dna(700, 300)
    X = tokens.reshape(700, 300)
    combos = np.arange(0, 495, 33, dtype=np.int32)
    want = folded_oracle(port, X, ACGT, 12, 8, combos)
    tris = []
    for path in (1, 2):
        e = native.Engine(12, 8, path=path, revcomp=ACGT)
        e.load_sequences(tokens, offsets, 700, 0)
        e.accumulate(combos)
        e.finalize()
        st = e.stats()
        assert st["path_used"] == path and st["revcomp"] and st["n_feat"] == 2 * 700 * 289 and st["max_windows"] == 578
        assert np.array_equal(e.get_counts(), want), path
        tris.append(e.get_triangle())
        e.close()
    assert np.array_equal(tris[0], tris[1]) and np.array_equal(tris[0], port.normalise(want.astype(np.float64), 700))


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(native, path):
    from test_emu_revcomp import load_revcomp_golden
    tokens, offsets, comp, g, m, counts, tri = load_revcomp_golden()
    e = native.Engine(g, m, path=path, revcomp=comp)
    e.compute(tokens, offsets, 40, 20)
    assert np.array_equal(e.get_counts(), counts) and np.array_equal(e.get_triangle(), tri)
    e.close()


# ---- 12 -----------------------------------------------------------------------------------------------------------------
SPARSE_FORMS = cases.SPARSE_FORMS


def test_sparse_forms_forced_on_dna_k8(native, port):
    """DNA, k = 8 (g = 12, m = 4), N = 12,000: every form of the sparse dataflow's update stage forced by its tuning keys sees
    twice the features and nothing else of this mode — a seeded 350-sequence subset against the fold, one digest for all forms.
    The dense dataflow cannot hold 4^8 keys (count panels: alphabet^k <= 16384), so its digest is compared one position
    shorter, k = 7 (g = 12, m = 5), on the same sequences."""
    N, L, g, m = 12000, 100, 12, 4
    tokens, offsets = synthetic_dna(N, L, seed=812)
    X = tokens.reshape(N, L)
    combos = np.array([0, 247, 494], dtype=np.int32)
    idx = np.sort(np.random.Generator(np.random.PCG64(12)).choice(N, size=350, replace=False))
    digests = {}
    for name, tun, form in SPARSE_FORMS:
        e = native.Engine(g, m, path=2, revcomp=ACGT, tuning=tun)
        e.load_sequences(tokens, offsets, N, 0)
        e.accumulate(combos)
        e.finalize()
        st = e.stats()
        assert st["path_used"] == 2 and st["n_feat"] == 2 * N * (L - g + 1), name
        if form is not None:
            assert st["sparse_form"] == form, name
        if "sparse_desc" in tun:
            assert st["sparse_desc"] == (1 if tun["sparse_desc"] == 1 else 0), name
        subset_against_fold(port, e, X, idx, ACGT, g, m, combos)
        digests[name] = e.counts_digest()
        e.close()
    assert len(set(digests.values())) == 1, digests
    with pytest.raises(native.FskError):   # (what the docstring says about the dense dataflow at k = 8)
        e = native.Engine(g, m, path=1, revcomp=ACGT)
        e.load_sequences(tokens, offsets, N, 0)
    m7 = 5
    combos7 = np.array([0, 400, 791], dtype=np.int32)
    both = []
    for path in (1, 2):
        e = native.Engine(g, m7, path=path, revcomp=ACGT)
        e.load_sequences(tokens, offsets, N, 0)
        e.accumulate(combos7)
        e.finalize()
        assert e.stats()["path_used"] == path
        if path == 1:
            subset_against_fold(port, e, X, idx, ACGT, g, m7, combos7)
        both.append(e.counts_digest())
        e.close()
    assert both[0] == both[1]


# ---- 13 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"devices": [0, 0]}, {"skip_test_block": "lazy"}])
def test_drop_in_class_end_to_end(native, port, tmp_path, kw):
    """FastaUtility -> FastSK(g=10, m=6, revcomp=reader.complement()) -> compute_kernel -> numpy and DLPack getters, a seeded
    subset of rows against the oracle; over two engines on one GPU; with the test x test block left for later."""
    import torch
    from fastsk_amd import FastSK, FastaUtility
    reader = FastaUtility()
    Xtr, _ = reader.read_data(reference_fasta("EP300.train", tmp_path))
    Xte, _ = reader.read_data(reference_fasta("EP300.test", tmp_path))
    comp = reader.complement()
    assert len(comp) == 4 and all(comp[comp[t]] == t and comp[t] != t for t in comp)
    g, m = 10, 6
    f = FastSK(g=g, m=m, revcomp=comp, **kw)
    f.compute_kernel(Xtr, Xte)
    st = f.stats()
    ntr, nte = len(Xtr), len(Xte)
    X = Xtr + Xte
    assert st["revcomp"] is True and st["n_seq"] == ntr + nte and st["n_feat"] == 2 * sum(len(x) - g + 1 for x in X)
    rng = np.random.Generator(np.random.PCG64(13))
    idx = np.sort(np.concatenate([rng.choice(ntr, size=90, replace=False), ntr + rng.choice(nte, size=60, replace=False)]))
    n_sub_tr = 90
    combos = np.arange(port.num_combos(g, m), dtype=np.int32)
    fold = folded_oracle(port, [X[i] for i in idx], comp, g, m, combos)
    want = tri_to_square(port.normalise(fold.astype(np.float64), len(idx)), len(idx))
    train, test = f.get_train_kernel_np(), f.get_test_kernel_np()
    assert train.shape == (ntr, ntr) and test.shape == (nte, ntr)
    tr_i, te_i = idx[:n_sub_tr], idx[n_sub_tr:] - ntr
    assert np.array_equal(train[np.ix_(tr_i, tr_i)], want[:n_sub_tr, :n_sub_tr])
    assert np.array_equal(test[np.ix_(te_i, tr_i)], want[n_sub_tr:, :n_sub_tr])
    assert np.array_equal(torch.from_dlpack(f.get_train_kernel_dlpack()).cpu().numpy(), train)
    assert np.array_equal(torch.from_dlpack(f.get_test_kernel_dlpack()).cpu().numpy(), test)
    a, b = np.tril_indices(len(idx))
    if kw.get("skip_test_block") == "lazy":
        assert st["test_block_computed"] is False
    assert np.array_equal(f.get_counts_cells(idx[a], idx[b]), fold)   # (test x test cells: the lazy block is computed now)
    assert f.stats()["test_block_computed"] is True
    blk = f.get_block(ntr, ntr + nte, ntr, ntr + nte)
    assert np.array_equal(blk[np.ix_(te_i, te_i)], want[n_sub_tr:, n_sub_tr:])
    if "devices" in kw:
        assert st["devices"] == [0, 0] and st["collective"] == "p2p"
    with pytest.raises(ValueError):
        FastSK(g=g, m=m, revcomp={1: 2, 2: 3, 3: 1})
    prot = FastSK(g=g, m=m, revcomp=comp)
    with pytest.raises(ValueError) as ei:   # protein given to a DNA map fails loudly
        prot.compute_train([[1, 2, 3, 4, 9, 1, 2, 3, 4, 1, 2, 3]] * 3)
    assert "token 9 " in str(ei.value)


# ---- 14 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_variance_mode_on_ep300(native, port, path):
    """Variance mode, T = 1, the seed's own order, 400 EP300 sequences: the reference's chain (tests/test_emu_revcomp.py:
    variance_restated) on per-combination folded counts, bit for bit."""
    from test_emu_revcomp import variance_restated
    tokens, offsets, _, _, _, _ = load_tokens("EP300")
    N, ntr, g, m, seed, max_iters, delta = 400, 300, 10, 6, 20201214, 12, 0.025
    tokens, offsets = tokens[:offsets[N]].copy(), offsets[:N + 1].copy()
    X = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in range(N)]
    comp = {1: 2, 2: 1, 3: 4, 4: 3}   # the fixture's ids (tests/golden/revcomp_ep300_60.npz holds the same map)
    from test_emu_revcomp import load_revcomp_golden
    assert load_revcomp_golden()[2] == comp
    order = native.library().seed_order(seed, port.num_combos(g, m))
    cache = {}

    def per_combo(c):
        if c not in cache:
            cache[c] = folded_oracle(port, X, comp, g, m, np.array([c], dtype=np.int32))
        return cache[c]

    want, sds = variance_restated(per_combo, order, N, ntr, 1, delta, max_iters)
    e = native.Engine(g, m, t=1, approx=True, delta=delta, max_iters=max_iters, path=path, revcomp=comp)
    e.set_seed(seed)
    e.compute(tokens, offsets, ntr, N - ntr)
    assert e.stats()["path_used"] == path
    assert np.array_equal(e.get_stdevs(), sds)
    assert np.array_equal(e.get_triangle(), want)
    e.close()


# ---- 15: the edges of this mode's kernels ----------------------------------------------------------------------------------
# tests/revcomp_cases.py at scale 1, through the checks of tests/test_emu_revcomp.py (section 11 there runs the same cases on
# the emulator, scaled down): what the emulator cannot show — races between the four waves of k_dense_count on the histogram
# and on the second strand's buffer, a missing barrier between staging a strand and counting it — and the sizes it cannot
# afford. Every comparison is bit-exact against folded_oracle.
@pytest.fixture(scope="module")
def make(native):
    return lambda g, m, **kw: native.Engine(g, m, revcomp=cases.DNA, **kw)


@pytest.mark.parametrize("lmax,m,rare_n,planned,planned_whole", cases.DENSE_REGIMES)
def test_dense_staging_regimes_on_ragged_dna(make, port, lmax, m, rare_n, planned, planned_whole):
    check_dense_regime(make, port, lmax, m, rare_n, planned, planned_whole, 1.0)


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("name", ["hi_plane", "overflow"])
def test_counts_crossing_a_plane_with_both_strands(make, port, name, path):
    check_planes(make, port, name, path, 1.0)


@pytest.mark.parametrize("sparse_global", [0, 1])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("windows", [32767, 32768])
def test_sparse_entry_formats_at_the_doubled_feature_count(make, port, windows, skip, sparse_global):
    check_long_sequence(make, port, windows, skip, sparse_global, 1.0)


@pytest.mark.parametrize("sparse_global", [0, 1])
def test_sparse_products_beyond_one_update_word(make, port, sparse_global):
    check_products(make, port, sparse_global, 1.0)


@pytest.mark.parametrize("path", [1, 2])
def test_windows_wider_than_128_bits(make, port, path):
    check_wide_windows(make, port, path, 1.0)


def test_sparse_update_stages_on_ragged_low_complexity_dna(make, port):
    check_update_stages(make, port, 1.0)


@pytest.mark.parametrize("windows,narrow", [(10000, False), (4000, True)])
def test_group_narrowing_sees_both_strands(make, port, windows, narrow):
    check_narrowing(make, port, windows, narrow, 1.0)
