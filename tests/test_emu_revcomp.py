"""Reverse-complement mode (fsk_set_complement, ``revcomp=``) on the CPU: the engine's HIP source compiled against
tests/emu/hip_emu.h must reproduce, to the bit, the CPU oracle run on the 2N sequences [X ; rc(X)] with the four N x N
blocks of its raw counts added,

    Krc_c(x, y) = K_c(x, y) + K_c(x, rc y) + K_c(rc x, y) + K_c(rc x, rc y)    per combination c,

and everything after the per-combination counts (sum over combinations, the Welford chain and stop test of approx mode,
normalisation) the reference's algorithm on those counts."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, load_golden, tri_to_square

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

DNA = {1: 4, 4: 1, 2: 3, 3: 2, 5: 5}   # a = 1, c = 2, g = 3, t = 4, n = 5


@pytest.fixture(scope="session")
def emu_lib():
    import build_emu
    from fastsk_amd import _native
    return _native.Library(build_emu.build())


def folded_oracle(port, seqs, comp, g, m, combos, threads=1):
    """THE oracle of this mode: ``port.raw_counts`` on [X ; rc(X)], the four blocks added -> uint64 lower triangle."""
    from oracle import loader
    n = len(seqs)
    both = [list(s) for s in seqs] + [[comp[t] for t in reversed(list(s))] for s in seqs]
    tok, off = loader.flatten(both)
    tri2, _, _ = port.raw_counts(tok, off, g, m, combos, threads=threads)
    sq = tri_to_square(tri2, 2 * n)
    f = sq[:n, :n] + sq[:n, n:] + sq[n:, :n] + sq[n:, n:]
    assert np.array_equal(f, f.T)
    return f[np.tril_indices(n)]


def variance_restated(per_combo, order, N, n_train, T, delta, max_iters):
    """oracle/fastsk_oracle.c:279-349 in plain Python floats on the per-combination triangles ``per_combo(c)``: sequential
    sums in index order over the ``train_pairs`` prefix, the stop test, chains added in worker order. Returns (normalised
    triangle, chain 0's stdevs)."""
    pairs, train_pairs = N * (N + 1) // 2, n_train * (n_train + 1) // 2
    T = max(1, min(T, len(order)))
    K = np.zeros(pairs, dtype=np.float64)
    sds = []
    for tid in range(T):
        K_hat = np.zeros(pairs, dtype=np.float64)
        it, item, working = 1, tid, True
        while working:
            Ks = per_combo(int(order[item])).astype(np.float64)
            d = Ks - K_hat
            K_hat = K_hat + d / float(it)
            d2 = Ks - K_hat
            avg = 0.0
            for v in (d * d2)[:train_pairs].tolist():
                avg += v
            avg /= train_pairs
            avg = 9999999.0 if it == 1 else avg / (it - 1)
            sd = math.sqrt(avg / it)
            if tid == 0:
                sds.append(sd)
            if sd == 0.0 or delta / sd > 1.96:
                working = False
            if max_iters != -1 and it >= max_iters:
                working = False
            item += T
            if item >= len(order):
                working = False
            it += 1
        K = K + K_hat
    tri = K.copy()
    il = np.tril_indices(N)
    diag = tri[[i * (i + 1) // 2 + i for i in range(N)]]
    tri = tri / np.sqrt(diag[il[0]] * diag[il[1]])
    return tri, np.array(sds, dtype=np.float64)


def ragged_dna(n=24, seed=7, lo=8, hi=40):
    """n ragged sequences of tokens 1..4, one of them holding a run of n (token 5)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs = [rng.integers(1, 5, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]
    seqs[3][2:7] = [5] * 5
    return seqs


def engine(emu_lib, g, m, comp, **kw):
    from fastsk_amd import _native
    return _native.Engine(g, m, lib=emu_lib, revcomp=comp, **kw)


def run_exact(emu_lib, seqs, comp, g, m, n_train, path, **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(seqs)
    e = engine(emu_lib, g, m, comp, path=path, **kw)
    e.compute(tok, off, n_train, len(seqs) - n_train)
    return e


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_exact_equals_the_folded_oracle(emu_lib, port, path):
    seqs = ragged_dna()
    g, m, N, ntr = 8, 3, 24, 16
    want = folded_oracle(port, seqs, DNA, g, m, np.arange(port.num_combos(g, m)))
    e = run_exact(emu_lib, seqs, DNA, g, m, ntr, path)
    st = e.stats()
    assert st["revcomp"] is True and st["path_used"] == path
    assert st["n_feat"] == 2 * sum(len(s) - g + 1 for s in seqs)
    assert st["max_windows"] == 2 * (max(len(s) for s in seqs) - g + 1)
    got = e.get_counts()
    assert np.array_equal(got, want)
    assert not (got & np.uint64(1)).any()   # all combos: the combo set is closed under mirroring, every cell is even
    tri = port.normalise(want.astype(np.float64), N)
    assert np.array_equal(e.get_triangle(), tri)
    sq = tri_to_square(tri, N)
    assert np.array_equal(e.get_train(), sq[:ntr, :ntr])
    assert np.array_equal(e.get_test(), sq[ntr:, :ntr])
    e.close()


def test_mode_off_is_the_plain_kernel(emu_lib):
    """revcomp=None / False / {} and a map switched off again: the plain golden."""
    from fastsk_amd import _native
    d = load_golden("f3_ragged_sigma7_g6m3")
    for off in (None, False, {}):
        e = _native.Engine(d["g"], d["m"], lib=emu_lib, revcomp=off)
        e.compute(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
        assert e.stats()["revcomp"] is False and np.array_equal(e.get_counts(), d["counts"])
        e.close()
    e = _native.Engine(d["g"], d["m"], lib=emu_lib, revcomp={t: t for t in range(1, 8)})
    e.set_complement(None)
    e.compute(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
    assert np.array_equal(e.get_counts(), d["counts"])
    e.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_alphabet_is_closed_under_the_map(emu_lib, port, path):
    """Sequences of a and c only: their second strands are made of t and g."""
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [rng.integers(1, 3, size=int(rng.integers(7, 30))).tolist() for _ in range(12)]
    g, m = 6, 2
    want = folded_oracle(port, seqs, DNA, g, m, np.arange(port.num_combos(g, m)))
    e = run_exact(emu_lib, seqs, DNA, g, m, 12, path)
    assert e.stats()["alphabet"] == 4
    assert np.array_equal(e.get_counts(), want)
    e.close()
    # a complement beyond the byte table (token ids >= 256 take the general packing path)
    comp = {1: 300, 300: 1, 2: 2}
    want = folded_oracle(port, seqs, comp, g, m, np.arange(port.num_combos(g, m)))
    e = run_exact(emu_lib, seqs, comp, g, m, 12, path)
    assert e.stats()["alphabet"] == 3 and np.array_equal(e.get_counts(), want)
    e.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def low_complexity_sets():
    acgt = [[1, 2, 3, 4] * r for r in (3, 4, 5, 7, 9)] + [[2, 3, 4, 1] * 4, [3, 4, 1, 2] * 6]   # every window a reverse palindrome's shift
    hi_plane = [[1] * 30, [4] * 33, [1] * 14 + [4] * 15, [1, 4] * 12, [2] * 25 + [1] * 9, [4] * 12 + [3] * 12]   # counts above 15
    overflow = [[1] * 150 + [4] * 150, [4] * 140, [1] * 20 + [2, 3] * 5 + [4] * 170, [1, 2, 3, 4] * 8]        # counts above 255
    return {"palindromes": acgt, "hi_plane": hi_plane, "overflow": overflow}


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("name", ["palindromes", "hi_plane", "overflow"])
def test_palindromes_and_low_complexity(emu_lib, port, name, path):
    """A reverse-palindromic window counts twice; poly-A / poly-T put a k-mer's two strands into ONE counter: above 15 (the hi
    plane) and above 255 (the dense dataflow's overflow fallback to the sparse one)."""
    seqs = low_complexity_sets()[name]
    g, m = 5, 2
    want = folded_oracle(port, seqs, DNA, g, m, np.arange(port.num_combos(g, m)))
    e = run_exact(emu_lib, seqs, DNA, g, m, len(seqs), path)
    assert np.array_equal(e.get_counts(), want)
    if name == "palindromes":   # x == rc(x) for the first five: four equal blocks
        from fastsk_amd import _native
        tok, off = _native.flatten(seqs[:5])
        plain, _, _ = port.raw_counts(tok, off, g, m, np.arange(port.num_combos(g, m)))
        assert np.array_equal(tri_to_square(want, len(seqs))[:5, :5][np.tril_indices(5)], 4 * plain)
    if name == "overflow" and path == 1:
        assert e.stats()["sort_records"] > 0   # the sparse dataflow took the batch over
    e.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_windows_wider_than_128_bits(emu_lib, port, path):
    """4-bit symbols, g = 33: no packed window array, the sparse dataflow gathers the symbols (k_sx_extract) — of the second
    strand from the far end backwards."""
    from fastsk_amd import _native
    rng = np.random.Generator(np.random.PCG64(3))
    seqs = [rng.integers(1, 6, size=int(rng.integers(33, 70))).tolist() for _ in range(10)]
    g, m = 33, 28
    nc = port.num_combos(g, m)
    combos = np.array([0, 1, 777, nc // 2, nc - 1], dtype=np.int32)
    want = folded_oracle(port, seqs, DNA, g, m, combos)
    tok, off = _native.flatten(seqs)
    e = engine(emu_lib, g, m, DNA, path=path)
    e.load_sequences(tok, off, len(seqs), 0)
    assert e.stats()["bits_per_symbol"] == 4
    e.accumulate(combos[:2])
    e.accumulate(combos[2:])
    e.finalize()
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [{"compact": 1}, {"compact": 0}, {"compact": 1, "compact_rare": 1}, {"compact": 1, "dense_chunk": 7},
                                    {"dense_chunk": 5}, {}])
def test_key_compaction_sees_both_strands(emu_lib, port, tuning):
    """One n in otherwise 4-letter DNA, key compaction forced both ways (and with the shortcut from the rare symbols' places
    asked for, which this mode answers with the marking pass over both strands); staging chunk by chunk."""
    rng = np.random.Generator(np.random.PCG64(5))
    seqs = [rng.integers(1, 5, size=int(rng.integers(20, 60))).tolist() for _ in range(70)]
    seqs[17][9] = 5
    g, m = 7, 3
    want = folded_oracle(port, seqs, DNA, g, m, np.arange(port.num_combos(g, m)))
    e = run_exact(emu_lib, seqs, DNA, g, m, 50, 1, tuning=tuning)
    st = e.stats()
    assert st["path_used"] == 1
    if tuning.get("compact") == 1:
        assert st["compact_keys_avg"] > 0
    assert np.array_equal(e.get_counts(), want)
    e.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_approx_skip_variance_is_the_fold_over_the_sampled_combos(emu_lib, port, path):
    from fastsk_amd import _native
    seqs = ragged_dna()
    g, m, N, ntr = 8, 3, 24, 16
    order = np.array([0, 5, 17, 40, 3, 21, 9], dtype=np.int32)
    tok, off = _native.flatten(seqs)
    for T, max_iters, used in ((1, 3, [0, 5, 17]), (2, 2, [0, 5, 17, 40])):
        want = folded_oracle(port, seqs, DNA, g, m, np.array(used, dtype=np.int32))
        e = engine(emu_lib, g, m, DNA, path=path, t=T, approx=True, skip_variance=True, max_iters=max_iters)
        e.set_combo_order(order)
        e.compute(tok, off, ntr, N - ntr)
        got = e.get_counts()
        assert np.array_equal(got, want)
        assert (got & np.uint64(1)).any()   # a subset of the combos is not closed under mirroring: evenness is no shortcut
        assert np.array_equal(e.get_triangle(), port.normalise(want.astype(np.float64), N))
        e.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("T", [1, 2])
def test_variance_mode_is_the_references_chain_on_folded_counts(emu_lib, port, T, path):
    from fastsk_amd import _native
    seqs = ragged_dna(n=24, seed=13)
    g, m, N, ntr = 8, 3, 24, 17
    rng = np.random.Generator(np.random.PCG64(99))
    order = rng.permutation(port.num_combos(g, m)).astype(np.int32)
    cache = {}

    def per_combo(c):
        if c not in cache:
            cache[c] = folded_oracle(port, seqs, DNA, g, m, np.array([c], dtype=np.int32))
        return cache[c]

    tok, off = _native.flatten(seqs)
    for delta, max_iters in ((0.025, 9), (3.0, -1)):   # stopped by max_iters; stopped by the test
        want, sds = variance_restated(per_combo, order, N, ntr, T, delta, max_iters)
        e = engine(emu_lib, g, m, DNA, path=path, t=T, approx=True, delta=delta, max_iters=max_iters)
        e.set_combo_order(order)
        e.compute(tok, off, ntr, N - ntr)
        assert np.array_equal(e.get_stdevs(), sds), (delta, max_iters)
        assert np.array_equal(e.get_triangle(), want), (delta, max_iters)
        if max_iters == -1:
            assert 1 < len(sds) < len(order) // T   # the stop test ended the chain
        e.close()


def test_variance_restatement_is_the_oracle_chain(port):
    """The restatement above, fed plain per-combination counts, is ``port.compute``: what makes it a yardstick."""
    from fastsk_amd import _native
    seqs = ragged_dna(n=20, seed=2)
    g, m, N, ntr = 7, 3, 20, 14
    tok, off = _native.flatten(seqs)
    order = np.random.Generator(np.random.PCG64(4)).permutation(port.num_combos(g, m)).astype(np.int32)
    for T, delta, max_iters in ((1, 0.025, 6), (2, 2.0, -1)):
        want, sd, _ = port.compute(tok, off, ntr, N - ntr, g, m, t=T, approx=True, delta=delta, max_iters=max_iters, order=order)
        got, sds = variance_restated(lambda c: port.raw_counts(tok, off, g, m, np.array([c], dtype=np.int32))[0], order, N, ntr, T,
                                     delta, max_iters)
        assert np.array_equal(sds, sd) and np.array_equal(got, want)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_bad_maps_fail_at_the_call(emu_lib):
    from fastsk_amd import _native
    e = _native.Engine(6, 3, lib=emu_lib)
    for tokens, comps, what in (([1, 2, 3], [2, 3, 1], "involution"), ([1, 1], [1, 1], "twice"), ([1], [4], "not listed"),
                                ([1, 4, 4], [4, 1, 1], "twice")):
        with pytest.raises(_native.FskError) as ei:
            e.set_complement_arrays(tokens, comps)
        assert ei.value.code == -1 and what in str(ei.value)
        assert e.stats()["revcomp"] is False
    for bad in ({1: 2, 2: 3, 3: 1}, {1: 4}, {1: "t"}, [1, 2], "acgt"):
        with pytest.raises(ValueError):
            e.set_complement(bad)
        with pytest.raises(ValueError):
            _native.Engine(6, 3, lib=emu_lib, revcomp=bad)
    e.set_complement({1: 1, 2: 3, 3: 2})   # self-pairs are allowed
    assert e.stats()["revcomp"] is True
    e.close()


def test_a_token_outside_the_map_fails_the_load_and_names_it(emu_lib):
    from fastsk_amd import _native
    d = load_golden("f3_ragged_sigma7_g6m3")   # tokens 1..7
    for comp in ({1: 4, 4: 1, 2: 3, 3: 2}, {1: 4, 4: 1, 2: 3, 3: 2, 300: 300}):
        e = _native.Engine(d["g"], d["m"], lib=emu_lib, revcomp=comp)
        first = next(int(t) for t in d["tokens"] if int(t) not in comp)
        with pytest.raises(_native.FskError) as ei:
            e.compute(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
        assert ei.value.code == -1 and ("token %d " % first) in str(ei.value)
        with pytest.raises(_native.FskError):
            e.load_sequences(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
        e.set_complement(None)   # usable afterwards with the mode off: the plain golden
        e.compute(d["tokens"], d["offsets"], d["n_train"], d["n_test"])
        assert np.array_equal(e.get_counts(), d["counts"]) and np.array_equal(e.get_triangle(), d["tri"])
        e.close()


def test_fasta_reader_complement(tmp_path):
    from fastsk_amd import FastaUtility
    p = tmp_path / "dna.fasta"
    p.write_text(">1\nACCA\n>0\ncanca\n")
    r = FastaUtility()
    X, _ = r.read_data(str(p))
    comp = r.complement()
    a, c, n = X[0][0], X[0][1], X[1][2]
    assert comp[a] != a and comp[comp[a]] == a and comp[c] != c and comp[comp[c]] == c and comp[n] == n
    assert len(comp) == 5 and len({a, c, n, comp[a], comp[c]}) == 5   # t and g got ids of their own
    p2 = tmp_path / "more.fasta"
    p2.write_text(">1\ntg\n")
    X2, _ = r.read_data(str(p2))
    assert X2[0] == [comp[a], comp[c]]   # ... which a later file read through the same object agrees with
    prot = FastaUtility()
    prot.read_data(os.path.join(GOLD, "fasta", "protein.train.fasta"))
    with pytest.raises(ValueError) as ei:
        prot.complement()
    assert "symbol" in str(ei.value)


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_group_of_two_engines_on_one_device(emu_lib, port):
    """fsk_create_multi over devices [0, 0] with the P2P collective: the setting reaches both engines, the result is the
    single engine's; and the int32 narrowing of the exchange (C(g,m) * max_windows^2 < 2^31) sees the doubled windows."""
    from fastsk_amd import _native
    seqs = ragged_dna()
    g, m = 8, 3
    tok, off = _native.flatten(seqs)
    one = engine(emu_lib, g, m, DNA)
    one.compute(tok, off, 16, 8)
    for path in (1, 2):
        e = engine(emu_lib, g, m, DNA, devices=[0, 0], collective=_native.COLL_P2P, path=path)
        e.compute(tok, off, 16, 8)
        info = e.multi_info()
        assert info["ndev"] == 2 and info["collective"] == "p2p" and info["narrow"]
        assert np.array_equal(e.get_counts(), one.get_counts()) and np.array_equal(e.get_triangle(), one.get_triangle())
        assert e.counts_digest() == one.counts_digest()
        e.close()
    one.close()
    # 15 combos x 7995^2 < 2^31 <= 15 x (2 x 7995)^2: the plain exchange is int32, this mode's must be 64 bits wide
    rng = np.random.Generator(np.random.PCG64(21))
    seqs = [rng.integers(1, 5, size=n).tolist() for n in (8000, 50, 64, 41, 77, 58)]
    g, m = 6, 2
    tok, off = _native.flatten(seqs)
    want = folded_oracle(port, seqs, DNA, g, m, np.arange(port.num_combos(g, m)))
    plain = _native.Engine(g, m, lib=emu_lib, devices=[0, 0], collective=_native.COLL_P2P)
    plain.compute(tok, off, 4, 2)
    assert plain.multi_info()["narrow"]
    plain.close()
    one = engine(emu_lib, g, m, DNA)
    one.compute(tok, off, 4, 2)
    assert np.array_equal(one.get_counts(), want)
    for path in (0, 2):
        e = engine(emu_lib, g, m, DNA, devices=[0, 0], collective=_native.COLL_P2P, path=path)
        e.compute(tok, off, 4, 2)
        info = e.multi_info()
        assert not info["narrow"] and info["reduce_bytes"] == 8 * 21
        assert np.array_equal(e.get_counts(), want) and np.array_equal(e.get_triangle(), one.get_triangle())
        e.close()
    one.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def load_revcomp_golden():
    z = np.load(os.path.join(GOLD, "revcomp_ep300_60.npz"))
    comp = {int(a): int(b) for a, b in zip(z["comp_tokens"], z["comp_complements"])}
    return z["tokens"].astype(np.int32), z["offsets"].astype(np.int64), comp, int(z["g"]), int(z["m"]), z["counts"], z["tri"]


@pytest.mark.parametrize("path", [0, 1, 2])
def test_golden_from_the_compiled_reference(emu_lib, port, path):
    """tests/golden/revcomp_ep300_60.npz (tests/make_golden_revcomp.py: the COMPILED reference on [X ; rc(X)], folded): the
    port's fold == the fixture == the engine."""
    tokens, offsets, comp, g, m, counts, tri = load_revcomp_golden()
    N = len(offsets) - 1
    seqs = [tokens[offsets[i]:offsets[i + 1]].tolist() for i in range(N)]
    assert np.array_equal(folded_oracle(port, seqs, comp, g, m, np.arange(port.num_combos(g, m)), threads=4), counts)
    assert np.array_equal(port.normalise(counts.astype(np.float64), N), tri)
    e = engine(emu_lib, g, m, comp, path=path)
    e.compute(tokens, offsets, 40, 20)
    assert np.array_equal(e.get_counts(), counts)
    assert np.array_equal(e.get_triangle(), tri)
    e.close()
