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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import revcomp_cases as cases  # noqa: E402

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


# ---- 11: the edges of this mode's kernels -----------------------------------------------------------------------------------
# The cases of tests/revcomp_cases.py, each checked by ONE function that both suites call: here on the emulator at a reduced
# scale (fewer ordinary sequences; the lengths that define an edge are kept), in tests/test_gpu_revcomp.py on the device at
# scale 1. The emulator switches a workgroup's threads only at barriers and wave collectives, so a case that passes here and
# fails there points at a race or at something only the larger size reaches — not at the logic of the edge.
# ``make(g, m, **kw)`` creates an engine with the DNA map set. Every comparison is bit-exact against folded_oracle.
EMU_SCALE = 0.2
_FOLDS = {}


def fold_once(port, key, case, with_updates=False):
    """The fold (and, asked for, its update count) of a case, computed once per session and shared: treat as read-only."""
    if key not in _FOLDS:
        want = folded_oracle(port, case["seqs"], cases.DNA, case["g"], case["m"], case["combos"], threads=cases.THREADS)
        want.setflags(write=False)
        _FOLDS[key] = [want, None]
    if with_updates and _FOLDS[key][1] is None:
        _FOLDS[key][1] = cases.fold_updates(port, case["seqs"], cases.DNA, case["g"], case["m"], case["combos"])
    return _FOLDS[key]


def accumulate_case(make, case, path, tuning=None, how="whole", n_train=None, **kw):
    from fastsk_amd import _native
    tok, off = _native.flatten(case["seqs"])
    n = len(case["seqs"])
    e = make(case["g"], case["m"], path=path, tuning=dict(tuning or {}), **kw)
    e.load_sequences(tok, off, n if n_train is None else n_train, 0 if n_train is None else n - n_train)
    combos = case["combos"]
    if how == "whole":
        e.accumulate(combos)
    elif how == "three calls":
        for part in np.array_split(combos, 3):
            e.accumulate(part)
    else:
        for lo, hi in case["bands"]:
            e.accumulate_rows(combos, lo, hi)
    e.finalize()
    return e


def assert_kept_cells(got, want, n, n_train):
    """skip_test_block: every cell whose column is a train sequence or that lies on the diagonal equals the oracle's; the
    rest is zero in the engine and is not all zero in the oracle; at least half the cells are of the first kind."""
    a, b = np.tril_indices(n)
    keep = (b < n_train) | (a == b)
    assert keep.mean() >= 0.5
    assert np.array_equal(got[keep], want[keep]) and not got[~keep].any() and want[~keep].any()


def check_dense_regime(make, port, lmax, m, rare_n, planned, planned_whole, scale):
    """k_dense_count<., ., RC>'s strand loop in each staging regime accumulate_dense can put it in (revcomp_cases.dense_regime
    names them). The arithmetic — fsk_engine_dense.hip:dense_plan with PANEL = 64 bytes a staged row, at most 64 KiB = 1024
    rows of symbols, LDS_BUDGET = 150 KiB = 153,600 bytes, 512 bytes of histogram a key quad — for DNA at g = 12, where a
    strand of L symbols stages L rows = 64 L bytes:
        one pass per strand   <=> 64 L <= 65,536                        <=> L <= 1024        (beyond: C, 1013 windows a chunk)
        second buffer fits    <=> 64 L + 64 L + table + 1024 <= 153,600 <=> L <= 1192 - table / 128
        key quads a sweep      =  (153,600 - 128 L - table) / 512, rounded down to even
      m = 8: 256 keys = 64 key quads, no table.
        L = 300: A, one sweep (64 quads fit up to L = 944).   L = 1000: A, (153,600 - 128,000) / 512 = 50 quads: two sweeps, the
        second without staging.   L = 1025, 2500: C, two and three chunks a strand, every chunk of every strand restaged.
      m = 5: 16,384 keys = 4096 key quads. L = 1000: A, 50 quads: 82 sweeps, 81 of them on the kept buffers.
      m = 7 with a few n: 3125 keys = 782 key quads, key compaction on, a table of 6250 bytes. L = 1000: A,
        (153,600 - 128,000 - 6250) / 512 = 37 -> 36 quads: up to 22 sweeps (fewer for a combo whose compacted keys are
        fewer), keys through the rank table.
    B (a strand fits in one pass, the second buffer does not) cannot come out of this plan: with L <= 1024 the second buffer
    fails only for a table above 153,600 - 1024 - 131,072 = 21,504 bytes = 10,752 keys, and the engine compacts keys up to
    4096 only (fsk_engine.hip: compact = ... && V <= 4096; compact=1 at 16,384 keys leaves compaction off). What does reach it
    is the tuning key dense_chunk at or above the strand's windows: CH stays max_win, rc_rows stays 0. Every case that
    fits one pass is run once more that way (dense_chunk=2^20): L = 1000 at m = 5 is then B with (153,600 - 64,000) / 512 =
    175 -> 174 quads, 24 sweeps, each restaging strand by strand.
    The load is ragged (the second strand reads len - 1 - p per lane); dense_chunk=7 is regime C with 7 windows a chunk;
    path=2 is the sparse dataflow on the same sequences, whose backward half crosses many 256-feature blocks of
    k_sx_windows. No stat names the regime and none is added for this: the restated plan is what is asserted."""
    case = cases.dense_regime_case(port, lmax, m, rare_n, scale)
    g, keys, compact = case["g"], case["keys"], case["compact"]
    assert cases.dense_regime(lmax, g, keys, compact) == planned
    assert cases.dense_regime(lmax, g, keys, compact, cases.WHOLE_STRAND) == planned_whole
    assert cases.dense_regime(lmax, g, keys, compact, case["tiny_chunk"])[0] == "C"
    lens = [len(s) for s in case["seqs"]]
    assert max(lens) == lmax and min(lens) == g and len(set(lens)) > len(lens) // 4
    want, _ = fold_once(port, ("dense", lmax, m, scale), case)
    for path, tun in ((1, {}), (1, {"dense_chunk": cases.WHOLE_STRAND}), (1, {"dense_chunk": case["tiny_chunk"]}), (2, {})):
        e = accumulate_case(make, case, path, tun)
        st = e.stats()
        assert st["path_used"] == path and st["revcomp"] and st["max_windows"] == case["max_windows"], (path, tun)
        assert st["key_space"] == keys and (path != 1 or (st["compact_keys_avg"] > 0) == compact), (path, tun)
        assert np.array_equal(e.get_counts(), want), (planned, path, tun)
        e.close()


def check_planes(make, port, name, path, scale):
    """Counts that pass 15 (the hi plane of the count panels) or 255 (the hand-over to the sparse dataflow) only because both
    strands land in one counter: revcomp_cases.plane_case."""
    from fastsk_amd import _native
    case = cases.plane_case(name, scale)
    n = len(case["seqs"])
    want, _ = fold_once(port, ("planes", name, scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], path=path)
    e.compute(tok, off, n, 0)
    st = e.stats()
    assert np.array_equal(e.get_counts(), want), (name, path)
    assert np.array_equal(e.get_triangle(), port.normalise(want.astype(np.float64), n))
    if path == 1:   # the hand-over ran exactly when a count passed 255
        assert (st["sort_records"] > 0) == (name == "overflow")
    e.close()


def check_long_sequence(make, port, windows, skip, sparse_global, scale):
    """The packed / unpacked entry formats on either side of max_windows = 65,536 (revcomp_cases.long_sequence_case), update
    streams and 64-bit atomics, with and without skip_test_block."""
    case = cases.long_sequence_case(windows, scale)
    n, ntr = len(case["seqs"]), case["n_train"]
    want, U = fold_once(port, ("long", windows, scale), case, with_updates=True)
    e = accumulate_case(make, case, 2, {"sparse_global": sparse_global}, n_train=ntr, skip_test_block=skip)
    st = e.stats()
    assert st["path_used"] == 2 and st["max_windows"] == case["max_windows"] == 2 * windows
    got = e.get_counts()
    if skip:
        assert_kept_cells(got, want, n, ntr)
        assert st["cell_updates"] < U
    else:
        assert np.array_equal(got, want)
        assert st["cell_updates"] == U
    e.close()


def check_products(make, port, sparse_global, scale):
    """Products beyond the product field of one 32-bit update word, in a cell that is zero without this mode
    (revcomp_cases.products_case); update streams and 64-bit atomics."""
    case = cases.products_case(scale)
    want, U = fold_once(port, ("products", scale), case, with_updates=True)
    ia, it = case["poly_a"], case["poly_t"]
    assert want[it * (it + 1) // 2 + ia] == len(case["combos"]) * 2 * 1491 * 1391   # (they pair through this mode only)
    e = accumulate_case(make, case, 2, {"sparse_global": sparse_global})
    assert np.array_equal(e.get_counts(), want)
    assert e.stats()["cell_updates"] == U
    e.close()


def check_wide_windows(make, port, path, scale):
    """g x bits a symbol > 128: revcomp_cases.wide_window_case, the combos in two calls."""
    from fastsk_amd import _native
    case = cases.wide_window_case(port, scale)
    want, _ = fold_once(port, ("wide", scale), case)
    tok, off = _native.flatten(case["seqs"])
    e = make(case["g"], case["m"], path=path)
    e.load_sequences(tok, off, len(case["seqs"]), 0)
    assert e.stats()["bits_per_symbol"] == 4
    e.accumulate(case["combos"][:2])
    e.accumulate(case["combos"][2:])
    e.finalize()
    assert e.stats()["path_used"] == path and np.array_equal(e.get_counts(), want)
    e.close()


def check_update_stages(make, port, scale):
    """Every form of the sparse update stage (revcomp_cases.SPARSE_FORMS and the two-level blocks forced small) on ragged
    low-complexity sequences: in one call, in three calls, in row bands at multiples of 128 — whole triangle and U."""
    case = cases.low_complexity_case(scale)
    want, U = fold_once(port, ("stages", scale), case, with_updates=True)
    digests = set()
    for name, tun, form in cases.SPARSE_FORMS + [cases.SMALL_BLOCKS]:
        for how in ("whole", "three calls", "row bands"):
            e = accumulate_case(make, case, 2, tun, how)
            st = e.stats()
            assert st["path_used"] == 2 and (form is None or st["sparse_form"] == form), (name, how)
            assert np.array_equal(e.get_counts(), want), (name, how)
            assert st["cell_updates"] == U, (name, how)
            digests.add(e.counts_digest())
            e.close()
    assert len(digests) == 1


def check_narrowing(make, port, windows, narrow, scale):
    """fsk_multi.hip narrows the exchange of a group to int32 when combos x max_windows^2 < 2^31, max_windows counting both
    strands (revcomp_cases.narrowing_case: the cell that needs it)."""
    from fastsk_amd import _native
    case = cases.narrowing_case(windows, scale)
    n, ntr, at = len(case["seqs"]), case["n_train"], case["long_at"]
    assert (15 * (2 * windows) ** 2 < 2 ** 31) == narrow and (narrow or 15 * windows ** 2 < 2 ** 31 <= case["diagonal"])
    want, _ = fold_once(port, ("narrow", windows, scale), case)
    diag = at * (at + 1) // 2 + at
    assert want[diag] == case["diagonal"]
    tok, off = _native.flatten(case["seqs"])
    one = make(case["g"], case["m"])
    one.compute(tok, off, ntr, n - ntr)
    e = make(case["g"], case["m"], devices=[0, 0], collective=_native.COLL_P2P)
    e.compute(tok, off, ntr, n - ntr)
    info = e.multi_info()
    assert info["ndev"] == 2 and info["collective"] == "p2p" and info["narrow"] == narrow
    got = e.get_counts()
    assert got[diag] == case["diagonal"]
    assert np.array_equal(got, want)
    assert np.array_equal(e.get_triangle(), port.normalise(want.astype(np.float64), n))
    assert e.counts_digest() == one.counts_digest()
    one.close(); e.close()


@pytest.fixture(scope="module")
def make_emu(emu_lib):
    return lambda g, m, **kw: engine(emu_lib, g, m, cases.DNA, **kw)


def test_fold_updates_is_the_oracles_count_on_one_strand(port):
    """revcomp_cases.fold_updates with the second strand left out is ``port.raw_counts``' U: what makes it a yardstick."""
    from fastsk_amd import _native
    case = cases.low_complexity_case(0.1)
    tok, off = _native.flatten(case["seqs"])
    _, _, U = port.raw_counts(tok, off, case["g"], case["m"], case["combos"])
    assert cases.fold_updates(port, case["seqs"], None, case["g"], case["m"], case["combos"]) == U
    seqs = ragged_dna()
    tok, off = _native.flatten(seqs)
    _, _, U = port.raw_counts(tok, off, 8, 3, np.arange(56, dtype=np.int32))
    assert cases.fold_updates(port, seqs, None, 8, 3, np.arange(56)) == U


def test_plane_cases_cross_their_planes_only_with_both_strands(port):
    """revcomp_cases.plane_case at both scales, from the definition: 'hi_plane' at most 15 a strand, more than 15 and at most
    255 together; 'overflow' at most 255 a strand, more together. At scale 1 its rows sit in three panels and two tiles."""
    for scale in (1.0, EMU_SCALE):
        for name, plane in (("hi_plane", 15), ("overflow", 255)):
            case = cases.plane_case(name, scale)
            one, both = cases.strand_maxima(port, case["seqs"], cases.DNA, case["g"], case["m"], case["combos"])
            assert one <= plane < both and (name == "overflow" or both <= 255), (name, scale, one, both)
            rows = case["flagged"]
            assert len({r // 64 for r in rows}) >= 2 and (scale < 1.0 or (len({r // 64 for r in rows}) == 3 and len({r // 128 for r in rows}) == 2))


@pytest.mark.parametrize("lmax,m,rare_n,planned,planned_whole", cases.DENSE_REGIMES)
def test_edges_dense_staging_regimes(make_emu, port, lmax, m, rare_n, planned, planned_whole):
    check_dense_regime(make_emu, port, lmax, m, rare_n, planned, planned_whole, EMU_SCALE)


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("name", ["hi_plane", "overflow"])
def test_edges_counts_crossing_a_plane(make_emu, port, name, path):
    check_planes(make_emu, port, name, path, EMU_SCALE)


@pytest.mark.parametrize("windows,skip,sparse_global", [(32767, False, 0), (32767, True, 1), (32768, True, 0), (32768, False, 1)])
def test_edges_sparse_entry_formats(make_emu, port, windows, skip, sparse_global):
    check_long_sequence(make_emu, port, windows, skip, sparse_global, EMU_SCALE)


@pytest.mark.parametrize("sparse_global", [0, 1])
def test_edges_sparse_products_beyond_one_update_word(make_emu, port, sparse_global):
    check_products(make_emu, port, sparse_global, EMU_SCALE)


@pytest.mark.parametrize("path", [1, 2])
def test_edges_windows_wider_than_128_bits(make_emu, port, path):
    check_wide_windows(make_emu, port, path, EMU_SCALE)


def test_edges_sparse_update_stages(make_emu, port):
    check_update_stages(make_emu, port, EMU_SCALE / 2)


@pytest.mark.parametrize("windows,narrow", [(10000, False), (4000, True)])
def test_edges_group_narrowing(make_emu, port, windows, narrow):
    check_narrowing(make_emu, port, windows, narrow, EMU_SCALE)
