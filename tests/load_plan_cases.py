"""Yardstick and inputs of the load plan (fastsk_amd/csrc/fsk_load_plan.cpp), for tests/test_load_plan_host.py. Nothing
here touches an engine.

``reference_plan`` restates the definitions in numpy, field by field: which windows are windows and what they weigh
(``wildcard_cases.valid_windows`` and ``center_weight_cases.window_weights`` are the yardsticks of the two modes: the
positions used here are checked against them), the alphabet as the sorted tokens that occur closed under the complement
map, ranks packed ``bits`` a symbol into words of 32 bits, low bits first, every sequence word-aligned.

A case is a dict: seqs, g, k, n_train, and optionally comp (token -> complement), wild, profile, prefix (tokens in front of
offsets[0]), offsets (given as they are: the malformed ones)."""
import numpy as np

import center_weight_cases
import wildcard_cases

EINVAL, ESHORT, ENOMEM, EUNSUPPORTED = -1, -2, -5, -6
DNA = wildcard_cases.DNA
G = 6


def flatten(case):
    prefix = list(case.get("prefix", []))
    tokens = prefix + [t for s in case["seqs"] for t in s]
    offsets = case.get("offsets")
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in case["seqs"]])]) + len(prefix)
    return np.asarray(tokens, dtype=np.int64), np.asarray(offsets, dtype=np.int64)


def write_case(path, case):
    tokens, offsets = flatten(case)
    comp = case.get("comp") or {}
    lists = [[v for t in sorted(comp) for v in (t, comp[t])], sorted(case.get("wild", [])), case.get("profile", []), offsets.tolist(), tokens.tolist()]
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (case["g"], case["k"], case["n_train"], len(offsets) - 1 - case["n_train"]))
        for v in lists:
            f.write("%d %s\n" % (len(v), " ".join(str(int(x)) for x in v)))


def read_plan(path):
    """The program's output: {"code", "msg"} and, for a plan, every field as an int64 array (``scalars`` named)."""
    out = {}
    with open(path) as f:
        for line in f:
            name, _, rest = line.rstrip("\n").partition(" ")
            if name == "msg":
                out["msg"] = rest
            elif name == "code":
                out["code"] = int(rest)
            elif name == "scalars":
                names = "N nfeat longest shortest most_valid sigma bits V key_symbits total_sym total n_words rc_on wild_on cw_on".split()
                out.update(zip(names, (int(v) for v in rest.split())))
            else:
                vals = rest.split()
                assert int(vals[0]) == len(vals) - 1
                out[name] = np.array([int(v) for v in vals[1:]], dtype=np.int64)
    return out


def _windows(seq, g, wild, profile):
    """(is window p a window, its weight), p = 0 .. len - g."""
    x = np.asarray(seq, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(x, g)
    wt = center_weight_cases.window_weights(len(x), g, profile) if profile else np.ones(len(win), dtype=np.int64)
    keep = wt > 0
    if wild:
        keep &= ~np.isin(win, list(wild)).any(axis=1)
        assert int((~np.isin(win, list(wild)).any(axis=1)).sum()) == len(wildcard_cases.valid_windows(seq, wild, g))
    if profile:
        assert np.array_equal(wt[keep], center_weight_cases.weighted_windows(seq, g, profile, wild)[1])
    return keep, wt


def _pack(ranks, bits):
    """One sequence's ranks, ``bits`` each, low bits first, into its own 32-bit words."""
    per = 32 // bits
    r = np.zeros(-(-len(ranks) // per) * per, dtype=np.uint64)
    r[:len(ranks)] = ranks
    return (r.reshape(-1, per) << (np.arange(per, dtype=np.uint64) * np.uint64(bits))).sum(axis=1).astype(np.int64)


def reference_plan(case):
    g, k, n_train = case["g"], case["k"], case["n_train"]
    comp, wild_set, profile = case.get("comp") or {}, set(case.get("wild", [])), list(case.get("profile", []))
    tokens, offsets = flatten(case)
    n = len(offsets) - 1

    def fail(code, msg):
        return {"code": code, "msg": msg}
    for t in sorted(comp):
        if wild_set and t in wild_set and comp[t] not in wild_set:
            return fail(EINVAL, "wildcard token %d has the complement %d, which is not a wildcard" % (t, comp[t]))
    lens = np.diff(offsets)
    if (lens < 0).any():
        return fail(EINVAL, "offsets must be non-decreasing")
    for what, part in (("train", lens[:n_train]), ("test", lens[n_train:])):
        if len(part) and g > part.min():
            return fail(ESHORT, "g cannot be longer than the shortest sequence in a dataset. g = %d, but shortest %s sequence has length %d" % (g, what, part.min()))
    seqs = [tokens[offsets[i]:offsets[i + 1]] for i in range(n)]
    data = tokens[offsets[0]:offsets[n]]
    strands = 2 if comp else 1
    longest = int(lens.max())
    # ---- modes in force
    reach = profile[:min((longest - g) // 2, len(profile) - 1) + 1] if profile else []
    cw_on, cw_zero = any(w != 1 for w in reach), any(w == 0 for w in reach)
    wild = wild_set if np.isin(data, list(wild_set)).any() else set()
    wild_on = bool(wild) or cw_zero
    nw = lens - g + 1
    p = {"code": 0, "msg": "", "N": n, "longest": longest, "shortest": int(lens.min()), "rc_on": int(bool(comp)), "wild_on": int(wild_on), "cw_on": int(cw_on),
         "total": len(data), "len32": lens}
    empty = np.zeros(0, dtype=np.int64)
    p.update(nvalid=empty, vstart=empty, vbits=empty, fwin=empty, comp_rank=empty)
    counts = nw
    if wild_on or cw_on:
        wins = [_windows(s, g, wild, profile if cw_on else []) for s in seqs]
        nvalid = np.array([int(wt[keep].sum()) for keep, wt in wins], dtype=np.int64)
        if (nvalid == 0).any():
            return fail(ESHORT, "sequence %d has no window of length g = %d that is free of wildcards%s: it would have no features"
                        % (int(np.argmax(nvalid == 0)), g, " and has a center weight above 0" if cw_on else ""))
        fwin = []
        for (keep, wt), w in zip(wins, nw):
            fwin += [j for j in range(w) if keep[j] for _ in range(wt[j])]
            if comp:   # second strand: window j of rc(x) is forward window w - 1 - j, listed as w + j
                fwin += [w + j for j in range(w) if keep[w - 1 - j] for _ in range(wt[w - 1 - j])]
        p.update(nvalid=nvalid, fwin=np.array(fwin, dtype=np.int64))
        counts = nvalid
        if wild_on:
            vstart = np.concatenate([[0], np.cumsum((nw + 31) // 32)])
            vbits = np.zeros(vstart[-1] + 1, dtype=np.int64)
            for (keep, _), at in zip(wins, vstart):
                for j in np.nonzero(keep)[0]:
                    vbits[at + j // 32] |= 1 << (j % 32)
            p.update(vstart=vstart, vbits=vbits)
    p.update(nfeat=strands * int(counts.sum()), most_valid=int(counts.max()), fstart=np.concatenate([[0], np.cumsum(strands * counts)]))
    # ---- alphabet
    real = data[~np.isin(data, list(wild))] if wild else data
    distinct = set(int(t) for t in real)
    if comp:
        for t in real:
            if int(t) not in comp:
                return fail(EINVAL, "token %d occurs in the sequences but not in the complement map" % t)
        distinct |= {comp[t] for t in distinct}
    distinct = np.array(sorted(distinct), dtype=np.int64)
    if len(distinct) > 65536:
        return fail(EUNSUPPORTED, "alphabet of %d symbols (> 65536)" % len(distinct))
    sigma = max(1, len(distinct))
    bits = 2 if sigma <= 4 else 4 if sigma <= 16 else 8 if sigma <= 256 else 16
    V, symbits = sigma ** k, 0
    if V > 2 ** 62:
        V, symbits = 2 ** 62, max(1, (sigma - 1).bit_length())
        if symbits * k > 96:
            return fail(EUNSUPPORTED, "a k-mer of %d symbols of %d bits does not fit the 128-bit sort records" % (k, symbits))
    p.update(distinct=distinct, sigma=sigma, bits=bits, V=V, key_symbits=symbits)
    # ---- words: a wildcard travels as rank 0 and is counted nowhere
    words, freq = [], np.zeros(max(256, len(distinct)), dtype=np.int64)
    for s in seqs:
        is_real = ~np.isin(s, list(wild)) if wild else np.ones(len(s), dtype=bool)
        ranks = np.where(is_real, np.searchsorted(distinct, s), 0)
        assert np.array_equal(distinct[ranks[is_real]], s[is_real])
        freq += np.bincount(ranks[is_real], minlength=len(freq))
        words.append(_pack(ranks, bits))
    wstart = np.concatenate([[0], np.cumsum([len(w) for w in words])])
    if comp:
        comp_rank = np.searchsorted(distinct, [comp[int(t)] for t in distinct])
        freq[:len(distinct)] = freq[:len(distinct)] + freq[comp_rank]
        p.update(comp_rank=comp_rank)
    p.update(sym_freq=freq, total_sym=int(freq[:len(distinct)].sum()) if wild else strands * len(data), n_words=int(wstart[-1]), wstart=wstart[:-1],
             staging=np.concatenate(words + [np.zeros(4, dtype=np.int64), wstart[:-1], lens, p["fstart"]]))
    return p


# ---- the cases --------------------------------------------------------------------------------------------------------------
def _case(seqs, g=G, m=2, n_train=None, **more):
    seqs = [[int(t) for t in s] for s in seqs]
    return dict(seqs=seqs, g=g, k=g - m, n_train=len(seqs) if n_train is None else n_train, **more)


def _cover(ids, lengths, seed):
    """Sequences of ``lengths`` (repeated as long as needed) in which every id of ``ids`` occurs, shuffled."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = np.array(ids, dtype=np.int64)
    pool = rng.permutation(np.concatenate([pool, rng.choice(pool, size=(-len(pool)) % sum(lengths))]))
    seqs, at, i = [], 0, 0
    while at < len(pool):
        seqs.append(pool[at:at + lengths[i % len(lengths)]].tolist())
        at += lengths[i % len(lengths)]
        i += 1
    if len(seqs[-1]) < min(lengths):
        seqs[-1] += pool[:min(lengths) - len(seqs[-1])].tolist()
    return seqs


def _dna(lengths, seed, symbols=(1, 2, 3, 4)):
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs = [rng.choice(symbols, size=n).tolist() for n in lengths]
    seqs[-1][:len(symbols)] = symbols   # (every symbol occurs)
    return seqs


WIDE_IDS = [1, 7, 300, 70000, 2 ** 20 + 5]
TEAM = "team_of_four"


def cases():
    """name -> case; ``expect``: what the issue states outright about the case, asserted beside the restatement."""
    c = {}
    # word and alphabet edges
    c["words_2bit"] = _case(_dna([6, 7, 16, 17, 33], 1), expect={"bits": 2, "n_words_each": [1, 1, 1, 2, 3]})
    c["words_4bit_5"] = _case(_cover(range(1, 6), [8, 9], 2), expect={"bits": 4, "sigma": 5})
    c["words_4bit_16"] = _case(_cover(range(16), [8, 9], 3), expect={"bits": 4, "sigma": 16})
    c["words_8bit_17"] = _case(_cover(range(3, 20), [6, 7], 4), expect={"bits": 8, "sigma": 17})
    c["words_8bit_256"] = _case(_cover(range(256), [6, 7], 5), expect={"bits": 8, "sigma": 256})
    c["words_16bit_seen_table"] = _case(_cover(range(44, 301), [6, 7, 9], 6), expect={"bits": 16, "sigma": 257})
    c["general_sort_search"] = _case(_cover(WIDE_IDS, [6, 7, 17, 33], 7), expect={"bits": 4, "sigma": 5})
    c["offsets0_byte"] = dict(c["words_2bit"], prefix=[9, 300, 2, 2, 1], same_as="words_2bit")
    c["offsets0_general"] = dict(c["general_sort_search"], prefix=[4, 4, 12345678], same_as="general_sort_search")
    # reverse complement
    c["rc_closure"] = _case(_dna([6, 9, 20, 31], 8, symbols=(1, 2, 4)), comp=DNA, expect={"sigma": 4, "distinct": [1, 2, 3, 4], "comp_rank": [3, 2, 1, 0]})
    c["rc_unlisted_token"] = _case([[1, 2, 4, 9, 7, 1, 2], [7, 1, 1, 2, 2, 4]], comp=DNA,
                                   expect={"code": EINVAL, "msg": "token 9 occurs in the sequences but not in the complement map"})
    # wildcards
    c["wild_absent"] = _case(_dna([6, 12, 25], 9), wild=[5, 1000], expect={"wild_on": 0, "nvalid": []})
    s = _dna([6, 14, 30, 40], 10)
    c["wild_small_id"] = _case([s[0], wildcard_cases.plant(s[1], [0]), wildcard_cases.plant(s[2], [7, 13, 29]), wildcard_cases.plant(s[3], [11, 12])],
                               wild=[5], expect={"wild_on": 1, "sigma": 4})
    s = _dna([8, 14, 30], 11)
    c["wild_large_id"] = _case([s[0], wildcard_cases.plant(s[1], [13], 1000), wildcard_cases.plant(s[2], [9, 15], 1000)], wild=[6, 1000],
                               expect={"wild_on": 1, "sigma": 4})
    s = _dna([G + 31, G + 32, G + 63, G + 63], 12)
    c["wild_vbits_words"] = _case([wildcard_cases.plant(s[0], [0]), wildcard_cases.plant(s[1], [0]), wildcard_cases.plant(s[2], [0]), wildcard_cases.plant(s[3], [40])],
                                  wild=[5], expect={"vstart": [0, 1, 3, 5, 7]})
    c["wild_no_window"] = _case([_dna([12], 13)[0], wildcard_cases.plant(_dna([14], 14)[0], [3, 9]), _dna([9], 15)[0]], wild=[5],
                                expect={"code": ESHORT, "msg": "sequence 1 has no window of length g = 6 that is free of wildcards: it would have no features"})
    c["wild_complement_not_wild"] = _case(_dna([8, 9], 16), comp={**DNA, 5: 6, 6: 5}, wild=[5],
                                          expect={"code": EINVAL, "msg": "wildcard token 5 has the complement 6, which is not a wildcard"})
    # centre weights: lengths up to 26 reach distance 10
    lens = [6, 7, 8, 26, 15, 20]
    c["cw_all_one_in_reach"] = _case(_dna(lens, 17), profile=[1] * 11 + [7, 0], expect={"cw_on": 0, "wild_on": 0, "nvalid": [], "fwin": []})
    c["cw_zero_in_reach"] = _case(_dna(lens, 18), profile=[1, 1, 0, 1, 0], expect={"cw_on": 1, "wild_on": 1})
    c["cw_zero_no_window"] = _case([_dna([20], 19)[0], wildcard_cases.plant(_dna([17], 20)[0], [8])], profile=[1, 0], wild=[5],
                                   expect={"code": ESHORT, "msg": "sequence 1 has no window of length g = 6 that is free of wildcards and has a center weight above 0: "
                                                                  "it would have no features"})
    c["cw_sums"] = _case(_dna(lens, 21), profile=[3, 2, 2, 5, 1], expect={"cw_on": 1, "wild_on": 0, "vbits": []})
    c["cw_revcomp"] = _case(_dna(lens, 22), profile=[3, 2, 0, 4, 1], comp=DNA, expect={"cw_on": 1, "wild_on": 1, "rc_on": 1})
    c["cw_wild_revcomp"] = _case([wildcard_cases.plant(q, [len(q) // 3]) if len(q) > 14 else q for q in _dna(lens, 23)], profile=[2, 1, 3], comp=DNA, wild=[5],
                                 expect={"cw_on": 1, "wild_on": 1, "rc_on": 1})
    # wide keys
    c["wide_keys"] = _case(_cover(range(300), [10, 11], 24), g=10, expect={"sigma": 300, "key_symbits": 9, "V": 2 ** 62})
    c["wide_keys_too_wide"] = _case(_cover(range(300), [13, 14], 25), g=13,
                                    expect={"code": EUNSUPPORTED, "msg": "a k-mer of 11 symbols of 9 bits does not fit the 128-bit sort records"})
    # errors
    c["offsets_decreasing"] = dict(_case(_dna([8, 8, 8], 26)), offsets=[0, 8, 7, 24], expect={"code": EINVAL, "msg": "offsets must be non-decreasing"})
    short = "g cannot be longer than the shortest sequence in a dataset. g = 6, but shortest %s sequence has length 5"
    c["short_train"] = _case(_dna([8, 5, 9, 4], 27), n_train=2, expect={"code": ESHORT, "msg": short % "train"})
    c["short_test"] = _case(_dna([8, 7, 9, 5], 28), n_train=2, expect={"code": ESHORT, "msg": short % "test"})
    # the team: 1024 x 257 = 263,168 tokens >= 2^18, four threads
    c[TEAM] = _case(_dna([257] * 1024, 29), expect={"bits": 2, "n_words": 1024 * 17})
    return c
