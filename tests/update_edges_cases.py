"""Inputs, the restated plan and the reach proofs of the sparse dataflow's UPDATE stage — k_sx_seg_write's classification,
k_sx_ucol_*, k_sx_emit, k_sx_parts, k_sx_consume with sx_expand_descriptors, the by-slot stores and k_sxb_count / scan / scatter /
drecords / consume — shared by tests/test_emu_update_edges.py and tests/test_gpu_update_edges.py. Nothing here touches an engine.

The yardsticks are sort_edges_cases' (imported, not copied): ``counts_by_definition_wide`` for the cells and U, proved against the
CPU oracle by ``check_reference``; ``sorted_records`` for the entries (every record its own line: a segment tile is the 2048
records ``first // SG_TILE`` names, as ``segment_tiles`` cuts them). Three things are added:

  the plan    ``band_plan`` (plan_owner_bands), ``choose_form`` (sx_choose_form), ``blocks_pass_plan`` (blocks_plan_pass) and
              ``blocks_passes`` (the loop of sx_update_blocks): what the host derives from N and the tuning alone;
  the model   ``update_model``: per entry its row, multiplicity, rank, partners that take a word, unit mark, words a pair, the
              class k_sx_emit gives it, its owner band and how far before its tile its run begins; per tile the short-word total
              and the passes; per band the words, paired cells, descriptors and the parts k_sx_parts cuts;
  the inputs  ``key_rows``: with g = 2, m = 1 and combination 0 the key of a window is its first symbol, so a sequence that holds
              symbol v c times (and one closing symbol) has one entry of multiplicity c in the run of v. Runs, ranks,
              multiplicities and their place against the 2048-record tiles are chosen one by one.

The model exists to PROVE REACH: every case asserts from it that it sits on the edge it is named after, and a case that drifts off
fails before an engine is asked. Its output is never compared with an engine: engines are compared with the reference alone."""
import numpy as np

import sort_edges_cases as sec
from sort_edges_cases import SG_TILE, THREADS, sorted_records

# ---- the constants of the update stage, restated once (test_constants_match_the_sources greps the engine for each) --------------
SX_SHORT = 48            # fsk_sparse_kernels.inc:65
EM_SLOTS = 11800         # fsk_sparse_kernels.inc:71
EM_CAP = EM_SLOTS - SX_SHORT
EM_MAX_PASS = SG_TILE * SX_SHORT // EM_CAP + 1
SX_CAP = 20480           # fsk_engine_sparse.hip:18
SX_MAX_ROUNDS = 16       # fsk_engine_sparse.hip:19
SX_BLOCKS_FROM_ROUNDS = 4
SX_MAX_OWNERS = 512      # fsk_sparse_kernels.inc:42
SX_DESC_WORDS = 4
SX_DESC_WEIGHT = 16      # fsk_sparse_kernels.inc:2103
SX_DESC_MULT_BITS = 20
DESC_GROUP = {1: 16, 2: 8}             # lanes a descriptor: owner bands, two-level blocks
DESC_PER = {0: 4, 1: 2, 2: 8, 3: 4}    # partners a 16-byte load, by partner format (sx_expand_descriptors' FMT)
SXB_TILE = 1024 * 8      # words a tile of k_sxb_scatter
SXD_PIECE = 1024 * 8     # records a piece of k_sxb_drecords
SXB_MAX_SUB = 2048
CS_THREADS = 1024

SOURCE_CONSTANTS = [   # (file, text that must occur in it)
    ("fsk_sparse_kernels.inc", "#define FSK_SX_SHORT %d " % SX_SHORT),
    ("fsk_sparse_kernels.inc", "#define FSK_EM_SLOTS %d " % EM_SLOTS),
    ("fsk_sparse_kernels.inc", "#define FSK_SG_TILE %d " % SG_TILE),
    ("fsk_sparse_kernels.inc", "#define FSK_SX_MAX_OWNERS %d\n" % SX_MAX_OWNERS),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t EM_CAP = EM_SLOTS - SX_SHORT;"),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t EM_MAX_PASS = (uint32_t)SG_TILE * SX_SHORT / EM_CAP + 1u;"),
    ("fsk_sparse_kernels.inc", "return short_words <= EM_SLOTS;"),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t SX_DESC_WORDS = %d;" % SX_DESC_WORDS),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t SX_DESC_WEIGHT = %d;" % SX_DESC_WEIGHT),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t SX_DESC_MULT_BITS = %d;" % SX_DESC_MULT_BITS),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t PER = FMT == 0 ? 4u : FMT == 1 ? 2u : FMT == 2 ? 8u : 4u;"),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t CHUNK = GROUP * PER;"),
    ("fsk_sparse_kernels.inc", "#define FSK_DESC_GROUP %du " % DESC_GROUP[1]),
    ("fsk_sparse_kernels.inc", "constexpr uint32_t CS_THREADS = %d;" % CS_THREADS),
    ("fsk_sparse_kernels.inc", "my_np[q] <= 32u"),
    ("fsk_sparse_blocks.inc", "sx_expand_descriptors_fmt<SXB_THREADS, false, %du>" % DESC_GROUP[2]),
    ("fsk_sparse_blocks.inc", "constexpr uint32_t SXB_THREADS = 1024;"),
    ("fsk_sparse_blocks.inc", "constexpr uint32_t SXB_PER = 8; "),
    ("fsk_sparse_blocks.inc", "constexpr uint32_t SXD_PER = 8, SXD_PIECE = 1024 * SXD_PER;"),
    ("fsk_sparse_blocks.inc", "constexpr uint32_t SXB_MAX_SUB = %d; " % SXB_MAX_SUB),
    ("fsk_engine_sparse.hip", "constexpr uint32_t SX_CAP = %d; " % SX_CAP),
    ("fsk_engine_sparse.hip", "constexpr uint32_t SX_MAX_ROUNDS = %d;" % SX_MAX_ROUNDS),
    ("fsk_engine_sparse.hip", "constexpr uint32_t SX_CAP_SLOT = %d; " % SX_CAP),
    ("fsk_engine_sparse.hip", "constexpr uint32_t SX_BLOCKS_FROM_ROUNDS = %d; " % SX_BLOCKS_FROM_ROUNDS),
    ("fsk_engine_sparse.hip", "largest <= 32766"),
]


def tri(i):
    return i * (i + 1) // 2


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def _first_rows(rows, base, t, nb, fill):
    """r0[o] = the first row of ``rows`` whose first cell, counted from ``base``, reaches o << t (``fill`` where none does)."""
    r0, o = [fill] * (nb + 1), 0
    for i in rows:
        while o <= nb and tri(i) - base >= (o << t):
            r0[o] = i
            o += 1
    return r0


def band_plan(N, pairs_asked=True):
    """plan_owner_bands (fsk_engine_sparse.hip:64-107): the owner bands of N sequences — shift t, bands, their first rows, the
    largest band's cells, product bits, whether unit products travel in pairs, LDS rounds and cells a round; ``lists``: the
    bands exist (line 105)."""
    cells, t = tri(N), 13
    while t < 20 and (1 << (t + 1)) + N <= SX_CAP:
        t += 1
    while (cells + (1 << t) - 1) >> t > SX_MAX_OWNERS:
        t += 1
    n_owners = (cells + (1 << t) - 1) >> t
    r0 = _first_rows(range(N), 0, t, n_owners, N)
    largest = max([tri(r0[q + 1]) - tri(r0[q]) for q in range(n_owners)] or [0])
    L = 1
    while (1 << L) < largest:
        L += 1
    pb = 32 - L
    pairs = bool(pairs_asked) and largest <= 32766
    if pairs:
        pb = 16
    rounds = max(1, (largest + SX_CAP - 1) // SX_CAP)
    return dict(N=N, t=t, n_owners=n_owners, r0=r0, largest=largest, pb=pb, pairs=pairs, rounds=rounds, cap=max(1, min(SX_CAP, largest)),
                lists=n_owners <= SX_MAX_OWNERS and rounds <= SX_MAX_ROUNDS and pb >= 8)


def blocks_pass_plan(N, ra, rb, tuning=None, exists_only=False):
    """blocks_plan_pass (fsk_engine_sparse.hip:28-62) for rows [ra, rb) under the tuning's blocks_sub_shift / blocks_max_bands /
    blocks_band_shift_max: None when the range is no pass, else t, bands, their first rows, product bits, sub-bands a band.
    ``exists_only`` (the call with out == nullptr): True when the form exists for N sequences at all."""
    tuning = tuning or {}
    sub_shift, max_bands, t_max = tuning.get("blocks_sub_shift", 14), tuning.get("blocks_max_bands", 512), tuning.get("blocks_band_shift_max", 23)
    c_lo, cells = tri(ra), tri(rb) - tri(ra)
    while t_max > sub_shift and (1 << t_max) + N > (1 << 24):
        t_max -= 1
    if (1 << t_max) + N > (1 << 24) or ((((1 << t_max) + N) >> sub_shift) + 1) > SXB_MAX_SUB:
        return None
    if exists_only:
        return True
    if rb - ra > 1 and (cells > ((max_bands - 1) << t_max) or cells >= 1 << 32):
        return None
    t = sub_shift
    while t < t_max and ((cells + (1 << t) - 1) >> t) > max_bands:
        t += 1
    nb = max(1, (cells + (1 << t) - 1) >> t)
    if nb > SX_MAX_OWNERS:
        return None
    r0 = _first_rows(range(ra, rb), c_lo, t, nb, rb)
    largest = max(tri(r0[q + 1]) - tri(r0[q]) for q in range(nb))
    L = 1
    while (1 << L) < largest:
        L += 1
    submax = ((largest + (1 << sub_shift) - 1) >> sub_shift) + 1
    if 32 - L < 8 or submax > SXB_MAX_SUB:
        return None
    return dict(ra=ra, rb=rb, t=t, sub_shift=sub_shift, n_owners=nb, r0=r0, largest=largest, pb=32 - L, submax=submax, own_base=c_lo)


def blocks_passes(N, words_of, tuning=None, nrec=0):
    """The loop of sx_update_blocks (fsk_engine_sparse.hip:751-816) for the FIRST batch (of ``nrec`` records) of a set of
    sequences: the passes in the order they run. ``words_of(plan)``: the update words rows [ra, rb) emit under the pass's bands.
    A range that is no pass, or whose words reach blocks_pass_words, is halved by cells — and so is one that the words per record
    seen in the passes so far (fsk_engine_internal.h:352-354) say would pass 0.9 of blocks_pass_words."""
    tuning = tuning or {}
    pass_words = tuning.get("blocks_pass_words", 0) or 1 << 31
    todo, out, wpr, total = [(0, N)], [], 0.0, tri(N)
    while todo:
        ra, rb = todo.pop()
        if rb <= ra:
            continue
        cells = tri(rb) - tri(ra)
        too_many = wpr != 0 and rb - ra > 1 and float(int(wpr * float(nrec)) + 1) * (float(cells) / float(max(1, total))) > 0.9 * float(pass_words)
        P = None if too_many else blocks_pass_plan(N, ra, rb, tuning)
        if P is not None:
            P["words"] = words_of(P)
        if P is None or (P["words"] >= pass_words and rb - ra > 1):
            assert rb - ra > 1
            mid = tri(ra) + (tri(rb) - tri(ra)) // 2
            lo, hi = ra + 1, rb - 1
            while lo < hi:
                mm = (lo + hi) // 2
                if tri(mm) < mid:
                    lo = mm + 1
                else:
                    hi = mm
            todo.append((lo, rb))
            todo.append((ra, lo))
            continue
        out.append(P)
        if P["words"] and nrec:
            wpr = max(wpr, max(1e-9, float(P["words"] * max(1, total // max(1, cells))) / float(nrec)))
    return out


def choose_form(plan, tuning=None, desc_now=False):
    """sx_choose_form (fsk_engine_sparse.hip:112-126) -> stats()["sparse_form"]: 0 owner bands, 2 two-level blocks, 1 atomics."""
    tuning = tuning or {}
    want = tuning.get("sparse_form", 0)
    blocks_ok = blocks_pass_plan(plan["N"], 0, plan["N"], tuning, exists_only=True) is not None
    max_rounds = 1 if desc_now and tuning.get("sparse_desc_blocks", 1) else SX_BLOCKS_FROM_ROUNDS
    if want == 3 or tuning.get("sparse_global"):
        return 1
    if want == 2 and blocks_ok:
        return 2
    if want == 1 and plan["lists"]:
        return 0
    if plan["lists"] and plan["rounds"] <= max_rounds:
        return 0
    return 2 if blocks_ok else 0 if plan["lists"] else 1


# ---- the inputs -----------------------------------------------------------------------------------------------------------------
def key_rows(N, keys, private=True):
    """Sequences for g = 2, m = 1, combination 0. ``keys``: one dict {row: multiplicity} a key, in key order (key q is symbol
    q + 1). Sequence i = symbol v repeated keys[v][i] times for every key that names it, then one closing symbol (the largest of
    all: it starts no window). ``private``: a row no key names gets a key of its own behind the others (a run of one entry, no
    update word). -> the sequences."""
    per = [[] for _ in range(N)]
    for q, rows in enumerate(keys):
        for i, c in rows.items():
            assert 0 <= i < N and c >= 1
            per[i] += [q + 1] * c
    nk = len(keys)
    for i in range(N):
        if not per[i]:
            assert private, "row %d holds no key" % i
            nk += 1
            per[i] = [nk]
    return [s + [nk + 1] for s in per]


def run(rows, c=1):
    """One key: the rows given, each with multiplicity c."""
    return {int(i): c for i in rows}


def triangular_runs(words, dmax):
    """Run lengths d <= dmax whose d (d - 1) / 2 sum to ``words`` (greedy: the largest first)."""
    out = []
    while words:
        d = 2
        while d < dmax and tri(d) <= words:
            d += 1
        out.append(d)
        words -= tri(d - 1)
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------
def entries_of(X, g=2, m=1, combo=0, n_train=None, skip=False):
    """The entries of one slot from its sorted records: arrays row, c (multiplicity), P (rank in the run, from 1), T (partners
    before itself: P - 1; a test row under skip_test_block: the run's train entries), first (its first record), head (the entry
    index of its run's head)."""
    rec, sb = sorted_records(X, g, combo, m)
    prev = np.concatenate([[-1], rec[:-1]])
    start = np.flatnonzero(rec != prev)
    row = (rec[start] & ((1 << sb) - 1)).astype(np.int64)
    key = rec[start] >> sb
    c = np.diff(np.concatenate([start, [len(rec)]]))
    is_head = np.concatenate([[True], key[1:] != key[:-1]])
    head = np.maximum.accumulate(np.where(is_head, np.arange(len(start)), 0))
    P = np.arange(len(start)) - head + 1
    T = P - 1
    if skip:
        ntr = len(X) if n_train is None else n_train
        train_in_run = np.add.reduceat((row < ntr).astype(np.int64), np.flatnonzero(is_head))
        T = np.where(row >= ntr, train_in_run[np.cumsum(is_head) - 1], T)
    return dict(row=row, c=c, P=P, T=T, first=start, head=head, nrec=len(rec))


def update_model(X, n_train=None, skip=False, tuning=None, bands=None, desc=None, g=2, m=1, combo=0):
    """What the update stage makes of one slot. ``bands``: the owner bands (band_plan) or one pass of the blocks form
    (blocks_pass_plan); None: band_plan under the tuning's sparse_pairs. ``desc``: 0 none, 1 one descriptor an entry, 2 one per
    sub-band (None: 1 when the tuning forces sparse_desc on owner bands, 2 on blocks).
    Per entry (k_sx_seg_write, fsk_sparse_kernels.inc:1067-1118, and k_sx_emit's classes, 1465-1479):
      np      partners that take a word: T, and itself when its multiplicity is above 1
      unit    k_sx_seg_write's mark: pairs on, multiplicity 1, its run's head in the same 512 records of the same tile and no
              entry of multiplicity above 1 from the head up to it; in band and short
      wpp     sx_words_per_pair (line 884)
      cls     0 none, 1 short, 4 short and unit, 5 descriptor, 3 half-wave (at most 32 partners), 2 long
      band    sx_owner_of its row;   tile, el: its segment tile and index among the tile's entries
      before  how many entries before its tile's first its first partner lies (0: inside the tile)
    Per tile: entries, short-word total, one_pass, and the passes [ea, eb, words] k_sx_emit takes (lines 1543-1571, 1747-1756).
    Per band: 32-bit words, paired cells, containers, descriptor words, the stream offsets and the parts of k_sx_parts /
    k_sx_consume (lines 2107-2211): (band, part, parts, a, b, first descriptor, stride)."""
    tuning = tuning or {}
    N = len(X)
    blocks = bands is not None and "sub_shift" in bands
    if bands is None:
        bands = band_plan(N, tuning.get("sparse_pairs", 1))
    if desc is None:
        desc = 0 if tuning.get("sparse_desc", 0) != 1 else 2 if blocks else 1
    if blocks and not tuning.get("sparse_desc_blocks", 1):
        desc = 0
    pairs = bool(bands.get("pairs")) and not blocks
    pb, t, O, r0 = bands["pb"], bands["t"], bands["n_owners"], bands["r0"]
    own_base = bands.get("own_base", 0)
    row0, row1 = (bands["ra"], bands["rb"]) if blocks else (0, N)
    maxW = max(len(s) - g + 1 for s in X)
    maxprod = (1 << pb) - 1
    cmax, cwide = maxprod // max(1, maxW), 0xffffffff // max(1, maxW)
    short_max = min(tuning.get("sparse_desc_min", 16), SX_SHORT) if desc else SX_SHORT
    E = entries_of(X, g, m, combo, n_train, skip)
    n = len(E["row"])
    row, c, P, T, first, head = (E[k] for k in ("row", "c", "P", "T", "first", "head"))
    np_ = T + (c > 1)
    in_band = (row >= row0) & (row < row1)
    wpp = np.where(c <= cmax, 1, -(-(c * maxW) // maxprod))
    is_short = (np_ != 0) & (np_ <= short_max) & (c <= cmax)
    desc_ok = (c < (1 << SX_DESC_MULT_BITS)) & (c <= cwide) & ((c <= cmax) | (desc == 1)) & bool(desc)
    tile = first // SG_TILE
    ebase = np.searchsorted(tile, np.arange(tile.max() + 2))   # (first entry of every tile)
    el = np.arange(n) - ebase[tile]
    # the unit mark: the run's head in the same wave (512 records) of the same tile, a clean run up to the entry
    many = np.cumsum(c > 1)                                     # entries of multiplicity above 1 up to and including e
    many_before_head = many[head] - (c[head] > 1)
    clean = pairs & (c == 1) & (first[head] // 512 == first // 512) & (many == many_before_head)
    unit = clean & in_band & is_short
    cls = np.zeros(n, dtype=np.int64)
    act = in_band & (np_ != 0)
    one_word = wpp == 1
    short_e = act & (np_ <= short_max) & one_word
    cls[short_e] = np.where(unit[short_e], 4, 1)
    rest = act & ~short_e
    cls[rest & desc_ok] = 5
    rest &= ~desc_ok
    cls[rest] = np.where(one_word[rest] & (np_[rest] <= 32) & (not skip), 3, 2)
    band = (np.array([tri(int(i)) for i in row], dtype=np.int64) - own_base) >> t
    before = np.maximum(0, (P - 1) - el) * (np_ != 0)
    if skip:   # (a test row pairs with its run's FIRST T entries, however far back the run began)
        before = np.maximum(0, (P - 1) - el) * (T != 0)
    wide = c > cwide
    words_e = np.where(cls == 5, 0, np.where(act & wide, 1, np_ * wpp)) * act
    rec_e = ((row >> bands["sub_shift"]) + 2 if desc == 2 else np.ones(n, dtype=np.int64)) * (cls == 5)
    own_e = (cls == 5) & (desc == 2) & (c > 1)                  # (blocks: a descriptor entry's own cell as one update word)
    tiles, cnt = [], np.zeros((len(ebase) - 1, O), dtype=np.int64)
    cntu, cntd = np.zeros_like(cnt), np.zeros_like(cnt)
    for tl in range(len(ebase) - 1):
        a, b = int(ebase[tl]), int(ebase[tl + 1])
        sw = np.where((cls[a:b] == 1) | (cls[a:b] == 4), np_[a:b], 0)
        allw = int(sw.sum())
        one_pass = allw <= EM_SLOTS
        passes = [[0, b - a, allw]]
        if not one_pass:
            after = np.cumsum(sw)
            bnd = [0] + [b - a] * EM_MAX_PASS
            for e in np.flatnonzero(sw):
                if after[e] >= EM_CAP and (after[e] - sw[e]) // EM_CAP != after[e] // EM_CAP:
                    bnd[after[e] // EM_CAP] = int(e) + 1
            n_pass = allw // EM_CAP + 1
            ends = [bnd[p + 1] if p + 1 < n_pass else b - a for p in range(n_pass)]
            passes = [[bnd[p], ends[p], int(sw[bnd[p]:ends[p]].sum())] for p in range(n_pass)]
        for e in range(a, b):
            if not act[e]:
                continue
            if cls[e] == 5:
                cntd[tl, band[e]] += SX_DESC_WORDS * rec_e[e]
                cnt[tl, band[e]] += int(own_e[e])
            elif unit[e]:
                cntu[tl, band[e]] += words_e[e]
            else:
                cnt[tl, band[e]] += words_e[e]
        tiles.append(dict(n=b - a, e0=a, short_words=allw, one_pass=one_pass, passes=passes))
    one = np.array([tl["one_pass"] for tl in tiles])[:, None]
    containers = np.where(one, (cntu + 1) >> 1, cntu) if pairs else np.zeros_like(cntu)
    words_b = (cnt + containers).sum(axis=0)
    dwords_b = cntd.sum(axis=0)
    off_d = np.concatenate([[0], np.cumsum(dwords_b)])
    off_w = off_d[-1] + np.concatenate([[0], np.cumsum(words_b)])
    # k_sx_parts / k_sx_consume
    total = int(words_b.sum() + dwords_b.sum())
    target = tuning.get("sparse_parts_target", 0) or max(4 * bands.get("cap", 1), (total + 1023) // 1024)
    work = words_b + (SX_DESC_WEIGHT * dwords_b if desc else 0)
    if desc:
        target = max(target, -(-int(work.sum()) // max(1, tuning.get("sparse_desc_parts", 2048))))
    parts = []
    for o in range(O):
        nparts = -(-int(work[o]) // target)
        for p in range(nparts):
            if not desc:
                a = int(off_w[o]) + p * target
                b = min(int(off_w[o + 1]), a + target)
            else:
                ln = int(words_b[o])
                piece = (-(-ln // nparts) + 3) & ~3
                a = int(off_w[o]) + min(p * piece, ln)
                b = min(int(off_w[o + 1]), a + piece)
            parts.append(dict(band=o, part=p, parts=nparts, a=a, b=b, nd=max(0, -(-(int(dwords_b[o]) // SX_DESC_WORDS - p) // nparts)) if desc else 0))
    return dict(N=N, bands=bands, pairs=pairs, desc=desc, short_max=short_max, cmax=cmax, maxW=maxW, n=n,
                ent=dict(row=row, c=c, P=P, T=T, np=np_, unit=unit, wpp=wpp, cls=cls, band=band, before=before, tile=tile, el=el, first=first, head=head),
                tiles=tiles, band_words=cnt.sum(axis=0), band_cells=cntu.sum(axis=0), band_containers=containers.sum(axis=0),
                band_stream=words_b, band_desc=dwords_b // SX_DESC_WORDS, off_w=off_w, off_d=off_d, target=target, parts=parts,
                tile_cells=cntu, U=int(((T + 1) * in_band).sum()))


def updates_by_definition(X, n_train, g=2, m=1, combos=(0,)):
    """U under skip_test_block by definition, from the windows alone (no entries, no model): a key that d_tr train and d_te test
    sequences hold costs d_tr (d_tr + 1) / 2 updates for its train rows and d_tr + 1 for each test row (its train columns and
    its own diagonal cell)."""
    win, seq = sec.windows_of(X, g)
    U = 0
    for c in combos:
        kept = np.ascontiguousarray(win[:, list(sec.combo_positions(g, g - m, c))])
        _, inv = np.unique(kept, axis=0, return_inverse=True)
        pairs = np.unique(np.stack([np.asarray(inv).reshape(-1), seq]), axis=1)   # (key, sequence), each once
        nk = int(pairs[0].max()) + 1
        d_tr = np.bincount(pairs[0][pairs[1] < n_train], minlength=nk)
        d_te = np.bincount(pairs[0][pairs[1] >= n_train], minlength=nk)
        U += int((d_tr * (d_tr + 1) // 2 + d_te * (d_tr + 1)).sum())
    return U


def sub_band_counts(model):
    """Blocks form: ({(band, sub-band): update words}, {(band, sub-band): descriptor records with partners}). A word goes to the
    sub-band of its cell; a descriptor entry leaves one record for every sub-band its partners fall into and its own cell
    (multiplicity above 1) as a word."""
    ent, bands = model["ent"], model["bands"]
    sh = bands["sub_shift"]
    words, recs = {}, {}
    for e in np.flatnonzero(ent["cls"] != 0):
        o = int(ent["band"][e])
        cells = partner_cells(model, e) >> sh
        own = (tri(int(ent["row"][e])) - tri(bands["r0"][o]) + int(ent["row"][e])) >> sh
        if ent["cls"][e] == 5:
            for x in set(cells.tolist()):
                recs[o, x] = recs.get((o, x), 0) + 1
        else:
            for x in cells.tolist():
                words[o, x] = words.get((o, x), 0) + int(ent["wpp"][e])
        if ent["c"][e] > 1:
            words[o, own] = words.get((o, own), 0) + (1 if ent["cls"][e] == 5 else int(ent["wpp"][e]))
    return words, recs


def partner_cells(model, e):
    """The cells, counted from its band's first cell, that entry e's T partners before itself go to (rising with the partner)."""
    ent, bands = model["ent"], model["bands"]
    h = int(ent["head"][e])
    cols = ent["row"][h:h + int(ent["T"][e])]
    return tri(int(ent["row"][e])) - tri(bands["r0"][int(ent["band"][e])]) + cols


# ---- cases ----------------------------------------------------------------------------------------------------------------------
_ONCE = {}


def case(name, build, n_train=None, combos=(0,), g=2, m=1, oracle=False, port=None):
    """A case and its reference, computed once per process and shared read-only: X, N, n_train, combos, want (the lower triangle,
    uint64), U, top. ``oracle``: the cells from port.raw_counts (group A's large N: int64 C C^T is too slow there) — asserted to
    stay far below 2^32, where the oracle's cells would wrap."""
    if name not in _ONCE:
        X = build()
        combos_a = np.asarray(combos, dtype=np.int32)
        if oracle:
            from oracle import loader
            tok, off = loader.flatten(X)
            want, _, U = port.raw_counts(tok, off, g, m, combos_a, threads=THREADS)
            assert int(want.max()) < 2 ** 28
        else:
            want, U, _ = sec.counts_by_definition_wide(X, g, m, combos_a)
        top = max(len(s) - g + 1 for s in X)   # (stats()["max_windows"])
        want.setflags(write=False)
        _ONCE[name] = dict(X=X, N=len(X), n_train=len(X) if n_train is None else n_train, combos=combos_a, g=g, m=m, want=want, U=U, top=top)
    return _ONCE[name]


def padded(keys_front, n_pad_records, per=16):
    """Keys whose runs hold nothing but one entry each, ``n_pad_records`` records in all, to be put in front of the keys under test:
    they move what follows along the record axis (and so against the 2048-record tiles). -> (list of {row: c} with rows counted
    from 0, rows used). Each pad entry has multiplicity <= per: one own-cell word, short."""
    keys, i, left = [], 0, n_pad_records
    while left:
        cc = min(per, left)
        keys.append({i: cc})
        i, left = i + 1, left - cc
    return keys, i


def with_test_rows(N, keys):
    """Adds the key {N - 3, N - 2, N - 1} behind the others and returns n_train = N - 2: two test rows that share a key with each
    other and with one train row, so that skip_test_block has a test x test cell to leave alone — rows no other key names."""
    for rows in keys:
        assert not set(rows) & {N - 3, N - 2, N - 1}
    return keys + [run([N - 3, N - 2, N - 1])], N - 2


# ---- group B: the entry classes of k_sx_emit, one tile ------------------------------------------------------------------------
def b_partners():
    """Key 0: rows 0..49, multiplicity 1 — partners 0..49. Key 1: rows 0..48, rows 47 and 48 with multiplicity 2: 47 + own = 48,
    48 + own = 49. Key 2: rows 0..9, row 3 with multiplicity 2 — clean up to its third entry, not after."""
    N = 64
    keys, ntr = with_test_rows(N, [run(range(50)), {**run(range(47)), 47: 2, 48: 2}, {**run(range(10)), 3: 2}])
    return key_rows(N, keys), ntr


def b_cmax():
    """max_windows = 257 by row 0 (a key of its own); a run over rows 1..5 with multiplicities 1, 255, 256, 1, 1: under pairs
    cmax = 65535 // 257 = 255 — one word a pair at 255, two at 256."""
    N = 12
    keys, ntr = with_test_rows(N, [{0: 257}, {1: 1, 2: 255, 3: 256, 4: 1, 5: 1}])
    return key_rows(N, keys), ntr


def b_skip():
    """skip_test_block, n_train = 60: test rows with T = 0 (a run of test rows only), 1, 48 and 49 train partners."""
    N, ntr = 70, 60
    keys = [run([60, 61]), run([0, 62, 63]), run(list(range(48)) + [64, 65]), run(list(range(49)) + [66, 67])]
    return key_rows(N, keys), ntr


# ---- group C: the slot array -------------------------------------------------------------------------------------------------
def c_slots(front, full, N=420):
    """One tile, six owner bands. In key order: row 0 alone with multiplicity 2 (the tile's entry 0 is a binned entry of one word,
    its own cell: its record is what a slot beyond the slot array would overwrite); runs of 2, 3 and 4 rows in bands 1, 2 and 3
    (1, 3 and 6 words: one, an odd and an even number of unit cells); runs over rows 0.. of band 0 that bring the words so far
    to ``front``; ``full`` runs of 49 rows (1176 words each: partners 0..48); the test rows' run in band 5 (3 words; 2 under
    skip_test_block). Band 4 holds rows 362..404, none of which any key names: no word, no paired cell. The running sum over the
    tile's short entries is ``front`` before the full runs and front + 1176 full + 3 (2) in all."""
    keys = [{0: 2}, run([181, 182]), run([256, 257, 258]), run([314, 315, 316, 317])]
    keys += [run(range(d)) for d in triangular_runs(front - 11, 48)] + [run(range(49)) for _ in range(full)]
    keys, ntr = with_test_rows(N, keys)
    return key_rows(N, keys), ntr


def c_total(front, full, skip=False):
    return front + tri(48) * full + (2 if skip else 3)


def c_fullest():
    """skip_test_block: 2000 records of single-entry keys (rows 0..124, 16 windows each), then ONE run of 48 train rows and 2048
    test rows: under skip every test entry has exactly 48 partners, and the run's test entries are exactly tile 1 — 2048 entries
    of 48 words, the most a tile can hold (EM_MAX_PASS passes)."""
    pad, used = padded([], 2000)
    N = used + 48 + 2048
    return key_rows(N, pad + [run(range(used, N))]), used + 48


# ---- group D: runs across tile edges -----------------------------------------------------------------------------------------
def d_straddle(pad_records, d, N=None):
    """``pad_records`` records of single-entry keys, then one run of d rows of multiplicity 1: the run's entry number
    2048 - pad_records is the first of tile 1."""
    pad, used = padded([], pad_records)
    N = N or used + d + 3
    keys, ntr = with_test_rows(N, pad + [run(range(used, used + d))])
    return key_rows(N, keys), ntr


def d_e0(e0):
    """Tile 0 holds exactly e0 entries — one run of e0 rows whose multiplicities sum to 2048 — and the run goes on into tile 1
    with 20 rows of multiplicity 1: tile 1's first entry has e0 partners, all of them the e0 entries in front of the tile."""
    lo, extra = divmod(2048, e0)
    N = e0 + 20 + 3
    keys, ntr = with_test_rows(N, [{**{i: lo + (1 if i < extra else 0) for i in range(e0)}, **run(range(e0, e0 + 20))}])
    return key_rows(N, keys), ntr


def d_far():
    """One run of 4200 rows of multiplicity 1: the entries of tile 2 have 4096 and more partners before the tile."""
    return key_rows(4200, [run(range(4200))]), 4200


# ---- group E: parts and streams of k_sx_consume ------------------------------------------------------------------------------
def band_rows(N, pairs_asked=True):
    p = band_plan(N, pairs_asked)
    return [(p["r0"][o], p["r0"][o + 1]) for o in range(p["n_owners"])]


def e_words(N, per_band, unit=True):
    """Band o gets the runs whose words sum to per_band[o] (0: none), over the band's first rows; multiplicity 1 (``unit``: every
    word a unit cell under pairs) or, else, the run's first row with multiplicity 2 (no unit entry: every word 32 bits)."""
    keys = []
    for (lo, hi), w in zip(band_rows(N), per_band):
        for d in triangular_runs(w if unit else 0, hi - lo):
            keys.append(run(range(lo, lo + d)))
        if not unit and w:   # a head of multiplicity 2: own cell + d - 1 partner words, none of them unit
            left = w
            while left:
                d = 2
                while d < hi - lo and 1 + tri(d) <= left:
                    d += 1
                d = min(d, hi - lo)
                if 1 + tri(d - 1) > left:
                    keys.append({lo: 2})   # (one own-cell word)
                    left -= 1
                    continue
                keys.append({**run(range(lo, lo + d)), lo: 2})
                left -= 1 + tri(d - 1)
    return key_rows(N, keys), N


def e_desc(N=150, runs=8, d=130, big=None):
    """``runs`` runs over rows 0..d-1 with ONE single-entry key between two runs, so that the runs' first entries lie at entry
    indices 0, d + 1, 2 (d + 1), ...: every residue of a 16-byte load. Row 1 has multiplicity 2 in every run (a partner of
    multiplicity above 1, and an own cell); ``big``: row 2's multiplicity in run 0 (256: it does not fit a 2-byte column)."""
    keys = []
    for r in range(runs):
        k = {**run(range(d)), 1: 2}
        if big and r == 0:
            k[2] = big
        keys += [k, {d + r: 1}]
    return key_rows(N, keys), N
