// fsk_sparse_kernels.inc — the sparse dataflow of the gapped-k-mer engine (included by fsk_kernels_sparse.h,
// inside namespace fsk, after the shared helpers: SeqView, fetch_sym, tri_index, the block scans).
// The reference's own dataflow — gather kept positions, stable LSD counting sort (cntsrtna,
// shared.cpp:156-191), run-length co-occurrence count (countAndUpdateTri, shared.cpp:268-333) —
// rebuilt so that every pass streams and nothing gathers.
// =============================================================================================
// SPARSE PATH — the reference's dataflow (gather -> sort -> run-length -> K +=), as streams
// =============================================================================================
// Per batch of B combos ("slots"):
//   k_sx_extract   one packed record per (slot, g-mer): rec = (k-mer << sb) | sequence id, u32 when
//                  that fits 32 bits (every BASELINE config), else u64, else 128 bits; slot s owns rec[s*nfeat ..):
//                  the slot is implicit in the position, so B independent sorts run in one launch.
//   k_sx_hist / k_sx_scan_slot / k_sx_scatter   stable LSD radix sort over the k-mer bits only
//                  (records are generated in sequence order and every pass is stable), 8-bit digits,
//                  4096-record tiles ranked with wave64 ballot matching, permuted in LDS and written
//                  out in digit runs.
//   k_sx_seg_count / k_sx_seg_scan / k_sx_seg_write   sorted records -> compact entries
//                  E[e] = {sequence, multiplicity} (distinct (k-mer, sequence) pairs, compacted through
//                  LDS so the write is coalesced) and Pk[e] = rank of the entry inside its run of
//                  equal k-mers, counted from 1: entry e pairs with entries e-Pk[e]+1 .. e — exactly
//                  the `+=` of countAndUpdateTri (shared.cpp:316-327).
//   k_sx_emit      every (entry, partner) pair becomes one 32-bit update word {cell inside its owner's
//                  band of rows of K, product of the two multiplicities}; the words of a tile are
//                  binned by owner in LDS and leave as contiguous runs (long entries write their
//                  partner range directly, one wave per entry).
//   k_sx_consume   one workgroup per owner band sums its update stream in LDS (u32 cells) and adds
//                  the non-zero cells into the 64-bit triangle, row-contiguous, no atomics needed
//                  (a cell has one owner; launches are ordered on the stream).
// When a band of K does not fit the LDS budget (very large N) or FSK_SPARSE_GLOBAL=1, k_sx_emit adds
// every product into K with a 64-bit atomicAdd instead (DIRECT).
#ifndef FSK_SX_TILE
#define FSK_SX_TILE 4096                // (tools/build_variant.sh builds the A/B variants)
#endif
constexpr int SX_TILE = FSK_SX_TILE;    // records per sort tile
constexpr int SX_ITEMS = SX_TILE / 256;
#ifndef FSK_SG_TILE
#define FSK_SG_TILE 2048                // (tools/build_variant.sh builds the A/B variants: 1024 measured 6 % slower on config 4)
#endif
constexpr int SG_TILE = FSK_SG_TILE;    // records per segment tile = most entries one emit workgroup holds
constexpr int SG_ITEMS = SG_TILE / 256;
#ifndef FSK_SX_MAX_OWNERS
#define FSK_SX_MAX_OWNERS 512
#endif
constexpr int SX_MAX_OWNERS = FSK_SX_MAX_OWNERS;  // owner bands of K (bins of the update streams)
// DESCRIPTORS (owner bands, tuning sparse_desc): an entry of many partners does not leave k_sx_emit as one update word per
// partner but as ONE descriptor {entry index of its run's first partner, partners, row, multiplicity} in a stream of
// descriptors its owner band has beside its stream of words; k_sx_consume walks the partners' entries itself (a
// contiguous piece of E, shared by every entry of the run: an L2 read) and adds the products into its LDS cells. The
// per-(tile, band) count matrix then has two columns a band — descriptors first (their streams start the buffer: 16-byte
// aligned), words behind.
constexpr uint32_t SX_DESC_WORDS = 4;
constexpr int SX_MAX_COLS = 2 * SX_MAX_OWNERS;
constexpr uint32_t SX_DESC_MULT_BITS = 20;  // a descriptor's multiplicity field (its last word's low bits)
// `desc` of k_sx_seg_write / k_sx_emit: 0 = none; 1 = owner bands, one descriptor an entry; 2 = two-level blocks
// (fsk_sparse_blocks.inc): one descriptor per SUB-BAND the entry's partners fall into — {first partner of the piece, partners
// of the piece, cell of column 0 of the row inside the band, multiplicity | sub-band << 20} — reserved by the most a row of
// that length can take, (row >> sub_shift) + 2, the rest left as empty records (T = 0); the entry's own cell (multiplicity
// above 1) travels as an ordinary update word. May an entry of multiplicity c that is not binned be a descriptor?
// (cwide: see sx_wide_entry — an entry beyond it is no descriptor either)
__device__ __forceinline__ bool sx_desc_entry(uint32_t desc, uint32_t c, uint32_t cmax, uint32_t cwide) {
    return desc != 0u && c < (1u << SX_DESC_MULT_BITS) && c <= cwide && (desc == 1u || c <= cmax);
}
__device__ __forceinline__ uint32_t sx_desc_records(uint32_t desc, uint32_t row, int sub_shift) { return desc == 2u ? (row >> sub_shift) + 2u : 1u; }
#ifndef FSK_SX_SHORT
#define FSK_SX_SHORT 48                 // (A/B of 8 .. 96 on configs 4 / 1 and the large-g regime: profiles/r04_emit_short_ab.txt)
#endif
constexpr uint32_t SX_SHORT = FSK_SX_SHORT;  // entries with up to this many partners are binned by owner in LDS
// update words of short entries k_sx_emit bins per pass (u16 each in LDS; 11900, not 12288: with the u16 table of the paired
// cells the kernel's LDS stays inside the 105 granules of 512 bytes that three workgroups a CU allow)
#ifndef FSK_EM_SLOTS
#define FSK_EM_SLOTS 11800              // (11900 before the SX_SHORT entries in front of the tile's own moved into LDS: 192 bytes)
#endif
constexpr uint32_t EM_SLOTS = FSK_EM_SLOTS;
// k_sx_emit bins a tile's short entries — `short_words` words in all — in ONE pass when they fit the slot array, else in as
// many as their words take. k_sx_seg_write asks the same question: only a one-pass tile sends the cells of its unit entries
// in pairs.
static_assert(EM_SLOTS > 2u * SX_SHORT, "a pass of short entries must always fit the slot array");
__device__ __forceinline__ bool sx_one_pass(uint32_t short_words) { return short_words <= EM_SLOTS; }

// An ENTRY is a distinct (k-mer, sequence) pair: {sequence, multiplicity}, plus its rank P inside its run of
// equal k-mers (and T, skip_test_block). Two formats in HBM and in k_sx_emit's LDS: the general one (8 + 4 + 4
// bytes) and, when sequence ids, multiplicities and ranks all fit 16 bits (N < 65535 sequences of fewer than
// 65536 windows: every workload the update streams are used for), the PACKED one — 4 + 2 + 2 bytes: half the
// entry traffic of k_sx_seg_write and k_sx_emit, and an LDS footprint that lets three emit workgroups share a CU.
// UNIT entries (update streams with PAIRS): an entry of multiplicity 1 all of whose partners have multiplicity 1 too — every
// update word it sends is a bare cell with product 1 — is marked by a multiplicity field of 0 (no entry has none); sx_mult()
// gives the multiplicity back. k_sx_seg_write decides (conservatively: only when the run started inside the wave's own 512
// records, so that no carry between waves or tiles is needed), k_sx_emit follows the mark.
__device__ __forceinline__ uint32_t sx_mult(uint32_t field) { return field ? field : 1u; }
template <bool PACKED> struct SxEnt;
template <> struct SxEnt<false> {
    typedef uint2 ent_t;
    typedef uint32_t rank_t;
    static __device__ __forceinline__ ent_t pack(uint32_t seq, uint32_t cnt) { return make_uint2(seq, cnt); }
    static __device__ __forceinline__ uint2 unpack(ent_t v) { return v; }
    static __device__ __forceinline__ uint2 lds(const ent_t* p) {
        const u64 raw = FSK_LDS_LOAD_U64(p);
        return make_uint2((uint32_t)raw, (uint32_t)(raw >> 32));
    }
};
template <> struct SxEnt<true> {
    typedef uint32_t ent_t;
    typedef uint16_t rank_t;
    static __device__ __forceinline__ ent_t pack(uint32_t seq, uint32_t cnt) { return seq | (cnt << 16); }
    static __device__ __forceinline__ uint2 unpack(ent_t v) { return make_uint2(v & 0xffffu, v >> 16); }
    static __device__ __forceinline__ uint2 lds(const ent_t* p) { return unpack(FSK_LDS_LOAD_U32(p)); }
};


// XCD-aware block order: workgroups b, b + 8, b + 16, ... of a launch run on one XCD and share its L2, so XCD x
// is given the CONTIGUOUS range [x * ceil(n/8), ...) of the launch's n work items instead of every eighth one.
// What it buys here: the pieces neighbouring tiles append to one output stream (digit runs of the sort's
// scatter, an owner band's update words) meet in one write-back L2 and leave as whole lines, not as two partial
// ones from two XCDs. The launch has xcd_grid(n) = 8 * ceil(n/8) blocks; returns n for a block without an item.
__device__ __forceinline__ uint32_t xcd_contiguous(uint32_t block, uint32_t n) {
    const uint32_t per = (n + 7u) / 8u;
    const uint32_t item = (block & 7u) * per + (block >> 3);
    return item < n ? item : n;
}
inline uint32_t xcd_grid(uint32_t n) { return 8u * ((n + 7u) / 8u); }

// block-wide exclusive running maximum of one int per thread (256 threads); identity = -1 (all
// values are >= -1). Every thread of the block must call it.
__device__ __forceinline__ int block_excl_maxscan_256(int v, int* tmp, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d && y > x) x = y;
    }
    int prev = __shfl_up(x, 1);
    if (lane == 0) prev = -1;
    __syncthreads();  // tmp may still be read from a previous call
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    int base = -1, tot = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = tmp[w];
        if (w < wave && t > base) base = t;
        if (t > tot) tot = t;
    }
    if (total) *total = tot;
    return base > prev ? base : prev;
}

// rec = (k-mer << sb) | sequence id, one per (slot, g-mer), and the first sort pass's digit histogram
// of the tile (blockhist[slot][tile][digit], digit = the lowest k-mer bits under dmask); grid = (sort tiles per slot, slots).
// The kept positions of slot s: combo_pos[s][k] (uploaded per batch) — or, for a batch of at most 16
// combos (variance mode), row ids.id[s] of the resident table of all combos (by_id): the
// batch then needs no copy command at all; this kernel also zeroes the batch's counters (batch_stats).
// RC (reverse-complement mode): a sequence owns 2 (len - g + 1) features; feature j of its second half is window
// j - (len - g + 1) of rc(x), whose symbol c is comp[x[len - 1 - (j - (len - g + 1)) - c]].
// WILD (wildcard mode): a sequence owns its valid windows only, so feature f is no longer window f - fstart[seq]: fwin[f] is
// (the second strand's windows numbered on after the first's, as above).
struct SxIds { int32_t id[16]; };
template <typename RecT, bool RC, bool WILD = false>
__global__ __launch_bounds__(256) void k_sx_extract(SeqView S, const uint32_t* feat_seq, const uint32_t* fstart, uint32_t nfeat, uint32_t tps,
                                                    int k, uint32_t sigma, int sb, const uint8_t* combo_pos, RecT* rec,
                                                    uint32_t* blockhist, uint32_t dmask, SxIds ids, u64* batch_stats, int by_id,
                                                    int symbits, const uint16_t* comp, int g, const uint32_t* fwin) {
    // (symbits != 0: a k-mer space beyond 2^62 — the key is the symbols' bit fields side by side, which a 128-bit record holds)
    typedef typename std::conditional<sizeof(RecT) == 16, RecT, u64>::type key_t;
    __shared__ uint32_t h[256];
    __shared__ uint8_t s_pos[16];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y;
    h[tid] = 0u;
    combo_pos += (size_t)(by_id ? (uint32_t)ids.id[slot & 15u] : slot) * k;
    if (batch_stats && tile == 0 && slot == 0 && tid < 3u) batch_stats[tid] = 0;
    if (tid < 16u) s_pos[tid] = (int)tid < k ? combo_pos[tid] : (uint8_t)0;
    __syncthreads();
    const bool pos_in_lds = k <= 16;  // (uniform; two explicit reads below instead of one generic pointer)
    const uint32_t base = tile * (uint32_t)SX_TILE;
    // Three dependent gathers per record (sequence of the g-mer, where the sequence starts, its symbols):
    // eight records per thread go through each stage together, so that a stage costs one memory latency
    // for the eight and no store sits between the loads.
    constexpr int EX_B = 8;
    static_assert(SX_ITEMS % EX_B == 0, "records per thread");
    for (int it0 = 0; it0 < SX_ITEMS; it0 += EX_B) {
        uint32_t seq[EX_B], j[EX_B], wbase[EX_B];
        bool back[EX_B];  // (RC) the feature is a window of the second strand; j is then the place of its FIRST symbol's source
#pragma unroll
        for (int u = 0; u < EX_B; ++u) {
            const uint32_t f = base + (uint32_t)(it0 + u) * 256u + tid;
            seq[u] = f < nfeat ? feat_seq[f] : 0u;
        }
#pragma unroll
        for (int u = 0; u < EX_B; ++u) {
            const uint32_t f = base + (uint32_t)(it0 + u) * 256u + tid;
            j[u] = WILD ? (f < nfeat ? fwin[f] : 0u) : f - fstart[seq[u]];
            wbase[u] = S.wstart[seq[u]];
            back[u] = false;
            if (RC && f < nfeat) {
                const uint32_t len = S.len[seq[u]], nwin = len - (uint32_t)g + 1u;
                if (j[u] >= nwin) { back[u] = true; j[u] = len - 1u - (j[u] - nwin); }
            }
        }
        key_t key[EX_B];
#pragma unroll
        for (int u = 0; u < EX_B; ++u) key[u] = 0;
        for (int c = 0; c < k; ++c) {
            const uint32_t pc = pos_in_lds ? (uint32_t)FSK_LDS_LOAD_U8(&s_pos[c & 15]) : (uint32_t)combo_pos[c];
#pragma unroll
            for (int u = 0; u < EX_B; ++u) {
                const uint32_t f = base + (uint32_t)(it0 + u) * 256u + tid;
                uint32_t sym = 0u;
                if (RC && back[u]) sym = comp[fetch_sym(S.words, wbase[u], j[u] - pc, S.bits)];
                else if (f < nfeat) sym = fetch_sym(S.words, wbase[u], j[u] + pc, S.bits);
                key[u] = symbits ? (key_t)((key[u] << symbits) | (key_t)sym) : (key_t)(key[u] * sigma + sym);
            }
        }
#pragma unroll
        for (int u = 0; u < EX_B; ++u) {
            const uint32_t f = base + (uint32_t)(it0 + u) * 256u + tid;
            if (f < nfeat) {
                rec[(size_t)slot * nfeat + f] = ((RecT)key[u] << sb) | (RecT)seq[u];
                atomicAdd(&h[(uint32_t)key[u] & dmask], 1u);
            }
        }
    }
    __syncthreads();
    blockhist[((size_t)slot * tps + tile) * 256u + tid] = h[tid];
}

// feat_seq[f] = the sequence feature (g-mer) f belongs to; one wave per sequence. grid = ceil(sequences / 4)
__global__ __launch_bounds__(256) void k_sx_featseq(const uint32_t* fstart, uint32_t n_seq, uint32_t* feat_seq) {
    const uint32_t seq = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (seq >= n_seq) return;
    const uint32_t f1 = fstart[seq + 1];
    for (uint32_t f = fstart[seq] + lane; f < f1; f += 64u) feat_seq[f] = seq;
}

// The g-mer windows themselves: win[f] = the g symbols of feature f, `bits` each from bit 0, in WW 32-bit words
// (g * bits <= 32 * WW). Built once per set of sequences. k_sx_extract_win then gets a record's symbols with ONE
// coalesced load of 8 or 16 bytes — not three dependent gathers (sequence of the g-mer, where it starts, its
// words) and a load per kept symbol, for every slot of every batch — and the array, read by every slot, stays in
// L2 / MALL (16 bytes x features).
// RC (reverse-complement mode): the second half of a sequence's features are the windows of rc(x), written reversed and
// complemented (see k_sx_extract) — everything that reads the window array then sees twice the features and no strands.
// WILD (wildcard mode): the window of feature f is fwin[f] (see k_sx_extract); the array holds the valid windows only.
template <int WW, bool RC, bool WILD = false>
__global__ __launch_bounds__(256) void k_sx_windows(SeqView S, const uint32_t* feat_seq, const uint32_t* fstart, uint32_t nfeat, int g,
                                                    uint32_t* win, const uint16_t* comp, const uint32_t* fwin) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nfeat) return;
    const uint32_t seq = feat_seq[f], wbase = S.wstart[seq];
    uint32_t j = WILD ? fwin[f] : f - fstart[seq];
    bool back = false;
    if (RC) {
        const uint32_t len = S.len[seq], nwin = len - (uint32_t)g + 1u;
        if (j >= nwin) { back = true; j = len - 1u - (j - nwin); }
    }
    const int per = 32 / S.bits;  // symbols per word
#pragma unroll
    for (int ww = 0; ww < WW; ++ww) {
        uint32_t acc = 0u;
        for (int q = 0; q < per; ++q) {
            const int c = ww * per + q;
            if (c < g) {
                const uint32_t sym = RC && back ? (uint32_t)comp[fetch_sym(S.words, wbase, j - (uint32_t)c, S.bits)]
                                                : fetch_sym(S.words, wbase, j + (uint32_t)c, S.bits);
                acc |= sym << (q * S.bits);
            }
        }
        win[(size_t)f * WW + ww] = acc;
    }
}
// Records from the window array. The slot's kept position c is the same for the whole workgroup, so which word of the
// window it lies in is a scalar branch and the symbol is one v_bfe_u32; SMALL (the k-mer space fits 24 bits): key *
// sigma + symbol is one full-rate v_mad_u32_u24 (a 32-bit multiply issues at a quarter of that) — two instructions
// per kept position and record. f[u]: the features (clamped here; the caller ignores what lies beyond nfeat);
// s_pos: the slot's positions in LDS when k <= 16, else combo_pos (global) is read.
template <int WW> struct SxWin;
template <> struct SxWin<2> {
    typedef uint2 vec_t;
    template <int I> static __device__ __forceinline__ uint32_t at(const uint2& v) { return I == 0 ? v.x : v.y; }
};
template <> struct SxWin<4> {
    typedef uint4 vec_t;
    template <int I> static __device__ __forceinline__ uint32_t at(const uint4& v) { return I == 0 ? v.x : I == 1 ? v.y : I == 2 ? v.z : v.w; }
};
// where the kept positions of a workgroup's slot come from (see k_sx_extract)
struct SxSrc {
    const uint32_t* win;
    const uint32_t* feat_seq;
    const uint8_t* combo_pos;
    int k, sb, bits, by_id;
    uint32_t sigma;
    int symbits;  // != 0: keys are the symbols' symbits-bit fields side by side (a k-mer space beyond 2^62), not mixed radix
    SxIds ids;
    int c0;       // the key is built from kept positions c0 .. k - 1 (0 but for k_sx_extract_shared: the leading ones are in the part records)
};
template <int WW, int EX_B>
__device__ __forceinline__ void sx_window_load(const SxSrc& src, uint32_t nfeat, const uint32_t (&f)[EX_B],
                                               typename SxWin<WW>::vec_t (&w)[EX_B], uint32_t (&seq)[EX_B]) {
    const typename SxWin<WW>::vec_t* wv = reinterpret_cast<const typename SxWin<WW>::vec_t*>(src.win);
#pragma unroll
    for (int u = 0; u < EX_B; ++u) {  // (unconditional loads of a clamped index)
        const uint32_t fc = f[u] < nfeat ? f[u] : nfeat - 1u;
        w[u] = wv[fc];
        seq[u] = src.feat_seq[fc];
    }
}
template <typename RecT, int WW, bool SMALL, int EX_B, typename PartT>
__device__ __forceinline__ void sx_window_records(const SxSrc& src, const typename SxWin<WW>::vec_t (&w)[EX_B], const PartT (&seq)[EX_B],
                                                  const uint8_t* s_pos, const uint8_t* combo_pos, RecT (&out)[EX_B]) {
    // (a 32-bit record holds a k-mer below 2^32; a 128-bit one may hold a bit-field key beyond 2^64)
    typedef typename std::conditional<sizeof(RecT) == 4, uint32_t, typename std::conditional<sizeof(RecT) == 16, RecT, u64>::type>::type key_t;
    const int symbits = SMALL ? 0 : src.symbits;
    static_assert(!SMALL || sizeof(RecT) == 4, "24-bit k-mers travel in 32-bit records");
    const bool pos_in_lds = src.k <= 16;  // (uniform; two explicit reads below instead of one generic pointer)
    key_t key[EX_B];
#pragma unroll
    for (int u = 0; u < EX_B; ++u) key[u] = 0;
    const uint32_t sigma = src.sigma, bits = (uint32_t)src.bits;
#define SX_STEP(comp)                                                                                    \
    _Pragma("unroll") for (int u = 0; u < EX_B; ++u) {                                                   \
        const uint32_t sym = fsk_hw::bfe(SxWin<WW>::template at<comp>(w[u]), sh, bits);                  \
        key[u] = SMALL ? (key_t)fsk_hw::mad24((uint32_t)key[u], sigma, sym)                              \
                 : symbits ? (key_t)((key[u] << symbits) | (key_t)sym) : (key_t)(key[u] * sigma + sym); \
    }
    for (int c = src.c0; c < src.k; ++c) {
        const uint32_t pc = fsk_hw::readlane(pos_in_lds ? (uint32_t)FSK_LDS_LOAD_U8(&s_pos[c & 15]) : (uint32_t)combo_pos[c], 0u);
        const uint32_t o = pc * bits, wi = o >> 5, sh = o & 31u;
        if (WW == 2) {
            if (wi == 0u) SX_STEP(0) else SX_STEP(1)
        } else {
            if (wi == 0u) SX_STEP(0) else if (wi == 1u) SX_STEP(1) else if (wi == 2u) SX_STEP(2) else SX_STEP(3)
        }
    }
#undef SX_STEP
#pragma unroll
    for (int u = 0; u < EX_B; ++u) out[u] = ((RecT)key[u] << src.sb) | (RecT)seq[u];
}
// row of the position table of a slot (see k_sx_extract)
__device__ __forceinline__ const uint8_t* sx_slot_positions(const SxSrc& src, uint32_t slot) {
    return src.combo_pos + (size_t)(src.by_id ? (uint32_t)src.ids.id[slot & 15u] : slot) * src.k;
}

// k_sx_extract from the window array (same outputs). A workgroup takes its tile of windows through SPW slots: the
// windows are loaded once (16 + 4 bytes a record from L2) and every slot costs arithmetic and the store only.
// grid = (sort tiles per slot, ceil(slots / SPW))
template <typename RecT, int WW, bool SMALL, int SPW>
__global__ __launch_bounds__(256) void k_sx_extract_win(SxSrc src, uint32_t nfeat, uint32_t tps, uint32_t n_slots, RecT* rec,
                                                        uint32_t* blockhist, uint32_t dmask, u64* batch_stats) {
    __shared__ uint32_t h[SPW][256];
    __shared__ uint8_t s_pos[SPW][16];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, slot0 = blockIdx.y * (uint32_t)SPW;
    const uint32_t ns = n_slots - slot0 < (uint32_t)SPW ? n_slots - slot0 : (uint32_t)SPW;
#pragma unroll
    for (int s = 0; s < SPW; ++s) h[s][tid] = 0u;
    if (batch_stats && tile == 0 && slot0 == 0 && tid < 3u) batch_stats[tid] = 0;
    if (tid < 16u * ns) {
        const uint8_t* cp = sx_slot_positions(src, slot0 + (tid >> 4));
        s_pos[tid >> 4][tid & 15u] = (int)(tid & 15u) < src.k ? cp[tid & 15u] : (uint8_t)0;
    }
    __syncthreads();
    const uint32_t base = tile * (uint32_t)SX_TILE;
    constexpr int EX_B = 8;
    static_assert(SX_ITEMS % EX_B == 0, "records per thread");
    for (int it0 = 0; it0 < SX_ITEMS; it0 += EX_B) {
        uint32_t f[EX_B], seq[EX_B];
        typename SxWin<WW>::vec_t w[EX_B];
#pragma unroll
        for (int u = 0; u < EX_B; ++u) f[u] = base + (uint32_t)(it0 + u) * 256u + tid;
        sx_window_load<WW, EX_B>(src, nfeat, f, w, seq);
        for (uint32_t s = 0; s < ns; ++s) {
            RecT r[EX_B];
            sx_window_records<RecT, WW, SMALL, EX_B>(src, w, seq, s_pos[s], sx_slot_positions(src, slot0 + s), r);
#pragma unroll
            for (int u = 0; u < EX_B; ++u) {
                if (f[u] < nfeat) {
                    rec[(size_t)(slot0 + s) * nfeat + f[u]] = r[u];
                    atomicAdd(&h[s][(uint32_t)(r[u] >> src.sb) & dmask], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t s = 0; s < ns; ++s) blockhist[((size_t)(slot0 + s) * tps + tile) * 256u + tid] = h[s][tid];
}

// ---- shared prefixes -------------------------------------------------------------------------------------------------
// Consecutive combos (an exact accumulate walks them in lexicographic order) keep the same LEADING positions for long
// stretches. Grouping needs equal k-mers side by side, not a particular order of them, so the key is split
//     key = (mixed radix / bit fields of the first `share` kept positions) << lowbits | (the same of the others)
// and the windows are sorted by the leading part ONCE per group of consecutive slots that share it (the "presort": pseudo
// slots through the same extraction / histogram / scatter kernels, records (top << wb) | window). Every slot of the group
// then starts from that order and sorts by its `lowbits` alone — stable passes, so the result is ordered by (low, top,
// window): equal keys contiguous, sequence ids ascending. Config 4 (k = 4 of 20 symbols, 250 slots a batch): one pass of
// 5 bits per slot after a presort of ~70 groups, instead of three passes of 7 + 6 + 6 bits.

// group_of[slot] = the slot's group, head[group] = its first slot: a slot starts a group when its first `share` kept
// positions differ from its predecessor's. One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_sx_group_tables(SxSrc src, uint32_t n_slots, int share, uint32_t* group_of, uint32_t* head) {
    __shared__ uint32_t tmp[16];
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_slots; base += 1024u) {
        const uint32_t s = base + tid;
        uint32_t starts = 0u;
        if (s < n_slots) {
            starts = s == 0u ? 1u : 0u;
            if (s > 0u) {
                const uint8_t *a = sx_slot_positions(src, s), *b = sx_slot_positions(src, s - 1u);
                for (int c = 0; c < share; ++c) starts |= a[c] != b[c] ? 1u : 0u;
            }
        }
        uint32_t tot;
        const uint32_t ex = block_excl_scan<uint32_t, 16>(starts, tmp, &tot) + carry;
        if (s < n_slots) {
            group_of[s] = ex + starts - 1u;
            if (starts) head[ex] = s;
        }
        carry += tot;
        __syncthreads();
    }
}

// The presort's records: pre[group][f] = (top(f) << wb) | f for every window f — top from the first `share` kept positions
// of the group's first slot — and the first pass's digit histogram. grid = (sort tiles per slot, groups)
template <typename PreT, int WW, bool SMALL>
__global__ __launch_bounds__(256) void k_sx_group_extract(SxSrc src, const uint32_t* head, int share, int wb, uint32_t nfeat, uint32_t tps,
                                                          PreT* pre, uint32_t* blockhist, uint32_t dmask) {
    __shared__ uint32_t h[256];
    __shared__ uint8_t s_pos[16];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, grp = blockIdx.y;
    h[tid] = 0u;
    const uint8_t* cp = sx_slot_positions(src, head[grp]);
    if (tid < 16u) s_pos[tid] = (int)tid < share ? cp[tid] : (uint8_t)0;
    __syncthreads();
    src.k = share; src.c0 = 0; src.sb = wb;
    const uint32_t base = tile * (uint32_t)SX_TILE;
    constexpr int EX_B = 8;
    const typename SxWin<WW>::vec_t* wv = reinterpret_cast<const typename SxWin<WW>::vec_t*>(src.win);
    for (int it0 = 0; it0 < SX_ITEMS; it0 += EX_B) {
        uint32_t f[EX_B], fc[EX_B];
        typename SxWin<WW>::vec_t w[EX_B];
#pragma unroll
        for (int u = 0; u < EX_B; ++u) {
            f[u] = base + (uint32_t)(it0 + u) * 256u + tid;
            fc[u] = f[u] < nfeat ? f[u] : nfeat - 1u;
            w[u] = wv[fc[u]];
        }
        PreT r[EX_B];
        sx_window_records<PreT, WW, SMALL, EX_B>(src, w, fc, s_pos, cp, r);
#pragma unroll
        for (int u = 0; u < EX_B; ++u) {
            if (f[u] < nfeat) {
                pre[(size_t)grp * nfeat + f[u]] = r[u];
                atomicAdd(&h[(uint32_t)(r[u] >> wb) & dmask], 1u);
            }
        }
    }
    __syncthreads();
    blockhist[((size_t)grp * tps + tile) * 256u + tid] = h[tid];
}

// The presorted order, materialised for the group's slots: winp[group][i] = the window at place i, part[group][i] = the
// part of its record every slot of the group shares, (top << up) | sequence id (up = lowbits + sb). grid = (ceil(nfeat / 256), groups)
template <typename PreT, typename RecT, int WW>
__global__ __launch_bounds__(256) void k_sx_group_gather(const PreT* pre, const uint32_t* win, const uint32_t* feat_seq, uint32_t nfeat, int wb,
                                                         int up, uint32_t* winp, RecT* part) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, grp = blockIdx.y;
    if (i >= nfeat) return;
    const PreT r = pre[(size_t)grp * nfeat + i];
    const uint32_t f = (uint32_t)(r & (PreT)(((u64)1 << wb) - 1u));
    typedef typename SxWin<WW>::vec_t vec_t;
    reinterpret_cast<vec_t*>(winp)[(size_t)grp * nfeat + i] = reinterpret_cast<const vec_t*>(win)[f];
    part[(size_t)grp * nfeat + i] = ((RecT)(r >> wb) << up) | (RecT)feat_seq[f];
}

// k_sx_extract_win over the presorted order: a slot reads its group's windows and part records (src.win = winp) and adds
// the key of its own kept positions src.c0 .. k - 1. The SPW slots of a workgroup mostly lie in one group: the loads are
// repeated only when the group changes (uniform). grid = (sort tiles per slot, ceil(slots / SPW))
template <typename RecT, int WW, bool SMALL, int SPW>
__global__ __launch_bounds__(256) void k_sx_extract_shared(SxSrc src, const uint32_t* group_of, const RecT* part, uint32_t nfeat, uint32_t tps,
                                                           uint32_t n_slots, RecT* rec, uint32_t* blockhist, uint32_t dmask, u64* batch_stats) {
    __shared__ uint32_t h[SPW][256];
    __shared__ uint8_t s_pos[SPW][16];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, slot0 = blockIdx.y * (uint32_t)SPW;
    const uint32_t ns = n_slots - slot0 < (uint32_t)SPW ? n_slots - slot0 : (uint32_t)SPW;
#pragma unroll
    for (int s = 0; s < SPW; ++s) h[s][tid] = 0u;
    if (batch_stats && tile == 0 && slot0 == 0 && tid < 3u) batch_stats[tid] = 0;
    if (tid < 16u * ns) {
        const uint8_t* cp = sx_slot_positions(src, slot0 + (tid >> 4));
        s_pos[tid >> 4][tid & 15u] = (int)(tid & 15u) < src.k ? cp[tid & 15u] : (uint8_t)0;
    }
    __syncthreads();
    const uint32_t base = tile * (uint32_t)SX_TILE;
    constexpr int EX_B = 8;
    const typename SxWin<WW>::vec_t* wv = reinterpret_cast<const typename SxWin<WW>::vec_t*>(src.win);
    for (int it0 = 0; it0 < SX_ITEMS; it0 += EX_B) {
        uint32_t f[EX_B];
        typename SxWin<WW>::vec_t w[EX_B];
        RecT pr[EX_B];
#pragma unroll
        for (int u = 0; u < EX_B; ++u) f[u] = base + (uint32_t)(it0 + u) * 256u + tid;
        uint32_t loaded = 0xffffffffu;
        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t grp = fsk_hw::readlane(group_of[slot0 + s], 0u);
            if (grp != loaded) {  // (uniform)
                loaded = grp;
#pragma unroll
                for (int u = 0; u < EX_B; ++u) {  // (unconditional loads of a clamped index)
                    const size_t at = (size_t)grp * nfeat + (f[u] < nfeat ? f[u] : nfeat - 1u);
                    w[u] = wv[at];
                    pr[u] = part[at];
                }
            }
            RecT r[EX_B];
            sx_window_records<RecT, WW, SMALL, EX_B>(src, w, pr, s_pos[s], sx_slot_positions(src, slot0 + s), r);
#pragma unroll
            for (int u = 0; u < EX_B; ++u) {
                if (f[u] < nfeat) {
                    rec[(size_t)(slot0 + s) * nfeat + f[u]] = r[u];
                    atomicAdd(&h[s][(uint32_t)(r[u] >> src.sb) & dmask], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t s = 0; s < ns; ++s) blockhist[((size_t)(slot0 + s) * tps + tile) * 256u + tid] = h[s][tid];
}

// digit histogram of one tile of one slot -> blockhist[slot][tile][digit]; grid = (tiles per slot, slots)
template <typename RecT>
__global__ __launch_bounds__(256) void k_sx_hist(const RecT* rec, uint32_t nfeat, uint32_t tps, int shift, uint32_t dmask,
                                                 uint32_t* blockhist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y;
    h[tid] = 0u;
    __syncthreads();
    const RecT* r = rec + (size_t)slot * nfeat;
    const uint32_t base = tile * (uint32_t)SX_TILE;
    // (a streaming read: every load of the thread is issued before the first LDS atomic; 4-byte records of a full
    // tile go 16 bytes per load from the first 16-byte boundary on — a slot starts wherever slot * nfeat falls —
    // and the up to three records before it and after the last whole piece one per thread)
    if (sizeof(RecT) == 4 && base + (uint32_t)SX_TILE <= nfeat) {
        const uint32_t head = (4u - (uint32_t)(((size_t)slot * nfeat + base) & 3u)) & 3u;
        const uint32_t nvec = ((uint32_t)SX_TILE - head) / 4u, tail0 = head + nvec * 4u;
        const uint4* r4 = reinterpret_cast<const uint4*>(r + base + head);
        uint4 v[SX_ITEMS / 4];
#pragma unroll
        for (int it = 0; it < SX_ITEMS / 4; ++it) {
            const uint32_t idx = (uint32_t)it * 256u + tid;
            v[it] = r4[idx < nvec ? idx : 0u];
        }
        uint32_t edge = 0xffffffffu;  // (no digit)
        if (tid < head) edge = (uint32_t)(r[base + tid] >> shift) & dmask;
        else if (tid - head < (uint32_t)SX_TILE - tail0) edge = (uint32_t)(r[base + tail0 + (tid - head)] >> shift) & dmask;
#pragma unroll
        for (int it = 0; it < SX_ITEMS / 4; ++it) {
            if ((uint32_t)it * 256u + tid < nvec) {
                atomicAdd(&h[(v[it].x >> shift) & dmask], 1u);
                atomicAdd(&h[(v[it].y >> shift) & dmask], 1u);
                atomicAdd(&h[(v[it].z >> shift) & dmask], 1u);
                atomicAdd(&h[(v[it].w >> shift) & dmask], 1u);
            }
        }
        if (edge != 0xffffffffu) atomicAdd(&h[edge], 1u);
    } else {
        RecT v[SX_ITEMS];
#pragma unroll
        for (int it = 0; it < SX_ITEMS; ++it) {
            const uint32_t i = base + (uint32_t)it * 256u + tid;
            v[it] = i < nfeat ? r[i] : (RecT)0;
        }
#pragma unroll
        for (int it = 0; it < SX_ITEMS; ++it) {
            const uint32_t i = base + (uint32_t)it * 256u + tid;
            if (i < nfeat) atomicAdd(&h[(uint32_t)(v[it] >> shift) & dmask], 1u);
        }
    }
    __syncthreads();
    blockhist[((size_t)slot * tps + tile) * 256u + tid] = h[tid];
}

// One workgroup of 1024 threads per slot, thread = (quarter of the slot's tiles, digit): the digit's tile
// counts become exclusive offsets inside the digit's block (in place), and dbase[slot][digit] = where
// that block starts inside the slot. Two passes over the quarter (sum, then write), so that four
// chains of dependent loads run side by side.
__global__ __launch_bounds__(1024) void k_sx_scan_slot(uint32_t* blockhist, uint32_t tps, uint32_t* dbase) {
    __shared__ uint32_t part[4][256];
    __shared__ uint32_t tmp[16];
    const uint32_t tid = threadIdx.x, digit = tid & 255u, quarter = tid >> 8, slot = blockIdx.x;
    uint32_t* h = blockhist + (size_t)slot * tps * 256u + digit;
    const uint32_t per = (tps + 3u) / 4u;
    const uint32_t t0 = quarter * per < tps ? quarter * per : tps, t1 = t0 + per < tps ? t0 + per : tps;
    uint32_t sum = 0;
#pragma unroll 4
    for (uint32_t t = t0; t < t1; ++t) sum += h[(size_t)t * 256u];
    part[quarter][digit] = sum;
    __syncthreads();
    uint32_t run = 0, total = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t v = part[q][digit];
        if (q < quarter) run += v;
        total += v;
    }
#pragma unroll 4
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t v = h[(size_t)t * 256u];
        h[(size_t)t * 256u] = run;
        run += v;
    }
    const uint32_t ex = block_excl_scan<uint32_t, 16>(quarter == 0 ? total : 0u, tmp, nullptr);
    if (quarter == 0) dbase[(size_t)slot * 256u + digit] = ex;
}

// Stable scatter of one tile of one slot. Wave w owns the contiguous quarter w of the tile, so the
// four waves rank their records independently (wave64 ballot matching: 8 ballots give the lanes
// holding the same digit; a per-wave LDS counter carries the digit's count from round to round)
// and meet at ONE barrier; the records are then permuted into digit order in LDS and written out
// so that equal digits go to consecutive addresses. grid = (tiles per slot, slots)
// NB = ballots per round, a compile-time bound of the pass's digit width nbits (bits above nbits are zero
// under the digit mask and cost a ballot each: the host instantiates NB = max(nbits, 4)): the matching loop is
// what this kernel issues, so it is unrolled and kept to four instructions per bit (sign-extended bit, one
// compare into a scalar mask, one v_bitop3 — and-xnor — per half of the 64-lane peer mask).
// (Tried instead of the ballots: every lane ORs its bit into a per-wave LDS mask of its digit and reads the mask
// back — a third of the VALU instructions, but three dependent LDS round trips per round: 2.65 ms against
// 2.42 ms for the three passes of config 4, same box.)
// (Tried: the first pass building its records from the window array instead of reading them, extraction then only
// counting digits — 16 + 4 bytes per record through L2 instead of 4 from HBM, and with the XCD-contiguous order every
// XCD streams the whole array through its 4 MB L2 once per slot: 1.31 + 0.32 ms against 0.78 + 0.62 ms on config 4.)
template <typename RecT, int NB>
__global__ __launch_bounds__(256) void k_sx_scatter(const RecT* in, RecT* out, uint32_t nfeat, uint32_t tps, uint32_t n_slots, int shift,
                                                    int nbits, const uint32_t* blockhist, const uint32_t* dbase) {
    __shared__ uint32_t goff[256];         // destination, inside the slot, of this tile's first record of each digit
    __shared__ uint32_t wave_run[4][256];  // per wave: records of the digit so far; later: where the wave's share starts in LDS
    __shared__ uint32_t blk_start[256];    // exclusive scan of the tile's digit totals
    __shared__ uint32_t tmp[4];
    __shared__ RecT s_rec[SX_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t item = xcd_contiguous(blockIdx.x, tps * n_slots);  // grid = xcd_grid(tiles per slot x slots)
    if (item == tps * n_slots) return;  // (uniform)
    const uint32_t tile = item % tps, slot = item / tps;
    const uint32_t dmask = (1u << nbits) - 1u;
    const RecT* r = in + (size_t)slot * nfeat;
    RecT* o = out + (size_t)slot * nfeat;
    goff[tid] = dbase[(size_t)slot * 256u + tid] + blockhist[((size_t)slot * tps + tile) * 256u + tid];
#pragma unroll
    for (int q = 0; q < 4; ++q) wave_run[q][tid] = 0u;
    __syncthreads();
    RecT key[SX_ITEMS];
    uint32_t rank[SX_ITEMS];
    const uint32_t base = tile * (uint32_t)SX_TILE + (uint32_t)wave * (SX_TILE / 4);
    uint32_t* my_run = wave_run[wave];
    // (all of the wave's records first: the ranking rounds below touch a volatile LDS counter, which the
    // loads could not be moved across — sixteen memory latencies in a row)
    // (unconditional loads of a clamped index: sixteen exec-mask diamonds otherwise; what lies beyond the slot is
    // never ranked)
#pragma unroll
    for (int it = 0; it < SX_ITEMS; ++it) {
        const uint32_t i = base + (uint32_t)it * 64u + (uint32_t)lane;
        key[it] = r[i < nfeat ? i : nfeat - 1u];
    }
    // (a FULL tile — all but the last of a slot — ranks without the per-lane validity: uniform choice between two copies of the rounds)
    auto rounds = [&](auto full_tag) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
        for (int it = 0; it < SX_ITEMS; ++it) {
            if (!FULL && base + (uint32_t)it * 64u >= nfeat) {  // (wave-uniform) nothing of the slot left for this wave
                rank[it] = 0xffffffffu;
                continue;
            }
            const uint32_t i = base + (uint32_t)it * 64u + (uint32_t)lane;
            const bool valid = FULL || i < nfeat;
            const uint32_t digit = (uint32_t)(key[it] >> shift) & dmask;
            uint32_t p_lo = 0xffffffffu, p_hi = 0xffffffffu;
            if (!FULL) {
                const u64 live = __ballot(valid);
                p_lo = (uint32_t)live; p_hi = (uint32_t)(live >> 32);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int t = fsk_hw::sbfe1(digit, b);             // 0 or -1: bit b of the digit, sign-extended
                const u64 m = __ballot(t < 0);
                p_lo = fsk_hw::and_xnor(p_lo, (uint32_t)m, (uint32_t)t);          // bit set: the lanes whose bit is set; clear: the others
                p_hi = fsk_hw::and_xnor(p_hi, (uint32_t)(m >> 32), (uint32_t)t);
            }
            const uint32_t rank_in_wave = fsk_mbcnt(p_lo, p_hi);  // peers in the lanes below this one
            const uint32_t prior = valid ? FSK_LDS_VOLATILE_U32(&my_run[digit]) : 0u;
            (void)__ballot(true);  // every lane has read the counter before the group's first lane adds to it
            if (valid && rank_in_wave == 0) atomicAdd(&wave_run[wave][digit], (uint32_t)(__popc(p_lo) + __popc(p_hi)));
            rank[it] = valid ? prior + rank_in_wave : 0xffffffffu;
        }
    };
    if (tile * (uint32_t)SX_TILE + (uint32_t)SX_TILE <= nfeat) rounds(std::true_type());
    else rounds(std::false_type());
    __syncthreads();
    {
        uint32_t c[4], tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = wave_run[q][tid]; tot += c[q]; }
        uint32_t ex = block_excl_scan_256<uint32_t>(tot, tmp, nullptr);
        blk_start[tid] = ex;
#pragma unroll
        for (int q = 0; q < 4; ++q) { wave_run[q][tid] = ex; ex += c[q]; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SX_ITEMS; ++it) {
        if (rank[it] != 0xffffffffu) {
            const uint32_t digit = (uint32_t)(key[it] >> shift) & dmask;
            s_rec[wave_run[wave][digit] + rank[it]] = key[it];
        }
    }
    __syncthreads();
    const uint32_t first = tile * (uint32_t)SX_TILE;
    const uint32_t nvalid = nfeat - first < (uint32_t)SX_TILE ? nfeat - first : (uint32_t)SX_TILE;
#pragma unroll
    for (int it = 0; it < SX_ITEMS; ++it) {
        const uint32_t p = (uint32_t)it * 256u + (uint32_t)tid;
        if (p < nvalid) {
            const RecT kx = s_rec[p];
            const uint32_t digit = (uint32_t)(kx >> shift) & dmask;
            o[goff[digit] + (p - blk_start[digit])] = kx;
        }
    }
}

// ---- segments --------------------------------------------------------------------------------
// Inside a slot, record j starts an ENTRY when it differs from record j-1 (new k-mer or new sequence)
// and a RUN when its k-mer differs; j = 0 starts both. Thread t of a tile looks at SG_ITEMS
// consecutive records.
// skip_from (skip_test_block): sequences >= skip_from are test sequences. Inside a run the entries are
// in sequence order, train entries first; the first test entry of a run is a TEST HEAD. tile_lth gets the
// tile-local index of the tile's last test head (only when skip_from != 0xffffffff).
// SKIP: skip_test_block is on (skip_from != 0xffffffff) — a template parameter, not a test of skip_from: this kernel and
// k_sx_seg_write are bound by the VALU instructions they issue, and the test-head ballots, their scan and the compares
// against skip_from are a fifth of them.
template <typename RecT, bool SKIP>
__global__ __launch_bounds__(256) void k_sx_seg_count(const RecT* rec, uint32_t nfeat, uint32_t tpg, int sb, uint32_t* tile_ent,
                                                      int* tile_lrh, uint32_t skip_from, int* tile_lth) {
    // Wave w takes records [512 w, 512 w + 512) of the tile, 64 consecutive ones per round: every load is
    // coalesced and issued before the first use, and what a round contributes — how many entries, where
    // its last run head / test head sits among them — comes from three ballots, in scalar registers.
    __shared__ uint32_t s_n[4];
    __shared__ int s_h[4], s_t[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, t = blockIdx.x, slot = blockIdx.y;
    const RecT* r = rec + (size_t)slot * nfeat;
    constexpr int ROUNDS = SG_TILE / 256;
    const uint32_t j0 = t * (uint32_t)SG_TILE + wave * (uint32_t)(64 * ROUNDS) + lane;
    const RecT seq_mask = (RecT)(((u64)1 << sb) - 1);
    RecT cur[ROUNDS], prev[ROUNDS];
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {  // (unconditional loads of clamped indices: what lies beyond the slot is never an entry)
        const uint32_t j = j0 + (uint32_t)q * 64u, jc = j < nfeat ? j : nfeat - 1u;
        cur[q] = r[jc];
        prev[q] = r[jc > 0u ? jc - 1u : 0u];  // (the neighbour lane's line: an L1 hit)
    }
    uint32_t n = 0;
    int lrh = -1, lth = -1;  // among this wave's entries, the last one that starts a run / is a test head
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const uint32_t j = j0 + (uint32_t)q * 64u;
        const bool entry = j < nfeat && (j == 0 || cur[q] != prev[q]);
        const bool run_head = entry && (j == 0 || (cur[q] >> sb) != (prev[q] >> sb));
        const u64 H = __ballot(entry), R = __ballot(run_head);
        if (R) lrh = (int)n + __popcll(H & (((u64)1 << (63 - __clzll((long long)R))) - 1));
        if (SKIP) {
            const bool test_head = entry && (uint32_t)(cur[q] & seq_mask) >= skip_from &&
                                   (run_head || (uint32_t)(prev[q] & seq_mask) < skip_from);
            const u64 T = __ballot(test_head);
            if (T) lth = (int)n + __popcll(H & (((u64)1 << (63 - __clzll((long long)T))) - 1));
        }
        n += (uint32_t)__popcll(H);
    }
    if (lane == 0) { s_n[wave] = n; s_h[wave] = lrh; s_t[wave] = lth; }
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        int h = -1, th = -1;
        for (int w = 0; w < 4; ++w) {
            if (s_h[w] >= 0) h = (int)tot + s_h[w];
            if (s_t[w] >= 0) th = (int)tot + s_t[w];
            tot += s_n[w];
        }
        tile_ent[(size_t)slot * tpg + t] = tot;
        tile_lrh[(size_t)slot * tpg + t] = h;  // tile-local index of the last entry that starts a run, or -1
        if (SKIP) tile_lth[(size_t)slot * tpg + t] = th;
    }
}

// running maximum, exclusive, over a block of NW waves; identity -1. tmp: >= NW ints.
template <int NW>
__device__ __forceinline__ int block_excl_maxscan(int v, int* tmp, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d && y > x) x = y;
    }
    int prev = __shfl_up(x, 1);
    if (lane == 0) prev = -1;
    __syncthreads();
    if (lane == 63) tmp[wave] = x;
    __syncthreads();
    int base = -1, tot = -1;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int t = tmp[w];
        if (w < wave && t > base) base = t;
        if (t > tot) tot = t;
    }
    if (total) *total = tot;
    return base > prev ? base : prev;
}

// ebase[tile] = entries before the tile (ebase[ntiles] = D); tile_rs[tile] = global index of the last
// run start before the tile (the run the tile's first entries may continue); tile_ts[tile] = likewise the
// last test head before the tile (skip_test_block only). 1024 threads per workgroup, three forms:
//  * one workgroup walks the whole array (c_ex, o_tot null): batches of up to a few thousand tiles;
//  * larger batches, three launches: (1) o_tot != null, grid = chunks of 1024 tiles: the chunk's entry
//    count and its last run / test head relative to the chunk's first entry; (2) the first form over those
//    chunk records (a chunk record has exactly the meaning of a tile record); (3) c_ex != null, grid =
//    chunks: the chunk's tiles with the carries of (2).
__global__ __launch_bounds__(1024) void k_sx_seg_scan(const uint32_t* tile_ent, const int* tile_lrh, uint32_t ntiles, uint32_t* ebase,
                                                      int* tile_rs, const int* tile_lth, int* tile_ts, const uint32_t* c_ex,
                                                      const int* c_h, const int* c_t, uint32_t* o_tot, int* o_h, int* o_t) {
    __shared__ uint32_t tmp[16];
    __shared__ int tmpi[16];
    const uint32_t tid = threadIdx.x;
    const bool chunked = c_ex != nullptr || o_tot != nullptr;  // (uniform)
    uint32_t carry = c_ex ? c_ex[blockIdx.x] : 0u;
    int carry_h = c_h ? c_h[blockIdx.x] : -1, carry_t = (c_t && tile_lth) ? c_t[blockIdx.x] : -1;
    const uint32_t begin = chunked ? blockIdx.x * 1024u : 0u;
    const uint32_t end = chunked ? (begin + 1024u < ntiles ? begin + 1024u : ntiles) : ntiles;
    for (uint32_t base = begin; base < end; base += 1024) {
        const uint32_t i = base + tid;
        const uint32_t v = i < end ? tile_ent[i] : 0u;
        const int lr = i < end ? tile_lrh[i] : -1;
        const int lt = (tile_lth && i < end) ? tile_lth[i] : -1;
        uint32_t tot;
        const uint32_t ex = block_excl_scan<uint32_t, 16>(v, tmp, &tot) + carry;
        const int h = lr >= 0 ? (int)ex + lr : -1;
        int htot;
        const int hx = block_excl_maxscan<16>(h, tmpi, &htot);
        if (i < end && !o_tot) {
            ebase[i] = ex;
            tile_rs[i] = hx > carry_h ? hx : carry_h;
        }
        if (tile_lth) {  // (uniform)
            const int th = lt >= 0 ? (int)ex + lt : -1;
            int ttot;
            const int tx = block_excl_maxscan<16>(th, tmpi, &ttot);
            if (i < end && !o_tot) tile_ts[i] = tx > carry_t ? tx : carry_t;
            if (ttot > carry_t) carry_t = ttot;
        }
        carry += tot;
        if (htot > carry_h) carry_h = htot;
    }
    if (tid == 0) {
        if (o_tot) {
            o_tot[blockIdx.x] = carry;
            o_h[blockIdx.x] = carry_h;
            if (tile_lth) o_t[blockIdx.x] = carry_t;
        } else if (!chunked) {
            ebase[ntiles] = carry;
        } else if (end == ntiles) {
            ebase[ntiles] = carry;  // (the last chunk)
        }
    }
}

// Owner band of row i: band o holds the rows whose first cell index tri_index(i, 0) lies in
// [o << own_shift, (o + 1) << own_shift), i.e. owner_r0[o] <= i < owner_r0[o + 1].
// tri_index(i, 0) modulo 2^32: i (i + 1) / 2 = (i | 1) * ((i >> 1) + (i & 1)), one 24-bit multiply (full rate; i < 2^24:
// the update streams exist for N up to some ten thousand sequences). Differences of two such values are exact
// whenever the true difference fits 32 bits (a cell inside its owner band does).
__device__ __forceinline__ uint32_t sx_tri32(uint32_t i) { return fsk_hw::mul24(i | 1u, (i >> 1) + (i & 1u)); }
// the owner band of a row (update streams only), counted from the first cell of the rows the streams cover: `own_base` =
// sx_tri32(first row) — 0 for the whole triangle; a pass of the two-level form (fsk_sparse_blocks.inc) covers fewer than
// 2^32 cells from its first row on, so the difference is exact there too
__device__ __forceinline__ uint32_t sx_owner_of(uint32_t seq, int own_shift, uint32_t own_base) { return (sx_tri32(seq) - own_base) >> own_shift; }
// update words one (entry, partner) pair becomes: 1 while multiplicity * max_windows cannot overflow the
// product field, i.e. multiplicity <= cmax = maxprod / max_windows (everything but extreme
// low-complexity sequences); beyond that every pair of the entry takes `S` words
__device__ __forceinline__ uint32_t sx_words_per_pair(uint32_t count, uint32_t cmax, uint32_t max_win, uint32_t maxprod) {
    if (count <= cmax) return 1u;
    return (uint32_t)(((u64)count * max_win + maxprod - 1) / maxprod);
}

// WIDE entries. The consume kernels (k_sx_consume, k_sxb_consume) sum a batch's contributions to a cell in u32 LDS cells. A
// cell (i, j) takes sum_v c_i(v) c_j(v) a combination, the entries of row i sending the products: while every c_i(v) stays at
// or below cwide = (2^32 - 1) / max_windows that sum is at most cwide * sum_v c_j(v) <= cwide * max_windows < 2^32. The host
// keeps a batch to (2^32 - 1) / max_windows^2 combinations, which makes cwide >= max_windows — no entry is wide — until
// max_windows reaches 65,536; from there on a batch is ONE combination and an entry of multiplicity above cwide (a
// homopolymer's) adds its products into K itself, one 64-bit atomic each (k_sx_emit, as its DIRECT form does for every entry):
// it is neither binned nor a descriptor, and so that every count of words, every stream offset and every "no words, no launch"
// on the host stays what it is, it sends ONE word of product 0 to the first cell of its row. (By-slot batches — variance
// mode, u32 triangles by design — pass cwide = 2^32 - 1: never.)
__device__ __forceinline__ bool sx_wide_entry(uint32_t c, uint32_t cwide) { return c > cwide; }

// Entries of one tile: E (sequence, multiplicity), Pk (rank in run), and — unless `ucount` is null —
// the number of update words the tile will emit per owner band, ucount[tile][owner].
// stats[0] += pairs (the reference's `+=` count U), stats[1] += update words.
// skip_test_block (skip_from != 0xffffffff): Tk[e] = how many of the P partners of entry e, counted from
// the run start, it really pairs with before itself: all P - 1 for a train row; for a test row only the
// run's train entries (test x test cells other than the diagonal are left alone) — P minus its rank among
// the run's test entries. An entry then has Tk + 1 partners: Tk from the run start, and itself.
// Lane = record, like k_sx_seg_count: wave w takes records [512 w, 512 w + 512) of the tile in eight rounds of 64, and what
// a record needs to know — its entry index, the entry that heads its run, where the next entry starts (its
// multiplicity) — comes from the rounds' ballots (scalar registers), a popcount below the lane and one DPP running
// maximum per round: no per-thread serial scan, no LDS staging of the entries (consecutive entries sit in consecutive
// lanes, so E / Pk / Tk are written straight from the registers).
template <typename RecT, bool PACKED, bool PAIRS, bool SKIP, bool DESC = false>
__global__ __launch_bounds__(256) void k_sx_seg_write(const RecT* rec, uint32_t nfeat, uint32_t tpg, int sb, const uint32_t* ebase,
                                                      const int* tile_rs, typename SxEnt<PACKED>::ent_t* E,
                                                      typename SxEnt<PACKED>::rank_t* Pk, int own_shift, uint32_t n_owners,
                                                      uint32_t* ucount, uint32_t row0, uint32_t row1, uint32_t max_win,
                                                      uint32_t maxprod, uint32_t cmax, uint32_t cwide, u64* tile_stat, uint32_t skip_from,
                                                      const int* tile_ts, typename SxEnt<PACKED>::rank_t* Tk, uint32_t own_base,
                                                      uint32_t short_max_in, uint32_t desc_in, int desc_sub_shift, void* cols_in, int col16) {
    // (DESC: a template parameter — this kernel is bound by the instructions it issues, and the instantiation without
    // descriptors is the kernel as it was: config 4, 301 us a batch against 343 with the tests at run time)
    const uint32_t short_max = DESC ? short_max_in : SX_SHORT, desc = DESC ? desc_in : 0u;
    void* const cols = DESC ? cols_in : nullptr;
    // cols (may be null): the column array of the entries — sequence id | multiplicity << colbits (0 where it does not fit); 2 bytes
    // an entry or 4 (col16 = colbits << 1 | two bytes) — what k_sx_consume / k_sxb_consume read the partners of a descriptor from
    // short_max: most partners of an entry that k_sx_emit bins in LDS (SX_SHORT; fewer when descriptors take over earlier);
    // desc != 0: every other in-band entry leaves as a descriptor, and ucount has 2 * n_owners columns (descriptor words
    // of band o at column o, its update words at column n_owners + o)
    constexpr int ROUNDS = SG_TILE / 256;
    constexpr uint32_t NONE = 0xffffffffu;
    __shared__ uint32_t s_n[4], s_first[4];
    __shared__ int s_h[4], s_t[4];
    // per owner band: the tile's 32-bit words and, PAIRS, the bare cells of its unit entries
    __shared__ uint32_t s_cnt[SX_MAX_OWNERS];
    __shared__ uint32_t s_cntu[PAIRS ? SX_MAX_OWNERS : 1];
    __shared__ uint32_t s_cntd[DESC ? SX_MAX_OWNERS : 1];  // descriptor words per owner band (desc)
    __shared__ uint32_t s_short_words;
    __shared__ uint32_t s_end;
    __shared__ u64 s_red[8];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, t = blockIdx.x, slot = blockIdx.y;
    const uint32_t tile = slot * tpg + t;
    const RecT* r = rec + (size_t)slot * nfeat;
    const uint32_t first = t * (uint32_t)SG_TILE, w0 = wave * (uint32_t)(64 * ROUNDS);  // (w0: the wave's first record inside the tile)
    const uint32_t j0 = first + w0 + lane;
    if (ucount)
        for (uint32_t i = tid; i < n_owners; i += 256) {
            s_cnt[i] = 0u;
            if (PAIRS) s_cntu[i] = 0u;
            if (desc) s_cntd[i] = 0u;
        }
    if (tid == 0) s_short_words = 0u;
    // (the tile's carries, asked for now: needed only after the barrier below)
    const uint32_t eb = ebase[tile];
    const int before = tile_rs[tile];
    constexpr bool skipping = SKIP;
    const int before_t = skipping ? tile_ts[tile] : -1;
    const RecT seq_mask = (RecT)(((u64)1 << sb) - 1);
    RecT cur[ROUNDS], prev[ROUNDS];
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {  // (unconditional loads of clamped indices: what lies beyond the slot is never an entry)
        const uint32_t j = j0 + (uint32_t)q * 64u, jc = j < nfeat ? j : nfeat - 1u;
        cur[q] = r[jc];
        prev[q] = r[jc > 0u ? jc - 1u : 0u];  // (the neighbour lane's line: an L1 hit)
    }
    // (the tile's entries go to E / Pk / Tk [eb, ...): a scalar base and a 32-bit tile-local index per store)
    typename SxEnt<PACKED>::ent_t* const E_t = E + (size_t)eb;
    typename SxEnt<PACKED>::rank_t* const Pk_t = Pk + (size_t)eb;
    typename SxEnt<PACKED>::rank_t* const Tk_t = SKIP ? Tk + (size_t)eb : nullptr;
    if (tid == 255) {
        // where the tile's last entry ends: it may run on into the following tiles (bounded by the
        // number of windows of one sequence); the first look-ahead load rides with the loads above
        const uint32_t nv = nfeat - first < (uint32_t)SG_TILE ? nfeat - first : (uint32_t)SG_TILE;
        uint32_t j = first + nv;
        if (nv == (uint32_t)SG_TILE && j < nfeat && r[j] == cur[ROUNDS - 1]) {
            ++j;
            while (j < nfeat && r[j] == r[j - 1]) ++j;
        }
        s_end = j - first;
    }
    // ---- the wave's rounds as ballots; per lane one bit per round: entry / run head / test head
    u64 H[ROUNDS], R[ROUNDS], TH[ROUNDS];
    uint32_t is_entry = 0u, is_head = 0u, is_thead = 0u;
    uint32_t n = 0, firstpos = NONE;
    int lrh = -1, lth = -1;  // among this wave's entries, the last one that starts a run / is a test head
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const uint32_t j = j0 + (uint32_t)q * 64u;
        const bool entry = j < nfeat && (j == 0 || cur[q] != prev[q]);
        const bool run_head = entry && (j == 0 || (cur[q] >> sb) != (prev[q] >> sb));
        H[q] = __ballot(entry); R[q] = __ballot(run_head);
        is_entry |= (entry ? 1u : 0u) << q; is_head |= (run_head ? 1u : 0u) << q;
        TH[q] = 0;
        if (SKIP) {
            const bool test_head = entry && (uint32_t)(cur[q] & seq_mask) >= skip_from &&
                                   (run_head || (uint32_t)(prev[q] & seq_mask) < skip_from);
            TH[q] = __ballot(test_head);
            is_thead |= (test_head ? 1u : 0u) << q;
        }
        if (R[q]) lrh = (int)n + __popcll(H[q] & (((u64)1 << (63 - __clzll((long long)R[q]))) - 1));
        if (SKIP && TH[q]) lth = (int)n + __popcll(H[q] & (((u64)1 << (63 - __clzll((long long)TH[q]))) - 1));
        if (firstpos == NONE && H[q]) firstpos = (uint32_t)q * 64u + (uint32_t)(__ffsll((long long)H[q]) - 1);
        n += (uint32_t)__popcll(H[q]);
    }
    if (lane == 0) { s_n[wave] = n; s_h[wave] = lrh; s_t[wave] = lth; s_first[wave] = firstpos == NONE ? NONE : w0 + firstpos; }
    __syncthreads();
    // what the waves before this one hand over: their entries, the tile-local index of the last run / test head
    uint32_t base_w = 0;
    int carry_h = -1, carry_t = -1;
    for (uint32_t w = 0; w < wave; ++w) {
        if (s_h[w] >= 0) carry_h = (int)base_w + s_h[w];
        if (s_t[w] >= 0) carry_t = (int)base_w + s_t[w];
        base_w += s_n[w];
    }
    // where the next entry after round q starts (position inside the tile; after the last wave: the end of the tile's last entry)
    uint32_t nxt[ROUNDS];
    {
        uint32_t beyond = s_end;
        for (uint32_t w = 3; w > wave; --w)
            if (s_first[w] != NONE) beyond = s_first[w];
        nxt[ROUNDS - 1] = beyond;
#pragma unroll
        for (int q = ROUNDS - 2; q >= 0; --q)
            nxt[q] = H[q + 1] ? w0 + (uint32_t)(q + 1) * 64u + (uint32_t)(__ffsll((long long)H[q + 1]) - 1) : nxt[q + 1];
    }
    const u64 above = lane == 63u ? (u64)0 : ~(u64)0 << (lane + 1u);  // the lanes above this one
    // (PACKED: a lane's eight entries have fewer than 2^16 partners each, their sums fit 32 bits; words of
    // multi-word entries — extreme low-complexity sequences — are kept apart in 64 bits)
    typedef typename std::conditional<PACKED, uint32_t, u64>::type acc_t;
    acc_t pairs_t = 0, words_t = 0;
    u64 words_multi = 0;
    uint32_t nb = 0;          // entries of the wave's earlier rounds
    // wave-local entry index of the last run / test head of the earlier rounds. PAIRS: the run head's value is PACKED —
    // index << 10 | the number of entries of multiplicity > 1 the wave has seen before it —, so that the one running maximum
    // that finds a lane's run head also says how many such entries precede the head (512 entries a wave: 9 + 10 bits)
    int lrh_b = -1, lth_b = -1;
    uint32_t mb = 0;          // PAIRS: entries of multiplicity > 1 of the wave's earlier rounds
    uint32_t short_t = 0;     // PAIRS: words of this lane's SHORT entries (what k_sx_emit bins in LDS)
#pragma unroll
    for (int q = 0; q < ROUNDS; ++q) {
        const uint32_t ew = nb + fsk_mbcnt((uint32_t)H[q], (uint32_t)(H[q] >> 32));  // wave-local entry index (of an entry lane)
        // this lane's multiplicity (an entry lane): the distance to the next entry
        uint32_t c_mine = 0u;
        if ((is_entry >> q) & 1u) {
            const u64 later = H[q] & above;
            const uint32_t pos = w0 + (uint32_t)q * 64u + lane;
            c_mine = (later ? w0 + (uint32_t)q * 64u + (uint32_t)(__ffsll((long long)later) - 1) : nxt[q]) - pos;
        }
        u64 M = 0;
        uint32_t m_before = 0u;  // PAIRS: entries of multiplicity > 1 among the wave's entries before this lane
        if (PAIRS) {
            M = __ballot(c_mine > 1u);
            m_before = mb + fsk_mbcnt((uint32_t)M, (uint32_t)(M >> 32));
        }
        // the run head / test head that governs this lane: a running maximum over the lanes, then the earlier rounds, then the earlier waves
        int hv = fsk_hw::wave_incl_max_i32((is_head >> q) & 1u ? (PAIRS ? (int)((ew << 10) | m_before) : (int)ew) : -1);
        if (hv < lrh_b) hv = lrh_b;
        // UNIT entry: its run began in this wave and no entry of multiplicity > 1 lies in the run up to and including it
        const bool clean = PAIRS && hv >= 0 && c_mine == 1u && m_before == ((uint32_t)hv & 1023u);
        if (PAIRS && hv >= 0) hv >>= 10;
        const int head = hv >= 0 ? (int)base_w + hv : carry_h;
        int thead = -1;
        if (skipping) {  // (uniform)
            int tv = fsk_hw::wave_incl_max_i32((is_thead >> q) & 1u ? (int)ew : -1);
            if (tv < lth_b) tv = lth_b;
            thead = tv >= 0 ? (int)base_w + tv : carry_t;
        }
        if ((is_entry >> q) & 1u) {
            const uint32_t e = base_w + ew;
            const uint32_t rs = head >= 0 ? eb + (uint32_t)head : (uint32_t)before;
            const uint32_t seq = (uint32_t)(cur[q] & seq_mask);
            const uint32_t P = eb + e - rs + 1u;
            // partners before itself: everything from the run start (train row), or only the run's train
            // entries = P - (rank among the run's test entries)
            uint32_t T = P - 1u;
            if (SKIP && seq >= skip_from) {
                const uint32_t ts = thead >= 0 ? eb + (uint32_t)thead : (uint32_t)before_t;
                T = P - (eb + e - ts + 1u);
            }
            const uint32_t c = c_mine;
            // (the entry's own cell takes a word only when its multiplicity is above 1: see k_sx_diag_windows)
            const uint32_t np = T + (c > 1u ? 1u : 0u);
            const bool in_band = seq >= row0 && seq < row1;
            const bool is_short = np != 0u && np <= short_max && c <= cmax;  // (k_sx_emit's class 1: binned in LDS)
            const bool is_desc = np != 0u && !is_short && sx_desc_entry(desc, c, cmax, cwide);  // (k_sx_emit's class 5: descriptors)
            const bool unit = clean && in_band && is_short;
            E_t[e] = SxEnt<PACKED>::pack(seq, unit ? 0u : c);
            if (cols) {
                const int colbits = col16 >> 1, width = (col16 & 1) ? 16 : 32;
                const uint32_t h = seq | ((c >> (width - colbits)) ? 0u : c << colbits);
                if (col16 & 1) reinterpret_cast<uint16_t*>(cols)[(size_t)eb + e] = (uint16_t)h;
                else reinterpret_cast<uint32_t*>(cols)[(size_t)eb + e] = h;
            }
            Pk_t[e] = (typename SxEnt<PACKED>::rank_t)P;
            if (SKIP) Tk_t[e] = (typename SxEnt<PACKED>::rank_t)T;
            if (in_band) {
                uint32_t w = np;
                pairs_t += T + 1u;
                if (is_desc) {
                    const uint32_t dw = SX_DESC_WORDS * sx_desc_records(desc, seq, desc_sub_shift);
                    const uint32_t own = desc == 2u && c > 1u ? 1u : 0u;  // (blocks: the entry's own cell as one update word)
                    words_t += dw + own;
                    if (ucount) {
                        atomicAdd(&s_cntd[sx_owner_of(seq, own_shift, own_base)], dw);
                        if (own) atomicAdd(&s_cnt[sx_owner_of(seq, own_shift, own_base)], 1u);
                    }
                } else if (np != 0u && sx_wide_entry(c, cwide)) {  // (its products go to K as 64-bit atomics: one word of product 0)
                    words_t += 1u;
                    w = 1u;
                } else if (c > cmax) {  // (rare)
                    const u64 wm = (u64)np * sx_words_per_pair(c, cmax, max_win, maxprod);
                    words_multi += wm;
                    w = (uint32_t)wm;
                } else {
                    words_t += np;
                }
                if (PAIRS && is_short) short_t += np;
                if (ucount && !is_desc) atomicAdd(unit ? &s_cntu[sx_owner_of(seq, own_shift, own_base)] : &s_cnt[sx_owner_of(seq, own_shift, own_base)], w);
            }
        }
        if (R[q]) {
            const u64 below_last = ((u64)1 << (63 - __clzll((long long)R[q]))) - 1;  // the lanes below the round's last run head
            lrh_b = (int)nb + __popcll(H[q] & below_last);
            if (PAIRS) lrh_b = (lrh_b << 10) | (int)(mb + (uint32_t)__popcll(M & below_last));
        }
        if (SKIP && TH[q]) lth_b = (int)nb + __popcll(H[q] & (((u64)1 << (63 - __clzll((long long)TH[q]))) - 1));
        nb += (uint32_t)__popcll(H[q]);
        if (PAIRS) mb += (uint32_t)__popcll(M);
    }
    // PAIRS: the bare cells of the unit entries travel two to a 32-bit container, a band's share of the tile padded to a whole
    // container — when k_sx_emit bins the tile's short entries in ONE pass (their words fit its slot array: sx_one_pass, the
    // same rule there); a tile of more words (long runs) keeps them as 32-bit words. `saved` = what that takes off the
    // tile's word count.
    u64 saved = 0;
    if (ucount) {
        bool one_pass = true;
        if (PAIRS) {
            const u64 sw = fsk_hw::wave_sum_u64((u64)short_t);
            if (lane == 0 && sw) atomicAdd(&s_short_words, (uint32_t)sw);
        }
        __syncthreads();
        if (PAIRS) one_pass = sx_one_pass(s_short_words);
        uint32_t sv = 0;
        const uint32_t n_cols = desc ? 2u * n_owners : n_owners, wcol = desc ? n_owners : 0u;
        for (uint32_t o = tid; o < n_owners; o += 256) {
            uint32_t cells = 0, containers = 0;
            if (PAIRS) {
                cells = s_cntu[o];
                containers = one_pass ? (cells + 1u) >> 1 : cells;
            }
            ucount[(size_t)tile * n_cols + wcol + o] = s_cnt[o] + containers;
            if (desc) ucount[(size_t)tile * n_cols + o] = s_cntd[o];
            sv += cells - containers;
        }
        if (PAIRS) saved = fsk_hw::wave_sum_u64((u64)sv);
    }
    // (one record per tile, summed by k_sx_stat_sum: hundreds of thousands of atomics on one address
    // would serialise at the memory side)
    const u64 pairs_w = fsk_hw::wave_sum_u64((u64)pairs_t), words = fsk_hw::wave_sum_u64((u64)words_t + words_multi) - saved;
    if (lane == 0) { s_red[2 * wave] = pairs_w; s_red[2 * wave + 1] = words; }
    __syncthreads();
    if (tid == 0) {
        tile_stat[2 * (size_t)tile] = s_red[0] + s_red[2] + s_red[4] + s_red[6];
        tile_stat[2 * (size_t)tile + 1] = s_red[1] + s_red[3] + s_red[5] + s_red[7];
    }
}

// stats[0] += sum of tile_stat[2t], stats[1] += sum of tile_stat[2t + 1]; grid = 32 workgroups. The
// workgroup that finishes last (stats[2] counts them) hands both totals to `host_out`, pinned host
// memory the device writes directly: no copy command on the stream for 16 bytes.
// one thread per workgroup: its partial totals into stats[0], stats[1]; the workgroup that arrives last
// (stats[2] counts them) hands both totals to the pinned host words
__device__ __forceinline__ void sx_stat_add(u64 a, u64 b, u64* stats, u64* host_out) {
    if (a) atomicAdd(&stats[0], a);
    if (b) atomicAdd(&stats[1], b);
    __threadfence();
    if (atomicAdd(&stats[2], (u64)1) == (u64)gridDim.x - 1u) {
        host_out[0] = atomicAdd(&stats[0], (u64)0);
        host_out[1] = atomicAdd(&stats[1], (u64)0);
        __threadfence_system();
    }
}
__global__ __launch_bounds__(256) void k_sx_stat_sum(const u64* tile_stat, uint32_t ntiles, u64* stats, u64* host_out) {
    __shared__ u64 red[8];
    u64 a = 0, b = 0;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < ntiles; t += gridDim.x * 256u) {
        a += tile_stat[2 * (size_t)t];
        b += tile_stat[2 * (size_t)t + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    if ((threadIdx.x & 63u) == 0) { red[2 * (threadIdx.x >> 6)] = a; red[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) sx_stat_add(red[0] + red[2] + red[4] + red[6], red[1] + red[3] + red[5] + red[7], stats, host_out);
}

// ---- offsets of the update streams: column scan of ucount[tile][owner] -----------------------
constexpr int UC_CHUNK = 64;  // tiles per chunk at most (the launches' `uc`: fewer for a batch of few tiles, whose chunks would
                              // otherwise be a few dozen workgroups walking 64 dependent steps each)
// chunk_tot[chunk][owner] = words of the chunk's tiles for the owner; grid = chunks. Also what k_sx_stat_sum
// does (the batch's pair and word totals from the per-tile records), one launch less per batch.
__global__ __launch_bounds__(256) void k_sx_ucol_sum(const uint32_t* ucount, uint32_t ntiles, uint32_t n_owners, uint32_t* chunk_tot,
                                                     const u64* tile_stat, u64* stats, u64* host_out, uint32_t uc) {
    const uint32_t chunk = blockIdx.x, t0 = chunk * uc;
    const uint32_t t1 = t0 + uc < ntiles ? t0 + uc : ntiles;
    static_assert(UC_CHUNK == 64, "one wave sums a chunk's tile records");
    if (threadIdx.x < 64u) {
        const uint32_t t = t0 + threadIdx.x;
        u64 a = t < t1 ? tile_stat[2 * (size_t)t] : 0, b = t < t1 ? tile_stat[2 * (size_t)t + 1] : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            a += __shfl_xor(a, d);
            b += __shfl_xor(b, d);
        }
        if (threadIdx.x == 0) sx_stat_add(a, b, stats, host_out);
    }
    // The chunk's (t1 - t0) x n_owners counts are one contiguous piece of the matrix: the threads stream it in 16-byte
    // pieces, every load issued before the first use, and add into the owners' LDS counters (a thread per owner walking its
    // column read 4 bytes a lane with a stride of n_owners words between its loads: 63 us a batch at config 4 for 52 MB).
    __shared__ uint32_t s_tot[SX_MAX_COLS];  // (n_owners: the columns of the matrix — two a band with descriptors)
    for (uint32_t o = threadIdx.x; o < n_owners; o += 256) s_tot[o] = 0u;
    __syncthreads();
    const size_t first = (size_t)t0 * n_owners;
    const uint32_t count = (t1 - t0) * n_owners;
    const uint32_t head = (uint32_t)((4u - (uint32_t)(first & 3u)) & 3u) < count ? (uint32_t)((4u - (uint32_t)(first & 3u)) & 3u) : count;
    const uint32_t n4 = (count - head) >> 2, tail0 = head + 4u * n4;
    // (the chunk starts on a row: the owner of element x of it is x mod n_owners)
    if (threadIdx.x < head) atomicAdd(&s_tot[threadIdx.x % n_owners], ucount[first + threadIdx.x]);
    else if (threadIdx.x - head < count - tail0) {
        const uint32_t i = tail0 + (threadIdx.x - head);
        atomicAdd(&s_tot[i % n_owners], ucount[first + i]);
    }
    const uint4* u4 = reinterpret_cast<const uint4*>(ucount + first + head);
    for (uint32_t q0 = threadIdx.x; q0 < n4; q0 += 4u * 256u) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t q = q0 + (uint32_t)u * 256u;
            v[u] = q < n4 ? u4[q] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t q = q0 + (uint32_t)u * 256u;
            if (q < n4) {
                uint32_t o = (head + 4u * q) % n_owners;
                if (v[u].x) atomicAdd(&s_tot[o], v[u].x);
                o = o + 1u == n_owners ? 0u : o + 1u;
                if (v[u].y) atomicAdd(&s_tot[o], v[u].y);
                o = o + 1u == n_owners ? 0u : o + 1u;
                if (v[u].z) atomicAdd(&s_tot[o], v[u].z);
                o = o + 1u == n_owners ? 0u : o + 1u;
                if (v[u].w) atomicAdd(&s_tot[o], v[u].w);
            }
        }
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < n_owners; o += 256) chunk_tot[(size_t)chunk * n_owners + o] = s_tot[o];
}
// per owner: exclusive scan over the chunks in place, owner total to utot; grid = owners
__global__ __launch_bounds__(256) void k_sx_ucol_scan(uint32_t* chunk_tot, uint32_t nchunks, uint32_t n_owners, uint32_t* utot) {
    __shared__ uint32_t tmp[4];
    const uint32_t o = blockIdx.x, tid = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nchunks; base += 256) {
        const uint32_t c = base + tid;
        const uint32_t v = c < nchunks ? chunk_tot[(size_t)c * n_owners + o] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_256<uint32_t>(v, tmp, &tot) + carry;
        if (c < nchunks) chunk_tot[(size_t)c * n_owners + o] = ex;
        carry += tot;
    }
    if (tid == 0) utot[o] = carry;
}
// ucount[tile][owner] -> words of the owner emitted by earlier tiles; grid = chunks. Workgroup 0 also turns
// the owner totals into where each owner's stream starts (list_off[n_owners] = all words).
__global__ __launch_bounds__(256) void k_sx_ucol_apply(uint32_t* ucount, uint32_t ntiles, uint32_t n_owners, const uint32_t* chunk_tot,
                                                       const uint32_t* utot, uint32_t* list_off, uint32_t uc) {
    if (blockIdx.x == 0) {  // (uniform)
        __shared__ uint32_t tmp[4];
        uint32_t carry = 0;
        for (uint32_t base = 0; base < n_owners; base += 256) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t v = i < n_owners ? utot[i] : 0u;
            uint32_t tot;
            const uint32_t ex = block_excl_scan_256<uint32_t>(v, tmp, &tot) + carry;
            if (i < n_owners) list_off[i] = ex;
            carry += tot;
        }
        if (threadIdx.x == 0) list_off[n_owners] = carry;
    }
    const uint32_t chunk = blockIdx.x, t0 = chunk * uc;
    const uint32_t t1 = t0 + uc < ntiles ? t0 + uc : ntiles;
    for (uint32_t o = threadIdx.x; o < n_owners; o += 256) {
        uint32_t run = chunk_tot[(size_t)chunk * n_owners + o];
        for (uint32_t t = t0; t < t1; ++t) {
            const uint32_t v = ucount[(size_t)t * n_owners + o];
            ucount[(size_t)t * n_owners + o] = run;
            run += v;
        }
    }
}

// ---- pair updates ----------------------------------------------------------------------------
// Entry e = (i, c) with rank P in its run pairs with entries e-P+1 .. e = (j <= i, c_j): K[i][j] += c * c_j.
// Update word = (cell - first cell of the owner band) << pb | product, cell = tri_index(i, j).
// One workgroup of 512 threads per entry tile (the entries one k_sx_seg_write tile produced).
// DIRECT: 64-bit atomicAdd per pair straight into K instead of update words.
// Partner `pl` (tile-local entry index; negative: the run started before the tile, that entry sits in global
// memory at e0 + pl). Always an LDS read (clamped) and, for the few lanes with pl < 0, a global load on top:
// written as `pl >= 0 ? s_ent[pl] : E[...]` the two address spaces meet in one generic pointer and every
// partner becomes a flat_load behind an exec-mask diamond.
template <bool PACKED>
__device__ __forceinline__ uint2 sx_partner_at(const typename SxEnt<PACKED>::ent_t* s_ent, const typename SxEnt<PACKED>::ent_t* E,
                                               uint32_t e0, int pl) {
    // (an explicit LDS-address-space load: through the generic pointer the two loads are merged back into one)
    uint2 pq = SxEnt<PACKED>::lds(&s_ent[pl >= 0 ? pl : 0]);
    if (pl < 0) pq = SxEnt<PACKED>::unpack(E[(size_t)e0 - (size_t)(-pl)]);
    pq.y = sx_mult(pq.y);  // (a unit entry carries 0 in its multiplicity field)
    return pq;
}
// The same from LDS alone: k_sx_emit keeps the SX_SHORT entries in front of the tile's first next to the tile's own (s_ent[-1]
// is the entry before the tile), which is as far back as a short or half-wave entry's run can begin. Why it matters: the
// word loops STORE a word per lane and trip, and on gfx950 loads and stores share one counter — a wait for a load (the
// compiler places one behind every conditional global read, taken or not) is a wait for every store before it, so each trip
// of the loops stood for a full round trip of the previous trip's stores (the vmcnt(0) in front of every store group in the ISA).
template <bool PACKED>
__device__ __forceinline__ uint2 sx_partner_lds(const typename SxEnt<PACKED>::ent_t* s_ent, int pl) {
    uint2 pq = SxEnt<PACKED>::lds(&s_ent[pl]);
    pq.y = sx_mult(pq.y);
    return pq;
}
template <bool PACKED>
__device__ __forceinline__ uint2 sx_entry_at(const typename SxEnt<PACKED>::ent_t* s_ent, uint32_t el) {
    uint2 a = SxEnt<PACKED>::unpack(s_ent[el]);
    a.y = sx_mult(a.y);
    return a;
}
// (measurement builds only — tools/build_variant.sh ... -DFSK_EM_CLOCKS=1 —: cycles per phase of k_sx_emit, summed over the
// workgroups by their first thread, read back with fsk_debug_emit_clocks; tools/emit_phases.py)
#if defined(FSK_EM_CLOCKS) && FSK_EM_CLOCKS
__device__ unsigned long long g_em_clk[16];
#define FSK_EM_MARK(i) { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long t_ = clock64(); atomicAdd(&g_em_clk[i], t_ - em_t0); em_t0 = t_; } }
#define FSK_EM_MARK_INIT unsigned long long em_t0 = clock64(); const unsigned long long em_tb = em_t0; if (threadIdx.x == 0) atomicAdd(&g_em_clk[15], 1ull);
// ([14]: the longest workgroup; [13] / [12]: workgroups beyond 200 k / 400 k cycles)
#define FSK_EM_MARK_END { if (threadIdx.x == 0) { const unsigned long long d_ = clock64() - em_tb; atomicMax(&g_em_clk[14], d_); if (d_ > 200000ull) atomicAdd(&g_em_clk[13], 1ull); if (d_ > 400000ull) atomicAdd(&g_em_clk[12], 1ull); } }
#else
#define FSK_EM_MARK(i)
#define FSK_EM_MARK_INIT
#define FSK_EM_MARK_END
#endif
#ifndef FSK_EM_THREADS
#define FSK_EM_THREADS 512              // (256 — with at most 256 owner bands — measured 10 % slower on config 4)
#endif
constexpr int EM_THREADS = FSK_EM_THREADS, EM_WAVES = EM_THREADS / 64;
#ifndef FSK_EM_MIN_WAVES
#define FSK_EM_MIN_WAVES 6             // waves per SIMD the register allocation aims at: three workgroups of eight waves a CU
#endif
constexpr int EM_PER = SG_TILE / EM_THREADS;              // entries per thread when a tile's short entries go in one pass
template <bool DIRECT, bool SKIP, bool PACKED, bool DESC = false>
__global__ __launch_bounds__(EM_THREADS, FSK_EM_MIN_WAVES) void k_sx_emit(const typename SxEnt<PACKED>::ent_t* E, const typename SxEnt<PACKED>::rank_t* Pk,
                                                        const uint32_t* ebase,
                                                        const uint32_t* owner_r0, int own_shift, uint32_t n_owners,
                                                        const uint32_t* list_off, const uint32_t* tile_off, uint32_t* list,
                                                        uint32_t row0, uint32_t row1, uint32_t max_win, uint32_t maxprod,
                                                        uint32_t cmax, uint32_t cwide, int pb, u64* K, uint32_t tpg, u64 slot_stride,
                                                        const typename SxEnt<PACKED>::rank_t* Tk, const u64* batch_stat, u64 cap_words,
                                                        uint32_t n_tiles, int pairs, uint32_t own_base, uint32_t short_max_in,
                                                        uint32_t desc_in, int desc_sub_shift) {
    // (DESC: a template parameter, as k_sx_seg_write's — without it this is the kernel as it was)
    const uint32_t short_max = DESC ? short_max_in : SX_SHORT, desc = DESC ? desc_in : 0u;
    // short_max, desc: as k_sx_seg_write's — with descriptors list_off / tile_off have 2 * n_owners columns, a band's
    // descriptor stream at column o and its update words at column n_owners + o
    typedef SxEnt<PACKED> X;
    typedef typename X::ent_t ent_t;
    typedef typename X::rank_t rank_t;
    // (the host may launch this before it knows the batch's word count: a batch that does not fit the
    // stream buffer is left alone — every workgroup sees the same total — and redone by the host)
    // (the 64-bit total of k_sx_stat_sum: the 32-bit stream offsets wrap for a batch beyond 2^32 words)
    // (the tile's entries behind the EM_PRE entries in front of the tile: s_ent[-1 .. -EM_PRE], see sx_partner_lds)
    constexpr int EM_PRE = (int)SX_SHORT;
    __shared__ __attribute__((aligned(8))) ent_t s_ent_store[SG_TILE + EM_PRE];
    ent_t* const s_ent = s_ent_store + EM_PRE;
    __shared__ rank_t s_P[SG_TILE];
    // partners before the entry itself, from its run's start: P - 1 unless skip_test_block (SKIP)
    __shared__ rank_t s_T[SKIP ? SG_TILE : 1];
    // per owner band: x = first slot of the band's segment of the pass at hand, then (address in the band's stream) -
    // (slot); y = the band's first cell
    __shared__ uint2 s_segc0[SX_MAX_OWNERS];
    __shared__ uint32_t s_cur[SX_MAX_OWNERS];   // next free word of this tile's share of each owner's stream
    // per owner band and pass: 32-bit words (low half) | bare cells of unit entries (high half); then (PAIRS) where the band's
    // containers of paired cells go: (address in the band's stream) - (container index in the pass)
    __shared__ uint32_t s_cnt[SX_MAX_OWNERS];
    __shared__ uint16_t s_startb[SX_MAX_OWNERS];  // PAIRS: the band's first container of paired cells inside the pass
    // a pass's update words in owner order: slot -> the entry it belongs to; per entry: its first slot,
    // the cell of column 0 of its row inside the owner band, its owner. (After the short entries the
    // slot array holds the list of long entries.)
    // (one block: the slot array, then the entries' records — the long entries' list and headers reuse both once the short entries are done)
    __shared__ __attribute__((aligned(8))) uint32_t s_pool[(EM_SLOTS + 1u) / 2u + SG_TILE];
    uint16_t* const slot_ent = reinterpret_cast<uint16_t*>(s_pool);
    // per binned entry: owner << 16 | (uint16_t)(first partner - first slot), both tile-local: slot i belongs to
    // partner (int16)(rec) + i (negative: the run started before the tile). (SKIP: -(first slot) instead.) The cell
    // of a word follows from the entry's row and its band's first cell (s_segc0).
    uint32_t* const ent_rec = s_pool + (EM_SLOTS + 1u) / 2u;
    __shared__ uint32_t s_nlong, s_nhalf, s_total;
    __shared__ uint32_t tmp[EM_WAVES];
    uint16_t* const s_long = slot_ent;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile = xcd_contiguous(blockIdx.x, n_tiles);  // grid = xcd_grid(n_tiles)
    if (tile == n_tiles) return;  // (uniform)
    FSK_EM_MARK_INIT
    // Everything the prologue reads that does not depend on something else it reads is asked for up front — the batch's word
    // total, the tile's entry range, the thread's band of the three band tables (n_owners <= EM_THREADS: one band a thread) —: as
    // written before (total -> return? -> entry range -> tables -> LDS -> entries) these were four round trips one behind the
    // other in front of the entries' own, a third of the kernel's time on short tiles (profiles/r06_emit_phases_large_g.txt).
    static_assert(SX_MAX_OWNERS <= EM_THREADS, "one owner band a thread in k_sx_emit's prologue");
    const uint32_t n_cols = desc ? 2u * n_owners : n_owners, wcol = desc ? n_owners : 0u;
    const u64 words_total = DIRECT ? (u64)0 : batch_stat[1];
    const uint32_t e0 = ebase[tile], e_end = ebase[tile + 1];
    uint32_t t_r0 = 0u, t_lo = 0u, t_to = 0u, t_dcur = 0u;
    if (!DIRECT && tid < n_owners) {
        t_r0 = owner_r0[tid];
        t_lo = list_off[wcol + tid];
        t_to = tile_off[(size_t)tile * n_cols + wcol + tid];
        if (DESC && desc) t_dcur = list_off[tid] + tile_off[(size_t)tile * n_cols + tid];  // (where the tile's descriptors of the band go)
    }
    // (the test names the entry range too — never true by it —: left to itself the compiler asks for the range only behind
    // the branch, a scalar round trip of its own behind the word total's)
    if (!DIRECT && (words_total > cap_words || e_end < e0)) return;  // (uniform; see above)
    const uint32_t n = e_end - e0;
    if (DIRECT) K += (u64)(tile / tpg) * slot_stride;  // one triangle per slot (variance mode) when slot_stride != 0
    // What the thread knows about ITS entries (e = q * EM_THREADS + tid, the ones it also counts, bins and
    // lists below) stays in registers: row, partner count, class (0: outside the row band / none, 1: short,
    // 2: long, 3: long with at most 32 partners and one word per pair) — the phases below would otherwise re-read and re-classify them from LDS three times.
    uint32_t my_row[EM_PER], my_np[EM_PER], my_cls[EM_PER];
    {   // the tile's entries: every load issued before the first LDS store (one memory latency, not EM_PER)
        ent_t le[EM_PER];
        rank_t lp[EM_PER], lt[EM_PER];
        ent_t pre = X::pack(0u, 0u);
        if (tid < (uint32_t)EM_PRE && e0 > tid) pre = E[(size_t)e0 - 1u - tid];
#pragma unroll
        for (int q = 0; q < EM_PER; ++q) {
            const uint32_t e = (uint32_t)q * EM_THREADS + tid;
            le[q] = X::pack(0u, 0u);
            lp[q] = lt[q] = 0u;
            if (e < n) {
                le[q] = E[(size_t)e0 + e];
                lp[q] = Pk[(size_t)e0 + e];
                if (SKIP) lt[q] = Tk[(size_t)e0 + e];
            }
        }
        if (!DIRECT && tid < n_owners) {  // (the band tables: asked for above, stored now that the entries' loads are on their way)
            s_segc0[tid].y = sx_tri32(t_r0);
            s_cur[tid] = t_lo + t_to;
        }
#pragma unroll
        for (int q = 0; q < EM_PER; ++q) {
            const uint32_t e = (uint32_t)q * EM_THREADS + tid;
            const uint2 ue = X::unpack(le[q]);
            if (q == 0 && tid < (uint32_t)EM_PRE) s_ent[-1 - (int)tid] = pre;
            my_row[q] = ue.x;
            // partners that take a word: the T (= P - 1 unless SKIP) entries before it in its run, and itself when its
            // multiplicity is above 1 (k_sx_diag_windows)
            my_np[q] = e < n ? (SKIP ? (uint32_t)lt[q] : (uint32_t)lp[q] - 1u) + (ue.y > 1u ? 1u : 0u) : 0u;
            my_cls[q] = 0u;
            if (e < n) {
                s_ent[e] = le[q];
                s_P[e] = lp[q];
                if (SKIP) s_T[e] = lt[q];
                if (ue.x >= row0 && ue.x < row1 && my_np[q] != 0u)
                {
                    const bool one_word = DIRECT || sx_words_per_pair(sx_mult(ue.y), cmax, max_win, maxprod) == 1u;
                    // (class 4: a UNIT entry — multiplicity field 0, k_sx_seg_write's mark: always short, every product 1)
                    // (class 5, descriptors: every entry that is not binned leaves as one descriptor)
                    my_cls[q] = (my_np[q] <= short_max && one_word) ? ((!DIRECT && ue.y == 0u) ? 4u : 1u)
                                : (!DIRECT && sx_desc_entry(desc, sx_mult(ue.y), cmax, cwide)) ? 5u
                                : (!DIRECT && !SKIP && one_word && my_np[q] <= 32u) ? 3u : 2u;
                }
            }
        }
    }
    __syncthreads();
    FSK_EM_MARK(0)  // entries loaded and classified
    // partner `ge` of an entry: the tile's own entries sit in LDS, a run that started before the tile
    // continues in global memory
#define SX_ENT(el) sx_entry_at<PACKED>(s_ent, el)
#define SX_PARTNER(ge) sx_partner_at<PACKED>(s_ent, E, e0, (int)(ge) - (int)e0)
    // partner number b (0 .. T) of tile-local entry el: the run's first T entries, then the entry itself
#define SX_NPART(el) ((SKIP ? (uint32_t)s_T[el] : (uint32_t)s_P[el] - 1u) + (SX_ENT(el).y > 1u ? 1u : 0u))
    // is partner number b of entry el the entry itself (its own cell: multiplicity * (multiplicity - 1), see k_sx_diag_windows)
#define SX_IS_SELF(el, b) (SKIP ? (b) >= (uint32_t)s_T[el] : (b) + 1u == (uint32_t)s_P[el])
#define SX_PARTNER_OF(el, b) SX_PARTNER((!SKIP || (b) < (uint32_t)s_T[el]) ? e0 + (el) - (uint32_t)s_P[el] + 1u + (b) : e0 + (el))
    // an entry is SHORT (binned below) with up to SX_SHORT partners and one word per pair, else LONG (a wave each, further down)
#define SX_IS_SHORT(el) (SX_NPART(el) != 0u && SX_NPART(el) <= short_max && (DIRECT || sx_words_per_pair(SX_ENT(el).y, cmax, max_win, maxprod) == 1u))
#define SX_IN_BAND(el) (SX_ENT(el).x >= row0 && SX_ENT(el).x < row1)
    if (DIRECT) {
        for (uint32_t e = tid; e < n; e += EM_THREADS) {
            if (SX_IN_BAND(e) && SX_IS_SHORT(e)) {
                const uint2 a = SX_ENT(e);
                const uint32_t P = SX_NPART(e);
                u64* row = K + tri_index((u64)a.x, 0);
                for (uint32_t b = 0; b < P; ++b) {
                    const uint2 pq = SX_PARTNER_OF(e, b);
                    atomicAdd(&row[pq.x], (u64)a.y * (pq.y - (SX_IS_SELF(e, b) ? 1u : 0u)));
                }
            }
        }
    } else {
        // ---- short entries. All of the tile's in one pass when their words fit the slot array (the usual case: ~4 partners per
        // entry) — straight-line code, every entry from the registers of the thread that loaded it; else in as few passes as
        // their WORDS need: the entries are taken in order, a pass ends where the running sum of their words reaches EM_CAP (a
        // tile of long runs, ten or twenty words an entry, takes two or three passes — it was SG_TILE * SX_SHORT / EM_SLOTS =
        // nine whatever the entries held), and a pass re-reads its entries from LDS (a loop over passes that kept them in
        // registers cost 30 VGPRs more for the whole kernel).
        // PAIRS: the words of UNIT entries (class 4) are bare 15-bit cells; they are binned like the others, in a region of
        // their own behind the 32-bit words' slots, and leave two to a container: {1, cell: 15 bits, 0, cell: 15 bits}
        // (0x7fff: none — the second half of a band's last container when its cells are odd in number). A band's share of
        // the pass in its stream: the containers of pairs first, then the 32-bit words. (One-pass tiles only: k_sx_seg_write
        // counted the unit entries' cells two to a word only there.)
        // The cell of column 0 of a binned entry's row inside its band replaces the entry's rank in s_P once the rank is used up
        // (not SKIP: the rank is read again per word) — when the rank type holds it: any band with 32-bit ranks, a band of at
        // most 2^16 cells (pb >= 16: every band one round of k_sx_consume sums) with 16-bit ones. (Uniform.)
        const bool CB_IN_P = !SKIP && (!PACKED || pb >= 16);
        constexpr uint32_t EM_CAP = EM_SLOTS - SX_SHORT;  // words a pass takes on before it ends (its last entry may add up to SX_SHORT - 1)
        constexpr uint32_t EM_MAX_PASS = (uint32_t)SG_TILE * SX_SHORT / EM_CAP + 1u;
        __shared__ uint32_t s_chunk[EM_PER][EM_WAVES];
        __shared__ uint32_t s_bnd[EM_MAX_PASS + 1];   // first entry of every pass (several passes only)
        // `all`: the words of the tile's short entries — one sum over the workgroup. Only a tile that needs several passes (long
        // runs) goes on to the running sums per entry that say where its passes end; for the usual tile those were a fifth of
        // the instructions this kernel issues.
        uint32_t all = 0;
        {
            uint32_t mine = 0;
#pragma unroll
            for (int q = 0; q < EM_PER; ++q) mine += (my_cls[q] == 1u || my_cls[q] == 4u) ? my_np[q] : 0u;
            const uint32_t wsum = fsk_hw::wave_sum_u32(mine);
            if (lane == 0u) s_chunk[0][wave] = wsum;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < EM_WAVES; ++w) all += s_chunk[0][w];
        }
        if (!sx_one_pass(all)) {  // (uniform)
            // the words of the short entries before each of the thread's entries, in entry order (entry q * EM_THREADS + tid: the
            // threads hold consecutive entries of chunk q, so a scan over the threads per chunk, all chunks behind one barrier)
            uint32_t incl[EM_PER], run = 0;
            __syncthreads();  // (s_chunk[0] has been read)
            if (tid <= EM_MAX_PASS) s_bnd[tid] = tid ? n : 0u;
#pragma unroll
            for (int q = 0; q < EM_PER; ++q) {
                incl[q] = fsk_hw::wave_incl_sum_u32((my_cls[q] == 1u || my_cls[q] == 4u) ? my_np[q] : 0u);
                if (lane == 63u) s_chunk[q][wave] = incl[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < EM_PER; ++q) {
                uint32_t before = 0, tot = 0;
#pragma unroll
                for (int w = 0; w < EM_WAVES; ++w) {
                    const uint32_t t = s_chunk[q][w];
                    if ((uint32_t)w < wave) before += t;
                    tot += t;
                }
                // (a pass ends with the one short entry whose words take the running sum to or past the next multiple of EM_CAP)
                if (my_cls[q] == 1u || my_cls[q] == 4u) {
                    const uint32_t after = run + before + incl[q], pass_after = after / EM_CAP;
                    if (after >= EM_CAP && (after - my_np[q]) / EM_CAP != pass_after) s_bnd[pass_after] = (uint32_t)q * EM_THREADS + tid + 1u;
                }
                run += tot;
            }
        }
        const bool one_pass = sx_one_pass(all);
        // one pass of the binning: the short entries [ea, eb) of the tile. OWN: every entry is the thread's own entry q (registers)
        auto bin_pass = [&](auto own_tag, const uint32_t ea, const uint32_t eb) __attribute__((always_inline)) {
            constexpr bool OWN = decltype(own_tag)::value;
            const bool paired = OWN && pairs;
            for (uint32_t o = tid; o < n_owners; o += EM_THREADS) s_cnt[o] = 0u;
            __syncthreads();
            // (what an entry of the pass learns here — its owner band, its place among the band's words or cells — waits in its
            // record in LDS, not in registers, for the scan below; `took`: which of the thread's EM_PER entries take part)
            uint32_t took = 0u;
#pragma unroll
            for (int q = 0; q < EM_PER; ++q) {
                const uint32_t e = ea + (uint32_t)q * EM_THREADS + tid;
                uint32_t o = 0u, np = 0u;
                bool unit = false, in = false;
                if (OWN) {
                    if (my_cls[q] == 1u || my_cls[q] == 4u) {
                        in = true;
                        o = sx_owner_of(my_row[q], own_shift, own_base);
                        np = my_np[q];
                        unit = paired && my_cls[q] == 4u;
                    }
                } else if (e < eb && SX_IN_BAND(e) && SX_IS_SHORT(e)) {
                    in = true;
                    o = sx_owner_of(SX_ENT(e).x, own_shift, own_base);
                    np = SX_NPART(e);
                }
                if (in) {
                    took |= 1u << q;
                    const uint32_t old = atomicAdd(&s_cnt[o], unit ? np << 16 : np);
                    ent_rec[e] = (o << 16) | (unit ? 0x8000u | (old >> 16) : old & 0x7fffu);  // (a band's words or cells of a pass: < 2^14)
                }
            }
            __syncthreads();
            // exclusive scan of the owner counts (n_owners <= 512 = one per thread): both halves at once — the 32-bit words
            // (low) and the cells (high) of a pass stay below 2^16 each
            {
                const uint32_t cnt_o = tid < n_owners ? s_cnt[tid] : 0u;
                uint32_t tot;
                const uint32_t ex = block_excl_scan<uint32_t, EM_WAVES>(cnt_o, tmp, &tot);
                if (tid < n_owners) {
                    const uint32_t cells = cnt_o >> 16, containers = (cells + 1u) >> 1;
                    s_segc0[tid].x = ex & 0xffffu;
                    s_startb[tid] = (uint16_t)(ex >> 16);
                    s_cnt[tid] = (cnt_o & 0xffffu) | (containers << 16);  // 32-bit words | containers of pairs
                    // (an odd number of cells: the second half of the band's last container holds none)
                    if (cells & 1u) reinterpret_cast<uint16_t*>(list + s_cur[tid])[cells] = (uint16_t)0xffffu;
                }
                if (tid == 0) s_total = tot;
            }
            __syncthreads();
            FSK_EM_MARK(6)  // (measurement builds: zeroed, binned, scanned — the fill of the slots follows)
            const uint32_t total = s_total & 0xffffu;  // 32-bit words (the cells' slots lie behind theirs)
#pragma unroll
            for (int q = 0; q < EM_PER; ++q) {
                if ((took >> q) & 1u) {
                    const uint32_t e = ea + (uint32_t)q * EM_THREADS + tid;
                    const uint32_t r0 = ent_rec[e], o = r0 >> 16;
                    const bool unit = (r0 & 0x8000u) != 0u;
                    // first slot of the entry's words: among the band's 32-bit words, or among its cells (region-relative)
                    const uint32_t at = (unit ? (uint32_t)s_startb[o] : s_segc0[o].x) + (r0 & 0x7fffu);
                    const uint32_t P = OWN ? my_np[q] : SX_NPART(e);  // (words, not the rank)
                    // (|first partner - first slot| < SG_TILE + EM_SLOTS < 2^15; SKIP: a test row may sit deep in a
                    // long run, so only -(first slot) is kept and the partner comes from s_P / s_T)
                    const int rel = SKIP ? -(int)at : (int)e - (int)(uint32_t)s_P[e] + 1 - (int)at;
                    ent_rec[e] = (o << 16) | ((uint32_t)rel & 0xffffu);
                    // (the rank of a binned entry has done its work — `rel` —: its place holds the cell of column 0 of the entry's
                    // row inside its band from here on, what every word of the entry starts from)
                    if (CB_IN_P) s_P[e] = (rank_t)(sx_tri32(OWN ? my_row[q] : SX_ENT(e).x) - s_segc0[o].y);
                    // the entry's P slots: an odd first slot alone, then two a 32-bit store, an odd last one alone. (Left as `for (b <
                    // P) dst[b] = e` the loop is vectorised — 128-, 64- and 16-bit store loops with their trip counts and guards, all of
                    // which a wave runs as soon as one lane has four words: ~65 VALU instructions an entry against ~35 here, and this
                    // kernel is bound by the instructions it issues.)
                    const uint32_t s0 = (unit ? total : 0u) + at, odd = s0 & 1u, rest = P - odd;  // (P >= 1)
                    if (odd) slot_ent[s0] = (uint16_t)e;
                    uint32_t* const d2 = reinterpret_cast<uint32_t*>(slot_ent + s0 + odd);
                    const uint32_t ee = e | (e << 16);
#pragma clang loop vectorize(disable) unroll(disable)
                    for (uint32_t j = 0; j < (rest >> 1); ++j) d2[j] = ee;
                    if (rest & 1u) slot_ent[s0 + P - 1u] = (uint16_t)e;
                }
            }
            __syncthreads();
            // slot -> address in the owner's stream (the band's pairs first: cnt_b / 2 containers)
            // (and, for the cells: 2 * (the band's share) - (its first cell slot), in halves; the share's next free word moves on here)
            if (tid < n_owners) {
                const uint32_t cur = s_cur[tid], c = s_cnt[tid];
                s_segc0[tid].x = cur + (c >> 16) - s_segc0[tid].x;
                s_cnt[tid] = 2u * cur - (uint32_t)s_startb[tid];
                s_cur[tid] = cur + (c & 0xffffu) + (c >> 16);
            }
            __syncthreads();
            FSK_EM_MARK(1)  // short entries binned, slots filled
            // ---- the 32-bit words: one update word per thread and trip, whatever the entries' partner counts: slot i is
            // partner i - (first slot) of its entry; neighbouring slots go to neighbouring addresses of one stream
            // (four words per thread and trip: their chains of LDS reads — slot, record, partner — are
            // independent, so the latencies overlap instead of adding up)
            for (uint32_t i0 = tid; i0 < total; i0 += 4u * EM_THREADS) {
                uint32_t el[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + (uint32_t)u * EM_THREADS;
                    el[u] = slot_ent[i < total ? i : i0];
                }
                uint32_t rec[4];
                uint2 me[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    rec[u] = ent_rec[el[u]];
                    me[u] = SX_ENT(el[u]);
                }
                int pl[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + (uint32_t)u * EM_THREADS;
                    pl[u] = (int)(int16_t)(uint16_t)rec[u] + (int)(i < total ? i : i0);  // tile-local index of the partner
                    if (SKIP)  // (here pl = b, the partner's number: the run's first T entries, then the entry itself)
                        pl[u] = (uint32_t)pl[u] < (uint32_t)s_T[el[u]] ? (int)el[u] - (int)s_P[el[u]] + 1 + pl[u] : (int)el[u];
                }
                uint2 pq[4];
                uint32_t dlt[4], cb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    // (a short entry's run begins at most SX_SHORT entries before it: LDS; SKIP pairs with the run's FIRST entries, however far)
                    pq[u] = SKIP ? sx_partner_at<PACKED>(s_ent, E, e0, pl[u]) : sx_partner_lds<PACKED>(s_ent, pl[u]);
                    // cell of column 0 of the entry's row inside the band: from the entry's record (CB_IN_P) or from the row and the band
                    if (CB_IN_P) {
                        dlt[u] = s_segc0[rec[u] >> 16].x;
                        cb[u] = (uint32_t)s_P[el[u]];
                    } else {
                        const uint2 seg = s_segc0[rec[u] >> 16];
                        dlt[u] = seg.x;
                        cb[u] = sx_tri32(me[u].x) - seg.y;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + (uint32_t)u * EM_THREADS;
                    const uint32_t cell = cb[u] + pq[u].x;
                    if (i < total) list[dlt[u] + i] = (cell << pb) | fsk_hw::mul24(me[u].y, pq[u].y - (pl[u] == (int)el[u] ? 1u : 0u));
                }
            }
            // ---- the bare cells of the unit entries: a cell per thread and trip, written as the 16-bit half of its container —
            // the low half a cell, the high half a cell | 0x8000 (bit 31 of the container: PAIRS) — neighbouring lanes write
            // neighbouring halves
            const uint32_t total_b = s_total >> 16;  // cells (the region behind the words' slots)
            for (uint32_t h0 = tid; h0 < total_b; h0 += 4u * EM_THREADS) {  // (four cells per thread and trip, as above)
                uint32_t el[4], rec[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t h = h0 + (uint32_t)u * EM_THREADS;
                    el[u] = slot_ent[total + (h < total_b ? h : h0)];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) rec[u] = ent_rec[el[u]];
                uint32_t cell[4], hb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t h = h0 + (uint32_t)u * EM_THREADS, hh = h < total_b ? h : h0;
                    int pl = (int)(int16_t)(uint16_t)rec[u] + (int)hh;  // tile-local index of the partner
                    if (SKIP) pl = (int)el[u] - (int)s_P[el[u]] + 1 + pl;  // (pl was the partner's number: a unit entry never pairs with itself)
                    const uint2 pq = SKIP ? sx_partner_at<PACKED>(s_ent, E, e0, pl) : sx_partner_lds<PACKED>(s_ent, pl);
                    cell[u] = (CB_IN_P ? (uint32_t)s_P[el[u]] : sx_tri32(X::unpack(s_ent[el[u]]).x) - s_segc0[rec[u] >> 16].y) + pq.x;
                    // where the cell goes, in 16-bit halves from the start of the stream buffer: (the band's share) + (the cell's number
                    // in it) — s_cnt[band] holds 2 * share - (the band's first cell slot) by now
                    hb[u] = s_cnt[rec[u] >> 16] + hh;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (h0 + (uint32_t)u * EM_THREADS < total_b)
                        reinterpret_cast<uint16_t*>(list)[hb[u]] = (uint16_t)(cell[u] | ((hb[u] & 1u) << 15));
            }
            __syncthreads();
            FSK_EM_MARK(2)  // the words of the short entries written
        };
        if (one_pass) {
            bin_pass(std::true_type{}, 0u, n);
        } else {
            __syncthreads();  // (the passes' first entries are in place)
            const uint32_t n_pass = all / EM_CAP + 1u;  // (the last one may be empty)
            for (uint32_t ps = 0; ps < n_pass; ++ps) {
                const uint32_t ea = s_bnd[ps], eb = ps + 1u < n_pass ? s_bnd[ps + 1u] : n;
                if (ea < eb) bin_pass(std::false_type{}, ea, eb);
            }
        }
    }
    __syncthreads();
    // ---- descriptors (class 5): one per entry, by the thread that holds it, into the band's descriptor stream — s_cnt (free
    // now) holds the next free word of this tile's share of every band's descriptor stream. {entry index of the run's first
    // partner, partners before the entry itself, row, multiplicity}: k_sx_consume walks E[first .. first + partners) and adds
    // the entry's own cell when its multiplicity is above 1.
    if (!DIRECT && desc) {  // (uniform)
        if (tid < n_owners) s_cnt[tid] = t_dcur;  // (asked for in the prologue)
        __syncthreads();
#pragma unroll
        for (int q = 0; q < EM_PER; ++q) {
            if (my_cls[q] == 5u) {
                const uint32_t e = (uint32_t)q * EM_THREADS + tid;
                const uint32_t o = sx_owner_of(my_row[q], own_shift, own_base);
                const uint32_t nrec = sx_desc_records(desc, my_row[q], desc_sub_shift);
                const uint32_t at = atomicAdd(&s_cnt[o], SX_DESC_WORDS * nrec);
                const uint32_t R = (uint32_t)s_P[e], T = SKIP ? (uint32_t)s_T[e] : R - 1u;
                const uint32_t mult = sx_mult(X::unpack(s_ent[e]).y);
                uint4* const out = reinterpret_cast<uint4*>(list + at);
                if (desc != 2u) {
                    out[0] = make_uint4(e0 + e - R + 1u, T, my_row[q], mult);
                } else {
                    // two-level blocks: the partners' cells rise with the partner number (a run's entries are in sequence order), so
                    // the partners inside one sub-band are a contiguous piece of the run: where the pieces end by bisection
                    // over the partners' columns (LDS; a run that began far before the tile: global reads), one record a piece
                    const uint32_t cb = sx_tri32(my_row[q]) - s_segc0[o].y;  // cell of column 0 of the row inside the band
                    const int pl0 = (int)e - (int)R + 1;                  // tile-local index of partner 0
                    uint32_t p = 0u, k = 0u;
                    while (p < T) {
                        const uint32_t sb = (cb + sx_partner_at<PACKED>(s_ent, E, e0, pl0 + (int)p).x) >> desc_sub_shift;
                        const uint32_t lim = ((sb + 1u) << desc_sub_shift) - cb;  // first column beyond the sub-band
                        uint32_t lo = p + 1u, hi = T;                              // first partner in [lo, hi] whose column is >= lim
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (sx_partner_at<PACKED>(s_ent, E, e0, pl0 + (int)mid).x >= lim) hi = mid; else lo = mid + 1u;
                        }
                        out[k++] = make_uint4(e0 + e - R + 1u + p, lo - p, cb, mult | (sb << SX_DESC_MULT_BITS));
                        p = lo;
                    }
                    for (; k < nrec; ++k) out[k] = make_uint4(0u, 0u, 0u, 0u);
                    if (mult > 1u) list[atomicAdd(&s_cur[o], 1u)] = ((cb + my_row[q]) << pb) | fsk_hw::mul24(mult, mult - 1u);
                }
            }
        }
        __syncthreads();
    }
    // entries with many partners (or a product that needs several words): listed now that the slot array is free
    // (one array: the long entries from the front, those a HALF wave can take — at most 32 partners, one
    // word each — from the back)
    if (tid == 0) { s_nlong = 0u; s_nhalf = 0u; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EM_PER; ++q) {
        const uint16_t el = (uint16_t)((uint32_t)q * EM_THREADS + tid);
        if (my_cls[q] == 2u) s_long[atomicAdd(&s_nlong, 1u)] = el;
        if (my_cls[q] == 3u) s_long[(uint32_t)SG_TILE - 1u - atomicAdd(&s_nhalf, 1u)] = el;
    }
    __syncthreads();
    // Per long entry, by one THREAD each and all of them up front: where its words go in its owner's
    // stream (one LDS atomic) and the cell its row starts at inside the owner band. In the wave loop below
    // every lane would compute these same two numbers (64-bit multiplies, an LDS atomic to wait for) before
    // every entry: that loop is bound by the instructions it issues, and this was most of them.
    uint2* const long_hdr = reinterpret_cast<uint2*>(slot_ent + SG_TILE);  // (behind the list: SG_TILE u16, then SG_TILE x 8 bytes)
    static_assert(SG_TILE * 2 + SG_TILE * 8 <= ((EM_SLOTS + 1u) / 2u + SG_TILE) * 4, "the long entries' list and headers share the slot array and the records");
    FSK_EM_MARK(3)  // long entries listed
    if (!DIRECT) {
        const uint32_t n_front = s_nlong, n_back = s_nhalf;
        for (uint32_t i = tid; i < n_front + n_back; i += EM_THREADS) {
            const uint32_t q = i < n_front ? i : (uint32_t)SG_TILE - 1u - (i - n_front);
            const uint32_t e = s_long[q];
            const uint2 a = SX_ENT(e);
            const uint32_t o = sx_owner_of(a.x, own_shift, own_base);
            // (a wide entry — sx_wide_entry — takes one word)
            const uint32_t at = atomicAdd(&s_cur[o], sx_wide_entry(a.y, cwide) ? 1u : SX_NPART(e) * sx_words_per_pair(a.y, cmax, max_win, maxprod));
            long_hdr[q] = make_uint2(at, sx_tri32(a.x) - s_segc0[o].y);
        }
        __syncthreads();
        // ---- two entries per wave and trip: lanes 0-31 one, lanes 32-63 the other (the loops over long
        // entries are bound by the instructions they issue, and an entry of 17..32 partners fills half a wave)
        for (uint32_t i = 2u * wave + (lane >> 5); i < n_back; i += 2u * EM_WAVES) {
            const uint32_t q = (uint32_t)SG_TILE - 1u - i;
            const uint32_t e = s_long[q];
            const uint2 a = SX_ENT(e), hdr = long_hdr[q];
            const uint32_t R = s_P[e], P = R - (a.y > 1u ? 0u : 1u), l = lane & 31u;  // rank in the run; words
            if (l < P) {
                const int pl = (int)e - (int)R + 1 + (int)l;  // tile-local index of the partner (>= -32: in LDS)
                const uint2 pq = sx_partner_lds<PACKED>(s_ent, pl);
                list[hdr.x + l] = ((hdr.y + pq.x) << pb) | fsk_hw::mul24(a.y, pq.y - (pl == (int)e ? 1u : 0u));
            }
        }
    }
    // ---- long entries: the lanes of a wave take the partners, the words of an entry are contiguous
    // (an entry's header — which entry, its row and multiplicity, its partner count, its place in the
    // stream — is fetched one entry ahead: three dependent LDS reads that would otherwise precede every entry)
    FSK_EM_MARK(4)  // long entries' headers, half-wave entries
    const uint32_t nlong = s_nlong;
    uint32_t n_e = 0, n_P = 0;
    uint2 n_a = make_uint2(0u, 0u), n_hdr = make_uint2(0u, 0u);
#define SX_FETCH_LONG(q)                      \
    {                                         \
        n_e = s_long[q];                      \
        n_a = SX_ENT(n_e);                    \
        n_P = SX_NPART(n_e);                  \
        if (!DIRECT) n_hdr = long_hdr[q];     \
    }
    // Two loops over the list. The first takes the entries whose whole run lies in LDS (the tile and the EM_PRE entries in front
    // of it) and one word a pair — nearly all of them — and has NO global read in its body: a loop with one anywhere ends every
    // trip in a wait for the memory counter (the compiler guards the load's destination registers at the back edge), which on
    // gfx950 is a wait for the trip's own stores. The second loop takes what is left, as before.
    if (!DIRECT && !SKIP) {
        // TWO entries a trip (q and q + EM_WAVES of the list): their headers, their partners and their words go side by side, so the
        // chains of dependent LDS reads of one entry (list -> entry -> rank -> header -> partner) overlap with the other's — in
        // the paper's large-g regime (runs of ~100 entries) this loop is two thirds of the kernel and a trip was ~2,800 cycles
        // for ~60 instructions (profiles/r06_emit_phases_large_g.txt).
        struct LongEnt { uint32_t e, P; uint2 a, hdr; bool ok; };
        auto fetch = [&](uint32_t q, LongEnt& L) {
            const uint32_t qq = q < nlong ? q : wave;  // (clamped: wave < nlong here)
            L.e = s_long[qq];
            L.a = SX_ENT(L.e);
            L.P = SX_NPART(L.e);
            L.hdr = long_hdr[qq];
            L.ok = q < nlong;
        };
        // one entry whose run lies in LDS, any partner count
        auto one = [&](const LongEnt& L, int pl0) {
            uint32_t* dst = list + L.hdr.x;
            const uint32_t cbase = L.hdr.y, P = L.P;
            for (uint32_t b0 = lane; b0 < P; b0 += 256u) {  // (four trips at a time)
                uint2 pq[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t b = b0 + (uint32_t)u * 64u;
                    pq[u] = sx_partner_lds<PACKED>(s_ent, pl0 + (int)(b < P ? b : b0));
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t b = b0 + (uint32_t)u * 64u;
                    if (b < P) dst[b] = ((cbase + pq[u].x) << pb) | fsk_hw::mul24(L.a.y, pq[u].y - (pl0 + (int)b == (int)L.e ? 1u : 0u));
                }
            }
        };
        for (uint32_t q = wave; q < nlong; q += 2u * EM_WAVES) {
            LongEnt A, B;
            fetch(q, A);
            fetch(q + EM_WAVES, B);
            // the entry's rank in its run (P counts its words: itself only with multiplicity > 1) -> tile-local index of partner 0
            const int plA = (int)A.e - (int)(A.P + (A.a.y > 1u ? 0u : 1u)) + 1, plB = (int)B.e - (int)(B.P + (B.a.y > 1u ? 0u : 1u)) + 1;
            // (wave-uniform) this loop's: the whole run in LDS, one word a pair; else the second loop's
            const bool okA = A.ok && plA >= -EM_PRE && sx_words_per_pair(A.a.y, cmax, max_win, maxprod) == 1u;
            const bool okB = B.ok && plB >= -EM_PRE && sx_words_per_pair(B.a.y, cmax, max_win, maxprod) == 1u;
            if (okA && okB && A.P <= 64u && B.P <= 64u) {  // (most trips: straight-line, both entries' reads before both stores)
                const int pa = plA + (int)(lane < A.P ? lane : 0u), pb2 = plB + (int)(lane < B.P ? lane : 0u);
                const uint2 qa = sx_partner_lds<PACKED>(s_ent, pa), qb = sx_partner_lds<PACKED>(s_ent, pb2);
                const uint32_t wa = ((A.hdr.y + qa.x) << pb) | fsk_hw::mul24(A.a.y, qa.y - (pa == (int)A.e ? 1u : 0u));
                const uint32_t wb = ((B.hdr.y + qb.x) << pb) | fsk_hw::mul24(B.a.y, qb.y - (pb2 == (int)B.e ? 1u : 0u));
                if (lane < A.P) list[A.hdr.x + lane] = wa;
                if (lane < B.P) list[B.hdr.x + lane] = wb;
                continue;
            }
            if (okA) one(A, plA);
            if (okB) one(B, plB);
        }
    }
    if (wave < nlong) SX_FETCH_LONG(wave)
    for (uint32_t q = wave; q < nlong; q += EM_WAVES) {
        const uint32_t e = n_e, P = n_P;
        const uint2 a = n_a, hdr = n_hdr;
        if (q + EM_WAVES < nlong) SX_FETCH_LONG(q + EM_WAVES)
        if (DIRECT) {
            u64* row = K + tri_index((u64)a.x, 0);
            for (uint32_t b = lane; b < P; b += 64) {
                const uint2 pq = SX_PARTNER_OF(e, b);
                atomicAdd(&row[pq.x], (u64)a.y * (pq.y - (SX_IS_SELF(e, b) ? 1u : 0u)));
            }
        } else if (sx_wide_entry(a.y, cwide)) {
            // (sx_wide_entry: the products as 64-bit atomics — the u32 cells of the consume kernels could not hold their sum —
            // and the one word of product 0 that k_sx_seg_write counted for the entry)
            if (lane == 0u) list[hdr.x] = hdr.y << pb;
            u64* row = K + tri_index((u64)a.x, 0);
            for (uint32_t b = lane; b < P; b += 64) {
                const uint2 pq = SX_PARTNER_OF(e, b);
                atomicAdd(&row[pq.x], (u64)a.y * (pq.y - (SX_IS_SELF(e, b) ? 1u : 0u)));
            }
        } else {
            const uint32_t S = sx_words_per_pair(a.y, cmax, max_win, maxprod);
            const uint32_t at = hdr.x, cbase = hdr.y;
            if (S == 1u && !SKIP) {
                // the common case, kept lean (long runs make this loop most of the kernel): partner b is
                // entry first + b — in LDS from `split` on, in global memory before — one word each
                uint32_t* dst = list + at;
                const uint32_t R = P + (a.y > 1u ? 0u : 1u);  // the entry's rank in its run (P counts its words: itself only with multiplicity > 1)
                if ((int)e - (int)R + 1 >= -EM_PRE) continue;  // (taken by the first loop)
                if (P <= 64u) {
                    if (lane < P) {
                        const int pl = (int)e - (int)R + 1 + (int)lane;  // tile-local index of the partner
                        const uint2 pq = sx_partner_at<PACKED>(s_ent, E, e0, pl);
                        dst[lane] = ((cbase + pq.x) << pb) | fsk_hw::mul24(a.y, pq.y - (pl == (int)e ? 1u : 0u));
                    }
                    continue;
                }
                const uint32_t first = e0 + e - R + 1u;                 // global index of partner 0
                const uint32_t split = first < e0 ? e0 - first : 0u;    // partners before the tile
                // (four trips at a time, loads first: partners before the tile are global reads)
                for (uint32_t b0 = lane; b0 < P; b0 += 256u) {
                    uint2 pq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t b = b0 + (uint32_t)u * 64u;
                        pq[u] = make_uint2(0u, 0u);
                        if (b < P) pq[u] = sx_partner_at<PACKED>(s_ent, E, e0, (int)(first + b) - (int)e0);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t b = b0 + (uint32_t)u * 64u;
                        if (b < P) dst[b] = ((cbase + pq[u].x) << pb) | fsk_hw::mul24(a.y, pq[u].y - (first + b == e0 + e ? 1u : 0u));
                    }
                }
                continue;
            }
            const uint32_t trips = (P + 63u) / 64u;
            for (uint32_t tr = 0; tr < trips; ++tr) {
                const uint32_t b = tr * 64u + lane;
                if (b < P) {
                    const uint2 pq = SX_PARTNER_OF(e, b);
                    u64 prod = (u64)a.y * (pq.y - (SX_IS_SELF(e, b) ? 1u : 0u));
                    for (uint32_t w = 0; w < S; ++w) {
                        const uint32_t part = prod < maxprod ? (uint32_t)prod : maxprod;
                        list[at + b * S + w] = ((cbase + pq.x) << pb) | part;
                        prod -= part;
                    }
                }
            }
        }
    }
    FSK_EM_MARK(5)  // long entries (a wave each)
    FSK_EM_MARK_END
#undef SX_FETCH_LONG
#undef SX_IN_BAND
#undef SX_IS_SHORT
#undef SX_IS_SELF
#undef SX_PARTNER_OF
#undef SX_NPART
#undef SX_PARTNER
#undef SX_ENT
}

// ---- descriptors, expanded into a workgroup's LDS cells (k_sx_consume, k_sxb_consume) ---------------------------------------
// A descriptor {first, T, z, mult} stands for the T update words of ONE entry: partner p is entry first + p = (column,
// multiplicity) and cell(row, column) += mult * multiplicity. ROWS (owner bands): z = the entry's row — its cells are
// counted from tri(row) - base — and its own cell (row, row) += mult * (mult - 1) when mult > 1; else (two-level blocks):
// z = the cell of column 0 of the row counted from the band's first cell, base = the block's first cell (the entry's own
// cell travels as an ordinary word); mult = the low 20 bits of the last word.
// A quarter wave (16 lanes) per descriptor — four descriptors a wave and trip. A lane reads FOUR partners (packed entries;
// two in the 8-byte format) with one aligned 16-byte load: the quarter wave's 16 loads are 256 contiguous bytes from the
// 16-byte boundary below the run's first partner (what lies in front of it, or behind the last one, is masked). One load
// instruction and whole 64-byte sectors per 64 partners, where a 4-byte load per partner was four instructions and pieces
// that straddle sectors: the partner reads miss the L2 (every entry of a run reads the same partners, but from another
// workgroup, at another time), and what bounds this loop is the REQUESTS a CU keeps in flight — large-g regime, k_sx_consume
// per batch: 7.1 -> 3.6 ms. A pipeline three descriptors deep per quarter wave: the descriptor of trip i + 2 is being fetched
// and the first piece of trip i + 1's partners is in flight while trip i's products go into the cells. (Measured and dropped:
// a pipeline over 64-partner CHUNKS instead — an entry's later chunks prefetched like the first —: 1.33 -> 1.39 s; an XCD
// taking a contiguous range of the parts instead of every eighth one: 1.33 -> 1.55 s.)
// D4[v * dstride], v < nd: the workgroup's descriptors. Every thread of the workgroup must call it.
// GROUP: the lanes that share a descriptor — 16 for the owner bands (an entry's partners: dozens to hundreds), 8 for the pieces of
// the two-level form (an entry's partners inside ONE sub-band: a dozen).
// FMT: what a partner is read from — 0 / 1: the entries themselves (packed 4 bytes / general 8 bytes); 2 / 3: the COLUMN ARRAY
// k_sx_seg_write leaves beside the entries when descriptors are on (`cols`: the sequence id alone, 2 bytes a partner when
// N < 32768, else 4, the multiplicity in the bits the sequence ids leave free — 0 where it does not fit: only then is the entry
// itself read, a dependent load inside the loop —): half the bytes and half the requests of the entries.
template <uint32_t THREADS, int FMT, bool ROWS, uint32_t GROUP = 16u>
__device__ __forceinline__ void sx_expand_descriptors(const uint4* D4, uint32_t nd, uint32_t dstride, uint32_t* cells, uint32_t span, uint32_t base,
                                                      const void* E, const void* cols, int packed, int colbits) {
    constexpr uint32_t PERW = 64u / GROUP;            // descriptors a wave and trip
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, sub = lane / GROUP, l16 = lane % GROUP;
    constexpr uint32_t STEP = (THREADS / 64u) * PERW;
    constexpr uint32_t PER = FMT == 0 ? 4u : FMT == 1 ? 2u : FMT == 2 ? 8u : 4u;  // partners a 16-byte load
    constexpr uint32_t CHUNK = GROUP * PER;           // partners a group of lanes and load instruction
    const uint4* const S4 = reinterpret_cast<const uint4*>(FMT >= 2 ? cols : E);
    auto desc_at = [&](uint32_t v) { return v < nd ? D4[(size_t)v * dstride] : make_uint4(0u, 0u, 0u, 0u); };  // (beyond the last: T = 0, mult = 0)
    auto fetchq = [&](uint32_t first, uint32_t T, uint32_t chunk) {
        const uint32_t piece = (first & ~(PER - 1u)) + chunk * CHUNK + l16 * PER;  // (entry index of the lane's first element)
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        if (piece < first + T) r = S4[piece / PER];
        return r;
    };
    auto addq = [&](uint32_t cb, uint32_t first, uint32_t T, uint32_t mult, uint32_t chunk, const uint4& r) {
        const uint32_t e0 = (first & ~(PER - 1u)) + chunk * CHUNK + l16 * PER;  // (entry index of element 0)
        const uint32_t p0 = e0 - first;                                        // (its partner number: may be "negative")
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < (int)PER; ++j) {
            uint32_t col, pm;
            bool fetch_mult = false;
            if (FMT == 0) { col = w[j] & 0xffffu; pm = w[j] >> 16; }
            else if (FMT == 1) { col = w[2 * j]; pm = w[2 * j + 1]; }
            else {  // (column | multiplicity << colbits; a multiplicity field of 0: it did not fit, read the entry)
                const uint32_t h = FMT == 2 ? (w[j >> 1] >> (16 * (j & 1))) & 0xffffu : w[j];
                col = h & ((1u << colbits) - 1u);
                pm = h >> colbits;
                fetch_mult = pm == 0u;
            }
            const bool valid = p0 + (uint32_t)j < T;
            if (FMT >= 2 && valid && fetch_mult)  // (rare: a partner of multiplicity above 1)
                pm = packed ? reinterpret_cast<const uint32_t*>(E)[(size_t)e0 + j] >> 16 : reinterpret_cast<const uint2*>(E)[(size_t)e0 + j].y;
            const uint32_t x = cb + col;
            if (valid && x < span) atomicAdd(&cells[x], mult * sx_mult(pm));
        }
    };
    uint32_t d = wave * PERW + sub;
    uint4 D = desc_at(d), nxt = desc_at(d + STEP);  // trips i, i + 1
    uint4 pq = fetchq(D.x, D.y, 0u);
    for (uint32_t d0 = wave * PERW; d0 < nd; d0 += STEP, d += STEP) {  // (wave-uniform trip count)
        const uint4 nn = desc_at(d + 2u * STEP);  // trip i + 2
        const uint4 pqn = fetchq(nxt.x, nxt.y, 0u);
        const uint32_t first = D.x, T = D.y, mult = D.w & ((1u << SX_DESC_MULT_BITS) - 1u);
        const uint32_t cb = (ROWS ? sx_tri32(D.z) : D.z) - base;
        addq(cb, first, T, mult, 0u, pq);
        const uint32_t span_e = (first & (PER - 1u)) + T;  // entries from the aligned start to the last partner
        for (uint32_t c = 1u; __ballot(c * CHUNK < span_e) != 0; ++c) {  // (entries of more partners than one piece)
            const uint4 more = fetchq(first, T, c);
            addq(cb, first, T, mult, c, more);
        }
        if (ROWS && l16 == 0u && mult > 1u) {  // (the entry's own cell)
            const uint32_t x = cb + D.z;
            if (x < span) atomicAdd(&cells[x], mult * (mult - 1u));
        }
        D = nxt; nxt = nn; pq = pqn;
    }
}
// (fmt: wave-uniform, one of the four instantiations)
template <uint32_t THREADS, bool ROWS, uint32_t GROUP>
__device__ __forceinline__ void sx_expand_descriptors_fmt(int fmt, const uint4* D4, uint32_t nd, uint32_t dstride, uint32_t* cells, uint32_t span,
                                                          uint32_t base, const void* E, const void* cols, int packed, int colbits) {
    if (fmt == 2) sx_expand_descriptors<THREADS, 2, ROWS, GROUP>(D4, nd, dstride, cells, span, base, E, cols, packed, colbits);
    else if (fmt == 3) sx_expand_descriptors<THREADS, 3, ROWS, GROUP>(D4, nd, dstride, cells, span, base, E, cols, packed, colbits);
    else if (fmt == 0) sx_expand_descriptors<THREADS, 0, ROWS, GROUP>(D4, nd, dstride, cells, span, base, E, cols, packed, colbits);
    else sx_expand_descriptors<THREADS, 1, ROWS, GROUP>(D4, nd, dstride, cells, span, base, E, cols, packed, colbits);
}

// Streams differ a lot in length (a band that holds a long or low-complexity sequence receives many
// times the average), so a stream is cut into parts of about `target` words, one workgroup each:
// part_base[o] = parts of the bands before o (single workgroup of 512 threads, n_owners <= 512).
// With descriptors (desc): a band's work is its words plus SX_DESC_WEIGHT words' worth per descriptor word, the target is
// set HERE (the host knows the batch's word total, not how it splits): about desc_parts parts in all, none below the
// host's `target`; part_base[n_owners + 1] = the target in force. A band's parts then cut its words and its descriptors
// into equal pieces each (k_sx_consume).
constexpr uint32_t SX_DESC_WEIGHT = 16;
// part_owner (may be null; 16-byte aligned, max_parts records of 16 bytes): what k_sx_consume's workgroup `part` starts from, ONE
// load (a table of the bands' bases in its LDS and a binary search took 2 KB off its cells: with all of a workgroup's 80 KiB a
// band of 2^14 cells + a row of up to 4096 is ONE round, e.g. N = 4000).
__global__ __launch_bounds__(512) void k_sx_parts(const uint32_t* list_off, uint32_t n_owners, uint32_t target, uint32_t* part_base,
                                                  const u64* batch_stat, u64 cap_words, uint32_t desc, uint32_t* part_owner, uint32_t max_parts,
                                                  uint32_t desc_parts) {
    __shared__ uint32_t tmp[8];
    __shared__ u64 s_work;
    const uint32_t tid = threadIdx.x;
    const bool fits = batch_stat[1] <= cap_words;  // (else: no parts, k_sx_consume has nothing to do)
    const uint32_t wcol = desc ? n_owners : 0u;
    const uint32_t len = (fits && tid < n_owners) ? list_off[wcol + tid + 1] - list_off[wcol + tid] : 0u;
    u64 work = len;
    if (desc) {
        if (fits && tid < n_owners) work += (u64)SX_DESC_WEIGHT * (list_off[tid + 1] - list_off[tid]);
        if (tid == 0) s_work = 0;
        __syncthreads();
        const u64 ws = fsk_hw::wave_sum_u64(work);
        if ((tid & 63u) == 0u && ws) atomicAdd(&s_work, ws);
        __syncthreads();
        const u64 t2 = (s_work + desc_parts - 1u) / desc_parts;
        if (t2 > (u64)target) target = t2 > 0xffffffffull ? 0xffffffffu : (uint32_t)t2;
    }
    const uint32_t parts = (uint32_t)((work + target - 1u) / target);
    uint32_t tot;
    const uint32_t ex = block_excl_scan<uint32_t, 8>(parts, tmp, &tot);
    if (tid < n_owners) part_base[tid] = ex;
    if (tid == 0) { part_base[n_owners] = tot < max_parts ? tot : max_parts; part_base[n_owners + 1] = target; }
    if (part_owner) {  // one record a part — {band, part of the band, parts of the band, target} —, band 0xffffffff beyond the last
        uint4* const rec = reinterpret_cast<uint4*>(part_owner);
        if (tid < n_owners)
            for (uint32_t j = 0; j < parts && ex + j < max_parts; ++j) rec[ex + j] = make_uint4(tid, j, parts, target);
        for (uint32_t i = tot + tid; i < max_parts; i += 512u) rec[i] = make_uint4(0xffffffffu, 0u, 0u, 0u);
    }
}

// One workgroup of 1024 threads per (part of an owner band's stream, round): sums its words into `cap`
// u32 cells in LDS and adds the non-zero ones into K — a plain read-modify-write when the band has a
// single part (a cell then has one writer and launches are ordered on the stream), 64-bit atomics
// otherwise. A band larger than `cap` cells takes several rounds over its stream.
// dynamic LDS: cap * 4 bytes. grid = (upper bound of the number of parts, rounds)
constexpr uint32_t CS_THREADS = 1024;
// By-slot form (variance mode, slot_stride != 0): grid = (owner bands, rounds, slots); the words a slot
// put into a band's stream are contiguous (tiles are slot-major), bounded by the tile offsets of the
// slot's first tile, and the sums are STORED as u32 into the slot's own triangle (uint32_t*)K + slot *
// slot_stride — every cell of it, so it needs no zero fill.
// (BYSLOT is a template parameter for the LDS: without the parts table the by-slot form can hold 80 KiB of cells — a
// whole band of up to 20480 cells in ONE round, where 64 KiB made two rounds of config 1's bands, each reading the
// band's stream — and still share a CU with a second workgroup)
// (SLOT16, by-slot form only: the slot triangles are u16 arrays — half the bytes written here and read by the Welford pass —;
// a sum above 65535 raises *ovf in pinned host memory and the host runs the batch again with u32 triangles)
template <bool BYSLOT, bool SLOT16 = false>
__global__ __launch_bounds__(1024) void k_sx_consume(const uint32_t* list, const uint32_t* list_off, const uint32_t* owner_r0,
                                                     const uint32_t* part_base, uint32_t n_owners, uint32_t target, uint32_t cap,
                                                     int pb, u64* K, const uint32_t* tile_off, uint32_t tpg, u64 slot_stride,
                                                     const u64* batch_stat, u64 cap_words, uint32_t* ovf = nullptr, int pairs = 0,
                                                     uint32_t desc = 0, const void* E = nullptr, int packed = 0, const void* cols = nullptr,
                                                     int col16 = 0) {
    // desc: list_off / tile_off have 2 * n_owners columns — band o's descriptors at column o, its words at n_owners + o;
    // E: the batch's entries (packed: 4 bytes each, else 8), which the descriptors index; cols (may be null): their column array
    // (col16 = bits of a sequence id << 1 | 1 when a partner takes 2 bytes, else 4) — see sx_expand_descriptors
    if (batch_stat[1] > cap_words) return;  // (see k_sx_emit)
    FSK_DYN_SHARED(uint32_t, cells);
    const uint32_t tid = threadIdx.x;
    const uint32_t r = blockIdx.y;
    uint32_t o, a, b, nparts = 1u;
    // the band's descriptors list[da .. db), SX_DESC_WORDS words each; this workgroup expands number dpart, dpart + dstride, ...
    uint32_t da = 0u, db = 0u, dpart = 0u, dstride = 1u;
    const uint32_t n_cols = desc ? 2u * n_owners : n_owners, wcol = desc ? n_owners : 0u;
    uint32_t* K32 = nullptr;  // by-slot form: the slot's triangle is a u32 array that this launch WRITES (no zero fill needed)
    if (BYSLOT) {
        o = blockIdx.x;
        const uint32_t slot = blockIdx.z;
        a = list_off[wcol + o] + tile_off[(size_t)slot * tpg * n_cols + wcol + o];
        b = slot + 1u < gridDim.z ? list_off[wcol + o] + tile_off[(size_t)(slot + 1u) * tpg * n_cols + wcol + o] : list_off[wcol + o + 1];
        if (desc) {
            da = list_off[o] + tile_off[(size_t)slot * tpg * n_cols + o];
            db = slot + 1u < gridDim.z ? list_off[o] + tile_off[(size_t)(slot + 1u) * tpg * n_cols + o] : list_off[o + 1];
        }
        K32 = reinterpret_cast<uint32_t*>(K) + (u64)slot * slot_stride;
    } else {
        // (k_sx_parts: one record a part behind the bands' bases — {band, part of the band, its parts, the target in force})
        const uint4 pr = reinterpret_cast<const uint4*>(part_base + ((n_owners + 2u + 3u) & ~3u))[blockIdx.x];
        if (pr.x == 0xffffffffu) return;  // (the grid is an upper bound of the parts)
        o = pr.x;
        const uint32_t part = pr.y;
        nparts = pr.z;
        target = pr.w;
        if (!desc) {
            a = list_off[o] + part * target;
            const uint32_t end = list_off[o + 1];
            b = end - a < target ? end : a + target;
        } else {
            // (k_sx_parts set the parts by words + descriptors: the band's words in nparts pieces of whole 16 bytes, its
            // descriptors in nparts pieces)
            const uint32_t w0 = list_off[wcol + o], w1 = list_off[wcol + o + 1];
            const uint32_t piece = (((w1 - w0) + nparts - 1u) / nparts + 3u) & ~3u;
            const u64 pa = (u64)part * piece;
            a = pa < (u64)(w1 - w0) ? w0 + (uint32_t)pa : w1;
            b = w1 - a < piece ? w1 : a + piece;
            // (descriptors: part p takes every nparts-th one from the p-th on — every part of every band then sweeps the
            // batch's entries from the first tile to the last, and parts of about equal work do so at about the same pace:
            // the partner reads of the workgroups that share an L2 fall into the same region of E at the same time)
            da = list_off[o];
            db = list_off[o + 1];
            dpart = part;
            dstride = nparts;
        }
    }
    if (a == b && da == db && !K32) return;
    const u64 c0 = tri_index((u64)owner_r0[o], 0), c1 = tri_index((u64)owner_r0[o + 1], 0);
    const uint32_t ncell = (uint32_t)(c1 - c0);
    const uint32_t lo = r * cap;
    if (lo >= ncell) return;
    const uint32_t span = ncell - lo < cap ? ncell - lo : cap;
    for (uint32_t i = tid; i < span; i += CS_THREADS) cells[i] = 0u;
    __syncthreads();
    const uint32_t mask = (1u << pb) - 1u;
    // one 32-bit container of the stream: {cell << pb | product}, or — PAIRS, bit 31 set — two bare cells of product 1
    // (0x7fff: none; a band then has fewer than 32767 cells, so that value never passes the range test)
    auto take = [&](uint32_t w) {
        const bool two = pairs && (w >> 31) != 0u;
        const uint32_t x = (two ? (w & 0x7fffu) : (w >> pb)) - lo;
        if (x < span) atomicAdd(&cells[x], two ? 1u : (w & mask));
        if (two) {
            const uint32_t y = ((w >> 16) & 0x7fffu) - lo;
            if (y < span) atomicAdd(&cells[y], 1u);
        }
    };
    // The stream [a, b) in 16-byte pieces (the order of the words does not matter): the up to three words before the first
    // 16-byte boundary and after the last one go one per thread, the pieces four per thread in flight.
    {
        const uint32_t a4 = (a + 3u) & ~3u, b4 = b & ~3u;
        if (a4 < b4) {
            if (tid < a4 - a) take(list[a + tid]);
            else if (tid - (a4 - a) < b - b4) take(list[b4 + (tid - (a4 - a))]);
            const uint4* l4 = reinterpret_cast<const uint4*>(list + a4);
            const uint32_t n4 = (b4 - a4) >> 2;
            uint32_t i = tid;
            for (; i + 3u * CS_THREADS < n4; i += 4u * CS_THREADS) {  // sixteen words in flight per thread (long streams come from HBM)
                uint4 w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = l4[i + (uint32_t)u * CS_THREADS];
#pragma unroll
                for (int u = 0; u < 4; ++u) { take(w[u].x); take(w[u].y); take(w[u].z); take(w[u].w); }
            }
            for (; i < n4; i += CS_THREADS) {
                const uint4 w = l4[i];
                take(w.x); take(w.y); take(w.z); take(w.w);
            }
        } else {  // (a stream of a few words)
            for (uint32_t i = a + tid; i < b; i += CS_THREADS) take(list[i]);
        }
    }
    // ---- descriptors (sx_expand_descriptors)
    if (desc && da != db) {  // (uniform)
        const uint32_t nd_all = (db - da) / SX_DESC_WORDS;
        const uint32_t nd = dpart < nd_all ? (nd_all - dpart + dstride - 1u) / dstride : 0u;  // (this workgroup's: every dstride-th from the dpart-th on)
        // (the band's first cell + the round's, mod 2^32: a cell inside the band's round is a small difference)
#ifndef FSK_DESC_GROUP
#define FSK_DESC_GROUP 16u  // (tools/build_variant.sh builds the A/B variant)
#endif
        sx_expand_descriptors_fmt<CS_THREADS, true, FSK_DESC_GROUP>(cols ? ((col16 & 1) ? 2 : 3) : (packed ? 0 : 1), reinterpret_cast<const uint4*>(list + da) + dpart, nd, dstride,
                                                                    cells, span, sx_tri32(owner_r0[o]) + lo, E, cols, packed, col16 >> 1);
    }
    __syncthreads();
    if (BYSLOT && SLOT16) {
        // the band's cells out as u16, 16 bytes (eight cells) per store where the triangle is aligned
        uint16_t* o16 = reinterpret_cast<uint16_t*>(K) + (u64)blockIdx.z * slot_stride + c0 + lo;
        const uint32_t head = (uint32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(o16) & 15u)) & 15u) >> 1);  // (cells before the first 16-byte boundary)
        const uint32_t h = head < span ? head : span, n8 = (span - h) >> 3, t0 = h + 8u * n8;
        uint32_t big = 0u;
        if (tid < h) { const uint32_t v = cells[tid]; big |= v; o16[tid] = (uint16_t)v; }
        else if (tid - h < span - t0) { const uint32_t v = cells[t0 + (tid - h)]; big |= v; o16[t0 + (tid - h)] = (uint16_t)v; }
        uint4* o4 = reinterpret_cast<uint4*>(o16 + h);
        for (uint32_t q = tid; q < n8; q += CS_THREADS) {
            const uint32_t c = h + 8u * q;
            const uint32_t v0 = cells[c], v1 = cells[c + 1u], v2 = cells[c + 2u], v3 = cells[c + 3u];
            const uint32_t v4 = cells[c + 4u], v5 = cells[c + 5u], v6 = cells[c + 6u], v7 = cells[c + 7u];
            big |= v0 | v1 | v2 | v3 | v4 | v5 | v6 | v7;
            o4[q] = make_uint4(v0 | (v1 << 16), v2 | (v3 << 16), v4 | (v5 << 16), v6 | (v7 << 16));
        }
        if (big > 0xffffu && ovf) *ovf = 1u;  // (a sum did not fit: the host redoes the batch with u32 triangles)
        return;
    }
    if (K32) {
        // the band's cells out, 16 bytes per store where the triangle is aligned (the band starts wherever its first row does)
        uint32_t* o32 = K32 + c0 + lo;
        const uint32_t head = (uint32_t)((4u - (uint32_t)((c0 + lo) & 3u)) & 3u);
        const uint32_t h = head < span ? head : span, n4 = (span - h) >> 2, t0 = h + 4u * n4;
        if (tid < h) o32[tid] = cells[tid];
        else if (tid - h < span - t0) o32[t0 + (tid - h)] = cells[t0 + (tid - h)];
        uint4* o4 = reinterpret_cast<uint4*>(o32 + h);
        for (uint32_t q = tid; q < n4; q += CS_THREADS) {
            const uint32_t c = h + 4u * q;
            o4[q] = make_uint4(cells[c], cells[c + 1u], cells[c + 2u], cells[c + 3u]);
        }
        return;
    }
    u64* dst = K + c0 + lo;
    if (nparts == 1u) {
        for (uint32_t c = tid; c < span; c += CS_THREADS) {
            const uint32_t v = cells[c];
            if (v) dst[c] += (u64)v;
        }
    } else {
        for (uint32_t c = tid; c < span; c += CS_THREADS) {
            const uint32_t v = cells[c];
            if (v) atomicAdd(&dst[c], (u64)v);
        }
    }
}

// The diagonal. K[i][i] grows per combo by sum_v c_i(v)^2 = (windows of i) + sum_v c_i(v) (c_i(v) - 1): the first
// term does not depend on the combo, so this kernel adds it for the `nb` combos of a batch at once, and the
// update streams carry the second only — an entry of multiplicity 1 (nearly all of them) sends no word for
// its own cell, a quarter of all words on protein data. grid = (rows / 256, slots or 1). By-slot form: after
// k_sx_consume has stored the slot's u32 triangle.
__global__ __launch_bounds__(256) void k_sx_diag_windows(const uint32_t* fstart, uint32_t row0, uint32_t row1, uint32_t nb, u64* K,
                                                         u64 slot_stride, const u64* batch_stat, u64 cap_words, int slot16 = 0,
                                                         uint32_t* ovf = nullptr) {
    if (batch_stat && batch_stat[1] > cap_words) return;  // (see k_sx_emit)
    const uint32_t i = row0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= row1) return;
    const uint32_t w = fstart[i + 1] - fstart[i];
    const u64 cell = tri_index((u64)i, (u64)i);
    if (slot_stride != 0 && slot16) {  // (u16 slot triangles: see k_sx_consume)
        uint16_t* d = reinterpret_cast<uint16_t*>(K) + (u64)blockIdx.y * slot_stride + cell;
        const uint32_t v = (uint32_t)*d + w;
        if (v > 0xffffu && ovf) *ovf = 1u;
        *d = (uint16_t)v;
    } else if (slot_stride != 0) (reinterpret_cast<uint32_t*>(K) + (u64)blockIdx.y * slot_stride)[cell] += w;
    else if (w) K[cell] += (u64)nb * w;
}
