// fsk_load_plan.cpp — the plan of fsk_load_sequences (fsk_load_plan.h): host code only, no device, no engine.
// Replaces the reference's length checks and dictionary (fastsk.cpp:32-85) with a census of the windows that count,
// a rank remap of the tokens that occur and the packed words the kernels read.
#include "fsk_load_plan.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../../include/fastsk_amd.h"

namespace fsk_load {
namespace {

// contiguous shares of the tokens on a few host threads
int host_threads_for(int64_t work_items) {
    if (work_items < ((int64_t)1 << 18)) return 1;
    const unsigned hw = std::thread::hardware_concurrency();
    // (a thread start costs ~50 us; the 3 * 10^7 tokens of the 100,000 x 300 workload are worth 32 of them)
    const unsigned want = work_items < ((int64_t)1 << 20) ? 4u : work_items < ((int64_t)1 << 23) ? 8u : work_items < ((int64_t)1 << 24) ? 16u : 32u;
    return (int)std::max(1u, std::min(want, hw ? hw : 1u));
}

// two phases over the same thread team with `between` run by one thread in the middle (one thread start
// per call instead of two; a spinning barrier: the team is a handful of threads for a fraction of a millisecond)
template <typename F1, typename FM, typename F2>
void parallel_two_phase(int nt, F1&& phase1, FM&& between, F2&& phase2) {
    if (nt <= 1) { phase1(0); between(); phase2(0); return; }
    std::atomic<int> arrived{0}, go{0};
    auto body = [&](int t) {
        phase1(t);
        if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == nt) {
            between();
            go.store(1, std::memory_order_release);
        } else {
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
        }
        phase2(t);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(body, t);
    body(0);
    for (auto& x : th) x.join();
}

// one sequence's tokens, rank-remapped through `lut`, BITS per symbol into its own words
template <int BITS>
inline void pack_sequence(const int32_t* sq, uint32_t len, const uint8_t* lut, uint32_t* w) {
    constexpr uint32_t PER = 32u / (uint32_t)BITS;
    uint32_t p = 0;
    for (; p + PER <= len; p += PER) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) word |= (uint32_t)lut[sq[p + q]] << (q * (uint32_t)BITS);
        *w++ = word;
    }
    if (p < len) {
        uint32_t word = 0;
        for (uint32_t q = 0; p + q < len; ++q) word |= (uint32_t)lut[sq[p + q]] << (q * (uint32_t)BITS);
        *w = word;
    }
}

constexpr int64_t FEAT_LIMIT = (int64_t)1 << 31;  // features are sort records and 32-bit offsets

struct Planner {
    const LoadInput& in;
    LoadPlan& P;
    const int g;
    const int64_t N, off0;
    const int32_t* const tokens;  // only tokens[offsets[0] .. offsets[N]) belong to the call: this is that window
    const int64_t* const offsets;
    int64_t strands = 1;          // reverse-complement mode: every sequence owns the windows of both its strands
    uint8_t wild_small[256] = {0};
    bool wild_tok = false;        // some sequence really holds a wildcard
    uint8_t lut8[256] = {0};      // byte-table regime: token -> rank
    bool byte_regime = false;

    Planner(const LoadInput& i, LoadPlan& p)
        : in(i), P(p), g(i.g), N(i.n_train + i.n_test), off0(i.offsets[0]), tokens(i.tokens ? i.tokens + i.offsets[0] : i.tokens), offsets(i.offsets) {
        for (size_t q = 0; q < in.n_wild; ++q)
            if (in.wild_tokens[q] >= 0 && in.wild_tokens[q] < 256) wild_small[in.wild_tokens[q]] = 1;
    }

    int fail(int code, const char* fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        P.msg = buf;
        return P.code = code;
    }
    int64_t len_of(int64_t i) const { return offsets[i + 1] - offsets[i]; }
    const int32_t* seq(int64_t i) const { return tokens + (offsets[i] - off0); }
    bool is_wild(int32_t t) const {
        return (uint32_t)t < 256u ? wild_small[t] != 0 : std::binary_search(in.wild_tokens, in.wild_tokens + in.n_wild, t);
    }
    // centre-weighted mode: window p of a sequence of nw windows lies d = |2 p - (nw - 1)| / 2 from its centre (2 p + g - len,
    // halved downwards) and counts w[min(d, n - 1)] times
    int64_t cw_of(int64_t p, int64_t nw) const {
        const int64_t t = 2 * p - (nw - 1);
        return (int64_t)in.cw[(size_t)std::min<int64_t>((t < 0 ? -t : t) / 2, (int64_t)in.n_cw - 1)];
    }
    bool rc_comp_of(int32_t t, int32_t* out) const {
        const int32_t* it = std::lower_bound(in.rc_tokens, in.rc_tokens + in.n_rc, t);
        if (it == in.rc_tokens + in.n_rc || *it != t) return false;
        *out = in.rc_comps[it - in.rc_tokens];
        return true;
    }
    // the windows of sequence i that are windows, in order: fn(window, weight). A window that holds a wildcard is none — the
    // wildcard-free run that ends at every symbol tells: the window that ends there is valid when the run reaches g —, and
    // neither is one of weight 0.
    template <typename F>
    void each_window(int64_t i, F&& fn) const {
        const int32_t* sq = seq(i);
        const int64_t len = len_of(i), nw = len - g + 1;
        int64_t run = 0;
        for (int64_t p = 0; p < len; ++p) {
            run = wild_tok && is_wild(sq[p]) ? 0 : run + 1;
            if (run < g) continue;
            const int64_t wgt = P.cw_on ? cw_of(p - g + 1, nw) : 1;
            if (wgt) fn(p - g + 1, wgt);
        }
    }

    int census_lengths();
    int census_windows();
    void layout_features();
    void count_bytes(int64_t lo, int64_t hi, std::array<int64_t, 256>& h, char* small) const;
    void distinct_general();
    int close_alphabet();
    int layout_words();
    int alphabet_and_staging(const std::vector<std::array<int64_t, 256>>& hist, const std::vector<char>& small, const StagingAlloc& staging);
    void pack_general();
    void both_strands();
};

// ---- validation and lengths (fastsk.cpp:32-58)
int Planner::census_lengths() {
    P.rc_on = in.n_rc != 0;
    strands = P.rc_on ? 2 : 1;
    if (in.n_wild && P.rc_on)
        for (size_t q = 0; q < in.n_rc; ++q)
            if (is_wild(in.rc_tokens[q]) && !is_wild(in.rc_comps[q]))
                return fail(FSK_EINVAL, "wildcard token %d has the complement %d, which is not a wildcard", in.rc_tokens[q], in.rc_comps[q]);
    int64_t shortest_train = INT64_MAX, shortest_test = INT64_MAX, longest = 0, nfeat = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int64_t len = len_of(i);
        if (len < 0) return fail(FSK_EINVAL, "offsets must be non-decreasing");
        if (i < in.n_train) shortest_train = std::min(shortest_train, len);
        else shortest_test = std::min(shortest_test, len);
        longest = std::max(longest, len);
        nfeat += len >= g ? strands * (len - g + 1) : 0;
    }
    if (g > shortest_train)
        return fail(FSK_ESHORT, "g cannot be longer than the shortest sequence in a dataset. g = %d, but shortest train sequence has length %lld", g, (long long)shortest_train);
    if (in.n_test > 0 && g > shortest_test)
        return fail(FSK_ESHORT, "g cannot be longer than the shortest sequence in a dataset. g = %d, but shortest test sequence has length %lld", g, (long long)shortest_test);
    if (nfeat >= FEAT_LIMIT || longest >= ((int64_t)1 << 24)) return fail(FSK_EUNSUPPORTED, "input too large (g-mers >= 2^31 or a sequence >= 2^24)");
    P.N = N; P.nfeat = nfeat; P.longest = longest; P.most_valid = longest - g + 1;
    P.shortest = std::min(shortest_train, in.n_test > 0 ? shortest_test : shortest_train);
    P.total = offsets[N] - off0;
    return FSK_OK;
}

// ---- the windows that count, when not every window counts once.
// Wildcard mode: `wild_on` when some sequence really holds one (a set whose tokens do not occur leaves this load the plain
// one, to the launch); per sequence the number of valid windows (nvalid) and one bit a window position (vbits, sequence i
// from word vstart[i]; bits past the last position stay zero).
// Centre-weighted mode: the distances the data reach are 0 .. (longest - g) / 2: `cw_on` when one of their weights is not 1
// (else this load is the plain one too), and a weight of 0 among them clears windows in the validity bitmap as a wildcard
// does. nvalid, nfeat and most_valid are then SUMS OF WEIGHTS.
int Planner::census_windows() {
    bool cw_zero = false;
    if (in.n_cw && P.longest >= g) {
        const size_t reach = std::min<size_t>((size_t)((P.longest - g) / 2), in.n_cw - 1);
        for (size_t d = 0; d <= reach; ++d) { P.cw_on = P.cw_on || in.cw[d] != 1; cw_zero = cw_zero || in.cw[d] == 0; }
    }
    if (in.n_wild)
        for (int64_t i = 0; i < P.total && !wild_tok; ++i) wild_tok = is_wild(tokens[i]);
    P.wild_on = wild_tok || cw_zero;
    if (!P.wild_on && !P.cw_on) return FSK_OK;
    P.nvalid.resize((size_t)N);
    if (P.wild_on) {
        P.vstart.resize((size_t)N + 1);
        uint64_t vw = 0;
        for (int64_t i = 0; i < N; ++i) {
            P.vstart[(size_t)i] = (uint32_t)vw;
            vw += (uint64_t)(len_of(i) - g + 1 + 31) / 32;
        }
        P.vstart[(size_t)N] = (uint32_t)vw;  // (fewer words than symbols: below 2^31)
        P.vbits.assign((size_t)vw + 1, 0u);
    }
    P.nfeat = 0;
    P.most_valid = 0;
    for (int64_t i = 0; i < N; ++i) {
        uint32_t* vb = P.wild_on ? P.vbits.data() + P.vstart[(size_t)i] : nullptr;
        int64_t nv = 0;
        each_window(i, [&](int64_t j, int64_t wgt) {
            if (vb) vb[j >> 5] |= 1u << (j & 31);
            nv += wgt;
        });
        if (nv == 0)
            return fail(FSK_ESHORT, "sequence %lld has no window of length g = %d that is free of wildcards%s: it would have no features", (long long)i, g,
                        P.cw_on ? " and has a center weight above 0" : "");
        if (nv >= FEAT_LIMIT) return fail(FSK_EUNSUPPORTED, "input too large (weighted g-mers >= 2^31)");
        P.nvalid[(size_t)i] = (uint32_t)nv;
        P.nfeat += strands * nv;
        P.most_valid = std::max(P.most_valid, nv);
    }
    // (the weighted features are the sort records and the 32-bit feature offsets: the bound again, now that they are known)
    if (P.nfeat >= FEAT_LIMIT) return fail(FSK_EUNSUPPORTED, "input too large (weighted g-mers >= 2^31)");
    return FSK_OK;
}

// lengths and feature starts; and, after a census, fwin, the window of every feature, for the sparse dataflow (by the
// census's own enumeration, now that the features are known to fit): a sequence's valid forward windows in order, then
// (second strand) window j' of rc(x), valid exactly when forward window (len - g) - j' is, as len - g + 1 + j'. A window is
// listed as often as it weighs — w(j') = w(forward twin) — and so becomes that many equal sort records: the run length of
// the segment stage is the weighted multiplicity.
void Planner::layout_features() {
    const bool census = P.wild_on || P.cw_on;
    P.len32.resize((size_t)N);
    P.fstart.resize((size_t)N + 1);
    if (census) P.fwin.resize((size_t)P.nfeat);
    uint32_t* out = P.fwin.data();
    uint32_t fcount = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int64_t len = len_of(i);
        P.len32[(size_t)i] = (uint32_t)len;
        P.fstart[(size_t)i] = fcount;
        fcount += (uint32_t)(strands * (census ? (int64_t)P.nvalid[(size_t)i] : len - g + 1));
        if (!census) continue;
        const uint32_t* const first = out;
        each_window(i, [&](int64_t j, int64_t wgt) { out = std::fill_n(out, wgt, (uint32_t)j); });
        const uint32_t top = 2u * (uint32_t)(len - g + 1) - 1u;
        if (P.rc_on)  // the forward list backwards: twin nw - 1 - j as nw + j
            for (const uint32_t* q = out; q > first;) *out++ = top - *--q;
    }
    P.fstart[(size_t)N] = fcount;
}

// ---- alphabet: rank-remap the tokens that occur (equality preserving; the reference's dict_size = |{0} U tokens|,
// fastsk.cpp:70-85, only serves as its counting-sort radix), then pack, every sequence word-aligned.

// one thread's share of the tokens: how often every value below 256 occurs, and whether all values are below 256
void Planner::count_bytes(int64_t lo, int64_t hi, std::array<int64_t, 256>& h, char* small) const {
    // (four interleaved sets of counters: neighbouring tokens are often equal — DNA has four symbols —, and one
    // counter incremented twice in a row waits for its own store: ~1.1 -> ~0.5 ns a token)
    uint32_t h4[4][256];
    memset(h4, 0, sizeof h4);
    uint32_t big = 0;
    int64_t i = lo;
    for (; i + 4 <= hi; i += 4) {
        const uint32_t v0 = (uint32_t)tokens[i], v1 = (uint32_t)tokens[i + 1], v2 = (uint32_t)tokens[i + 2], v3 = (uint32_t)tokens[i + 3];
        big |= v0 | v1 | v2 | v3;
        h4[0][v0 & 255u]++; h4[1][v1 & 255u]++; h4[2][v2 & 255u]++; h4[3][v3 & 255u]++;
    }
    for (; i < hi; ++i) { const uint32_t v = (uint32_t)tokens[i]; big |= v; h4[0][v & 255u]++; }
    *small = big < 256u;  // (a token id beyond 255 somewhere: the general regime)
    for (int v = 0; v < 256; ++v) h[(size_t)v] = (int64_t)h4[0][v] + h4[1][v] + h4[2][v] + h4[3][v];
}

// token values anywhere in int32: distinct values by a seen-table or by sort
void Planner::distinct_general() {
    std::vector<int32_t>& distinct = P.distinct;
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t i = 0; i < P.total; ++i) { lo = std::min(lo, tokens[i]); hi = std::max(hi, tokens[i]); }
    if (P.total > 0 && lo >= 0 && hi < (1 << 20)) {
        std::vector<char> seen((size_t)hi + 1, 0);
        for (int64_t i = 0; i < P.total; ++i) seen[tokens[i]] = 1;
        for (int32_t v = 0; v <= hi; ++v) if (seen[v]) distinct.push_back(v);
    } else {
        distinct.assign(tokens, tokens + P.total);
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    }
    if (wild_tok) distinct.erase(std::remove_if(distinct.begin(), distinct.end(), [&](int32_t t) { return is_wild(t); }), distinct.end());
}

// reverse-complement mode: `distinct` (the tokens present, ascending) becomes its closure under the map — data without
// a single 'g' still produce 'g' on their second strand —; a token the map does not list fails the load, named (the
// first one in the data: protein given to a DNA map must not be self-complemented silently)
int Planner::close_alphabet() {
    if (!P.rc_on) return FSK_OK;
    std::vector<int32_t>& distinct = P.distinct;
    const size_t present = distinct.size();
    for (size_t q = 0; q < present; ++q) {
        int32_t c = 0;
        if (!rc_comp_of(distinct[q], &c)) {
            int32_t first = distinct[q];
            for (int64_t i = 0; i < P.total; ++i)
                if (!rc_comp_of(tokens[i], &c) && !(wild_tok && is_wild(tokens[i]))) { first = tokens[i]; break; }
            return fail(FSK_EINVAL, "token %d occurs in the sequences but not in the complement map", first);
        }
        distinct.push_back(c);
    }
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    return FSK_OK;
}

// sigma, bits, V from `distinct`; where every sequence's words start
int Planner::layout_words() {
    // (cntsrtna's radix is the dictionary size, whatever it is — shared.cpp:156-191 — and its keys are tuples, never a
    // number: up to 65536 symbols travel as 16-bit fields, and a k-mer space beyond 2^62 is keyed by the symbols' bit
    // fields side by side instead of a mixed-radix number, see key_symbits)
    if (P.distinct.size() > 65536) return fail(FSK_EUNSUPPORTED, "alphabet of %zu symbols (> 65536)", P.distinct.size());
    const uint32_t sigma = P.sigma = (uint32_t)std::max<size_t>(1, P.distinct.size());
    P.bits = sigma <= 4 ? 2 : sigma <= 16 ? 4 : sigma <= 256 ? 8 : 16;
    P.V = 1;
    P.key_symbits = 0;
    for (int c = 0; c < in.k; ++c) {
        if (P.V > (((uint64_t)1 << 62) / sigma)) { P.key_symbits = 1; break; }
        P.V *= sigma;
    }
    if (P.key_symbits) {
        while (((uint64_t)1 << P.key_symbits) < sigma) ++P.key_symbits;
        P.V = (uint64_t)1 << 62;  // (at least: the dense dataflow and the 24-bit fast paths are out of the question)
        if ((int64_t)P.key_symbits * in.k > 96)
            return fail(FSK_EUNSUPPORTED, "a k-mer of %d symbols of %d bits does not fit the 128-bit sort records", in.k, P.key_symbits);
    }
    P.wstart.resize((size_t)N);
    uint64_t nwords = 0;
    for (int64_t i = 0; i < N; ++i) {
        P.wstart[(size_t)i] = (uint32_t)nwords;
        nwords += ((uint64_t)P.len32[(size_t)i] * P.bits + 31) / 32;
        if (nwords >= ((uint64_t)1 << 32)) return fail(FSK_EUNSUPPORTED, "packed sequences exceed 2^32 words");
    }
    P.n_words = nwords;
    return FSK_OK;
}

// the middle step of the team: the counts become the alphabet and the rank table (token ids below 256, every vocabulary
// in practice: the byte-table regime; else the general one), the words are laid out in the caller's staging
int Planner::alphabet_and_staging(const std::vector<std::array<int64_t, 256>>& hist, const std::vector<char>& small, const StagingAlloc& staging) {
    P.sym_freq.assign(256, 0);
    byte_regime = std::all_of(small.begin(), small.end(), [](char s) { return s != 0; });
    if (byte_regime) {
        int64_t cnt[256];
        for (int v = 0; v < 256; ++v) {
            cnt[v] = 0;
            for (const auto& h : hist) cnt[v] += h[(size_t)v];
            if (cnt[v] && !(wild_tok && wild_small[v])) P.distinct.push_back(v);
        }
        if (close_alphabet()) return P.code;
        if (P.distinct.size() > 256) { byte_regime = false; P.distinct.clear(); }  // (complements beyond the byte table)
        for (size_t r = 0; byte_regime && r < P.distinct.size(); ++r)
            if (P.distinct[r] >= 0 && P.distinct[r] < 256) { lut8[P.distinct[r]] = (uint8_t)r; P.sym_freq[r] = cnt[P.distinct[r]]; }
    }
    if (!byte_regime) {
        distinct_general();
        if (close_alphabet()) return P.code;
        if (P.distinct.size() > P.sym_freq.size()) P.sym_freq.assign(P.distinct.size(), 0);
    }
    if (layout_words()) return P.code;
    const size_t n = (size_t)N, need = (size_t)P.n_words + 4 + 3 * n + 1;
    P.staging = staging(need);
    if (!P.staging) return fail(FSK_ENOMEM, "cannot allocate %zu bytes of pinned staging", need * sizeof(uint32_t));
    uint32_t* tables = P.staging + P.n_words + 4;
    memcpy(tables, P.wstart.data(), n * sizeof(uint32_t));
    memcpy(tables + n, P.len32.data(), n * sizeof(uint32_t));
    memcpy(tables + 2 * n, P.fstart.data(), (n + 1) * sizeof(uint32_t));
    // (the byte-table packer stores whole words; the general one sets bits in zeroed ones)
    if (byte_regime) memset(P.staging + P.n_words, 0, 4 * sizeof(uint32_t));
    else memset(P.staging, 0, ((size_t)P.n_words + 4) * sizeof(uint32_t));
    return FSK_OK;
}

// general regime: ranks by table or binary search, one thread; counts the symbols as it goes
void Planner::pack_general() {
    const std::vector<int32_t>& distinct = P.distinct;
    const int32_t base = distinct.empty() ? 0 : distinct.front();
    const bool direct = !distinct.empty() && (int64_t)distinct.back() - base < (1 << 20);
    std::vector<uint16_t> lut;
    if (direct) {
        lut.assign((size_t)(distinct.back() - base) + 1, 0);
        for (size_t r = 0; r < distinct.size(); ++r) lut[(size_t)(distinct[r] - base)] = (uint16_t)r;
    }
    for (int64_t i = 0; i < N; ++i) {
        const int32_t* sq = seq(i);
        uint32_t* w = P.staging + P.wstart[(size_t)i];
        for (uint32_t p = 0; p < P.len32[(size_t)i]; ++p) {
            if (wild_tok && is_wild(sq[p])) continue;  // (rank 0 in the words, counted nowhere)
            const uint32_t r = direct ? lut[(size_t)(sq[p] - base)]
                                      : (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), sq[p]) - distinct.begin());
            const uint32_t bitpos = p * (uint32_t)P.bits;
            w[bitpos >> 5] |= r << (bitpos & 31u);
            P.sym_freq[r]++;
        }
    }
}

// the complement of every rank; a symbol's frequency over both strands is its own plus its complement's
void Planner::both_strands() {
    const std::vector<int32_t>& distinct = P.distinct;
    if (P.rc_on) {
        P.comp_rank.resize(distinct.size());
        for (size_t r = 0; r < distinct.size(); ++r) {
            int32_t c = 0;
            (void)rc_comp_of(distinct[r], &c);
            P.comp_rank[r] = (uint16_t)(std::lower_bound(distinct.begin(), distinct.end(), c) - distinct.begin());
        }
        std::vector<int64_t> both(P.sym_freq);
        for (size_t r = 0; r < distinct.size(); ++r) both[r] = P.sym_freq[r] + P.sym_freq[P.comp_rank[r]];
        P.sym_freq.swap(both);
    }
    P.total_sym = strands * P.total;  // symbols counted, both strands
    if (wild_tok) {
        P.total_sym = 0;
        for (size_t r = 0; r < distinct.size() && r < P.sym_freq.size(); ++r) P.total_sym += P.sym_freq[r];
    }
}

}  // namespace

void make_load_plan(const LoadInput& in, const StagingAlloc& staging, LoadPlan& plan) {
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    plan = LoadPlan{};
    Planner pl(in, plan);
    if (pl.census_lengths() || pl.census_windows()) return;
    pl.layout_features();
    plan.ms_census = ms();
    // ONE team of host threads counts the tokens of its share of the sequences (256 counters each), one of them turns
    // the counts into the rank table and lays out the words in the caller's staging, the team packs its sequences
    // there. (At 100k x 300 tokens this is the load time.)
    const int64_t N = pl.N, total = plan.total;
    const int nt = host_threads_for(total);
    std::vector<int64_t> bound((size_t)nt + 1, N);  // sequence ranges with about equal token counts
    bound[0] = 0;
    for (int t = 1; t < nt; ++t)
        bound[(size_t)t] = std::lower_bound(in.offsets, in.offsets + N, pl.off0 + total * t / nt) - in.offsets;
    std::vector<std::array<int64_t, 256>> hist((size_t)nt);
    std::vector<char> small((size_t)nt, 1);
    parallel_two_phase(
        nt,
        [&](int t) { pl.count_bytes(in.offsets[bound[(size_t)t]] - pl.off0, in.offsets[bound[(size_t)t + 1]] - pl.off0, hist[(size_t)t], &small[(size_t)t]); },
        [&] { pl.alphabet_and_staging(hist, small, staging); },
        [&](int t) {
            if (plan.code) return;
            if (!pl.byte_regime) { if (t == 0) pl.pack_general(); return; }
            for (int64_t i = bound[(size_t)t]; i < bound[(size_t)t + 1]; ++i) {  // a sequence's words are its own
                uint32_t* w = plan.staging + plan.wstart[(size_t)i];
                // (the symbol width as a compile-time constant: the 16 / 8 / 4 symbols of a word unroll)
                if (plan.bits == 2) pack_sequence<2>(pl.seq(i), plan.len32[(size_t)i], pl.lut8, w);
                else if (plan.bits == 4) pack_sequence<4>(pl.seq(i), plan.len32[(size_t)i], pl.lut8, w);
                else pack_sequence<8>(pl.seq(i), plan.len32[(size_t)i], pl.lut8, w);
            }
        });
    if (plan.code) return;
    pl.both_strands();
    plan.ms_pack = ms();
}

}  // namespace fsk_load
