// fsk_engine.hip — host side of the C ABI declared in include/fastsk_amd.h.
//
// Replaces, for the kernel-construction path only, the reference's host driver
// (FastSK::compute_kernel / compute_train, fastsk.cpp:30-188), its engine
// (KernelFunction::compute_kernel / kernel_build_parallel / get_variance,
// fastsk_kernel.cpp:24-322) and the getters (fastsk.cpp:190-237). No CPU compute fallback lives
// here: every count is produced by the HIP kernels of fsk_kernels_*.h, and construction fails
// loudly when no device is usable.
#include "fsk_engine_internal.h"
#include "fsk_kernels_result.h"
#include "fsk_load_plan.h"

using namespace fsk_detail;

// the staged calls in mismatch-weighted mode: their combination ids would belong to one level only
#define FSK_NOT_STAGED(e, what)                                                                                              \
    if ((e)->mm_on())                                                                                                        \
        return (e)->fail(FSK_ESTATE, what ": the staged path does not exist in mismatch-weighted mode (fsk_set_mismatch_weights): fsk_compute is the entry point")

namespace {

thread_local std::string g_create_error;

}  // namespace

namespace fsk_detail {

void set_create_error(const std::string& msg) { g_create_error = msg; }

// ---- tuning (fsk_tuning, fsk_engine_internal.h): one table of keys, defaults and ranges
namespace {
struct TuneKey { const char* name; int64_t fsk_tuning::*field; int64_t def, lo, hi; const char* doc; };
const TuneKey TUNE_KEYS[] = {
#define FSK_X(name, def, lo, hi, doc) {#name, &fsk_tuning::name, (int64_t)(def), (int64_t)(lo), (int64_t)(hi), doc},
    FSK_TUNING_KEYS(FSK_X)
#undef FSK_X
};
}  // namespace

int tuning_set(fsk_tuning& t, const char* key, int64_t value, std::string& err) {
    for (const TuneKey& k : TUNE_KEYS)
        if (key && !strcmp(k.name, key)) {
            if (value < k.lo || value > k.hi) {
                err = std::string("tuning key ") + key + " takes " + std::to_string(k.lo) + " .. " + std::to_string(k.hi) + ", not " + std::to_string(value);
                return FSK_EINVAL;
            }
            t.*(k.field) = value;
            return FSK_OK;
        }
    err = std::string("unknown tuning key '") + (key ? key : "(null)") + "'";
    return FSK_EINVAL;
}

// "key=value,key=value" (commas or blanks between the pairs)
int tuning_parse(fsk_tuning& t, const char* text, std::string& err) {
    std::string s(text ? text : "");
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && (s[i] == ',' || s[i] == ' ' || s[i] == ';')) ++i;
        size_t j = i;
        while (j < s.size() && s[j] != ',' && s[j] != ' ' && s[j] != ';') ++j;
        if (j > i) {
            const std::string pair = s.substr(i, j - i);
            const size_t eq = pair.find('=');
            char* end = nullptr;
            const long long v = eq == std::string::npos ? 0 : strtoll(pair.c_str() + eq + 1, &end, 0);
            if (eq == std::string::npos || eq == 0 || eq + 1 == pair.size() || (end && *end)) {
                err = "expected key=integer, got '" + pair + "'";
                return FSK_EINVAL;
            }
            const int rc = tuning_set(t, pair.substr(0, eq).c_str(), (int64_t)v, err);
            if (rc) return rc;
        }
        i = j;
    }
    return FSK_OK;
}

// the keys that differ from their defaults ("defaults" when none does)
std::string tuning_in_force(const fsk_tuning& t) {
    std::string out;
    for (const TuneKey& k : TUNE_KEYS)
        if (t.*(k.field) != k.def) out += (out.empty() ? "" : ",") + std::string(k.name) + "=" + std::to_string(t.*(k.field));
    return out.empty() ? "defaults" : out;
}

int64_t n_choose_k(int n, int k) {  // nchoosek, shared.cpp:335-345 (exact in 64 bits)
    if (k < 0 || k > n) return 0;
    if (k * 2 > n) k = n - k;
    int64_t r = 1;
    for (int i = 1; i <= k; ++i) {
        if (r > (INT64_MAX / 2) / (n - k + i)) return INT64_MAX / 2;  // saturate: callers reject >= 2^31
        r = r * (n - k + i) / i;
    }
    return r;
}

// all k-subsets of {0..g-1}, lexicographic (getCombinations, shared.cpp:347-360)
void enumerate_combos(int g, int k, std::vector<uint8_t>& out) {
    std::vector<int> pos(k);
    for (int i = 0; i < k; ++i) pos[i] = i;
    out.clear();
    while (true) {
        for (int i = 0; i < k; ++i) out.push_back((uint8_t)pos[i]);
        int i = k - 1;
        while (i >= 0 && pos[i] == g - k + i) --i;
        if (i < 0) break;
        ++pos[i];
        for (int j = i + 1; j < k; ++j) pos[j] = pos[j - 1] + 1;
    }
}

uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Which dataflow is cheaper per combo (path = auto)? The dense one multiplies every pair of
// sequences over the whole key space at the v_dot8 rate; the sparse one issues one scattered
// 64-bit atomic per (run, pair). Rates measured on MI355X.
bool dense_is_cheaper(const fsk_engine* e) {
    const double N = (double)e->N, V = (double)e->V;
    const double W = (double)e->nfeat / std::max(1.0, N);                 // windows per sequence
    // dense: every pair of sequences over the whole key space at the tile kernel's rate, plus the
    // count kernel: one pass over the windows per histogram sweep (large key spaces need many)
    // (count kernel, fitted on MI355X: 1e-12 s per window for the first histogram sweep, 2.6e-12 s
    // per window for every further sweep when the window keys are cached in LDS — as
    // accumulate_dense arranges when they fit — and 8e-12 s when they are recomputed; 7e-13 s per
    // (sequence, key) for zeroing and reading out the histograms)
    // (reverse-complement mode: nfeat and maxW count both strands; the kernel stages one strand's maxW1 windows at a time
    // and runs without the window-key cache)
    DensePlan plan = dense_plan(e->maxW1, e->cfg.g, e->Vq);
    double sweep_cost = 8e-12;
    if (plan.Vcq && plan.Vcq < e->Vq && plan.CH >= e->maxW1 && !e->revcomp) {
        const DensePlan p2 = dense_plan(e->maxW1, e->cfg.g, e->Vq, (size_t)e->maxW1 * fsk::PANEL * sizeof(uint16_t));
        if (p2.CH >= e->maxW1 && p2.Vcq >= 64) { plan = p2; sweep_cost = 2.6e-12; }
    }
    const double sweeps = plan.Vcq ? std::ceil((double)e->Vq / plan.Vcq) : 1.0;
    // (tile kernel: 3.0e14 count-MAC/s with thousands of tiles, ~2.4e14 with few)
    const double dense = 0.5 * N * N * (double)(((e->Vq + 1) / 2) * 8) / (N < 8192.0 ? 2.4e14 : 3.0e14) +
                         (double)e->nfeat * (1e-12 + (sweeps - 1.0) * sweep_cost) + N * V * 7e-13;
    // sparse: sort + segments per g-mer (3.1e-11 s each), then one update per (run, pair). d = sequences holding a given key.
    // SHORT runs — update words through emit + consume: 1.7e11 updates/s on owner bands of one LDS round, a band of several
    // rounds re-reads its stream once per round; beyond four rounds the two-level blocks, ~1.0e11/s (N = 100k: 9.3e10); where
    // neither exists per-pair global atomics, 1.6e10/s. LONG runs (12 += a sort record and more, i.e. d >= ~24) — DESCRIPTORS,
    // bands of one round or blocks: the longer the run the cheaper a pair (a descriptor's fixed cost, then four partners a
    // 16-byte load): 2.2e12 d / (d + 300) updates/s fits profiles/dense_vs_sparse_regimes.jsonl (DNA k = 4 .. 7, N = 4000 and
    // 16000: 0.2e12 at d = 22, 0.5 at 88, 1.2 at 300, 1.6 at 1000, 2.0 at 2700) within a fifth. The blocks sweep K once a batch
    // (16 B a cell at ~5 TB/s, a batch = 2^27 records). The approx modes' variance form (slot triangles, owner bands only)
    // does not have the blocks and expands a slot's few descriptors in workgroups of their own: priced as the word streams.
    const double d = N * (1.0 - std::exp(-W / V));
    const double U = V * d * (d + 1.0) / 2.0;
    const bool variance_form = e->cfg.approx && !e->cfg.skip_variance;
    const bool blocks_ok = !variance_form && blocks_plan_pass(const_cast<fsk_engine*>(e), 0, e->N, nullptr);
    const bool bands_few_rounds = e->sx_lists && e->sx_rounds <= 4;
    double rate = bands_few_rounds ? 1.7e11 / (1.0 + 0.3 * ((double)e->sx_rounds - 1.0))
                  : blocks_ok      ? 1.0e11
                  : e->sx_lists    ? 1.7e11 / (1.0 + 0.3 * ((double)e->sx_rounds - 1.0))
                                   : 1.6e10;
    const bool descriptors = !variance_form && e->tune.sparse_desc >= 0 && d >= 24.0 && ((e->sx_lists && e->sx_rounds <= 1) || blocks_ok);
    if (descriptors) rate = std::max(rate, 2.2e12 * d / (d + 300.0));
    double sparse = U / rate + (double)e->nfeat * 3.1e-11;
    if (!bands_few_rounds && blocks_ok) {
        const double per_batch = std::max(1.0, std::floor((double)SPARSE_MAX_RECORDS / std::max(1.0, (double)e->nfeat)));
        sparse += 0.5 * N * N * 16.0 / 5e12 / per_batch;
    }
    return dense <= sparse;
}

int choose_path(fsk_engine* e) {
    bool dense_ok = e->V <= DENSE_MAX_KEYS && e->bits <= 8 && e->k <= 16 && e->Lmax < 65536 && e->maxW < 65536 && dense_plan(e->maxW1, e->cfg.g, e->Vq, dense_mode_lds(e)).CH > 0;
    if (e->cfg.path == FSK_PATH_DENSE) {
        if (!dense_ok)
            return e->fail(FSK_EUNSUPPORTED, "dense path needs alphabet^k <= %llu and the panel histogram to fit in LDS",
                           (unsigned long long)DENSE_MAX_KEYS);
        e->path = FSK_PATH_DENSE;
    } else if (e->cfg.path == FSK_PATH_SPARSE) {
        e->path = FSK_PATH_SPARSE;
    } else {
        e->path = dense_ok && dense_is_cheaper(e) ? FSK_PATH_DENSE : FSK_PATH_SPARSE;
    }
    return FSK_OK;
}

// rows that fsk_reset_counts left for a storing tile launch get their zeros now (anything but such
// a launch is about to look at K)
int materialise_zero(fsk_engine* e) {
    if (e->ld.lazy_lo < 0) return FSK_OK;
    const u64 c0 = (u64)e->ld.lazy_lo * ((u64)e->ld.lazy_lo + 1) / 2, c1 = (u64)e->ld.lazy_hi * ((u64)e->ld.lazy_hi + 1) / 2;
    e->ld.lazy_lo = e->ld.lazy_hi = -1;
    if (c1 > c0) FSK_HIP(hipMemsetAsync(e->d_K + c0, 0, (size_t)(c1 - c0) * sizeof(u64), e->stream));
    return FSK_OK;
}
bool lazy_zero_possible(const fsk_engine* e) {
    return e->path == FSK_PATH_DENSE && !e->compact && !(e->cfg.skip_test_block && e->n_test > 0);
}

int do_accumulate(fsk_engine* e, const int32_t* combos, int n, u64* K, int64_t row0, int64_t row1, u64 slot_stride,
                  int defer) {
    if (row1 < 0) row1 = e->N;
    for (int i = 0; i < n; ++i)
        if (combos[i] < 0 || combos[i] >= e->ncomb) return e->fail(FSK_EINVAL, "combo id %d out of range [0,%lld)", combos[i], (long long)e->ncomb);
    Event a;
    if (e->cfg.profile) {  // (the whole call on the engine's stream; profile = 2: harvested later, see fsk_engine::tic)
        a = e->lazy_event();
        if (a) (void)hipEventRecord(a, e->stream);
    }
    int rc = e->path == FSK_PATH_DENSE ? accumulate_dense(e, combos, n, K, row0, row1) : accumulate_sparse(e, combos, n, K, row0, row1, slot_stride, defer);
    if (e->cfg.profile) {
        Event b = e->lazy_event();
        if (b) (void)hipEventRecord(b, e->stream);
        e->lazy_interval(std::move(a), std::move(b), &e->st.ms_total);
        if (e->profile_sync()) e->harvest_times();
    }
    if (rc == FSK_OK && row1 >= e->N) {  // a combo is done when its last row band is
        e->st.combos_done += n;
        e->st.combos_issued += (double)n;
    }
    return rc;
}

int make_diag(fsk_engine* e) {
    FSK_HIP(e->d_diag.reserve((size_t)e->N));
    const uint32_t blocks = (uint32_t)((e->N + 255) / 256);
    if (e->result_f64)
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_diag<double>), dim3(blocks), dim3(256), 0, e->stream, e->d_Kf64.p, e->d_diag.p, (uint32_t)e->N);
    else
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_diag<u64>), dim3(blocks), dim3(256), 0, e->stream, e->d_K, e->d_diag.p, (uint32_t)e->N);
    FSK_HIP(hipStreamSynchronize(e->stream));
    e->finalized = true;
    e->svm.valid = e->svm.cv.valid = e->svm.svr_cv.valid = e->svm.mc_cv.valid = false;  // (a model and a cross-validation belong to the result they were computed on)
    e->rows.drop();                          // (and so does the rows kernel)
    return FSK_OK;
}

// The order the reference draws for this seed: std::shuffle(indexes, std::default_random_engine{seed}) of libstdc++
// (fastsk_kernel.cpp:31-38 seeds it with time(0)), restated. default_random_engine is minstd_rand0, x <- 16807 x mod
// (2^31 - 1), values in [1, 2^31 - 2]; uniform_int_distribution over [0, r] takes its "downscaling" branch (reject draws
// from urange / (r + 1) * (r + 1) on, divide by the scaling); std::shuffle swaps element i with a draw from [0, i] —
// two elements per draw (one number below i * (i + 1) split by / and %) while n * n fits the generator's range, after
// a single swap up front when n is even.
void libstdcxx_shuffle_order(uint64_t seed, int64_t n, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = (int32_t)i;
    if (n < 2) return;
    const uint64_t M = 2147483647ull, RANGE = M - 2;  // max() - min()
    uint64_t x = seed % M;
    if (x == 0) x = 1;  // linear_congruential_engine::seed with c = 0
    auto below = [&](uint64_t count) {  // uniform in [0, count): uniform_int_distribution{0, count - 1}
        if (count - 1 == RANGE) { x = x * 16807ull % M; return x - 1; }
        const uint64_t scaling = RANGE / count, past = count * scaling;
        uint64_t r;
        do { x = x * 16807ull % M; r = x - 1; } while (r >= past);
        return r / scaling;
    };
    const uint64_t un = (uint64_t)n;
    if (RANGE / un >= un) {
        int64_t i = 1;
        if (un % 2 == 0) { std::swap(out[i], out[below(2)]); ++i; }
        while (i < n) {
            const uint64_t r = (uint64_t)i + 1, both = below(r * (r + 1));
            std::swap(out[i], out[both / (r + 1)]); ++i;
            std::swap(out[i], out[both % (r + 1)]); ++i;
        }
        return;
    }
    for (int64_t i = 1; i < n; ++i) std::swap(out[i], out[below((uint64_t)i + 1)]);
}

void default_order(fsk_engine* e) {
    e->order.resize((size_t)e->ncomb);
    if (e->tune.seed_splitmix == 0) {  // the reference's own sample for this seed
        libstdcxx_shuffle_order(e->seed, e->ncomb, e->order.data());
        return;
    }
    for (int64_t i = 0; i < e->ncomb; ++i) e->order[i] = (int32_t)i;
    uint64_t s = e->seed;
    for (int64_t i = e->ncomb - 1; i > 0; --i) {
        int64_t j = (int64_t)(splitmix64(s) % (uint64_t)(i + 1));
        std::swap(e->order[i], e->order[j]);
    }
}

int fetch_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double* out) {
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (i0 < 0 || j0 < 0 || i1 > e->N || j1 > e->N || i0 > i1 || j0 > j1) return e->fail(FSK_EINVAL, "block out of range");
    const int64_t rows = i1 - i0, cols = j1 - j0;
    if (rows == 0 || cols == 0) return FSK_OK;
    if (!out) return e->fail(FSK_EINVAL, "null output");
    const int64_t max_cells = (int64_t)32 << 20;  // 256 MB of doubles per staging round
    const int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(rows, max_cells / cols));
    FSK_HIP(e->d_stage.reserve((size_t)(rows_per * cols)));
    for (int64_t r = 0; r < rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, rows - r);
        const u64 cells = (u64)nr * cols;
        const uint32_t blocks = (uint32_t)((cells + 255) / 256);
        if (e->result_f64)
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_block<double>), dim3(blocks), dim3(256), 0, e->stream, e->d_Kf64.p, e->d_diag.p,
                       (u64)(i0 + r), (u64)nr, (u64)j0, (u64)cols, e->d_stage.p);
        else
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_block<u64>), dim3(blocks), dim3(256), 0, e->stream, e->d_K, e->d_diag.p,
                       (u64)(i0 + r), (u64)nr, (u64)j0, (u64)cols, e->d_stage.p);
        FSK_HIP(hipMemcpyAsync(out + r * cols, e->d_stage.p, cells * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    return FSK_OK;
}

}  // namespace fsk_detail

// =============================================================================================
extern "C" {

int fsk_abi_version(void) { return FSK_ABI_VERSION; }

int fsk_seed_order(uint64_t seed, int64_t n, int32_t* out) {
    if (n < 0 || n > 0x7fffffff || (n > 0 && !out)) return FSK_EINVAL;
    fsk_detail::libstdcxx_shuffle_order(seed, n, out);
    return FSK_OK;
}

int fsk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int64_t fsk_num_combos(int32_t g, int32_t m) { return n_choose_k(g, m); }

int fsk_combo_positions(int32_t g, int32_t k, int64_t combo, int32_t* out) {
    if (!out || k <= 0 || k > g || combo < 0 || combo >= n_choose_k(g, k)) return FSK_EINVAL;
    int next = 0;
    for (int d = 0; d < k; ++d)
        for (int p = next; p < g; ++p) {
            int64_t below = n_choose_k(g - p - 1, k - d - 1);
            if (combo < below) { out[d] = p; next = p + 1; break; }
            combo -= below;
        }
    return FSK_OK;
}

const char* fsk_last_error(const fsk_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int fsk_create(const fsk_config* cfg, fsk_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return FSK_EINVAL; }
    *out = nullptr;
    if (cfg->g <= 0 || cfg->m < 0 || cfg->m >= cfg->g) {
        g_create_error = "need 0 <= m < g";
        return FSK_EINVAL;
    }
    if (cfg->g > 255) { g_create_error = "g > 255 unsupported"; return FSK_EUNSUPPORTED; }
    if (cfg->t == 0 || cfg->t < -1) { g_create_error = "t must be -1 or >= 1"; return FSK_EINVAL; }
    if (cfg->profile < 0 || cfg->profile > 2) { g_create_error = "profile must be 0, 1 or 2"; return FSK_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_error = "no HIP device visible: the MI355X engine has no CPU fallback";
        return FSK_EDEVICE;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return FSK_EINVAL; }
    DeviceScope on_device(cfg->device);  // the caller's current device is restored on return
    if (on_device.err != hipSuccess) { g_create_error = "hipSetDevice failed"; return FSK_EDEVICE; }
    fsk_engine* e = new fsk_engine;
    e->cfg = *cfg;
    e->k = cfg->g - cfg->m;
    e->ncomb = n_choose_k(cfg->g, cfg->m);
    if (e->ncomb > 0x7fffffff) { delete e; g_create_error = "C(g,m) >= 2^31 unsupported"; return FSK_EUNSUPPORTED; }
    enumerate_combos(cfg->g, e->k, e->all_pos);
    // the one place the library reads the environment: FSK_TUNING="key=value,key=value" (see FSK_TUNING_KEYS)
    if (const char* env = getenv("FSK_TUNING")) {
        std::string why;
        if (tuning_parse(e->tune, env, why)) {
            delete e;
            g_create_error = "FSK_TUNING: " + why;
            return FSK_EINVAL;
        }
    }
    e->cfg_profile0 = e->cfg.profile;  // (what tuning key profile = -1 goes back to)
    if (e->tune.profile >= 0) e->cfg.profile = (int)e->tune.profile;
    if (e->trace()) fprintf(stderr, "[fsk] tuning: %s\n", tuning_in_force(e->tune).c_str());
    if (e->stream.create(0) != hipSuccess || e->ev0.create(0) != hipSuccess ||
        e->ev1.create(0) != hipSuccess) {
        delete e;
        g_create_error = "cannot create HIP stream/events";
        return FSK_EDEVICE;
    }
#ifndef FSK_EMU
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device) == hipSuccess && cus > 0) e->n_cu = cus;
    }
#else
    e->n_cu = 2;  // (the emulation: a few persistent workgroups, so that chunks of several tiles and several bands occur)
#endif
    e->st.n_combos_total = (int32_t)e->ncomb;
    *out = e;
    return FSK_OK;
}

void fsk_destroy(fsk_engine* e) {
    if (!e) return;
    if (e->group) { group_destroy(e); return; }
    one_destroy(e);
}

}  // extern "C"

// Everything the engine owns goes in its destructor (fsk_engine_internal.h: who owns what), on its device and after whatever
// may still run on its streams
void fsk_detail::one_destroy(fsk_engine* e) {
    DeviceScope on_device(e->cfg.device);
    (void)hipStreamSynchronize(e->stream);
    if (e->lane_stream) (void)hipStreamSynchronize(e->lane_stream);
    if (e->chain_stream) (void)hipStreamSynchronize(e->chain_stream);  // (variance mode may leave a dropped batch's sums running)
    e->harvest_times();
    delete e;
}

extern "C" {

int fsk_set_combo_order(fsk_engine* e, const int32_t* order, int32_t n) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_set_combo_order(e, order, n) : one_set_combo_order(e, order, n);
}

}  // extern "C"

int fsk_detail::one_set_combo_order(fsk_engine* e, const int32_t* order, int32_t n) {
    if (!order || n <= 0 || n > e->ncomb) return e->fail(FSK_EINVAL, "combo order must hold 1..C(g,m) ids");
    std::vector<char> seen((size_t)e->ncomb, 0);
    for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= e->ncomb || seen[order[i]]) return e->fail(FSK_EINVAL, "combo order: id %d invalid or repeated", order[i]);
        seen[order[i]] = 1;
    }
    e->order.assign(order, order + n);
    e->order_set = true;
    return FSK_OK;
}

// fsk_set_complement: the map is checked here and kept sorted by token; the next load packs with it
int fsk_detail::one_set_complement(fsk_engine* e, const int32_t* tokens, const int32_t* complements, int32_t n) {
    if (n < 0 || (n > 0 && (!tokens || !complements))) return e->fail(FSK_EINVAL, "complement map: null arrays or a negative length");
    std::vector<std::pair<int32_t, int32_t>> map((size_t)n);
    for (int32_t i = 0; i < n; ++i) map[(size_t)i] = {tokens[i], complements[i]};
    std::sort(map.begin(), map.end());
    for (size_t i = 1; i < map.size(); ++i)
        if (map[i].first == map[i - 1].first) return e->fail(FSK_EINVAL, "complement map: token %d is listed twice", map[i].first);
    auto find = [&](int32_t t) { return std::lower_bound(map.begin(), map.end(), std::make_pair(t, INT32_MIN)); };
    for (const auto& tc : map) {
        const auto back = find(tc.second);
        if (back == map.end() || back->first != tc.second)
            return e->fail(FSK_EINVAL, "complement map: token %d maps to %d, which is not listed", tc.first, tc.second);
        if (back->second != tc.first)
            return e->fail(FSK_EINVAL, "complement map is not an involution: %d -> %d -> %d", tc.first, tc.second, back->second);
    }
    e->rc_tokens.resize(map.size());
    e->rc_comps.resize(map.size());
    for (size_t i = 0; i < map.size(); ++i) { e->rc_tokens[i] = map[i].first; e->rc_comps[i] = map[i].second; }
    return FSK_OK;
}

// fsk_set_wildcards: kept sorted; the next load counts and packs with them
int fsk_detail::one_set_wildcards(fsk_engine* e, const int32_t* tokens, int32_t n) {
    if (n < 0 || (n > 0 && !tokens)) return e->fail(FSK_EINVAL, "wildcards: a null array or a negative length");
    std::vector<int32_t> w(tokens, tokens + n);
    std::sort(w.begin(), w.end());
    for (size_t i = 1; i < w.size(); ++i)
        if (w[i] == w[i - 1]) return e->fail(FSK_EINVAL, "wildcards: token %d is listed twice", w[i]);
    e->wild_tokens.swap(w);
    return FSK_OK;
}

// fsk_set_center_weights: the profile is checked here; the next load weighs its windows with it
int fsk_detail::one_set_center_weights(fsk_engine* e, const uint32_t* w, int32_t n) {
    if (n < 0 || (n > 0 && !w)) return e->fail(FSK_EINVAL, "center weights: a null array or a negative length");
    if (n > 4096) return e->fail(FSK_EINVAL, "center weights: %d entries, at most 4096", n);
    for (int32_t i = 0; i < n; ++i)
        if (w[i] > 255u) return e->fail(FSK_EINVAL, "center weights: entry %d is %u, at most 255", i, w[i]);
    if (n > 0 && w[0] == 0u) return e->fail(FSK_EINVAL, "center weights: the first entry (the centre's weight) must be at least 1");
    std::vector<uint8_t> p((size_t)n);
    for (int32_t i = 0; i < n; ++i) p[(size_t)i] = (uint8_t)w[i];
    e->cw_profile.swap(p);
    return FSK_OK;
}

extern "C" {

int fsk_set_center_weights(fsk_engine* e, const uint32_t* w, int32_t n) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_set_center_weights(e, w, n) : one_set_center_weights(e, w, n);
}

int fsk_set_wildcards(fsk_engine* e, const int32_t* tokens, int32_t n) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_set_wildcards(e, tokens, n) : one_set_wildcards(e, tokens, n);
}

int fsk_set_complement(fsk_engine* e, const int32_t* tokens, const int32_t* complements, int32_t n) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_set_complement(e, tokens, complements, n) : one_set_complement(e, tokens, complements, n);
}

int fsk_set_seed(fsk_engine* e, uint64_t seed) {
    if (!e) return FSK_EINVAL;
    if (e->group) return group_set_seed(e, seed);
    e->seed = seed;
    return FSK_OK;
}

int fsk_load_sequences(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train, int64_t n_test) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_load_sequences");
    return e->group ? group_load_sequences(e, tokens, offsets, n_train, n_test) : one_load_sequences(e, tokens, offsets, n_train, n_test);
}

}  // extern "C"

// ---- fsk_load_sequences: fsk_load_plan.cpp makes the plan on the host (lengths, window census, alphabet, packed words in
// the pinned staging); what follows commits it to the engine and the device
namespace {

using fsk_load::LoadPlan;

// the plan's words and tables go into the engine's pinned staging, grown when it is too small
uint32_t* grow_stage(fsk_engine* e, size_t need) {
    return e->h_stage.reserve(need, need / 4) == hipSuccess ? e->h_stage.p : nullptr;
}

// the engine's view of the loaded set: sizes, modes, the sparse dataflow's hint and key widths, the dataflow
int commit_load(fsk_engine* e, const LoadPlan& p, int64_t n_train, int64_t n_test) {
    const int64_t N = p.N;
    const uint32_t strands = p.rc_on ? 2u : 1u;
    // whatever was known about the previous set — what is resident, pending or promised (the triangle is zeroed, or promised
    // to be, by the caller), the per-load figures of fsk_stats — starts from its initial values
    e->ld = {};
    // (the dense dataflow's tile table depends on the number of sequences and the train / test split alone: a set of the same
    // shape keeps the one on the device)
    if (e->N != N || e->n_train != n_train) e->tab_n = 0;
    e->N = N; e->n_train = n_train; e->n_test = n_test; e->nfeat = p.nfeat;
    e->pairs = N * (N + 1) / 2;
    e->sigma = p.sigma; e->bits = p.bits; e->V = p.V; e->Vq = (uint32_t)((p.V + 3) / 4);
    e->Lmax = (uint32_t)p.longest; e->Lmin = (uint32_t)p.shortest;
    e->maxW1 = (uint32_t)(p.longest - e->cfg.g + 1);
    e->maxW = strands * (uint32_t)p.most_valid;
    e->revcomp = p.rc_on;
    e->wild = p.wild_on;
    e->cw = p.cw_on;
    e->cw_n = p.cw_on ? (uint32_t)e->cw_profile.size() : 0u;
    e->fwin_on = p.wild_on || p.cw_on;
    e->n_panels = (uint32_t)((N + fsk::PANEL - 1) / fsk::PANEL);
    e->h_len = p.len32; e->h_fstart = p.fstart;
    {
        // The update words per record seen on the previous set of sequences stay as a HINT when the new set has the same shape
        // (sequences, windows, alphabet, longest sequence: the same data loaded again, or its next fold): the first batch is then
        // enqueued under a guard like every later one instead of being capped at 2^25 records and waited for. A hint that is
        // too low costs what any overflowing guard costs — the batch leaves K alone and is redone sized exactly —, never a
        // result. Tuning sparse_hint = 0: every set of sequences starts from nothing (testing).
        const u64 shape[4] = {(u64)N, (u64)p.nfeat, (u64)p.sigma, (u64)p.longest};
        const bool same = e->tune.sparse_hint && e->loaded && std::equal(shape, shape + 4, e->sx_shape);
        if (!same) { e->sx_wpr = 0; e->sx_ppr = 0; e->slots16_ok = true; }
        std::copy(shape, shape + 4, e->sx_shape);
    }
    if (e->V > DENSE_MAX_KEYS) e->Vq = 1;  // unused on the sparse path
    // sparse dataflow: sort record = (k-mer << sx_sb) | sequence id; owner bands of K
    e->sx_sb = 1;
    while (((int64_t)1 << e->sx_sb) < N) ++e->sx_sb;
    e->sx_symbits = p.key_symbits;
    e->sx_keybits = 1;
    if (p.key_symbits) e->sx_keybits = p.key_symbits * e->k;
    else while (e->sx_keybits < 62 && ((u64)1 << e->sx_keybits) < p.V) ++e->sx_keybits;
    plan_owner_bands(e);
    return choose_path(e);
}

// key compaction pays when a symbol is rare (DNA with a few 'n'): most of the sigma^k key
// space is then empty and need not be multiplied
struct Compaction { bool compact = false, compact_rare = false; uint32_t rare_mask = 0, rare_places = 0; };
Compaction choose_compaction(const LoadPlan& p, const fsk_tuning& tune, int g, int k) {
    Compaction c;
    int64_t rarest = INT64_MAX;
    for (uint32_t r = 0; r < p.sigma; ++r) rarest = std::min(rarest, p.sym_freq[r]);
    c.compact = p.sigma >= 3 && p.V >= 64 && p.V <= 4096 && rarest * 50 < p.total_sym;
    if (tune.compact >= 0) c.compact = tune.compact != 0 && p.V <= 4096;
    // ... and the keys that occur follow from the places of the rare symbols when those are few (g windows per place
    // and combo are marked instead of every window) and every key of common symbols can be taken as present (16
    // windows per such key at least: one that is missing only costs an empty panel row)
    int64_t places = 0;
    uint32_t common = 0;
    for (uint32_t r = 0; r < p.sigma && r < 32u; ++r) {
        if (p.sym_freq[r] * 50 < p.total_sym) { c.rare_mask |= 1u << r; places += p.sym_freq[r]; }
        else ++common;
    }
    double common_keys = 1;
    for (int i = 0; i < k; ++i) common_keys *= (double)common;
    c.compact_rare = c.compact && p.sigma <= 32 && common >= 1 && places > 0 && places < ((int64_t)1 << 24) &&
                     places * (int64_t)g * 8 < std::max<int64_t>(1, p.nfeat) && (double)p.nfeat >= 16.0 * common_keys;
    if (tune.compact_rare >= 0) c.compact_rare = c.compact && tune.compact_rare != 0 && p.sigma <= 32 && places < ((int64_t)1 << 24);
    // (reverse-complement mode: the rare symbols' places are listed on one strand only — the marking pass over every
    // window of both strands, k_dense_count<true, ., true>, instead; wildcard mode likewise: the windows around a rare
    // symbol's place may hold a wildcard, which the marking pass knows; centre-weighted mode likewise: the marking pass,
    // whose keys are the counted ones)
    if (p.rc_on || p.wild_on || p.cw_on) c.compact_rare = false;
    c.rare_places = (uint32_t)places;
    return c;
}

// the small side tables of the modes, then words, word starts, lengths and feature starts from the pinned staging: four
// copies on the stream, nothing to wait for
int upload_load(fsk_engine* e, const LoadPlan& p) {
    const size_t N = (size_t)p.N, n_words = (size_t)p.n_words + 4;
    FSK_HIP(e->d_words.reserve(n_words));
    FSK_HIP(e->d_wstart.reserve(N));
    FSK_HIP(e->d_len.reserve(N));
    FSK_HIP(e->d_fstart.reserve(N + 1));
    auto table = [](auto& dev, const auto& host) {  // a whole host vector into its device buffer, waited for
        const hipError_t r = dev.reserve(std::max<size_t>(1, host.size()));
        return r != hipSuccess ? r : hipMemcpy(dev.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
    };
    if (p.rc_on) FSK_HIP(table(e->d_comp, p.comp_rank));
    if (p.wild_on || p.cw_on) FSK_HIP(table(e->d_fwin, p.fwin));
    if (p.cw_on) FSK_HIP(table(e->d_cw, e->cw_profile));
    if (p.wild_on) {
        FSK_HIP(table(e->d_vbits, p.vbits));
        FSK_HIP(table(e->d_vstart, p.vstart));
    }
    const uint32_t* tables = p.staging + n_words;  // [wstart N][len N][fstart N + 1]
    FSK_HIP(hipMemcpyAsync(e->d_words.p, p.staging, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(e->d_wstart.p, tables, N * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(e->d_len.p, tables + N, N * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(e->d_fstart.p, tables + 2 * N, (N + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    e->stage_in_flight = true;
    return FSK_OK;
}

}  // namespace

int fsk_detail::one_load_sequences(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train, int64_t n_test) {
    if (!offsets || n_train <= 0 || n_test < 0) return e->fail(FSK_EINVAL, "need n_train >= 1, n_test >= 0 and offsets");
    FSK_ON_DEVICE(e);
    const int64_t N = n_train + n_test;
    if (N >= ((int64_t)1 << 31)) return e->fail(FSK_EUNSUPPORTED, "more than 2^31 sequences");
    if (offsets[0] < 0) return e->fail(FSK_EINVAL, "offsets[0] must be >= 0");
    if (offsets[N] > offsets[0] && !tokens) return e->fail(FSK_EINVAL, "null tokens");
    if (e->stage_in_flight) {  // the previous call's upload reads the pinned staging this call is about to refill
        FSK_HIP(hipStreamSynchronize(e->stream));
        e->stage_in_flight = false;
    }
    const auto tl0 = std::chrono::steady_clock::now();  // (tuning trace = 1, stderr: where the host time of the load goes)
    const fsk_load::LoadInput in{e->cfg.g, e->k, e->rc_tokens.data(), e->rc_comps.data(), e->rc_tokens.size(), e->wild_tokens.data(), e->wild_tokens.size(),
                                 e->cw_profile.data(), e->cw_profile.size(), tokens, offsets, n_train, n_test};
    LoadPlan plan;
    fsk_load::make_load_plan(in, [e](size_t need) { return grow_stage(e, need); }, plan);
    if (plan.code) return e->fail(plan.code, "%s", plan.msg.c_str());
    int rc = commit_load(e, plan, n_train, n_test);
    if (rc) return rc;
    const Compaction c = choose_compaction(plan, e->tune, e->cfg.g, e->k);
    e->compact = c.compact; e->compact_rare = c.compact_rare; e->rare_mask = c.rare_mask; e->rare_places = c.rare_places;
    rc = upload_load(e, plan);
    if (rc) return rc;
    if (e->d_K && !e->K_owned) {
        if (e->bound_cells != e->pairs) return e->fail(FSK_EINVAL, "bound counts buffer holds %lld cells, need %lld", (long long)e->bound_cells, (long long)e->pairs);
    } else {
        hipError_t r = e->K_store.reserve((size_t)e->pairs);
        if (r != hipSuccess) return e->fail(FSK_ENOMEM, "cannot allocate the %lld-cell integer triangle", (long long)e->pairs);
        e->d_K = e->K_store.p;
        e->K_owned = true;
    }
    if (lazy_zero_possible(e)) {  // (as after fsk_reset_counts: the first tile launch stores its sums)
        e->ld.lazy_lo = 0; e->ld.lazy_hi = N;
    } else {
        FSK_HIP(hipMemsetAsync(e->d_K, 0, (size_t)e->pairs * sizeof(u64), e->stream));
    }
    FSK_HIP(e->d_U.reserve(2));  // [0] update count U (multi-chunk dense launches), [1] remainder row products of the dense tile launches
    FSK_HIP(hipMemsetAsync(e->d_U.p, 0, 2 * sizeof(u64), e->stream));
    e->loaded = true; e->finalized = false; e->result_f64 = false;
    fsk_stats& st = e->st;
    st = fsk_stats{};
    st.n_seq = N; st.n_train = n_train; st.n_test = n_test; st.n_feat = plan.nfeat; st.n_pairs = e->pairs;
    st.alphabet = (int32_t)plan.sigma; st.bits_per_symbol = plan.bits; st.key_space = (int64_t)plan.V; st.path_used = e->path;
    st.n_combos_total = (int32_t)e->ncomb;
    st.max_windows = (double)e->maxW;
    if (e->trace())
        fprintf(stderr, "[fsk] load: %lld tokens, lengths %.3f ms, alphabet + packing %.3f ms, plan + uploads enqueued %.3f ms\n", (long long)plan.total,
                plan.ms_census, plan.ms_pack - plan.ms_census,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count() - plan.ms_pack);
    return FSK_OK;
}

extern "C" {

int fsk_bind_counts(fsk_engine* e, void* device_u64, int64_t n_cells) {
    if (!e) return FSK_EINVAL;
    if (!device_u64 || n_cells <= 0) return e->fail(FSK_EINVAL, "bad counts buffer");
    if (e->loaded && n_cells != e->pairs) return e->fail(FSK_EINVAL, "counts buffer holds %lld cells, need %lld", (long long)n_cells, (long long)e->pairs);
    if (e->ld.lazy_lo >= 0) {
        FSK_ON_DEVICE(e);
        int rcz = materialise_zero(e);
        if (rcz) return rcz;
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    if (e->K_owned) e->K_store.release();
    e->bound_cells = n_cells;
    e->d_K = (u64*)device_u64;
    e->K_owned = false;
    e->finalized = false;
    // a group narrows its exchange to int32 when combos-since-reset x max_windows^2 < 2^31 bounds every cell: the
    // caller's memory holds whatever it holds, so no narrowing until fsk_reset_counts / fsk_load_sequences zero it
    if (e->group) group_note_bound_counts(e);
    return FSK_OK;
}

int fsk_counts_device_ptr(fsk_engine* e, void** out) {
    if (!e || !out) return FSK_EINVAL;
    if (!e->d_K) return e->fail(FSK_ESTATE, "no counts buffer yet");
    *out = e->d_K;
    return FSK_OK;
}

int fsk_reset_counts(fsk_engine* e) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_reset_counts");
    return e->group ? group_reset_counts(e, 0, -1) : one_reset_counts(e);
}

int fsk_reset_counts_rows(fsk_engine* e, int64_t row_begin, int64_t row_end) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_reset_counts_rows");
    if (e->group && (row_begin < 0 || row_end < row_begin)) return e->fail(FSK_EINVAL, "bad row range");
    return e->group ? group_reset_counts(e, row_begin, row_end) : one_reset_counts_rows(e, row_begin, row_end);
}

int fsk_accumulate(fsk_engine* e, const int32_t* combos, int32_t n) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_accumulate");
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (n < 0 || (n > 0 && !combos)) return e->fail(FSK_EINVAL, "bad combo list");
    if (e->group) return group_accumulate(e, combos, n);
    return one_accumulate_rows(e, combos, n, 0, e->N);
}

int fsk_accumulate_rows(fsk_engine* e, const int32_t* combos, int32_t n, int64_t row_begin, int64_t row_end) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_accumulate_rows");
    if (e->group) return e->fail(FSK_ESTATE, "fsk_accumulate_rows is a single-engine call: a group bands its accumulate itself");
    return one_accumulate_rows(e, combos, n, row_begin, row_end);
}

int fsk_synchronize(fsk_engine* e) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_synchronize(e) : one_synchronize(e);
}

// Ordering against a stream of the caller (torch's current stream, which RCCL collectives are
// ordered after) without blocking the host: an event recorded on one stream, waited for by the other
// (one event per direction: a wait captures the record that precedes it).
int fsk_stream_wait_engine(fsk_engine* e, void* hip_stream) {
    if (!e) return FSK_EINVAL;
    FSK_ON_DEVICE(e);
    FSK_HIP(e->ev_out.create(hipEventDisableTiming));
    FSK_HIP(hipEventRecord(e->ev_out, e->stream));
    FSK_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, e->ev_out, 0));
    return FSK_OK;
}

int fsk_engine_wait_stream(fsk_engine* e, void* hip_stream) {
    if (!e) return FSK_EINVAL;
    FSK_ON_DEVICE(e);
    FSK_HIP(e->ev_in.create(hipEventDisableTiming));
    FSK_HIP(hipEventRecord(e->ev_in, (hipStream_t)hip_stream));
    FSK_HIP(hipStreamWaitEvent(e->stream, e->ev_in, 0));
    return FSK_OK;
}

int fsk_finalize(fsk_engine* e) {
    if (!e) return FSK_EINVAL;
    return e->group ? group_finalize(e) : one_finalize(e);
}

int fsk_compute(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train, int64_t n_test) {
    if (!e) return FSK_EINVAL;
    if (e->group) return group_compute(e, tokens, offsets, n_train, n_test);
    FSK_ON_DEVICE(e);
    e->mm_ran_a.clear(); e->mm_ran_path.clear(); e->mm_ran_level_ms.clear(); e->mm_ran_fold_ms.clear();
    if (e->mm_on() && !e->mm_plain) return mismatch_compute(e, tokens, offsets, n_train, n_test);
    int rc = one_load_sequences(e, tokens, offsets, n_train, n_test);
    if (rc) return rc;
    if (e->mm_on()) {  // the weights are this kernel's own (a = e_m): one level, and it is the plain compute below
        e->mm_ran_a = e->mm_a;
        e->mm_ran_path.assign(e->mm_a.size(), 0);
        e->mm_ran_path.back() = e->path;
        e->mm_ran_level_ms.assign(e->mm_a.size(), 0.0);
        e->mm_ran_fold_ms.assign(e->mm_a.size(), 0.0);
    }
    const fsk_config& c = e->cfg;
    if (!c.approx) {  // exact: every combination, order irrelevant (integer sum)
        std::vector<int32_t> all((size_t)e->ncomb);
        for (int64_t i = 0; i < e->ncomb; ++i) all[i] = (int32_t)i;
        rc = do_accumulate(e, all.data(), (int)all.size(), e->d_K);
        if (rc) return rc;
        return make_diag(e);
    }
    if (!e->order_set) default_order(e);
    if (c.skip_variance) {  // chains only select which combos enter the integer sum
        std::vector<int32_t> used;
        skip_variance_combos(e, used);
        rc = do_accumulate(e, used.data(), (int)used.size(), e->d_K);
        if (rc) return rc;
        return make_diag(e);
    }
    rc = run_variance_mode(e, approx_chains(e));
    if (rc) return rc;
    return make_diag(e);
}

int fsk_run_chains(fsk_engine* e, int32_t first, int32_t step) {
    if (!e) return FSK_EINVAL;
    FSK_NOT_STAGED(e, "fsk_run_chains");
    if (e->group) return e->fail(FSK_ESTATE, "fsk_run_chains is a single-engine call: a group deals its chains itself (fsk_compute)");
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    const fsk_config& c = e->cfg;
    if (!c.approx || c.skip_variance) return e->fail(FSK_ESTATE, "fsk_run_chains is the variance mode (approx=1, skip_variance=0)");
    if (first < 0 || step < 1) return e->fail(FSK_EINVAL, "need first >= 0 and step >= 1");
    FSK_ON_DEVICE(e);
    if (!e->order_set) default_order(e);
    e->finalized = false;
    return run_variance_mode(e, approx_chains(e), first, step);
}

}  // extern "C"

namespace fsk_detail {

int approx_chains(const fsk_engine* e) {
    const int T = e->cfg.t == -1 ? 20 : e->cfg.t;  // fastsk_kernel.cpp:54-61
    return std::max(1, std::min<int>(T, (int)e->order.size()));
}

void skip_variance_combos(fsk_engine* e, std::vector<int32_t>& used) {
    const int T = approx_chains(e);
    used.clear();
    for (int tid = 0; tid < T; ++tid) {
        int iters = 0;
        for (size_t item = tid; item < e->order.size(); item += T) {
            used.push_back(e->order[item]);
            if (e->cfg.max_iters != -1 && ++iters >= e->cfg.max_iters) break;
        }
    }
}

int one_reset_counts(fsk_engine* e) {
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    FSK_ON_DEVICE(e);
    if (lazy_zero_possible(e)) {
        e->ld.lazy_lo = 0; e->ld.lazy_hi = e->N;  // (whatever was pending is covered by this range)
    } else {
        e->ld.lazy_lo = e->ld.lazy_hi = -1;
        FSK_HIP(hipMemsetAsync(e->d_K, 0, (size_t)e->pairs * sizeof(u64), e->stream));
    }
    e->finalized = false; e->result_f64 = false;
    e->st.combos_done = 0;
    e->ld.prep_valid = false;  // a new pass recounts its panels even when its first band starts at row > 0
    return FSK_OK;
}

int one_reset_counts_rows(fsk_engine* e, int64_t row_begin, int64_t row_end) {
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (row_begin < 0 || row_end > e->N || row_begin > row_end) return e->fail(FSK_EINVAL, "bad row range");
    FSK_ON_DEVICE(e);
    const u64 c0 = (u64)row_begin * ((u64)row_begin + 1) / 2, c1 = (u64)row_end * ((u64)row_end + 1) / 2;
    { int rcz = materialise_zero(e); if (rcz) return rcz; }  // an earlier, different reset
    if (lazy_zero_possible(e) && row_begin % fsk::TILE == 0 && row_end > row_begin) {
        e->ld.lazy_lo = row_begin; e->ld.lazy_hi = row_end;
    } else if (c1 > c0) {
        FSK_HIP(hipMemsetAsync(e->d_K + c0, 0, (size_t)(c1 - c0) * sizeof(u64), e->stream));
    }
    e->finalized = false; e->result_f64 = false;
    e->st.combos_done = 0;
    e->ld.prep_valid = false;
    return FSK_OK;
}

int one_accumulate_rows(fsk_engine* e, const int32_t* combos, int32_t n, int64_t row_begin, int64_t row_end) {
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (n < 0 || (n > 0 && !combos)) return e->fail(FSK_EINVAL, "bad combo list");
    if (row_begin < 0 || row_end > e->N || row_begin > row_end || row_begin % fsk::TILE != 0 ||
        (row_end % fsk::TILE != 0 && row_end != e->N))
        return e->fail(FSK_EINVAL, "row band must be [a,b) with a, b multiples of %d (b may be N)", fsk::TILE);
    if (row_begin == row_end) return FSK_OK;
    FSK_ON_DEVICE(e);
    if (n == 0) {
        // Nothing to add — but rows that a reset left to a storing launch get their zeros now: the caller
        // may hand these rows to another stream next (fsk_stream_wait_engine), e.g. a rank of a job with
        // more ranks than combos, whose share of the all-reduce must be zeros, not the previous pass.
        return materialise_zero(e);
    }
    e->finalized = false;
    return do_accumulate(e, combos, n, e->d_K, row_begin, row_end);
}

int one_synchronize(fsk_engine* e) {
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    return FSK_OK;
}

int one_finalize(fsk_engine* e) {
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    return make_diag(e);
}

}  // namespace fsk_detail

extern "C" {

int fsk_get_kernel_sum_device(fsk_engine* e, double* device_out) {
    if (!e) return FSK_EINVAL;
    if (!e->loaded || !e->result_f64) return e->fail(FSK_ESTATE, "no Welford chains have run");
    if (!device_out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    FSK_HIP(hipMemcpyAsync(device_out, e->d_Kf64.p, (size_t)e->pairs * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_set_kernel_sum_device(fsk_engine* e, const double* device_in) {
    if (!e) return FSK_EINVAL;
    if (!e->loaded || !e->result_f64) return e->fail(FSK_ESTATE, "no Welford chains have run");
    if (!device_in) return e->fail(FSK_EINVAL, "null input");
    FSK_ON_DEVICE(e);
    FSK_HIP(hipMemcpyAsync(e->d_Kf64.p, device_in, (size_t)e->pairs * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    e->finalized = false;
    return FSK_OK;
}

int fsk_get_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double* out) {
    if (!e) return FSK_EINVAL;
    FSK_ON_DEVICE(e);
    return fetch_block(e, i0, i1, j0, j1, out);
}
int fsk_get_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double* device_out) {
    if (!e) return FSK_EINVAL;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (i0 < 0 || j0 < 0 || i1 > e->N || j1 > e->N || i0 > i1 || j0 > j1) return e->fail(FSK_EINVAL, "block out of range");
    const u64 rows = (u64)(i1 - i0), cols = (u64)(j1 - j0);
    if (rows == 0 || cols == 0) return FSK_OK;
    if (!device_out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const u64 max_cells = (u64)1 << 31;  // grid.x limit: launch in row chunks
    const u64 rows_per = std::max<u64>(1, std::min<u64>(rows, max_cells / cols));
    for (u64 r = 0; r < rows; r += rows_per) {
        const u64 nr = std::min(rows_per, rows - r), cells = nr * cols;
        const uint32_t blocks = (uint32_t)((cells + 255) / 256);
        if (e->result_f64)
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_block<double>), dim3(blocks), dim3(256), 0, e->stream, e->d_Kf64.p, e->d_diag.p,
                       (u64)i0 + r, nr, (u64)j0, cols, device_out + r * cols);
        else
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_block<u64>), dim3(blocks), dim3(256), 0, e->stream, e->d_K, e->d_diag.p,
                       (u64)i0 + r, nr, (u64)j0, cols, device_out + r * cols);
    }
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_get_train(fsk_engine* e, double* out) {
    if (!e) return FSK_EINVAL;
    FSK_ON_DEVICE(e);
    return fetch_block(e, 0, e->n_train, 0, e->n_train, out);
}
int fsk_get_test(fsk_engine* e, double* out) {
    if (!e) return FSK_EINVAL;
    FSK_ON_DEVICE(e);
    return fetch_block(e, e->n_train, e->N, 0, e->n_train, out);
}

}  // extern "C"

// cells [c0, c0 + cnt) of the normalised triangle into device memory at `dst` (dst[0] = cell c0); fsk_engine_rows.hip fills
// its scratch with it
int fsk_detail::launch_triangle(fsk_engine* e, u64 c0, u64 cnt, double* dst) {
    const u64 per_block = (u64)256 * fsk::TR_ITEMS;
    const uint32_t blocks = (uint32_t)((cnt + per_block - 1) / per_block);
    if (e->result_f64)
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_triangle<double>), dim3(blocks), dim3(256), 0, e->stream, e->d_Kf64.p, e->d_diag.p, c0, cnt, dst);
    else
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_triangle<u64>), dim3(blocks), dim3(256), 0, e->stream, e->d_K, e->d_diag.p, c0, cnt, dst);
    return FSK_OK;
}

extern "C" {

int fsk_get_triangle(fsk_engine* e, double* out) {
    if (!e) return FSK_EINVAL;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel");
    if (!out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const u64 chunk = (u64)32 << 20;
    FSK_HIP(e->d_stage.reserve((size_t)std::min<u64>(chunk, (u64)e->pairs)));
    for (u64 c0 = 0; c0 < (u64)e->pairs; c0 += chunk) {
        const u64 cnt = std::min<u64>(chunk, (u64)e->pairs - c0);
        { int rc = launch_triangle(e, c0, cnt, e->d_stage.p); if (rc) return rc; }
        FSK_HIP(hipMemcpyAsync(out + c0, e->d_stage.p, cnt * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    return FSK_OK;
}

int fsk_get_triangle_device(fsk_engine* e, double* device_out) {
    if (!e) return FSK_EINVAL;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (!device_out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const u64 chunk = (u64)1 << 33;  // (grid.x stays far below its limit)
    for (u64 c0 = 0; c0 < (u64)e->pairs; c0 += chunk) {
        const int rc = launch_triangle(e, c0, std::min<u64>(chunk, (u64)e->pairs - c0), device_out + c0);
        if (rc) return rc;
    }
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_alloc_triangle_device(fsk_engine* e, double** device_out) {
    if (!e || !device_out) return FSK_EINVAL;
    *device_out = nullptr;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    FSK_ON_DEVICE(e);
    DevBuf<double> block;  // (the caller's from the moment it is handed out: fsk_free_device)
    if (block.reserve((size_t)e->pairs) != hipSuccess) {
        (void)hipGetLastError();
        return e->fail(FSK_ENOMEM, "cannot allocate the %lld-cell normalised triangle (%.1f GB) on device %d", (long long)e->pairs,
                       (double)e->pairs * 8e-9, e->cfg.device);
    }
    const int rc = fsk_get_triangle_device(e, block.p);
    if (rc) return rc;
    *device_out = block.p;
    block.p = nullptr;
    return FSK_OK;
}

int fsk_get_counts(fsk_engine* e, uint64_t* out) {
    if (!e) return FSK_EINVAL;
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (e->result_f64) return e->fail(FSK_ESTATE, "variance mode keeps a floating-point mean, not integer counts");
    if (!out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipMemcpy(out, e->d_K, (size_t)e->pairs * sizeof(u64), hipMemcpyDeviceToHost));
    return FSK_OK;
}

int fsk_get_counts_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint64_t* out) {
    if (!e) return FSK_EINVAL;
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (e->result_f64) return e->fail(FSK_ESTATE, "variance mode keeps a floating-point mean, not integer counts");
    if (i0 < 0 || j0 < 0 || i1 > e->N || j1 > e->N || i0 > i1 || j0 > j1) return e->fail(FSK_EINVAL, "block out of range");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const int64_t rows = i1 - i0, cols = j1 - j0;
    if (rows == 0 || cols == 0) return FSK_OK;
    if (!out) return e->fail(FSK_EINVAL, "null output");
    const int64_t max_cells = (int64_t)32 << 20;
    const int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(rows, max_cells / cols));
    FSK_HIP(e->d_stage_u64.reserve((size_t)(rows_per * cols)));
    for (int64_t r = 0; r < rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, rows - r);
        const u64 cells = (u64)nr * cols;
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_block_raw<u64>), dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, e->stream, e->d_K,
                   (u64)(i0 + r), (u64)nr, (u64)j0, (u64)cols, e->d_stage_u64.p);
        FSK_HIP(hipMemcpyAsync(out + r * cols, e->d_stage_u64.p, cells * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    return FSK_OK;
}

int fsk_get_counts_cells(fsk_engine* e, const int64_t* rows, const int64_t* cols, int64_t n, uint64_t* out) {
    if (!e) return FSK_EINVAL;
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (e->result_f64) return e->fail(FSK_ESTATE, "variance mode keeps a floating-point mean, not integer counts");
    if (n < 0 || (n > 0 && (!rows || !cols || !out))) return e->fail(FSK_EINVAL, "bad cell list");
    for (int64_t q = 0; q < n; ++q)
        if (rows[q] < 0 || rows[q] >= e->N || cols[q] < 0 || cols[q] >= e->N) return e->fail(FSK_EINVAL, "cell (%lld, %lld) out of range", (long long)rows[q], (long long)cols[q]);
    if (n == 0) return FSK_OK;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const int64_t chunk = (int64_t)16 << 20;
    FSK_HIP(e->d_cell_idx.reserve((size_t)std::min(n, chunk) * 2));
    FSK_HIP(e->d_stage_u64.reserve((size_t)std::min(n, chunk)));
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cnt = std::min(chunk, n - c0);
        FSK_HIP(hipMemcpyAsync(e->d_cell_idx.p, rows + c0, (size_t)cnt * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
        FSK_HIP(hipMemcpyAsync(e->d_cell_idx.p + cnt, cols + c0, (size_t)cnt * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
        FSK_LAUNCH(fsk::k_cells_raw, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, e->stream, e->d_K, (const int64_t*)e->d_cell_idx.p,
                   (const int64_t*)(e->d_cell_idx.p + cnt), (u64)cnt, e->d_stage_u64.p);
        FSK_HIP(hipMemcpyAsync(out + c0, e->d_stage_u64.p, (size_t)cnt * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    return FSK_OK;
}

int fsk_get_stdevs(fsk_engine* e, double* out, int32_t cap, int32_t* n) {
    if (!e || !n) return FSK_EINVAL;
    *n = (int32_t)e->ld.stdevs.size();
    for (int32_t i = 0; i < *n && i < cap && out; ++i) out[i] = e->ld.stdevs[i];
    return FSK_OK;
}

int fsk_save_kernel(fsk_engine* e, const char* path) {
    if (!e) return FSK_EINVAL;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel");
    if (!path || !*path) return FSK_OK;  // the reference silently does nothing for an empty name
    FILE* f = fopen(path, "w");
    if (!f) return e->fail(FSK_EINVAL, "cannot open %s", path);
    std::vector<double> row((size_t)e->N);
    for (int64_t i = 0; i < e->N; ++i) {
        int rc = fsk_get_block(e, i, i + 1, 0, e->N, row.data());
        if (rc) { fclose(f); return rc; }
        for (int64_t j = 0; j < e->N; ++j) fprintf(f, "%d:%e ", (int)(j + 1), row[(size_t)j]);
        fprintf(f, "\n");
    }
    fclose(f);
    return FSK_OK;
}

int fsk_get_stats(fsk_engine* e, fsk_stats* out) {
    if (!e || !out) return FSK_EINVAL;
    return e->group ? group_get_stats(e, out) : one_get_stats(e, out);
}

int fsk_counts_digest(fsk_engine* e, int64_t row_begin, int64_t row_end, uint64_t out[2]) {
    if (!e || !out) return FSK_EINVAL;
    if (!e->loaded) return e->fail(FSK_ESTATE, "load sequences first");
    if (e->result_f64) return e->fail(FSK_ESTATE, "variance mode keeps a floating-point mean, not integer counts");
    if (row_begin < 0 || row_end > e->N || row_begin > row_end) return e->fail(FSK_EINVAL, "bad row range");
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    const u64 c0 = (u64)row_begin * ((u64)row_begin + 1) / 2, c1 = (u64)row_end * ((u64)row_end + 1) / 2;
    FSK_HIP(e->d_stage_u64.reserve(2));
    FSK_HIP(hipMemsetAsync(e->d_stage_u64.p, 0, 2 * sizeof(u64), e->stream));
    if (c1 > c0) {
        const u64 per_block = (u64)256 * fsk::DG_ITEMS;
        const uint32_t blocks = (uint32_t)std::min<u64>((c1 - c0 + per_block - 1) / per_block, (u64)1 << 16);
        FSK_LAUNCH(fsk::k_digest, dim3(blocks), dim3(256), 0, e->stream, (const u64*)e->d_K, c0, c1 - c0, e->d_stage_u64.p);
    }
    FSK_HIP(hipMemcpyAsync(out, e->d_stage_u64.p, 2 * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_alloc_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double** device_out) {
    if (!e || !device_out) return FSK_EINVAL;
    *device_out = nullptr;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (i0 < 0 || j0 < 0 || i1 > e->N || j1 > e->N || i0 > i1 || j0 > j1) return e->fail(FSK_EINVAL, "block out of range");
    FSK_ON_DEVICE(e);
    const size_t cells = (size_t)(i1 - i0) * (size_t)(j1 - j0);
    DevBuf<double> block;  // (the caller's from the moment it is handed out: fsk_free_device)
    if (block.reserve(std::max<size_t>(1, cells)) != hipSuccess)
        return e->fail(FSK_ENOMEM, "cannot allocate a %lld x %lld block on device %d", (long long)(i1 - i0), (long long)(j1 - j0), e->cfg.device);
    const int rc = fsk_get_block_device(e, i0, i1, j0, j1, block.p);
    if (rc) return rc;
    *device_out = block.p;
    block.p = nullptr;
    return FSK_OK;
}

int fsk_free_device(fsk_engine* e, void* device_ptr) {
    if (!device_ptr) return FSK_OK;
    if (!e) return hipFree(device_ptr) == hipSuccess ? FSK_OK : FSK_EDEVICE;  // (the engine may be gone before its block)
    FSK_ON_DEVICE(e);
    FSK_HIP(hipFree(device_ptr));
    return FSK_OK;
}

}  // extern "C"

int fsk_detail::one_get_stats(fsk_engine* e, fsk_stats* out) {
    u64 rem_rows = 0;
    if (e->d_U.p && e->loaded) {
        DeviceScope on_device(e->cfg.device);
        u64 U[2] = {0, 0};
        e->harvest_times();
        if (hipStreamSynchronize(e->stream) == hipSuccess && fetch_pending_u(e) == FSK_OK &&
            hipMemcpy(U, e->d_U.p, sizeof U, hipMemcpyDeviceToHost) == hipSuccess) {
            e->st.cell_updates = U[0] + e->ld.u_extra;
            rem_rows = U[1];
        }
    }
    e->st.batches_redone = (double)e->sx_redone;
    e->st.sparse_form = (double)e->ld.sx_form_used;
    e->st.sparse_passes = (double)e->ld.sx_passes;
    e->st.sparse_desc = e->ld.sx_desc_used ? 1.0 : 0.0;
    e->st.share_positions = (double)e->ld.sx_share_used;
    e->st.share_groups = (double)e->ld.sx_share_groups;
    *out = e->st;
    // (every flagged-row remainder product is one more dot8 per cell of its tile: 8 count-MACs x 128 x 128)
    out->dense_macs += rem_rows * (u64)fsk::TILE * fsk::TILE * 8;
    return FSK_OK;
}

extern "C" int fsk_set_skip_test_block(fsk_engine* e, int32_t skip) {
    if (!e) return FSK_EINVAL;
    if (e->group) return fsk_detail::group_set_skip_test_block(e, skip);
    e->cfg.skip_test_block = skip ? 1 : 0;
    e->tab_n = 0;  // (the tile table leaves out test x test tiles)
    return FSK_OK;
}

// ---- tuning through the ABI (include/fastsk_amd.h)
extern "C" int fsk_set_tuning(fsk_engine* e, const char* key, int64_t value) {
    if (!e) return FSK_EINVAL;
    std::string why;
    // (a group: every engine runs with the same tuning; the group's own keys are read from engine 0 by fsk_multi.hip)
    const int rc = e->group ? fsk_detail::group_set_tuning(e, key, value, why) : fsk_detail::tuning_set(e->tune, key, value, why);
    if (rc) return e->fail(rc, "%s", why.c_str());
    {   // the profile key: 0 .. 2 from here on, -1 = as the engine was created (a group: every engine)
        const int want = e->tune.profile >= 0 ? (int)e->tune.profile : e->cfg_profile0;
        if (e->group) fsk_detail::group_set_profile(e, want);
        else if (want != e->cfg.profile) { e->harvest_times(); e->cfg.profile = want; }
    }
    if (e->trace()) fprintf(stderr, "[fsk] tuning: %s\n", fsk_detail::tuning_in_force(e->tune).c_str());
    return FSK_OK;
}

extern "C" int fsk_get_tuning(fsk_engine* e, const char* key, int64_t* value) {
    if (!e || !key || !value) return FSK_EINVAL;
    for (const TuneKey& k : TUNE_KEYS)
        if (!strcmp(k.name, key)) { *value = e->tune.*(k.field); return FSK_OK; }
    return e->fail(FSK_EINVAL, "unknown tuning key '%s'", key);
}

extern "C" const char* fsk_tuning_keys(void) {
    static const std::string text = [] {
        std::string t;
        for (const TuneKey& k : TUNE_KEYS)
            t += std::string(k.name) + "=" + std::to_string(k.def) + " [" + std::to_string(k.lo) + ".." + std::to_string(k.hi) + "] " + k.doc + "\n";
        return t;
    }();
    return text.c_str();
}

// =============================================================================================
// MISMATCH-WEIGHTED KERNELS (fsk_set_mismatch_weights): W = sum_h c_h N_h as sum_j a_j S_j over the raw triangles S_j of the
// levels (g, m = j), each run by an engine of its own into one scratch triangle and folded into K by k_tri_fold.
namespace fsk_detail {

namespace {
typedef __int128 i128;
// C(n, k) exactly, or false when it passes 2^126
bool binom_i128(int n, int k, i128* out) {
    if (k < 0 || k > n) { *out = 0; return true; }
    if (k * 2 > n) k = n - k;
    u128 r = 1;
    const u128 limit = (u128)1 << 126;
    for (int i = 1; i <= k; ++i) {
        const u128 f = (u128)(n - k + i);
        if (r > limit / f) return false;
        r = r * f / (u128)i;
    }
    *out = (i128)r;
    return true;
}
}  // namespace

int mismatch_solve(int g, const uint64_t* c, int n, std::vector<int64_t>& a, std::string& why) {
    a.clear();
    if (g <= 0 || g > 255 || !c || n < 1 || n > g) { why = "mismatch weights: need 1 <= n <= g <= 255 weights"; return FSK_EINVAL; }
    if (c[0] < 1) { why = "mismatch weights: c[0] must be at least 1 (it keeps every diagonal positive)"; return FSK_EINVAL; }
    int d = n - 1;
    while (d > 0 && c[d] == 0) --d;
    a.assign((size_t)d + 1, 0);
    const i128 lo = (i128)INT64_MIN, hi = (i128)INT64_MAX;
    for (int h = d; h >= 0; --h) {
        i128 v = (i128)c[h];
        for (int j = h + 1; j <= d; ++j) {
            if (a[(size_t)j] == 0) continue;
            i128 b = 0, term = 0;
            // (128-bit intermediates; a product or a sum that leaves them is reported like a coefficient that leaves int64)
            if (!binom_i128(g - h, j - h, &b) || __builtin_mul_overflow((i128)a[(size_t)j], b, &term) || __builtin_sub_overflow(v, term, &v)) {
                why = "mismatch weights: the coefficient of level " + std::to_string(h) + " does not fit 64 bits";
                a.clear();
                return FSK_EINVAL;
            }
        }
        if (v < lo || v > hi) {
            why = "mismatch weights: the coefficient of level " + std::to_string(h) + " does not fit 64 bits";
            a.clear();
            return FSK_EINVAL;
        }
        a[(size_t)h] = (int64_t)v;
    }
    return FSK_OK;
}

// K = (first ? 0 : K) + a * S over the whole triangle, on the engine's stream; HIP-event milliseconds into *ms
static int fold_level(fsk_engine* e, int64_t a, bool first, double* ms) {
    const u64 n = (u64)e->pairs;
    const bool vec = ((uintptr_t)e->d_K % 16 == 0) && ((uintptr_t)e->mm_scratch.p % 16 == 0);
    const u64 n2 = vec ? n / 2 : 0;
    const u64 work = std::max<u64>(std::max<u64>(n2, n - 2 * n2), 1);
    const uint32_t blocks = (uint32_t)std::min<u64>((work + 255) / 256, (u64)e->n_cu * 8);  // (a streaming pass: eight workgroups a compute unit, grid-stride beyond)
    FSK_HIP(hipEventRecord(e->ev0, e->stream));
    FSK_LAUNCH(fsk::k_tri_fold, dim3(blocks), dim3(256), 0, e->stream, e->d_K, (const u64*)e->mm_scratch.p, (u64)a, n2, n, first ? 1 : 0);
    FSK_HIP(hipEventRecord(e->ev1, e->stream));
    FSK_HIP(hipEventSynchronize(e->ev1));  // (the next level overwrites the scratch triangle from another stream)
    FSK_HIP(hipGetLastError());
    float t = 0;
    (void)hipEventElapsedTime(&t, e->ev0, e->ev1);
    *ms = (double)t;
    e->st.launches += 1;
    return FSK_OK;
}

int mismatch_compute(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train, int64_t n_test) {
    int rc = one_load_sequences(e, tokens, offsets, n_train, n_test);
    if (rc) return rc;
    e->ld.lazy_lo = e->ld.lazy_hi = -1;  // (the first fold stores every cell: no zeros are owed)
    const int g = e->cfg.g, d = (int)e->mm_a.size() - 1;
    // a failure from here on leaves the handle as it was before any sequences were loaded
    auto give_up = [&](int code) { e->loaded = false; e->finalized = false; return code; };
    for (int j = 0; j <= d; ++j) {  // a level's k-mer must fit the sort records (fsk_load_sequences' rule, at k = g - j)
        if (e->mm_a[(size_t)j] == 0) continue;
        u64 V = 1;
        bool wide = false;
        for (int q = 0; q < g - j; ++q) {
            if (V > (((u64)1 << 62) / e->sigma)) { wide = true; break; }
            V *= e->sigma;
        }
        int symbits = 1;
        while (((u64)1 << symbits) < e->sigma) ++symbits;
        if (wide && (int64_t)symbits * (g - j) > 96)
            return give_up(e->fail(FSK_EUNSUPPORTED, "mismatch-weighted mode, level %d: a k-mer of %d symbols of %d bits does not fit the 128-bit sort records", j,
                                   g - j, symbits));
    }
    {
        const uint64_t cmax = *std::max_element(e->mm_c.begin(), e->mm_c.end());
        if ((u128)cmax * (u128)e->maxW * (u128)e->maxW >= ((u128)1 << 64))
            return give_up(e->fail(FSK_EUNSUPPORTED, "mismatch-weighted mode: largest weight %llu x max_windows^2 = %u^2 reaches 2^64: the sums would not be exact",
                                   (unsigned long long)cmax, e->maxW));
    }
    if (e->mm_scratch.reserve((size_t)e->pairs) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(e->fail(FSK_ENOMEM, "mismatch-weighted mode: cannot allocate the %lld-cell scratch triangle", (long long)e->pairs));
    }
    e->mm_ran_a = e->mm_a;
    e->mm_ran_path.assign((size_t)d + 1, 0);
    e->mm_ran_level_ms.assign((size_t)d + 1, 0.0);
    e->mm_ran_fold_ms.assign((size_t)d + 1, 0.0);
    fsk_stats sum{};
    bool first = true;
    for (int step = 0; step <= d; ++step) {
        const int j = e->tune.mismatch_order ? d - step : step;
        const int64_t a = e->mm_a[(size_t)j];
        if (a == 0) continue;
        const auto t0 = std::chrono::steady_clock::now();
        // the level (g, m = j): an engine of its own on this device, bound to the scratch triangle, gone before the next one
        fsk_config cfg = e->cfg;
        cfg.m = j;
        cfg.approx = 0;
        fsk_engine* lv = nullptr;
        rc = fsk_create(&cfg, &lv);
        if (rc) return give_up(e->fail(rc, "mismatch-weighted mode, level %d: %s", j, fsk_last_error(nullptr)));
        lv->tune = e->tune;
        lv->cfg.profile = e->cfg.profile;
        lv->cfg_profile0 = e->cfg_profile0;
        lv->rc_tokens = e->rc_tokens;
        lv->rc_comps = e->rc_comps;
        lv->wild_tokens = e->wild_tokens;
        lv->cw_profile = e->cw_profile;
        rc = fsk_bind_counts(lv, e->mm_scratch.p, e->pairs);
        if (!rc) rc = one_load_sequences(lv, tokens, offsets, n_train, n_test);  // (zeroes the bound triangle, or owes the zeros to the first tile launch)
        if (!rc) {
            std::vector<int32_t> all((size_t)lv->ncomb);
            for (int64_t i = 0; i < lv->ncomb; ++i) all[(size_t)i] = (int32_t)i;
            rc = do_accumulate(lv, all.data(), (int)all.size(), lv->d_K);
        }
        if (!rc) rc = one_synchronize(lv);
        fsk_stats ls{};
        if (!rc) rc = one_get_stats(lv, &ls);
        if (rc) {
            const std::string why = lv->err;
            one_destroy(lv);
            return give_up(e->fail(rc, "mismatch-weighted mode, level %d (g = %d, m = %d): %s", j, g, j, why.c_str()));
        }
        e->mm_ran_path[(size_t)j] = lv->path;
        one_destroy(lv);
        sum.launches += ls.launches; sum.combos_done += ls.combos_done; sum.combos_issued += ls.combos_issued;
        sum.cell_updates += ls.cell_updates; sum.sort_records += ls.sort_records; sum.sort_passes = std::max(sum.sort_passes, ls.sort_passes);
        sum.ms_count += ls.ms_count; sum.ms_tile += ls.ms_tile; sum.ms_extract += ls.ms_extract; sum.ms_sort += ls.ms_sort;
        sum.ms_segment += ls.ms_segment; sum.ms_pairs += ls.ms_pairs; sum.ms_total += ls.ms_total;
        sum.n_tile_launches += ls.n_tile_launches; sum.dense_macs += ls.dense_macs; sum.panel_bytes += ls.panel_bytes;
        sum.u4_tile_launches += ls.u4_tile_launches; sum.count_launches += ls.count_launches; sum.batches_redone += ls.batches_redone;
        e->mm_ran_level_ms[(size_t)j] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        rc = fold_level(e, a, first, &e->mm_ran_fold_ms[(size_t)j]);
        if (rc) return give_up(rc);
        first = false;
    }
    // what the levels did, summed, in the statistics of this handle
    fsk_stats& st = e->st;
    st.launches += sum.launches; st.combos_done = sum.combos_done; st.combos_issued = sum.combos_issued;
    st.sort_records = sum.sort_records; st.sort_passes = sum.sort_passes;
    st.ms_count = sum.ms_count; st.ms_tile = sum.ms_tile; st.ms_extract = sum.ms_extract; st.ms_sort = sum.ms_sort;
    st.ms_segment = sum.ms_segment; st.ms_pairs = sum.ms_pairs; st.ms_total = sum.ms_total;
    st.n_tile_launches = sum.n_tile_launches; st.dense_macs = sum.dense_macs; st.panel_bytes = sum.panel_bytes;
    st.u4_tile_launches = sum.u4_tile_launches; st.count_launches = sum.count_launches;
    e->ld.u_extra = sum.cell_updates;
    return make_diag(e);
}

}  // namespace fsk_detail

extern "C" {

int fsk_mismatch_levels(int32_t g, const uint64_t* c, int32_t n, int64_t* a, int32_t* n_levels) {
    if (!a || !n_levels) return FSK_EINVAL;
    std::vector<int64_t> av;
    std::string why;
    const int rc = fsk_detail::mismatch_solve(g, c, n, av, why);
    if (rc) { g_create_error = why; return rc; }
    for (size_t j = 0; j < av.size(); ++j) a[j] = av[j];
    *n_levels = (int32_t)av.size();
    return FSK_OK;
}

int fsk_set_mismatch_weights(fsk_engine* e, const uint64_t* c, int32_t n) {
    if (!e) return FSK_EINVAL;
    if (e->group) return e->fail(FSK_EUNSUPPORTED, "mismatch weights on a group handle (fsk_create_multi) are not supported");
    if (n == 0) { e->mm_c.clear(); e->mm_a.clear(); e->mm_plain = false; return FSK_OK; }
    if (e->cfg.approx) return e->fail(FSK_EUNSUPPORTED, "mismatch weights with approx = 1: a sample of combinations under signed level coefficients estimates nothing");
    if (n != e->cfg.m + 1 || !c) return e->fail(FSK_EINVAL, "mismatch weights: need m + 1 = %d weights, got %d", e->cfg.m + 1, n);
    std::vector<int64_t> a;
    std::string why;
    const int rc = mismatch_solve(e->cfg.g, c, n, a, why);
    if (rc) return e->fail(rc, "%s", why.c_str());
    e->mm_c.assign(c, c + n);
    e->mm_a = a;
    e->mm_plain = (int)a.size() == n && a.back() == 1;
    for (size_t j = 0; j + 1 < a.size(); ++j) e->mm_plain = e->mm_plain && a[j] == 0;
    return FSK_OK;
}

int fsk_get_mismatch_info(fsk_engine* e, int32_t* n_levels, int64_t* a, int32_t* paths, int32_t cap) {
    if (!e || !n_levels) return FSK_EINVAL;
    *n_levels = (int32_t)e->mm_ran_a.size();
    for (int32_t j = 0; j < *n_levels && j < cap; ++j) {
        if (a) a[j] = e->mm_ran_a[(size_t)j];
        if (paths) paths[j] = e->mm_ran_path[(size_t)j];
    }
    return FSK_OK;
}

int fsk_get_mismatch_times(fsk_engine* e, double* level_ms, double* fold_ms, int32_t cap) {
    if (!e) return FSK_EINVAL;
    for (int32_t j = 0; j < (int32_t)e->mm_ran_a.size() && j < cap; ++j) {
        if (level_ms) level_ms[j] = e->mm_ran_level_ms[(size_t)j];
        if (fold_ms) fold_ms[j] = e->mm_ran_fold_ms[(size_t)j];
    }
    return FSK_OK;
}

}  // extern "C"

#ifdef FSK_TEST_HOOKS
// ---- test builds only (tests/hooks, the CPU emulation; never the product): the hand-written wave primitives of fsk_gfx950.h,
// one call each per element, for a direct comparison with their definitions (tests/test_gpu_parity.py::test_wave_primitives) —
// the emulator replaces them with shuffle loops, so the kernels' own tests never run the inline asm on the CPU.
namespace fsk {
__global__ __launch_bounds__(256) void k_test_wave_ops(const int32_t* in, const uint32_t* aux, int32_t n, int32_t* out_max, uint32_t* out_sum,
                                                       u64* out_sum64, uint32_t* out_xnor, int32_t* out_sbfe, uint32_t* out_mbcnt) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    const int32_t v = i < n ? in[i] : 0;  // (whole waves call the primitives: n is a multiple of 64)
    const uint32_t a = i < n ? aux[i] : 0u;
    const int32_t mx = fsk_hw::wave_incl_max_i32(v);
    const uint32_t sm = fsk_hw::wave_incl_sum_u32((uint32_t)v & 0xffffu);
    const u64 s64 = fsk_hw::wave_incl_sum_u64(((u64)a << 20) | ((uint32_t)v & 0xfffffu));
    const uint32_t xn = fsk_hw::and_xnor((uint32_t)v, a, a * 2654435761u);
    const int32_t sb = fsk_hw::sbfe1((uint32_t)v, (int)(a & 31u));
    const unsigned long long bal = __ballot((a & 1u) != 0u);
    const uint32_t mb = fsk_mbcnt((uint32_t)bal, (uint32_t)(bal >> 32));
    if (i < n) { out_max[i] = mx; out_sum[i] = sm; out_sum64[i] = s64; out_xnor[i] = xn; out_sbfe[i] = sb; out_mbcnt[i] = mb; }
}
}  // namespace fsk
extern "C" int fsk_test_wave_ops(const int32_t* in, const uint32_t* aux, int32_t n, int32_t* out_max, uint32_t* out_sum, unsigned long long* out_sum64,
                                 uint32_t* out_xnor, int32_t* out_sbfe, uint32_t* out_mbcnt) {
    if (n <= 0 || n % 64) return FSK_EINVAL;
    DevBuf<unsigned char> buf[8];
    void* d[8] = {nullptr};
    const size_t sz[8] = {4, 4, 4, 4, 8, 4, 4, 4};
    bool ok = true;
    for (int q = 0; q < 8 && ok; ++q) { ok = buf[q].reserve(sz[q] * (size_t)n) == hipSuccess; d[q] = buf[q].p; }
    if (ok) ok = hipMemcpy(d[0], in, 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d[1], aux, 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        FSK_LAUNCH(fsk::k_test_wave_ops, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t) nullptr, (const int32_t*)d[0], (const uint32_t*)d[1], n,
                   (int32_t*)d[2], (uint32_t*)d[3], (u64*)d[4], (uint32_t*)d[5], (int32_t*)d[6], (uint32_t*)d[7]);
        ok = hipDeviceSynchronize() == hipSuccess;
    }
    void* host[8] = {nullptr, nullptr, out_max, out_sum, out_sum64, out_xnor, out_sbfe, out_mbcnt};
    for (int q = 2; q < 8 && ok; ++q) ok = hipMemcpy(host[q], d[q], sz[q] * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? FSK_OK : FSK_EDEVICE;
}
#endif
