/*
 * fastsk_amd.h — C ABI of the MI355X-native gapped-k-mer kernel engine (libfastsk_amd.so).
 *
 * This is the drop-in boundary for ONE path of QData/FastSK: the per-mismatch-combination
 * partial-kernel worker behind fastsk.FastSK(g,m,...).compute_kernel(Xtrain,Xtest). Every entry
 * point names the reference interface it replaces (paths relative to
 * /root/reference/src/fastsk/_fastsk). Plain pointers and sizes only: no C++ types, no torch
 * types, no exceptions across the boundary. All functions return FSK_OK (0) or a negative
 * FSK_E* code; fsk_last_error() holds the message. INTEGRATION.md shows the pybind11 binding a
 * reference maintainer would write against this header.
 *
 * Data conventions (same as the reference):
 *   - sequences arrive as one int32 token array + int64 offsets (n_train rows first, then
 *     n_test rows), i.e. the flattened form of the vector<vector<int>> arguments of
 *     FastSK::compute_kernel (fastsk.cpp:30); buffers are caller-owned and only read during
 *     the call;
 *   - the kernel triangle is row-major lower-triangular, cell (i,j), j<=i, at i(i+1)/2+j
 *     (tri_access, shared.cpp:97-117), N = n_train + n_test;
 *   - combination id c is the c-th (g-m)-subset of {0..g-1} in lexicographic order
 *     (getCombinations, shared.cpp:347-360).
 */
#ifndef FASTSK_AMD_H
#define FASTSK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSK_ABI_VERSION 5  /* 2: fsk_create_multi + fsk_config.collective/bands, fsk_counts_digest, device-block allocation;
                              3: fsk_get_triangle_device / fsk_alloc_triangle_device, fsk_config.deadline_ms;
                              4: fsk_set_tuning / fsk_get_tuning / fsk_tuning_keys (one FSK_TUNING variable instead of
                                 two dozen FSK_* switches);
                              5: fsk_seed_order; fsk_set_seed draws the reference's own std::shuffle order
                                 (added since, no layout changed: fsk_set_complement; fsk_set_mismatch_weights and its helpers;
                                  fsk_set_wildcards; fsk_set_center_weights;
                                  fsk_svm_train, fsk_svm_get_model, fsk_svm_decision, fsk_svm_decision_device and fsk_svm_info;
                                  fsk_svm_cv, fsk_svm_cv_get, fsk_svm_cv_get_alpha and their three structs;
                                  fsk_rows_build, fsk_rows_get_block(_device), fsk_rows_get_info and fsk_rows_info,
                                  fsk_svm_set_kernel / fsk_svm_get_kernel;
                                  fsk_svm_set_class_weights / fsk_svm_get_class_weights, fsk_svm_platt_fit, fsk_svm_calibrate,
                                  fsk_svm_get_calibration, fsk_svm_proba and fsk_svm_platt_info;
                                  fsk_svr_train, fsk_svr_get_model, fsk_svr_cv, fsk_svr_cv_get and fsk_svr_cv_score;
                                  fsk_svm_train_multiclass, fsk_svm_multiclass_get_model, fsk_svm_multiclass_decision(_device),
                                  fsk_svm_multiclass_cv, fsk_svm_multiclass_cv_get and their two structs;
                                  fsk_svm_multiclass_calibrate, fsk_svm_multiclass_get_calibration,
                                  fsk_svm_multiclass_set_calibration, fsk_svm_multiclass_proba(_device) and fsk_exp_neg) */

enum {
    FSK_OK = 0,
    FSK_EINVAL = -1,   /* bad argument (g<=m, m<0, null pointer, bad combo id, ...)              */
    FSK_ESHORT = -2,   /* g > shortest sequence: the reference printf+exit(1)s, fastsk.cpp:53-58 */
    FSK_ESTATE = -3,   /* call out of order (e.g. getter before compute)                          */
    FSK_EDEVICE = -4,  /* HIP runtime error / no device                                           */
    FSK_ENOMEM = -5,   /* device or host allocation failed                                        */
    FSK_EUNSUPPORTED = -6 /* alphabet > 65536 symbols, (g-m) * ceil(log2(alphabet)) > 96 bits, g > 255 ...   */
};

/* accumulate dataflow */
enum {
    FSK_PATH_AUTO = 0,
    FSK_PATH_DENSE = 1,  /* k_dense_count: per-sequence LDS counting sort -> 4-bit count panels (lo + 16*hi);
                            k_dense_tile_dma: 128 x 128 tiles of K, panels DMA'd into LDS, v_dot8_u32_u4
                            co-occurrence sums kept in registers over all combos of the launch, then one
                            64-bit store (first launch after a reset) or atomicAdd per cell            */
    FSK_PATH_SPARSE = 2  /* the reference's dataflow (cntsrtna + countAndUpdateTri) as streams: packed
                            (k-mer, seq) records -> LSD radix sort in LDS-staged passes -> run-length
                            entries -> one 32-bit update word per += binned by owner band of K -> the
                            band's words summed in LDS, one 64-bit add per touched cell; beyond a few
                            LDS rounds a band (N > ~9,000) K is owned in two levels (bands, then blocks of
                            2^14 cells); where runs are long an entry of many partners travels as one
                            16-byte descriptor that the owning workgroup expands itself; a 64-bit
                            atomicAdd per (run, pair) only on request or for sequences in the millions   */
};

/* how the engines of fsk_create_multi sum their partial triangles (fastsk_kernel.cpp:286-315) */
enum {
    FSK_COLL_AUTO = 0,   /* RCCL when the listed devices are distinct and librccl can be loaded, else P2P  */
    FSK_COLL_RCCL = 1,   /* ncclAllReduce over xGMI, one communicator rank per listed device               */
    FSK_COLL_P2P = 2     /* the engine's own reduce-scatter + all-gather kernels over peer mappings (all
                            devices live in this process); also what lets a device be listed twice, i.e.
                            the multi-device host code exercised on a single GPU                          */
};

typedef struct fsk_engine fsk_engine; /* opaque; replaces class FastSK + KernelFunction state */

/* Constructor arguments of FastSK (bindings.cpp:14-22, fastsk.cpp:19-28), plus placement. */
typedef struct fsk_config {
    int32_t g;             /* g-mer length                                                      */
    int32_t m;             /* mismatch positions; k = g - m kept positions (fastsk.cpp:22)      */
    int32_t t;             /* host threads in the reference; here: number of approx-mode chains
                              (-1 -> 20, capped at #combos: fastsk_kernel.cpp:54-61)            */
    int32_t approx;        /* 0 exact, 1 approx (fastsk_kernel.cpp:188-262)                     */
    double delta;          /* approx convergence threshold (default 0.025)                      */
    int32_t max_iters;     /* approx: max combos per chain, -1 = unlimited                      */
    int32_t skip_variance; /* approx: integer sums, no Welford chain                            */
    int32_t device;        /* HIP device ordinal                                                */
    int32_t path;          /* FSK_PATH_*                                                        */
    int32_t profile;       /* 1: measurement mode — every kernel family timed with HIP events that are waited for on
                              the spot, the exact update count U computed (fsk_get_stats); the sparse dataflow on
                              one stream, every batch sized exactly. 2: the product dataflow untouched — the events
                              are only recorded (on the stream the kernels run on), fsk_get_stats harvests them */
    int32_t skip_test_block; /* 1: cells with both sequences in the test set (other than the diagonal)
                                may be left at zero — no getter of the reference exposes them
                                (fastsk.cpp:190-217). Dense dataflow: whole tiles of such cells
                                are not computed; sparse dataflow: a test row pairs only with the
                                train sequences of its k-mer runs (and itself).                 */
    /* fsk_create_multi only (ignored by fsk_create): */
    int32_t collective;    /* FSK_COLL_*                                                          */
    int32_t bands;         /* row bands of the overlapped all-reduce; 0 = automatic               */
    int32_t deadline_ms;   /* fail fast: bound, in milliseconds, on every host-side wait of the multi-GPU exchange —
                              ncclCommInitAll, the engines' barriers, a band's all-reduce having run on the device.
                              A wait that exceeds it returns FSK_EDEVICE naming the stage and the band, the
                              communicator is aborted (ncclCommAbort) and the group is dead: every later call
                              returns FSK_EDEVICE with that first message. 0 = the tuning key deadline_ms
                              (120000 unless set); negative = no deadline                                     */
    int32_t reserved[1];
} fsk_config;

/* Measured and algorithmic quantities of the work done so far. */
typedef struct fsk_stats {
    int64_t n_seq, n_train, n_test, n_feat, n_pairs;
    int32_t alphabet;        /* distinct tokens actually present (rank-remapped 0..alphabet-1)  */
    int32_t bits_per_symbol; /* packed width in HBM                                             */
    int64_t key_space;       /* alphabet^k                                                      */
    int32_t path_used;       /* FSK_PATH_DENSE / FSK_PATH_SPARSE                                */
    int32_t n_combos_total;  /* C(g,m)                                                          */
    int64_t combos_done;     /* combos accumulated so far                                       */
    uint64_t cell_updates;   /* U = sum over runs d(d+1)/2, exact on both dataflows (dense: counted from the
                                count panels by k_dense_distinct when profile = 1, else 0)                */
    uint64_t sort_records;   /* records pushed through the radix sort                           */
    int32_t sort_passes;     /* 8-bit LSD passes per batch                                      */
    int32_t launches;        /* kernel launches in accumulate (shift classes: the edge-key kernel, every group's
                                base launch and the correction launch count here only)         */
    /* HIP-event milliseconds on the engine's stream (profile=1), summed over launches         */
    double ms_count;         /* dense: k-mer extraction + LDS counting sort -> count panels     */
    double ms_tile;          /* dense: tiled co-occurrence accumulate + flush (shift classes: with the edge
                                keys and the corrections)                                       */
    double ms_extract;       /* sparse: key extraction                                          */
    double ms_sort;          /* sparse: radix sort                                              */
    double ms_segment;       /* sparse: run/segment detection + compaction                      */
    double ms_pairs;         /* sparse: per-run pair atomics                                    */
    double ms_total;         /* whole accumulate calls                                          */
    int64_t n_tile_launches; /* tile passes: one per chunk and row band, however many kernels a pass launches */
    uint64_t dense_macs;     /* count multiply-adds issued by the tile kernel: 8 per dword row and cell, the exact
                                remainder products of the rows with counts above 15 included (profile = 1). Shift
                                classes (tuning dense_shift): the chain bases alone, tiles x rows x bases x 8 x 128^2 —
                                the derived combinations cost lookups, not multiply-adds. Tuning dense_shift_packed
                                (0, the default: the lookups read key-major planes eight cells at a time; -1: the count
                                panels, one cell a read) cuts a chain after nine members when it is 0: a class of more
                                shifts is two chains, one more base                              */
    uint64_t panel_bytes;    /* bytes of count panels written (= read at least once)            */
    double u4_tile_launches; /* launches of the 4-bit tile kernel (v_dot8_u32_u4)                */
    double max_windows;      /* max over sequences of (length - g + 1), of both strands in reverse-complement mode: bounds a cell per combo
                                (wildcards set: of the windows free of them; centre weights set: of the sum of the windows' weights) */
    double count_launches;   /* launches of the segment-count kernel (panel cache misses)        */
    double compact_keys_avg; /* key compaction on: mean keys per combo that really occur (else 0) */
    double batches_redone;   /* sparse: batches enqueued ahead of their word count that did not fit */
    double combos_issued;    /* combos whose kernels ran: combos_done + the iterations variance mode ran ahead of
                                its stop test and dropped (cell_updates and the ms_* cover all of them)      */
    /* ABI 5 */
    double sparse_form;      /* sparse: the update stage the last batch took — 0 owner bands (k_sx_consume), 1 one 64-bit
                                atomic per +=, 2 two-level blocks (k_sxb_*); -1: no sparse batch yet               */
    double sparse_passes;    /* sparse, blocks: passes over disjoint row ranges run since the sequences were loaded */
    double share_positions;  /* sparse: leading kept positions the last batch sorted once per group of slots (0: none) */
    double share_groups;     /* ... and the groups it had                                                          */
    double sparse_desc;      /* sparse, owner bands and two-level blocks: 1 when the last batch sent its long entries as
                                descriptors that k_sx_consume / k_sxb_consume expand (tuning sparse_desc), else 0   */
} fsk_stats;

/* ---- lifecycle: replaces FastSK::FastSK (fastsk.cpp:19-28) and ~nothing (the reference leaks) */
int fsk_create(const fsk_config* cfg, fsk_engine** out);
void fsk_destroy(fsk_engine* e);
/* One engine over SEVERAL GPUs of this process — what FastSK(..., devices=[0,1,...]) creates. The reference
 * fans one compute_kernel call out over t host threads (fastsk_kernel.cpp:54-93: thread r takes work items
 * r, r+T, ...) and sum-reduces their private triangles (fastsk_kernel.cpp:286-315); here engine r of R lives
 * on devices[r], holds a replica of the packed sequences, takes combos r, r+R, ... of every accumulate and
 * the partial triangles are summed by ONE logical all-reduce (RCCL over xGMI, or the P2P kernels), issued per
 * row band on a communication stream under the next band's kernels, as int32 when every reduced cell provably
 * fits (C(g,m) * max_windows^2 < 2^31). Variance mode: Welford chain c runs on engine c mod R, one fp64
 * all-reduce of the chains' sums. Integer sums do not depend on their order: results are bit-identical to
 * fsk_create's for every R. The returned handle is engine 0 and takes every call of this header: load /
 * reset / accumulate / synchronize / finalize / compute act on the whole group (one host thread per
 * device), getters read engine 0's copy of the reduced triangle, fsk_bind_counts binds engine 0's triangle,
 * fsk_accumulate_rows and fsk_run_chains are single-engine calls and return FSK_ESTATE. ndev = 1 runs the
 * same banded, collective code with a world of one. */
int fsk_create_multi(const fsk_config* cfg, const int32_t* devices, int32_t ndev, fsk_engine** out);
typedef struct fsk_multi_info {
    int32_t ndev;            /* engines in the group (0: `e` came from fsk_create)                        */
    int32_t devices[16];
    int32_t collective;      /* FSK_COLL_RCCL or FSK_COLL_P2P: the one in use                              */
    int32_t comm_ranks;      /* ranks of the communicator the last collective ran over                     */
    int32_t bands;           /* row bands of the last accumulate                                           */
    int32_t narrow;          /* 1: the last accumulate exchanged int32                                     */
    int64_t reduce_bytes;    /* payload of the last accumulate's all-reduce, per engine                    */
    int64_t combos_per_engine[16]; /* combos of the last accumulate                                        */
    double reserved[4];
} fsk_multi_info;
int fsk_get_multi_info(fsk_engine* e, fsk_multi_info* out);
/* Tuning: every knob of the engine that is not a constructor argument of the reference — forcing one of two
 * equivalent code paths (tests), sizes of batches and launches (A/B measurements) — is a named integer key.
 * fsk_tuning_keys() lists them, one "key=default [lowest..highest] what it does" per line. A key is set per handle
 * with fsk_set_tuning (a group: on all its engines; takes effect from the next fsk_load_sequences / fsk_compute on),
 * or for every engine a process creates through ONE environment variable, FSK_TUNING="key=value,key=value", parsed
 * once by fsk_create — the only variable the library reads; an unknown key or a value out of range fails the call
 * (FSK_EINVAL). No key changes a result. trace=1 prints the keys in force (stderr). */
int fsk_set_tuning(fsk_engine* e, const char* key, int64_t value);
int fsk_get_tuning(fsk_engine* e, const char* key, int64_t* value);
const char* fsk_tuning_keys(void);
/* message of the last failure on `e` (or of the last failed fsk_create when e == NULL) */
const char* fsk_last_error(const fsk_engine* e);
int fsk_abi_version(void);
/* number of visible HIP devices (<0 on runtime error) */
int fsk_device_count(void);

/* ---- one-call path: replaces FastSK::compute_kernel (fastsk.cpp:30-118, n_test > 0) and
 * FastSK::compute_train (fastsk.cpp:120-188, n_test == 0) including
 * KernelFunction::compute_kernel (fastsk_kernel.cpp:24-106): exact / skip-variance / variance
 * modes per the config. Blocks until the result is resident on the device. */
int fsk_compute(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train,
                int64_t n_test);

/* Combo order used by the approx modes. Replaces the time(0)-seeded std::shuffle of
 * fastsk_kernel.cpp:29-38 with an explicit permutation (or prefix of one) of 0..C(g,m)-1.
 * Without it approx mode draws the order of fsk_set_seed's seed (0 when none was set). */
int fsk_set_combo_order(fsk_engine* e, const int32_t* order, int32_t n);
/* The seed of that shuffle: the order is the one the reference draws when time(0) == seed —
 * libstdc++'s std::shuffle over std::default_random_engine (minstd_rand0), fastsk_kernel.cpp:31-38,
 * restated in the engine (fsk_seed_order returns it). So FastSK(approx=True, seed=S) samples the
 * combos the reference sampled in the second S. */
int fsk_set_seed(fsk_engine* e, uint64_t seed);

/* Reverse-complement mode (DNA: a regulatory element reads the same from either strand; what gkm-SVM and LS-GKM
 * count by default, and the reference cannot). `tokens[i]` <-> `complements[i]`, i < n, is an involution on token ids
 * (a<->t, c<->g, n<->n ...); rc(x) is x reversed with every token complemented. With the mode on the feature multiset
 * of a sequence is that of x plus that of rc(x), multiplicities kept, so that per combination
 *     Krc(x, y) = K(x, y) + K(x, rc y) + K(rc x, y) + K(rc x, rc y),
 * and everything else (sum over combinations, approx modes, normalisation) is the reference's algorithm on these
 * counts. n = 0 switches the mode off (the default). Takes effect from the next fsk_load_sequences / fsk_compute; a
 * group handle sets it on every engine. FSK_EINVAL here when a token is listed twice or the map is not an involution
 * on its domain (every complement listed, comp(comp(t)) == t; self-pairs allowed); FSK_EINVAL at load, naming the
 * token, when the data hold a token the map does not list (nothing is self-complemented silently). The alphabet of
 * a load is the closure under the map of the tokens present. */
int fsk_set_complement(fsk_engine* e, const int32_t* tokens, const int32_t* complements, int32_t n);

/* Wildcard symbols (the unknown base 'n' of DNA, the 'x' of protein): the n token ids listed are WILDCARDS. A g-window
 * that holds a wildcard at ANY of its g positions is not a window — for every combination, whether or not the combination
 * keeps the position. Everything else is this header's algorithm on the windows that remain (per-combination counts, the
 * sum over combinations, reverse complement, the mismatch-weighted kernels, both approx modes, normalisation): with the
 * fragments of x its maximal wildcard-free runs of at least g symbols, K(x, y) = sum over the fragments s of x and t of y
 * of the plain K(s, t). n = 0 switches the mode off (the default). Takes effect from the next fsk_load_sequences /
 * fsk_compute; a group handle sets it on every engine; the levels of the mismatch-weighted mode inherit it. FSK_EINVAL on a
 * null array, a negative n or a token listed twice. At load: a sequence without a single wildcard-free window has no
 * features and would have a zero diagonal — FSK_ESHORT naming its index, as for a sequence shorter than g; in
 * reverse-complement mode a wildcard need not be listed in the complement map, and when it is its complement must be a
 * wildcard too, else FSK_EINVAL naming the token. fsk_stats: n_feat and max_windows count the valid windows (they bound a
 * cell), alphabet and key_space the real symbols only. A wildcard that does not occur in the data changes nothing. */
int fsk_set_wildcards(fsk_engine* e, const int32_t* tokens, int32_t n);

/* Centre-weighted kernels (the "wgkm" of LS-GKM, -t 4: a g-window counts more the closer it lies to the middle of its
 * sequence, the summit of a ChIP-seq / ATAC peak). The PROFILE is w[0..n-1], 1 <= n <= 4096, 0 <= w[d] <= 255, w[0] >= 1.
 * Window p (0 <= p <= L - g) of a sequence of length L lies d(p) = floor(|2p + g - L| / 2) from the sequence's centre and
 * has the weight W(p) = w[min(d(p), n - 1)]: the last entry extends outwards. Per combination c,
 *     K_c(x, y) = sum over windows p of x, q of y of W_x(p) W_y(q) [p and q agree at the kept positions of c],
 * i.e. the features of x hold window p W(p) times; everything else is this header's algorithm on these counts (the sum
 * over combinations, reverse complement — window p' of rc(x) is forward window L - g - p', at the same d —, wildcards — the
 * weights apply to the valid windows —, the mismatch-weighted kernels, whose levels inherit the profile, both approx modes,
 * normalisation). A window of weight 0 is not a window, as one that holds a wildcard is not; a sequence left without any
 * fails the load with FSK_ESHORT naming its index (only possible together with wildcards). n = 0 switches the mode off (the
 * default); a profile of ones, or one whose other entries no window of the data reaches, changes nothing, to the launch.
 * Takes effect from the next fsk_load_sequences / fsk_compute; a group handle sets it on every engine. FSK_EINVAL on a null
 * array, n < 0 or n > 4096, an entry above 255, w[0] == 0. fsk_stats: n_feat is the sum of all weights and max_windows the
 * largest sum of one sequence (both strands in reverse-complement mode): they bound a cell as they always did; the weighted
 * n_feat must stay below 2^31 (FSK_EUNSUPPORTED at load). The variance mode (approx without skip_variance) keeps 32-bit
 * cells per combination: with the mode on and max_windows^2 > 2^32 - 1, fsk_compute returns FSK_EUNSUPPORTED and the
 * engine stays usable. The sparse dataflow repeats a window's sort record W(p) times: its cost grows with the mean weight. */
int fsk_set_center_weights(fsk_engine* e, const uint32_t* w, int32_t n);

/* Mismatch-weighted kernels (the mismatch-truncated gapped k-mer kernel LS-GKM ships as "-l 11 -k 7 -d 3", the l-mer
 * filters of Ghandi et al., "pairs of l-mers within d mismatches"). With N_h(x, y) the number of pairs (one g-window of x,
 * one of y) that differ in exactly h positions, the kernel of this header is K = sum_{h<=m} C(g-h, m-h) N_h; this call
 * replaces the binomial weights by c[0..m] (non-negative integers; scale rational weights, the normalised kernel does
 * not see the scale):   W(x, y) = sum_{h<=m} c[h] N_h(x, y),   exact in 64 bits.
 * How: the raw triangle S_j of (g, m = j) over all its C(g, j) combinations is sum_{h<=j} C(g-h, j-h) N_h; with d the last
 * h whose c[h] != 0 and a_d = c[d], a_h = c[h] - sum_{j=h+1..d} a_j C(g-h, j-h) (h = d-1 .. 0; signed),
 * W = sum_{j<=d} a_j S_j mod 2^64 cell for cell — pairs further apart than d cancel. fsk_compute runs the levels with
 * a_j != 0 one after another (each with this engine's device, path, skip_test_block, tuning and complement map) into one
 * scratch triangle and folds it into the result (k_tri_fold); peak device memory is the result triangle, one scratch
 * triangle and one level's working set. When c is this header's own weights (a = e_m) nothing of that runs.
 * n = 0 switches the mode off (the default); otherwise n == m + 1 and c[0] >= 1 (every diagonal stays positive), else
 * FSK_EINVAL; FSK_EINVAL when a coefficient does not fit int64; FSK_EUNSUPPORTED on a group handle and on an engine
 * created with approx = 1 (a sample of combinations under signed coefficients estimates nothing). Takes effect from the
 * next fsk_compute. With the mode on fsk_compute is the entry point: fsk_load_sequences, fsk_accumulate*,
 * fsk_reset_counts* and fsk_run_chains return FSK_ESTATE (their combination ids belong to one level); every getter,
 * fsk_finalize and fsk_save_kernel work on W as they do on K. fsk_compute returns FSK_EUNSUPPORTED, naming the level,
 * when a level's k-mer does not fit the sort records ((g-j) * bits a symbol > 96), and when
 * max(c) * max_windows^2 >= 2^64 (the bound that makes the sums mod 2^64 exact); the engine stays usable. */
int fsk_set_mismatch_weights(fsk_engine* e, const uint64_t* c, int32_t n);
/* What the last fsk_compute did in that mode: *n_levels = d + 1 (0: mode off), and for j < min(cap, d + 1) the
 * coefficient a[j] (0: the level was skipped) and the dataflow paths[j] (FSK_PATH_DENSE / FSK_PATH_SPARSE) it took. */
int fsk_get_mismatch_info(fsk_engine* e, int32_t* n_levels, int64_t* a, int32_t* paths, int32_t cap);
/* ... and how long it took, in milliseconds: level_ms[j] the host time of level j (load, accumulate, wait), fold_ms[j]
 * the HIP-event time of its fold; zeros for skipped levels and when the weights were this header's own. */
int fsk_get_mismatch_times(fsk_engine* e, double* level_ms, double* fold_ms, int32_t cap);

/* ---- staged path (multi-GPU sharding, benchmarking with inputs resident in HBM) ------------ */
/* lengths check + dictionary + packing + H2D: fastsk.cpp:32-88 (extractFeatures is replaced by
 * bit-packed sequences that every combo re-reads) */
int fsk_load_sequences(fsk_engine* e, const int32_t* tokens, const int64_t* offsets, int64_t n_train,
                       int64_t n_test);
/* Use caller-provided device memory (uint64[n_pairs], e.g. a torch tensor that RCCL will
 * all-reduce) for the integer triangle instead of an engine-owned allocation. The buffer's contents are
 * taken as they are (call fsk_reset_counts for zeros); on a group handle the exchange stays 64 bits wide
 * until the next whole reset, because nothing bounds the cells the caller brought. */
int fsk_bind_counts(fsk_engine* e, void* device_u64, int64_t n_cells);
/* device address of the integer triangle (engine-owned or bound) */
int fsk_counts_device_ptr(fsk_engine* e, void** out);
/* Zero the integer triangle before another pass. The zeros may be written by the next tile launch
 * itself (it then stores its sums instead of adding them); every other reader of the triangle,
 * including fsk_synchronize — after which a caller may read a bound buffer — sees them. */
int fsk_reset_counts(fsk_engine* e);
/* zero only rows [row_begin, row_end) of the triangle (a rank that owns a band of rows) */
int fsk_reset_counts_rows(fsk_engine* e, int64_t row_begin, int64_t row_end);
/* THE HOT PATH. Adds the partial kernels of the listed combos into the integer triangle:
 * the loop body of kernel_build_parallel (fastsk_kernel.cpp:188-281) for each combo, and the
 * K += Ks reduce (fastsk_kernel.cpp:286-315). Asynchronous on the engine's stream. */
int fsk_accumulate(fsk_engine* e, const int32_t* combos, int32_t n);
/* The same, restricted to the cells (i, j<=i) with row_begin <= i < row_end (row bounds multiples
 * of 128, or N). Lets the host all-reduce finished row bands of the triangle while the next band
 * is still being accumulated; the count panels of an unchanged combo list are reused between
 * calls. fsk_accumulate(e, c, n) == fsk_accumulate_rows(e, c, n, 0, N). */
int fsk_accumulate_rows(fsk_engine* e, const int32_t* combos, int32_t n, int64_t row_begin, int64_t row_end);
/* wait for the engine's stream */
int fsk_synchronize(fsk_engine* e);
/* Order the engine's stream against a HIP stream of the caller (hipStream_t passed as void*; NULL =
 * the default stream) without blocking the host. fsk_stream_wait_engine: work enqueued on
 * `hip_stream` after the call waits for everything the engine has enqueued so far (e.g. RCCL's
 * all-reduce of a finished row band, issued on torch's stream, while the engine accumulates the next
 * band). Rows that an fsk_reset_counts left for a later storing launch are NOT filled by this call:
 * the other stream may read only rows already accumulated (fsk_synchronize fills the rest; an accumulate
 * with an empty combo list fills the rows it was given).
 * fsk_engine_wait_stream: the engine's later work waits for what `hip_stream` holds now.
 * `hip_stream` must be a stream of the engine's device. */
int fsk_stream_wait_engine(fsk_engine* e, void* hip_stream);
int fsk_engine_wait_stream(fsk_engine* e, void* hip_stream);
/* extract the raw diagonal for normalisation (fastsk_kernel.cpp:96-103); call after the last
 * accumulate (and after any cross-GPU all-reduce of the triangle) */
int fsk_finalize(fsk_engine* e);

/* ---- results: replace the getters of fastsk.cpp:190-221 ---------------------------------- */
/* normalised K[i0:i1, j0:j1] as row-major doubles, any sub-block of the symmetric N x N matrix */
int fsk_get_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double* out);
/* the same block written to DEVICE memory owned by the caller (e.g. a torch tensor): no host copy,
 * for consumers that keep the kernel matrix on the GPU */
int fsk_get_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double* device_out);
/* the same block in device memory the ENGINE allocates on its device (*device_out; release with
 * fsk_free_device, whose `e` may be NULL once the engine is destroyed): for host code that has no allocator of its own for the GPU — the pybind11 class wraps
 * it in a DLPack capsule, so the SVM stage can take the kernel matrix without a host bounce */
int fsk_alloc_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, double** device_out);
int fsk_free_device(fsk_engine* e, void* device_ptr);
/* change fsk_config.skip_test_block for later computes (a caller that finds it needs test x test cells after all) */
int fsk_set_skip_test_block(fsk_engine* e, int32_t skip);
int fsk_get_train(fsk_engine* e, double* out);      /* n_train x n_train, get_train_kernel()   */
int fsk_get_test(fsk_engine* e, double* out);       /* n_test  x n_train, get_test_kernel()    */
int fsk_get_triangle(fsk_engine* e, double* out);   /* double[N(N+1)/2], the reference's K     */
/* The whole normalised triangle (fastsk_kernel.cpp:96-103 applied to every cell) written to DEVICE memory:
 * N(N+1)/2 doubles at `device_out` (caller-owned), or in a buffer the engine allocates on its device
 * (*device_out; release with fsk_free_device). One streaming pass: 16 bytes per cell. */
int fsk_get_triangle_device(fsk_engine* e, double* device_out);
int fsk_alloc_triangle_device(fsk_engine* e, double** device_out);
/* The raw integer triangle of the exact and skip-variance modes: the EXACT 64-bit sum over the combinations accumulated, for
 * every form either dataflow takes and every tuning key. Where a kernel sums in 32 bits first, the host keeps what one launch
 * or batch can put into a cell below 2^32 (combinations per dense tile launch and per sparse batch: (2^32 - 1) / max_windows^2),
 * and where one combination alone can pass it (a sequence of 65,536 windows or more) the sparse dataflow adds the entries that
 * could make it do so into the 64-bit triangle directly. (Variance mode's per-combination triangles are 32 bits wide by
 * design, like the reference's `unsigned int Ks`; they are not what this returns.) */
int fsk_get_counts(fsk_engine* e, uint64_t* out);
int fsk_get_counts_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, uint64_t* out);
/* raw integer cells (rows[q], cols[q]), q < n, of the symmetric matrix: scattered spot checks of a
 * triangle too large to copy out (tri_access of arbitrary pairs, shared.cpp:97-117) */
int fsk_get_counts_cells(fsk_engine* e, const int64_t* rows, const int64_t* cols, int64_t n, uint64_t* out);
/* Order-free digest of the integer cells of rows [row_begin, row_end): out[0] = sum of the cells (mod 2^64),
 * out[1] = xor over the cells of cell * (index | 1) (mod 2^64), index = i(i+1)/2 + j. One pass on the device.
 * Digests of disjoint row ranges combine (add / xor), so a triangle held in row bands by several ranks — or
 * reduced over several GPUs — can be compared with the single-GPU one without copying it out: the
 * "bit-identical at 1/2/4/8 GPUs" gate of the exact mode (integer sums, fastsk_kernel.cpp:286-315). */
int fsk_counts_digest(fsk_engine* e, int64_t row_begin, int64_t row_end, uint64_t out[2]);
/* The reduction inside get_variance (fastsk_kernel.cpp:116-131): the sum of n doubles in INDEX ORDER,
 * s = fl(s + values[i]) for i = 0 .. n-1, to the last bit, computed on the device (the stop test of
 * approx mode depends on it). `values` is a host array. Exposed so that the summation can be verified
 * on its own. */
int fsk_sequential_sum(fsk_engine* e, const double* values, int64_t n, double* out);
/* Variance mode over several GPUs (the T Welford chains are the units): after
 * fsk_load_sequences, run the chains first, first + step, ... < T of this engine — one worker thread's
 * share of fastsk_kernel.cpp:188-281 — leaving the sum of their K_hat (fastsk_kernel.cpp:286-315) in the
 * engine's fp64 triangle; chain 0's engine holds get_stdevs(). The caller sums the triangles of all
 * engines (fsk_get_kernel_sum_device -> e.g. an RCCL all-reduce -> fsk_set_kernel_sum_device; device
 * buffers of N(N+1)/2 doubles) and calls fsk_finalize. With T > 1 the fp64 sum over chains depends on
 * its order, as it does between the reference's threads. */
int fsk_run_chains(fsk_engine* e, int32_t first, int32_t step);
int fsk_get_kernel_sum_device(fsk_engine* e, double* device_out);
int fsk_set_kernel_sum_device(fsk_engine* e, const double* device_in);
/* approx/variance mode: thread 0's convergence trace, get_stdevs() (fastsk.cpp:219-221) */
int fsk_get_stdevs(fsk_engine* e, double* out, int32_t cap, int32_t* n);
/* "%d:%e " text dump, one row per line, 1-based column ids: save_kernel (fastsk.cpp:223-237) */
int fsk_save_kernel(fsk_engine* e, const char* path);
int fsk_get_stats(fsk_engine* e, fsk_stats* out);

/* ---- the SVM stage on the resident triangle: replaces FastSK::fit / FastSK::score (fastsk.cpp:239-530, LIBSVM on the host)
 * for the sequences of ONE fsk_compute (or load / accumulate / finalize). Nothing leaves the device but three vectors.
 *
 * fsk_svm_train: a C-SVC (labels[t] in {-1, +1}, t < n = n_train) on the train x train part of the normalised result, solved
 * in the dual by SMO with LIBSVM's second-order working-set selection, without shrinking: alpha = 0, G = -1; per iteration
 * i = argmax of v_t = -y_t G_t over I_up, Gmax = v_i, Gmin = min v over I_low, stop when Gmax - Gmin <= eps; j = argmin over
 * I_low, b_t = Gmax - v_t > 0, of -(b_t b_t) / a_t with a_t = K_ii + K_tt - 2 K_it = 2 - 2 K_it (1e-12 where that is <= 0); the
 * two-variable step with its clips to [0, C]^2 in the order of LIBSVM's Solver::Solve (K_ii = 1); G_t += Q_it dalpha_i +
 * Q_jt dalpha_j, Q_it = y_i y_t K_it. Ties go to the lowest index. Every K_it is the IEEE value fsk_get_train returns, every
 * operation a single correctly rounded one, so alpha, rho and the iteration count do not depend on the form of the loop that
 * ran (tuning svm_wg_max: up to that many rows one workgroup with the state in LDS, beyond it two launches an iteration), on
 * tuning svm_chunk (iterations between two reads of the status record) or on the grid. rho is the mean of y_t G_t over the
 * free support vectors (0 < alpha < C), the midpoint of its two bounds when there is none; the dual objective
 * 1/2 sum alpha_t (G_t - 1); both summed on the host in index order, as LIBSVM does. max_iter < 0: 10,000,000; reaching
 * max_iter is FSK_OK with fsk_svm_info.converged = 0, and so is a selection that finds no j (LIBSVM's Gmin_idx == -1; only a
 * result whose normalised cells are not numbers, e.g. a zero diagonal, gets there): the step is not taken, the solve ends. A group handle trains on engine 0's reduced triangle.
 * FSK_ESTATE before a finalized result; FSK_EINVAL when n != n_train, a label is not -1 or +1, only one class is present, or
 * C or eps is not a positive finite number. The model belongs to the result: fsk_compute, fsk_load_sequences, an accumulate or
 * a reset drops it, and the calls below then return FSK_ESTATE. */
typedef struct fsk_svm_info {
    int64_t iterations;      /* two-variable steps taken                                                    */
    double gap;              /* Gmax - Gmin of the last selection                                           */
    double objective;        /* dual objective 1/2 sum alpha_t (G_t - 1)                                    */
    int64_t n_sv, n_bsv;     /* alpha_t > 0; alpha_t >= C_t (C, or the class's box under class weights)     */
    int32_t converged;       /* 1: gap <= eps; 0: max_iter reached first                                    */
    int32_t form;            /* 1: one workgroup (k_svm_wg); 2: two launches an iteration                   */
    int64_t launches;        /* kernel launches of the solve                                                */
    double ms;               /* host time of fsk_svm_train                                                  */
    double reserved[4];
} fsk_svm_info;
int fsk_svm_train(fsk_engine* e, const int32_t* labels, int64_t n, double C, double eps, int64_t max_iter);
/* alpha[n_train] (may be NULL), *rho and *info (either may be NULL) of the last fsk_svm_train */
int fsk_svm_get_model(fsk_engine* e, double* alpha, double* rho, fsk_svm_info* info);
/* out[r - r0] = sum_{i < n_train} alpha_i y_i K(r, i) - rho for rows r0 <= r < r1 <= N of the sequences (train rows first): the
 * decision values of the model, read from the triangle in place. Only cells with a train column are read, so the values of
 * test rows are whole under fsk_config.skip_test_block too. The _device form writes to DEVICE memory owned by the caller. */
int fsk_svm_decision(fsk_engine* e, int64_t r0, int64_t r1, double* out);
int fsk_svm_decision_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_out);

/* ---- cross-validation of the C-SVC over folds and a grid of C, every problem solved side by side on the resident triangle.
 *
 * fsk_svm_cv: fold[t] in [0, n_folds) for the n = n_train training rows; problem p = c n_folds + f trains, at Cs[c], on the rows
 * with fold[t] != f (in row order) — fsk_svm_train's algorithm on that sub-matrix, to the bit: alpha, rho, the objective, the
 * gap and the iteration count of a problem are those of a single solve of its rows, whichever form ran (one workgroup a
 * problem with its state in LDS while the largest training set has at most svm_wg_max rows, two launches an iteration over
 * (workgroups, problems) beyond; svm_chunk iterations between two reads of the problems' status records). Then the
 * out-of-fold decision values oof[c n + t] = sum_i alpha_i y_i K(t, i) - rho of problem c n_folds + fold[t], summed as
 * fsk_svm_decision sums, and from them on the host, per value of C,
 *   auc = (#{(pos, neg): oof_pos > oof_neg} + 0.5 #{oof_pos == oof_neg}) / (n_pos n_neg)   (integer counts; one multiply,
 *         one add, one divide in double),
 *   accuracy = the share of rows with (oof > 0) == (label > 0)   (LIBSVM's sign rule).
 * max_iter as for fsk_svm_train, for every problem alike. FSK_ESTATE before a finalized result. FSK_EINVAL, the message
 * naming the row, fold or C: n != n_train, a label that is not -1 or +1, a fold id out of range, a fold without rows, a fold
 * whose training rows are of one class, n_folds < 2, n_C < 1, a C or eps that is not a positive finite number, more than
 * FSK_SVM_CV_MAX_PROBLEMS problems. A refused call leaves an earlier result as it was. The result belongs to the finalized
 * kernel as the model does (a new or stale kernel: FSK_ESTATE); it neither needs nor touches the model of fsk_svm_train. A
 * group handle works on engine 0's reduced triangle. */
#define FSK_SVM_CV_MAX_PROBLEMS 65535
typedef struct fsk_svm_cv_problem {
    int64_t n_rows;          /* training rows of the problem                                                */
    int64_t iterations;
    double gap, objective, rho, C;
    int64_t n_sv, n_bsv;
    int32_t converged, fold; /* fold: the one held out                                                      */
    double reserved[2];
} fsk_svm_cv_problem;
typedef struct fsk_svm_cv_score {
    double C, auc, accuracy;
    double reserved;
} fsk_svm_cv_score;
typedef struct fsk_svm_cv_info {
    int64_t n;               /* training rows                                                               */
    int32_t n_folds, n_C;
    int32_t form;            /* 1: one workgroup a problem (k_svm_wg_batch); 2: two launches an iteration   */
    int32_t reserved0;
    int64_t launches;        /* kernel launches of the solves (the out-of-fold launch not counted)          */
    double ms;               /* host time of fsk_svm_cv                                                     */
    double reserved[4];
} fsk_svm_cv_info;
int fsk_svm_cv(fsk_engine* e, const int32_t* labels, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
               double eps, int64_t max_iter);
/* oof[n_C n], scores[n_C], problems[n_C n_folds], *info of the last fsk_svm_cv: every one may be NULL */
int fsk_svm_cv_get(fsk_engine* e, double* oof, fsk_svm_cv_score* scores, fsk_svm_cv_problem* problems, fsk_svm_cv_info* info);
/* alpha[n_train] of problem p, zero at its held-out rows */
int fsk_svm_cv_get_alpha(fsk_engine* e, int32_t p, double* alpha);

/* ---- the rows kernel: the SVM on the ROWS of the kernel matrix (the reference's kernel_type = "linear", fastsk.cpp:318-333,
 * and upstream's LinearSVC on Ktr: a linear model on the "empirical kernel map"), without the matrix leaving the device.
 *
 * With n = n_train and A(r, i) the normalised cell (r, i) of the finalized result — the IEEE value fsk_get_block returns,
 * whichever triangle holds the result —
 *   L(r, c)  = ((...((A(r,0) A(c,0)) + A(r,1) A(c,1)) + ...) + A(r,n-1) A(c,n-1))
 *   K2(r, c) = L(r, c) / sqrt(L(r, r) L(c, c))   (the three operations of every getter; a diagonal cell: L / sqrt(L L))
 * one accumulator a cell, summed in ascending i, every product and every sum a single correctly rounded fp64 operation (no
 * fused multiply-add, no split of the sum). L is computed for every cell with a train column and for the diagonal of the
 * test rows; an off-diagonal cell with both sequences in the test set is never computed and reads as 0.0. Only cells of the
 * result with a train column are read, so the rows kernel is whole under fsk_config.skip_test_block.
 *
 * fsk_rows_build: builds L (a packed fp64 triangle of N (N + 1) / 2 cells and its diagonal, resident beside the result)
 * from the finalized result; FSK_OK at once when it is there already. FSK_ESTATE before a finalized result; FSK_ENOMEM,
 * the message naming the bytes asked for, when L or the build's scratch (the normalised cells with a train column as fp64,
 * freed after the build) does not fit. A group handle works on engine 0's reduced triangle. The rows kernel belongs to the
 * result: whatever drops the SVM model drops it, and the getters then return FSK_ESTATE.
 * fsk_rows_get_block: cells [i0, i1) x [j0, j1) of the symmetric matrix, row-major, either order of (r, c): raw != 0 gives
 * L, raw = 0 gives K2. Range errors as fsk_get_block; FSK_ESTATE when no rows kernel is there (it does not build one).
 * fsk_svm_set_kernel: what fsk_svm_train and fsk_svm_cv solve on and fsk_svm_decision* read — FSK_SVM_KERNEL_RESULT (the
 * default): the normalised result; FSK_SVM_KERNEL_ROWS: K2, built when a train or a cross-validation needs it. K2 has a unit
 * diagonal, so the solver is the one of fsk_svm_train to the bit, fed K2; in a fold of fsk_svm_cv the held-out rows stay
 * feature columns (as in upstream's CalibratedClassifierCV on Ktr): one L serves every problem. A change of kind drops the
 * model and the cross-validation result; the kind stays with the handle. FSK_EINVAL on any other kind. */
enum { FSK_SVM_KERNEL_RESULT = 0, FSK_SVM_KERNEL_ROWS = 1 };
typedef struct fsk_rows_info {
    int64_t n_train, n_seq;
    int32_t tile, panel;     /* T and P of k_rows_syrk (the read-only tuning keys rows_tile, rows_panel)       */
    int64_t tiles;           /* T x T tiles computed by all builds of this handle so far                      */
    int64_t builds;          /* builds that launched                                                          */
    int64_t scratch_bytes;   /* the last build's fp64 scratch (freed)                                         */
    int64_t resident_bytes;  /* L and its diagonal                                                            */
    double ms_scratch;       /* the last build: the normalising passes into the scratch                       */
    double ms_product;       /*                 k_rows_syrk and k_rows_diag                                   */
    double reserved[4];
} fsk_rows_info;
int fsk_rows_build(fsk_engine* e);
int fsk_rows_get_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t raw, double* out);
int fsk_rows_get_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t raw, double* device_out);
int fsk_rows_get_info(fsk_engine* e, fsk_rows_info* out);
int fsk_svm_set_kernel(fsk_engine* e, int32_t kind);
int fsk_svm_get_kernel(fsk_engine* e, int32_t* kind);

/* ---- class weights and Platt probabilities: what the reference's svm_parameter carries as weight_label / weight and
 * probability = 1 (fastsk.hpp:26-30, fastsk.cpp:269-281), on the resident triangle.
 *
 * fsk_svm_set_class_weights: from then on fsk_svm_train and every problem of fsk_svm_cv solve LIBSVM's weighted C-SVC: the box
 * of row t is C_t = Cp = C w_pos where labels[t] = +1 and Cn = C w_neg where it is -1, each product formed once on the host
 * (one rounding). The algorithm is fsk_svm_train's with C_t in place of C: I_up and I_low test alpha_t against C_t; a step of
 * two rows of one class clips with that class's box; a step of two classes clips, after the clips at zero, by
 * `if (diff > C_i - C_j) { if (alpha_i > C_i) ... } else { if (alpha_j > C_j) ... }`, C_i - C_j one correctly rounded subtraction
 * (0.0 with equal weights: the code path is the unweighted one, to the bit and to the launch). rho's free support vectors are
 * 0 < alpha_t < C_t, its bounds and n_bsv count alpha_t >= C_t. The default is (1, 1). The weights stay with the handle, as
 * the kind of fsk_svm_set_kernel does; a call that changes them drops the model, the cross-validation result and the
 * calibration, a call with the values in force drops nothing. FSK_EINVAL unless both are positive finite numbers. */
int fsk_svm_set_class_weights(fsk_engine* e, double w_pos, double w_neg);
int fsk_svm_get_class_weights(fsk_engine* e, double* w_pos, double* w_neg);
/* fsk_svm_platt_fit: LIBSVM's sigmoid_train (Lin, Lin and Weng's form of Platt's fit) on n decision values and labels in
 * {-1, +1}, host only, no device and no handle: targets (n_pos + 1) / (n_pos + 2) and 1 / (n_neg + 2), start A = 0,
 * B = log((n_neg + 1) / (n_pos + 1)), Newton's method on H + 1e-12 I with a backtracking line search (sufficient decrease
 * 0.0001, smallest step 1e-10), at most 100 iterations, stop when both gradient entries are below 1e-5 — in LIBSVM's order
 * of operations, sums in index order, every operation a single correctly rounded double one, exp and log from libm.
 * FSK_EINVAL on a null pointer, n < 1 or a label that is not -1 or +1 (no message: there is no handle).
 * fsk_svm_calibrate: needs the model of fsk_svm_train (FSK_ESTATE before one). Solves, with the model's labels, C, eps,
 * max_iter, class weights and kernel kind, the n_folds problems "train on the rows with fold[t] != f" side by side — the
 * batch of fsk_svm_cv at the one C: same kernels, same choice of form — computes the out-of-fold decision values as
 * fsk_svm_cv does and runs fsk_svm_platt_fit on them. FSK_EINVAL, with fsk_svm_cv's messages: a fold id out of range, a fold
 * without rows, a fold whose training rows are of one class, n_folds < 2; a refused call leaves an earlier calibration. It
 * neither needs nor changes a stored cross-validation result, and fsk_svm_cv does not touch the calibration. The calibration
 * belongs to the model: whatever drops the model drops it, and so does a new fsk_svm_train.
 * fsk_svm_get_calibration: the out-of-fold decision values (n_train, may be NULL) and the fit (may be NULL).
 * fsk_svm_proba: P(y = +1) of rows r0 <= r < r1 <= N into a HOST array: fsk_svm_decision's values f, then LIBSVM's
 * sigmoid_predict on the host: with fApB = f A + B, exp(-fApB) / (1 + exp(-fApB)) where fApB >= 0, else 1 / (1 + exp(fApB)).
 * FSK_ESTATE without a calibration; range errors as fsk_svm_decision. */
typedef struct fsk_svm_platt_info {
    double A, B;             /* P(y = +1 | f) = 1 / (1 + exp(A f + B))                                       */
    int32_t iterations;      /* Newton iterations taken                                                     */
    int32_t status;          /* 0: gradient below 1e-5; 1: 100 iterations; 2: line search failed            */
    int32_t n_folds, form;   /* of the fold solves (form as in fsk_svm_cv_info); 0 from fsk_svm_platt_fit   */
    int64_t launches;        /* kernel launches of the fold solves                                          */
    double ms;               /* host time of fsk_svm_calibrate                                              */
    double reserved[4];
} fsk_svm_platt_info;
int fsk_svm_platt_fit(const double* dec, const int32_t* labels, int64_t n, fsk_svm_platt_info* out);
int fsk_svm_calibrate(fsk_engine* e, const int32_t* fold, int32_t n_folds);
int fsk_svm_get_calibration(fsk_engine* e, double* oof, fsk_svm_platt_info* out);
int fsk_svm_proba(fsk_engine* e, int64_t r0, int64_t r1, double* out);

/* ---- epsilon-SVR on the resident triangle: real-valued targets (what read_data(..., regression=True) loads), LIBSVM's
 * EPSILON_SVR without the kernel matrix leaving the device.
 *
 * fsk_svr_train: targets[t] finite, t < n = n_train >= 2. LIBSVM's formulation: 2n variables, element e < n is alpha_e with
 * y = +1, element e + n is alpha*_e with y = -1, both stand for kernel row e: Q(e, f) = y_e y_f K(e mod n, f mod n); the
 * linear term is p_e = epsilon - targets[e] and p_{e+n} = epsilon + targets[e] (one rounding each, on the host); alpha = 0 and
 * G = p at the start; one box C for all. The iteration is fsk_svm_train's, operation for operation, over the 2n elements, ties
 * to the lowest element in [0, 2n): the results do not depend on the form that ran (one workgroup while 2n <= svm_wg_max, two
 * launches an iteration beyond — each thread owns both twins of a row, so a kernel cell is read once for the two), on
 * svm_chunk or on the grid. Finished on the host in element order as LIBSVM does: rho by calculate_rho over the 2n elements,
 * objective = 1/2 sum alpha_e (G_e + p_e), coef[t] = alpha_t - alpha*_t; fsk_svm_info.n_sv counts coef != 0, n_bsv
 * |coef| >= C. max_iter, the kernel kind of fsk_svm_set_kernel and a group handle as for fsk_svm_train. Class weights do not
 * apply to a regression (LIBSVM ignores them there): fsk_svm_set_class_weights changes nothing in a solve of these calls.
 * FSK_ESTATE before a finalized result; FSK_EINVAL, with a message: n != n_train, n < 2, a target that is not finite, C not
 * positive and finite, epsilon < 0 or not finite, eps not positive and finite. A refused call leaves the earlier model.
 * THE MODEL SLOT is one: an SVR model replaces a C-SVC model and the reverse, and whatever drops the one drops the other.
 * fsk_svm_decision(_device) serve either: sum_i coef_i K(r, i) - rho. fsk_svm_get_model, fsk_svm_calibrate,
 * fsk_svm_get_calibration and fsk_svm_proba on an SVR model, and fsk_svr_get_model on a C-SVC model, return FSK_ESTATE with a
 * message that names the kind of the model.
 * fsk_svr_get_model: alpha2[2 n_train] (alpha, then alpha*), coef[n_train], *rho, *info; every one may be NULL.
 *
 * fsk_svr_cv: problem p = (c n_eps + q) n_folds + f trains at (Cs[c], epsilons[q]) on the rows with fold[t] != f, all side by
 * side in the batch launches, each to the bit fsk_svr_train on its sub-matrix (form 1 while twice the largest training set is
 * at most svm_wg_max). Then oof[(c n_eps + q) n + t] = sum_i coef_i K(t, i) - rho of problem (c n_eps + q) n_folds + fold[t],
 * summed as fsk_svm_decision sums, and per grid point on the host, every sum a plain loop over the rows in row order, one
 * accumulator each, z = targets:
 *   zm = (sum z_t) / n, om = (sum oof_t) / n; then in ONE pass d = oof_t - z_t, dz = z_t - zm, dq = oof_t - om:
 *   sse += d d, sae += |d|, sst += dz dz, soo += dq dq, szo += dq dz;
 *   mse = sse / n, mae = sae / n, r2 = 1 - sse / sst, r = szo / sqrt(soo sst)   (constant targets: sst = 0, r2 and r are not numbers).
 * fsk_svm_cv_problem.reserved[0] holds the problem's epsilon, fsk_svm_cv_info.reserved0 n_eps. Limits and refusals are
 * fsk_svm_cv's (FSK_SVM_CV_MAX_PROBLEMS, a fold without rows, a fold id out of range, n_folds < 2, n_C or n_eps < 1, a C,
 * epsilon or eps out of range, a fold that leaves fewer than 2 training rows) and fsk_svr_train's for the targets; a refused
 * call leaves the earlier result. The result lives beside fsk_svm_cv's and under the same rules; neither touches the model. */
typedef struct fsk_svr_cv_score {
    double C, epsilon;
    double mse, mae, r2, r;
    double reserved[2];
} fsk_svr_cv_score;
int fsk_svr_train(fsk_engine* e, const double* targets, int64_t n, double C, double epsilon, double eps, int64_t max_iter);
int fsk_svr_get_model(fsk_engine* e, double* alpha2, double* coef, double* rho, fsk_svm_info* info);
int fsk_svr_cv(fsk_engine* e, const double* targets, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
               const double* epsilons, int32_t n_eps, double eps, int64_t max_iter);
/* oof[n_C n_eps n], scores[n_C n_eps], problems[n_C n_eps n_folds], *info of the last fsk_svr_cv: every one may be NULL */
int fsk_svr_cv_get(fsk_engine* e, double* oof, fsk_svr_cv_score* scores, fsk_svm_cv_problem* problems, fsk_svm_cv_info* info);

/* ---- multi-class C-SVC, one-vs-one, on the resident triangle: what LIBSVM's C-SVC does with more than two classes, every
 * pair of classes solved side by side in the batch launches of fsk_svm_cv.
 *
 * fsk_svm_train_multiclass: labels[t], t < n = n_train, are any int32 values; the classes are the distinct values in ascending
 * order, classes[0] < ... < classes[k-1], 2 <= k <= FSK_SVM_MAX_CLASSES (more: FSK_EUNSUPPORTED). Pair p runs over (a, b),
 * a < b, in lexicographic order of the class indices (P = k (k - 1) / 2; scikit-learn's decision_function_shape="ovo" order).
 * Its problem is the training rows of class a or b IN ASCENDING ROW ORDER, class a as y = +1 and class b as y = -1, with the
 * boxes Cp = C w[a], Cn = C w[b] (class_weight[k] by class index, each product formed once; NULL: every w = 1). The class
 * weights of fsk_svm_set_class_weights are neither consulted nor changed; fsk_svm_set_kernel applies as to fsk_svm_train. A
 * pair is fsk_svm_train's algorithm on its sub-matrix, to the bit, whichever form ran (form 1 while the LARGEST pair has at
 * most svm_wg_max rows), finished on the host as a problem of fsk_svm_cv is.
 * NOT LIBSVM'S ORDER: LIBSVM groups the rows by class before it solves a pair (all of class a, then all of class b). The
 * sub-problems here are in ascending row order, so that every tie falls as in fsk_svm_train on the same rows: a pair's alpha
 * equals this project's restatement bit for bit, and LIBSVM's only within the stopping tolerance.
 * The model takes the one model slot: fsk_svm_get_model, fsk_svm_decision(_device), fsk_svm_calibrate,
 * fsk_svm_get_calibration, fsk_svm_proba and fsk_svr_get_model then return FSK_ESTATE with a message that names the model, and
 * the calls below return it on a C-SVC or an SVR model. A later fsk_svm_train or fsk_svr_train replaces it; what drops a model
 * drops it. FSK_EINVAL: n != n_train, one class only, a weight, C or eps that is not a positive finite number. A refused call
 * leaves the earlier model as it was.
 * fsk_svm_multiclass_get_model: classes[k], pairs[P], alpha (the pairs' alpha one after another in pair order, pair p at its
 * own length n_rows and in its own row order: (k - 1) n_train values in all), *info; every one may be NULL (call with info
 * alone to learn k).
 * fsk_svm_multiclass_decision: for rows r0 <= r < r1 <= N of the sequences, dec[(r - r0) P + p] = sum_q coef_p[q] K(r, row_p[q])
 * - rho_p over pair p's own row list — a lane of a wave takes the list positions lane, lane + 64, ... in order, zero
 * coefficients skipped, then the xor shuffles, as fsk_svm_decision sums — and pred[r - r0] the label that wins LIBSVM's vote:
 * dec_p > 0 votes for class a, anything else for class b; most votes win, the lowest class among equals. Either output may be
 * NULL. Only cells with a train column are read. The _device form writes DEVICE memory of the caller.
 *
 * fsk_svm_multiclass_cv: problem (c n_folds + f) P + p trains pair p at Cs[c] on its rows with fold[t] != f; all n_C n_folds P
 * <= FSK_SVM_CV_MAX_PROBLEMS problems in one batch. The out-of-fold label of row t at Cs[c] is the vote of the P problems of
 * (c, fold[t]); accuracy[c] = #{t: label == labels[t]} / n, an integer count divided once. There is no AUC for more than two
 * classes: fsk_svm_cv_score.auc is NaN. fsk_svm_cv_problem.reserved[0], [1] hold the pair's class_a, class_b (label values,
 * exact in a double); fsk_svm_cv_info.reserved0 holds k. FSK_EINVAL, beyond fsk_svm_cv's refusals (which stay, but for the
 * label values): a fold whose training rows hold no row of some class, the message naming the class and the fold. The result
 * lives beside fsk_svm_cv's: neither call disturbs the other's, nor any model. */
#define FSK_SVM_MAX_CLASSES 64  /* one vote counter a lane of a wave */
typedef struct fsk_svm_multiclass_pair {
    int32_t class_a, class_b;   /* label values: y = +1 / y = -1 of the pair's problem                   */
    int64_t n_rows, iterations;
    double gap, objective, rho;
    int64_t n_sv, n_bsv;
    int32_t converged, reserved0;
    double reserved[2];
} fsk_svm_multiclass_pair;
typedef struct fsk_svm_multiclass_info {
    int32_t k, n_pairs;
    int32_t form;            /* 1: one workgroup a pair (k_svm_wg_batch); 2: two launches an iteration      */
    int32_t reserved0;
    int64_t launches;        /* kernel launches of the solves                                               */
    int64_t n_sv;            /* training rows that are a support vector of any pair                         */
    int64_t n_alpha;         /* length of the concatenated alpha: (k - 1) n_train                           */
    double ms;               /* host time of fsk_svm_train_multiclass                                       */
    double reserved[4];
} fsk_svm_multiclass_info;
int fsk_svm_train_multiclass(fsk_engine* e, const int32_t* labels, int64_t n, double C, const double* class_weight, double eps,
                             int64_t max_iter);
int fsk_svm_multiclass_get_model(fsk_engine* e, int32_t* classes, fsk_svm_multiclass_pair* pairs, double* alpha,
                                 fsk_svm_multiclass_info* info);
int fsk_svm_multiclass_decision(fsk_engine* e, int64_t r0, int64_t r1, double* dec, int32_t* pred);
int fsk_svm_multiclass_decision_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_dec, int32_t* device_pred);
int fsk_svm_multiclass_cv(fsk_engine* e, const int32_t* labels, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs,
                          int32_t n_C, const double* class_weight, double eps, int64_t max_iter);
/* pred[n_C n] (out-of-fold labels), scores[n_C], problems[n_C n_folds P], *info of the last fsk_svm_multiclass_cv: every one
 * may be NULL */
int fsk_svm_multiclass_cv_get(fsk_engine* e, int32_t* pred, fsk_svm_cv_score* scores, fsk_svm_cv_problem* problems,
                              fsk_svm_cv_info* info);

/* ---- class probabilities of the multi-class model: a Platt sigmoid a pair and pairwise coupling on the device — what
 * LIBSVM's svm_parameter.probability = 1 gives (svm_binary_svc_probability, sigmoid_train, svm_predict_probability with
 * multiclass_probability, Wu, Lin and Weng's second method).
 *
 * fsk_svm_multiclass_calibrate: needs the model of fsk_svm_train_multiclass (FSK_ESTATE naming the model otherwise). fold[t],
 * t < n_train, in 0..n_folds-1 as for fsk_svm_calibrate. Problem f P + p is pair p on the rows of its two classes with
 * fold[t] != f, in ascending row order, with the model's boxes C w[a], C w[b], its eps, max_iter and kernel kind; all n_folds P
 * problems are solved in one batch (fsk_svm_multiclass_cv with the model's one C; its limits and refusals apply, FSK_EINVAL
 * with its messages: a fold id out of range, a fold without rows, n_folds < 2, a fold whose training rows lack a class — naming
 * class and fold). Then oof[t P + p] is the decision value of row t under problem fold[t] P + p, summed as
 * fsk_svm_multiclass_decision sums, and for every pair fsk_svm_platt_fit runs on the oof values of the rows of classes a and
 * b, ascending, label +1 for class a: A[p], B[p].
 * NOT LIBSVM'S FOLDS AND ORDER: LIBSVM shuffles each pair's rows on its own (rand()) into 5 folds and solves each fold's
 * sub-problem grouped by class. Here the folds are ONE assignment over all rows, given by the caller (a stratified draw in the
 * Python layer), and the sub-problems are in ascending row order, as the fit's are. A and B therefore equal this project's
 * restatement bit for bit and LIBSVM's only statistically.
 * The calibration belongs to the model: a later fsk_svm_train_multiclass, fsk_svm_train or fsk_svr_train drops it, and so does
 * whatever drops the model; a refused call leaves the earlier one. A stored fsk_svm_multiclass_cv result is neither needed nor
 * touched.
 * fsk_svm_multiclass_get_calibration: oof[n_train P] and fits[P] (A, B, iterations, status of every pair; n_folds, form,
 * launches and ms of the whole call in each); either may be NULL. After fsk_svm_multiclass_set_calibration there are no
 * out-of-fold values: asking for oof is FSK_ESTATE, the fits hold A and B alone.
 * fsk_svm_multiclass_set_calibration: installs the P sigmoids A[p], B[p] on the model without a solve (a saved calibration put
 * back). FSK_EINVAL where an A is not finite; B is not checked.
 *
 * fsk_svm_multiclass_proba: for rows r0 <= r < r1 <= N, one launch (k_svm_ovo_proba): the pairs' decision values v_p as above;
 * LIBSVM's sigmoid_predict with fApB = v_p A[p] + B[p] (two roundings): e / (1 + e), e = fsk_exp_neg(-fApB), where fApB >= 0,
 * else 1 / (1 + fsk_exp_neg(fApB)); clamped as LIBSVM clamps, (x > 1e-7 ? x : 1e-7) then (y < 1 - 1e-7 ? y : 1 - 1e-7), so a NaN
 * becomes 1e-7; r[a][b] that value, r[b][a] = 1 - r[a][b]. k = 2: prob = (r[0][1], r[1][0]), iters = 0. Otherwise
 * multiclass_probability operation for operation, one rounding each: Q[t][t] = sum_{j != t} r[j][t]^2 in ascending j,
 * Q[t][j] = -(r[j][t] r[t][j]), p = 1 / k, eps = 0.005 / k, at most max(100, k) iterations, each: Qp[t] = sum_j Q[t][j] p[j]
 * and pQp = sum_t p[t] Qp[t] in ascending order from 0.0; stop when max_t |Qp[t] - pQp| < eps; else for t = 0 .. k - 1 in turn
 * diff = (-Qp[t] + pQp) / Q[t][t], p[t] += diff, pQp = (pQp + diff (diff Q[t][t] + 2 Qp[t])) / (1 + diff) / (1 + diff), and
 * for all j Qp[j] = (Qp[j] + diff Q[t][j]) / (1 + diff), p[j] /= (1 + diff).
 * prob[(r - r0) k + c] is the probability of classes[c]; pred[r - r0] the label of the largest (the lowest class among equals:
 * LIBSVM's svm_predict_probability label, which need not be the vote's); iters[r - r0] the iterations taken. Each output may
 * be NULL. The _device form writes DEVICE memory of the caller. FSK_ESTATE before a calibration ("no calibration: ...") and,
 * naming the model, on a C-SVC or an SVR model; FSK_EINVAL for rows out of range.
 * fsk_svm_calibrate, fsk_svm_get_calibration and fsk_svm_proba stay the binary model's and keep refusing this one.
 *
 * fsk_exp_neg: exp(x) for x <= 0 as a fixed sequence of IEEE double operations, the same bits on the host and on the device:
 * NaN -> NaN; x < -708 -> 0.0 (no subnormal is formed); else n = floor(x (1 / ln 2) + 0.5), r = (x - n ln2_hi) - n ln2_lo
 * (Cody and Waite), the Taylor polynomial of degree 13 in r by Horner, times 2^n. Within 2 ulp of a correctly rounded exp on
 * [-708, 0] (measured: 1). x > 0 is not supported. Host only, no device needed. */
int fsk_svm_multiclass_calibrate(fsk_engine* e, const int32_t* fold, int32_t n_folds);
int fsk_svm_multiclass_get_calibration(fsk_engine* e, double* oof, fsk_svm_platt_info* fits);
int fsk_svm_multiclass_set_calibration(fsk_engine* e, const double* A, const double* B);
int fsk_svm_multiclass_proba(fsk_engine* e, int64_t r0, int64_t r1, double* prob, int32_t* pred, int32_t* iters);
int fsk_svm_multiclass_proba_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_prob, int32_t* device_pred,
                                    int32_t* device_iters);
double fsk_exp_neg(double x);

/* ---- helpers shared with the host side --------------------------------------------------- */
int64_t fsk_num_combos(int32_t g, int32_t m);                              /* nchoosek */
int fsk_combo_positions(int32_t g, int32_t k, int64_t combo, int32_t* out); /* getCombinations */
/* the permutation of 0..n-1 that std::shuffle(begin, end, std::default_random_engine{seed}) of libstdc++ produces
 * (fastsk_kernel.cpp:31-38 with n = C(g,m) and seed = time(0)); host only */
int fsk_seed_order(uint64_t seed, int64_t n, int32_t* out);
/* the solver of fsk_set_mismatch_weights on its own: weights c[0..n-1] (n <= g, c[0] >= 1) at window length g ->
 * coefficients a[0..d] (room for n) and *n_levels = d + 1, d the last h with c[h] != 0; FSK_EINVAL as above; host only */
int fsk_mismatch_levels(int32_t g, const uint64_t* c, int32_t n, int64_t* a, int32_t* n_levels);


/* ---- input: native counterpart of FastaUtility.read_data + Vocabulary (src/fastsk/utils.py:5-96)
 * Alternating ">label" / sequence lines; every line stripped and lower-cased; labels in {-1,0,1};
 * token ids in first-seen order from *next_id (1 for a fresh vocabulary; id 0 stays reserved),
 * kept in vocab256[byte] (0 = not seen yet) so that successive files share ids as the files read
 * through one FastaUtility do. Host only, no device needed. Call once with tokens = offsets =
 * labels = NULL to learn *n_seq and *n_tokens (the vocabulary is already updated; the second call
 * finds every symbol assigned), then with buffers tokens[n_tokens], offsets[n_seq + 1],
 * labels[n_seq]. Returns FSK_EINVAL on a malformed file (where the reference's asserts fire) and
 * FSK_EUNSUPPORTED on non-ASCII bytes (the caller's text-mode fallback handles those); the message
 * goes to err[err_cap]. */
int fsk_read_fasta(const char* path, int32_t* vocab256, int32_t* next_id, int32_t* tokens, int64_t tokens_cap,
                   int64_t* offsets, int32_t* labels, int64_t seq_cap, int64_t* n_seq, int64_t* n_tokens, char* err,
                   int32_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* FASTSK_AMD_H */
