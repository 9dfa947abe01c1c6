// fsk_engine_svm.hip — the SVM stage on the resident result triangle: fsk_svm_train, fsk_svm_get_model, fsk_svm_decision(_device),
// fsk_svm_cv, fsk_svm_cv_get(_alpha), the class weights (fsk_svm_set_class_weights) and the Platt calibration
// (fsk_svm_platt_fit, fsk_svm_calibrate, fsk_svm_get_calibration, fsk_svm_proba), the epsilon-SVR (fsk_svr_train,
// fsk_svr_get_model, fsk_svr_cv, fsk_svr_cv_get) and the one-vs-one multi-class C-SVC (fsk_svm_train_multiclass,
// fsk_svm_multiclass_get_model, fsk_svm_multiclass_decision(_device), fsk_svm_multiclass_cv, fsk_svm_multiclass_cv_get) with its
// probabilities (fsk_svm_multiclass_calibrate, fsk_svm_multiclass_get_calibration, fsk_svm_multiclass_set_calibration,
// fsk_svm_multiclass_proba(_device), fsk_exp_neg) of include/fastsk_amd.h. What FastSK::fit / FastSK::score do with LIBSVM on the host
// (fastsk.cpp:239-530), for the sequences of one compute call and without the kernel matrix ever leaving the device: the
// engine's consumer is an SVM, and the triangle it needs is 40 GB at 100,000 sequences.
//
// The solver (fsk_kernels_svm.h) reads the triangle in place, whichever it is — u64 counts with the raw diagonal, the fp64
// triangle of variance mode, the folded W of the mismatch-weighted mode (u64 as well) — through normalised_cell. Two forms of
// the same arithmetic: one workgroup with alpha, G and y in LDS up to svm_wg_max rows (the EP300-size problems, which two
// launches an iteration would leave launch-bound), two launches an iteration beyond. The host enqueues svm_chunk iterations,
// reads one status record, and goes on until it says done; launches that follow convergence inside a chunk return at once.
// No cooperative launch, no grid barrier, no graph. A translation unit of its own: nothing here reaches another kernel.
//
// BYTES AN ITERATION, two-launch form, n rows (the one statement; DESIGN.md and tools/bench_svm.py refer to it). Launch B reads
// alpha, G (8 n each), y (n) and row i (8 n), and writes the kept row (8 n): 33 n. Launch A reads alpha, G, y, the kept row and
// row j, and writes G: 41 n. 74 n at the least. A row is 8 i contiguous bytes and one cell of each of the n - i later triangle
// rows, a 64-byte line each: a middle row (i = n / 2) moves 4 n + 32 n = 36 n instead of 8 n, so 74 n + 2 x 28 n = 130 n with lines.
// The epsilon-SVR (fsk_svr_train: 2n elements on n rows, a thread owns both twins of a row): the bytes of KERNEL ROWS an iteration
// are those of an n-row C-SVC solve, not of a 2n-row one — row i and row j once each, 16 n (72 n with lines), for the two twins
// together. What doubles is the state: launch B reads alpha and G of 2n elements (32 n) and row i (8 n) and writes the kept row
// (8 n): 48 n; launch A reads alpha, G (32 n), the kept row and row j (16 n) and writes G (16 n): 64 n. 112 n at the least (no y is
// read: the sign is the half), 168 n with lines — against 148 n / 260 n for a C-SVC of 2n rows.
#include "fsk_engine_internal.h"
#include "fsk_kernels_svm.h"

using namespace fsk_detail;

namespace {

constexpr int64_t SVM_DEFAULT_MAX_ITER = 10000000;

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the records of a solve inside SvmState::d_rec
struct SvmRecords {
    fsk::SvmRecB* rb;
    fsk::SvmRecA* ra;
    fsk::SvmCandI* ci;
    fsk::SvmCandJ* cj;
};
size_t svm_record_bytes(uint32_t n_wg) {
    return 256 + 256 + (size_t)n_wg * (sizeof(fsk::SvmCandI) + sizeof(fsk::SvmCandJ));
}
SvmRecords svm_records(unsigned char* base, uint32_t n_wg) {
    SvmRecords r;
    r.rb = reinterpret_cast<fsk::SvmRecB*>(base);
    r.ra = reinterpret_cast<fsk::SvmRecA*>(base + 256);
    r.ci = reinterpret_cast<fsk::SvmCandI*>(base + 512);
    r.cj = reinterpret_cast<fsk::SvmCandJ*>(base + 512 + (size_t)n_wg * sizeof(fsk::SvmCandI));
    return r;
}
static_assert(sizeof(fsk::SvmRecB) <= 256 && sizeof(fsk::SvmRecA) <= 256 && sizeof(fsk::SvmCandI) % 8 == 0 && sizeof(fsk::SvmCandJ) % 8 == 0,
              "record layout");

// THE polling loop of every solve: `enqueue` puts one chunk of iterations on the stream, the n_rec status records (one of a
// single solve, P of a batch) come back in one copy, until every one says done. Launches that follow a problem's end inside a
// chunk return at once.
template <typename Enqueue>
int svm_poll(fsk_engine* e, const fsk::SvmRecB* rb, fsk::SvmRecB* status, uint32_t n_rec, Enqueue enqueue) {
    for (;;) {
        enqueue();
        FSK_HIP(hipMemcpyAsync(status, rb, (size_t)n_rec * sizeof(fsk::SvmRecB), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
        FSK_HIP(hipGetLastError());
        bool all = true;
        for (uint32_t p = 0; p < n_rec; ++p) all = all && status[p].done;
        if (all) return FSK_OK;
    }
}

// One problem. Form 1: one workgroup, alpha / G / y in LDS, a launch of up to `chunk` iterations a chunk; form 2: two launches
// an iteration, `chunk` (A, B) pairs a chunk.
template <typename SrcT>
int solve(fsk_engine* e, const SrcT* K, const double* diag, uint32_t n, double Cp, double Cn, double eps, int64_t max_iter, int form, uint32_t chunk, const SvmRecords& R,
          uint32_t n_wg, fsk::SvmRecB* status, int64_t* launches) {
    double *alpha = e->svm.d_alpha.p, *G = e->svm.d_G.p, *krow = e->svm.d_krow.p;  // (plain pointers: a launch takes its arguments by value)
    const signed char* y = e->svm.d_y.p;
    if (form == 1) {
        const uint32_t nt = std::min<uint32_t>(fsk::SVM_WG_THREADS, (n + 63u) & ~63u);
        const size_t lds = fsk::svm_wg_lds(n, nt);
        if (lds > 160 * 1024) return e->fail(FSK_EUNSUPPORTED, "k_svm_wg needs %zu bytes of LDS for %u rows", lds, n);
        FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_svm_wg<SrcT>, lds));
        return svm_poll(e, R.rb, status, 1, [=] {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_wg<SrcT>), dim3(1), dim3(nt), lds, e->stream, K, diag, n, Cp, Cn, eps, (long long)max_iter, chunk,
                       alpha, G, y, R.rb);
            ++*launches;
        });
    }
    return svm_poll(e, R.rb, status, 1, [=] {
        for (uint32_t c = 0; c < chunk; ++c) {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_i<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, Cp, Cn, alpha, G, y,
                       (const double*)krow, (const fsk::SvmRecB*)R.rb, R.ra, R.ci, (const fsk::SvmCandJ*)R.cj, n_wg);
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_j<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, Cp, Cn, eps,
                       (long long)max_iter, (const double*)alpha, (const double*)G, y, krow, R.rb, (const fsk::SvmRecA*)R.ra,
                       (const fsk::SvmCandI*)R.ci, R.cj, n_wg);
            *launches += 2;
        }
    });
}

// rho and the objective as LIBSVM's calculate_rho / calculate_objective_value, in element order, the box of an element by its
// class (Cp, Cn); coef[t] = alpha_t y_t
struct SvmFinish {
    double rho, objective;
    int64_t n_sv, n_bsv;
};
SvmFinish svm_finish(const double* alpha, const double* G, const signed char* y, uint32_t n, double Cp, double Cn, double* coef) {
    double ub = HUGE_VAL, lb = -HUGE_VAL, sum_free = 0.0, obj = 0.0;
    int64_t n_free = 0, n_sv = 0, n_bsv = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const double a = alpha[t], yG = y[t] > 0 ? G[t] : -G[t], C = y[t] > 0 ? Cp : Cn;
        if (a >= C) {
            if (y[t] < 0) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else if (a <= 0.0) {
            if (y[t] > 0) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else {
            ++n_free;
            sum_free += yG;
        }
        obj += a * (G[t] - 1.0);
        n_sv += a > 0.0;
        n_bsv += a >= C;
        coef[t] = y[t] > 0 ? a : -a;
    }
    return {n_free > 0 ? sum_free / (double)n_free : (ub + lb) / 2.0, obj / 2.0, n_sv, n_bsv};
}

// THE place that chooses what the stage solves on and reads (fsk_svm_set_kernel): the normalised result — u64 counts or the
// fp64 triangle, with the raw diagonal of make_diag — or the rows kernel, an fp64 triangle with its own raw diagonal
// (fsk_engine_rows.hip), which the <double> instantiations read through the same normalised_cell. build: a train or a
// cross-validation builds the rows kernel when it is not there; a decision needs a model, and a model of that kind has it.
struct SvmSource {
    bool f64;
    const u64* Ku;
    const double* Kf;
    const double* diag;
};
int svm_source(fsk_engine* e, bool build, SvmSource* s) {
    if (e->svm.kernel == FSK_SVM_KERNEL_ROWS) {
        if (build) { int rc = rows_build(e); if (rc) return rc; }
        else if (!e->rows.valid) return e->fail(FSK_ESTATE, "no rows kernel: the model's kernel is gone");
        *s = SvmSource{true, nullptr, e->rows.d_L.p, e->rows.d_diag.p};
    } else {
        *s = SvmSource{e->result_f64, e->d_K, e->d_Kf64.p, e->d_diag.p};
    }
    return FSK_OK;
}
// THE place that turns the source into a type: f(K) with K the u64 or the fp64 triangle; f's kernels are those of SrcOf<K>
template <typename F>
int svm_on_source(const SvmSource& s, F f) { return s.f64 ? f(s.Kf) : f(s.Ku); }
template <typename P>
using SrcOf = std::remove_const_t<std::remove_pointer_t<P>>;

// What fsk_svm_train and cv_run check alike: a finalized result, labels (null_text: what to say where the caller's arrays are
// not all there), one a training sequence, each -1 or +1 (n_pos: how many are +1), and eps.
int svm_check_problem(fsk_engine* e, const int32_t* labels, const char* null_text, int64_t n, double eps, int64_t* n_pos) {
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (!labels) return e->fail(FSK_EINVAL, "%s", null_text);
    if (n != e->n_train) return e->fail(FSK_EINVAL, "%lld labels for %lld training sequences", (long long)n, (long long)e->n_train);
    if (!(eps > 0.0) || !std::isfinite(eps)) return e->fail(FSK_EINVAL, "eps must be a positive finite number");
    *n_pos = 0;
    for (int64_t t = 0; t < n; ++t) {
        if (labels[t] != 1 && labels[t] != -1) return e->fail(FSK_EINVAL, "label %lld is %d: labels must be -1 or +1", (long long)t, labels[t]);
        *n_pos += labels[t] > 0;
    }
    return FSK_OK;
}

int model_ready(fsk_engine* e) {
    if (!e->finalized || !e->svm.valid) return e->fail(FSK_ESTATE, "no model: call fsk_svm_train on a finalized result first");
    return FSK_OK;
}
// The one model slot holds a C-SVC (fsk_svm_train), an epsilon-SVR (fsk_svr_train) or a one-vs-one multi-class C-SVC
// (fsk_svm_train_multiclass): the calls that are one kind's alone
constexpr int MODEL_SVC = 0, MODEL_SVR = 1, MODEL_MC = 2;
const char* model_text(int kind) {
    return kind == MODEL_SVR ? "an epsilon-SVR (fsk_svr_train)" : kind == MODEL_MC ? "a multi-class C-SVC (fsk_svm_train_multiclass)" : "a C-SVC (fsk_svm_train)";
}
int model_of_kind(fsk_engine* e, int kind, const char* call) {
    int rc = model_ready(e);
    if (rc) return rc;
    if (e->svm.model_kind != kind) return e->fail(FSK_ESTATE, "%s: the model is %s", call, model_text(e->svm.model_kind));
    return FSK_OK;
}

// the rows [r0, r1) into device memory at `dst`
int launch_decision(fsk_engine* e, int64_t r0, int64_t r1, double* dst) {
    const uint32_t blocks = (uint32_t)((r1 - r0 + 3) / 4), n_train = (uint32_t)e->n_train, a = (uint32_t)r0, b = (uint32_t)r1;
    SvmSource src;
    { int rc = svm_source(e, false, &src); if (rc) return rc; }
    const double *diag = src.diag, *coef = e->svm.d_coef.p;
    const double rho = e->svm.rho;
    return svm_on_source(src, [=](auto* K) -> int {
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_decision<SrcOf<decltype(K)>>), dim3(blocks), dim3(256), 0, e->stream, K, diag, coef, n_train, a, b, rho, dst);
        return FSK_OK;
    });
}

int decision_args(fsk_engine* e, int64_t r0, int64_t r1, const double* out) {
    int rc = model_ready(e);
    if (rc) return rc;
    if (e->svm.model_kind == MODEL_MC) return e->fail(FSK_ESTATE, "fsk_svm_decision: the model is %s", model_text(MODEL_MC));  // (one value a row: a C-SVC's or an SVR's)
    if (r0 < 0 || r1 > e->N || r0 > r1) return e->fail(FSK_EINVAL, "rows out of range");
    if (r1 > r0 && !out) return e->fail(FSK_EINVAL, "null output");
    return FSK_OK;
}

// ---- the batch of fsk_svm_cv ------------------------------------------------------------------------------------------------
// BYTES AN ITERATION OF A BATCH (the one statement; DESIGN.md and tools/bench_svm_cv.py refer to it). Problem p of n_p rows moves
// what a single solve of n_p rows moves, and 4 n_p bytes of row numbers for every pass over its elements that reads cells.
// Workgroup form (alpha, G and y in LDS): the cells of rows i and j, 16 n_p, and the row numbers once (kept in registers from
// step 2 to step 4): 20 n_p. Two-launch form: 74 n_p as above and the row numbers in either launch: 82 n_p. A row of cells is
// no longer contiguous where rows are held out, but touches no 64-byte line the full row does not. The batch moves the sum
// over its live problems; a problem that is done costs one record a workgroup of every further launch.
struct SvmBatch {
    uint32_t P, max_n, max_wg, total_wg;
    const fsk::SvmProb* probs;
    const uint32_t* idx;
    const signed char* y;
    double *alpha, *G, *krow;
    fsk::SvmRecB* rb;   // [P], read by the host in one copy
    fsk::SvmRecA* ra;   // [P]
    fsk::SvmCandI* ci;  // [total_wg]
    fsk::SvmCandJ* cj;
};
size_t svm_batch_record_bytes(uint32_t P, uint32_t total_wg) {
    return (size_t)P * (sizeof(fsk::SvmRecB) + sizeof(fsk::SvmRecA)) + (size_t)total_wg * (sizeof(fsk::SvmCandI) + sizeof(fsk::SvmCandJ));
}
static_assert(sizeof(fsk::SvmRecB) % 8 == 0 && sizeof(fsk::SvmRecA) % 8 == 0 && sizeof(fsk::SvmProb) == 40, "batch record layout");

// the batch in the two forms of solve(): a chunk is `chunk` iterations of every problem that is not done
template <typename SrcT>
int solve_batch(fsk_engine* e, const SrcT* K, const double* diag, const SvmBatch& B, double eps, int64_t max_iter, int form, uint32_t chunk,
                fsk::SvmRecB* status, int64_t* launches) {
    if (form == 1) {
        const uint32_t nt = std::min<uint32_t>(fsk::SVM_WG_THREADS, (B.max_n + 63u) & ~63u);
        const size_t lds = fsk::svm_wg_lds(B.max_n, nt);
        if (lds > 160 * 1024) return e->fail(FSK_EUNSUPPORTED, "k_svm_wg_batch needs %zu bytes of LDS for %u rows", lds, B.max_n);
        FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_svm_wg_batch<SrcT>, lds));
        return svm_poll(e, B.rb, status, B.P, [=] {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_wg_batch<SrcT>), dim3(B.P), dim3(nt), lds, e->stream, K, diag, B.probs, B.idx, B.y, eps,
                       (long long)max_iter, chunk, B.alpha, B.G, B.rb);
            ++*launches;
        });
    }
    return svm_poll(e, B.rb, status, B.P, [=] {
        for (uint32_t c = 0; c < chunk; ++c) {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_i_batch<SrcT>), dim3(B.max_wg, B.P), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag,
                       B.probs, B.idx, B.y, B.alpha, B.G, (const double*)B.krow, (const fsk::SvmRecB*)B.rb, B.ra, B.ci,
                       (const fsk::SvmCandJ*)B.cj);
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_j_batch<SrcT>), dim3(B.max_wg, B.P), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag,
                       B.probs, B.idx, B.y, eps, (long long)max_iter, (const double*)B.alpha, (const double*)B.G, B.krow, B.rb,
                       (const fsk::SvmRecA*)B.ra, (const fsk::SvmCandI*)B.ci, B.cj);
            *launches += 2;
        }
    });
}

// (#{pos > neg} + 0.5 #{pos == neg}) / (n_pos n_neg) and the share of rows on the right side of zero
void cv_metrics(const double* oof, const int32_t* labels, int64_t n, double* auc, double* accuracy) {
    std::vector<double> pos, neg;
    int64_t right = 0;
    bool numbers = true;
    for (int64_t t = 0; t < n; ++t) {
        (labels[t] > 0 ? pos : neg).push_back(oof[t]);
        right += (oof[t] > 0.0) == (labels[t] > 0);
        numbers = numbers && !std::isnan(oof[t]);
    }
    *accuracy = (double)right / (double)n;
    if (!numbers) { *auc = NAN; return; }  // (no order to count in)
    std::sort(neg.begin(), neg.end());
    int64_t above = 0, level = 0;
    for (double v : pos) {
        const auto lo = std::lower_bound(neg.begin(), neg.end(), v), hi = std::upper_bound(lo, neg.end(), v);
        above += lo - neg.begin();
        level += hi - lo;
    }
    *auc = ((double)above + 0.5 * (double)level) / (double)((int64_t)pos.size() * (int64_t)neg.size());
}

int cv_ready(fsk_engine* e) {
    if (!e->finalized || !e->svm.cv.valid) return e->fail(FSK_ESTATE, "no cross-validation: call fsk_svm_cv on a finalized result first");
    return FSK_OK;
}

// What fsk_svm_cv and fsk_svm_calibrate share — everything but where the result is kept: the checks, the problems
// p = c n_folds + f ("train at Cs[c] on the rows with fold[t] != f", boxes Cs[c] w_pos / Cs[c] w_neg of the handle's class
// weights), the batch solved side by side, each problem finished on the host, the out-of-fold decision values and the
// metrics, all into S. A refused call leaves S as it was.
int cv_run(fsk_engine* e, SvmCvState& S, const int32_t* labels, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
           double eps, int64_t max_iter) {
    const double t0 = now_ms();
    if (n_folds < 2) return e->fail(FSK_EINVAL, "n_folds is %d: at least 2 folds", n_folds);
    if (n_C < 1) return e->fail(FSK_EINVAL, "n_C is %d: at least one value of C", n_C);  // (before the arrays: an empty Cs may be null)
    int64_t n_pos = 0;
    { int rcc = svm_check_problem(e, fold && Cs ? labels : nullptr, "null labels, fold or Cs", n, eps, &n_pos); if (rcc) return rcc; }
    if ((int64_t)n_C * n_folds > FSK_SVM_CV_MAX_PROBLEMS)
        return e->fail(FSK_EINVAL, "%d folds x %d values of C are more than %d problems", n_folds, n_C, FSK_SVM_CV_MAX_PROBLEMS);
    for (int32_t c = 0; c < n_C; ++c)
        if (!(Cs[c] > 0.0) || !std::isfinite(Cs[c])) return e->fail(FSK_EINVAL, "C %d must be a positive finite number", c);
    const uint32_t F = (uint32_t)n_folds, nC = (uint32_t)n_C, P = F * nC, nn = (uint32_t)n;
    std::vector<int64_t> rows(F, 0), rows_pos(F, 0);
    for (int64_t t = 0; t < n; ++t) {
        if (fold[t] < 0 || fold[t] >= n_folds) return e->fail(FSK_EINVAL, "fold of row %lld is %d: folds are 0..%d", (long long)t, fold[t], n_folds - 1);
        ++rows[fold[t]];
        rows_pos[fold[t]] += labels[t] > 0;
    }
    for (uint32_t f = 0; f < F; ++f) {
        if (rows[f] == 0) return e->fail(FSK_EINVAL, "fold %u has no rows", f);
        const int64_t train = n - rows[f], train_pos = n_pos - rows_pos[f];
        if (train_pos == 0 || train_pos == train) return e->fail(FSK_EINVAL, "the training rows of fold %u are of one class only", f);
    }
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    // the problems: fold f's training rows once (idx, y), a slice of state for every (C, f)
    std::vector<uint32_t> idx;
    std::vector<signed char> y;
    std::vector<u64> fold_off(F), st_off(P), idx_off(P);
    idx.reserve((size_t)(F - 1) * nn);
    y.reserve((size_t)(F - 1) * nn);
    for (uint32_t f = 0; f < F; ++f) {
        fold_off[f] = idx.size();
        for (uint32_t t = 0; t < nn; ++t)
            if ((uint32_t)fold[t] != f) { idx.push_back(t); y.push_back((signed char)labels[t]); }
    }
    std::vector<fsk::SvmProb> probs(P);
    uint32_t max_n = 0, total_wg = 0;
    u64 total = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t f = p % F, np = (uint32_t)(n - rows[f]);
        probs[p].Cp = Cs[p / F] * e->svm.w_pos;  // (each product once, one rounding)
        probs[p].Cn = Cs[p / F] * e->svm.w_neg;
        probs[p].idx_off = idx_off[p] = fold_off[f];
        probs[p].st_off = st_off[p] = total;
        probs[p].n = np;
        probs[p].wg_off = total_wg;
        total += np;
        total_wg += (np + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS;
        max_n = std::max(max_n, np);
    }
    const int form = (int64_t)max_n <= e->tune.svm_wg_max ? 1 : 2;
    const uint32_t chunk = (uint32_t)e->tune.svm_chunk;

    const size_t rec_bytes = svm_batch_record_bytes(P, total_wg);
    FSK_HIP(S.d_alpha.reserve(total));
    FSK_HIP(S.d_G.reserve(total));
    if (form == 2) FSK_HIP(S.d_krow.reserve(total));
    FSK_HIP(S.d_idx.reserve(idx.size()));
    FSK_HIP(S.d_y.reserve(y.size()));
    FSK_HIP(S.d_prob.reserve((size_t)P * sizeof(fsk::SvmProb)));
    FSK_HIP(S.d_rec.reserve(rec_bytes));
    FSK_HIP(S.d_coef.reserve((size_t)P * nn));
    FSK_HIP(S.d_rho.reserve(P));
    FSK_HIP(S.d_fold.reserve(nn));
    FSK_HIP(S.d_oof.reserve((size_t)nC * nn));
    S.valid = false;  // (from here on the earlier result's buffers are written)

    SvmBatch B;
    B.P = P; B.max_n = max_n; B.max_wg = (max_n + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS; B.total_wg = total_wg;
    B.probs = reinterpret_cast<const fsk::SvmProb*>(S.d_prob.p);
    B.idx = S.d_idx.p; B.y = S.d_y.p; B.alpha = S.d_alpha.p; B.G = S.d_G.p; B.krow = S.d_krow.p;
    B.rb = reinterpret_cast<fsk::SvmRecB*>(S.d_rec.p);
    B.ra = reinterpret_cast<fsk::SvmRecA*>(B.rb + P);
    B.ci = reinterpret_cast<fsk::SvmCandI*>(B.ra + P);
    B.cj = reinterpret_cast<fsk::SvmCandJ*>(B.ci + total_wg);

    std::vector<double> G(total, -1.0);
    FSK_HIP(hipMemcpyAsync(S.d_prob.p, probs.data(), (size_t)P * sizeof(fsk::SvmProb), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_y.p, y.data(), y.size(), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_fold.p, fold, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_G.p, G.data(), total * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemsetAsync(S.d_alpha.p, 0, total * sizeof(double), e->stream));
    FSK_HIP(hipMemsetAsync(S.d_rec.p, 0, rec_bytes, e->stream));  // iter = 0, nothing pending, nobody done
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)

    std::vector<fsk::SvmRecB> status(P);
    int64_t launches = 0;
    const int rc = svm_on_source(src, [&](auto* K) { return solve_batch(e, K, src.diag, B, eps, max_iter, form, chunk, status.data(), &launches); });
    if (rc) return rc;
    S.alpha.resize(total);
    FSK_HIP(hipMemcpyAsync(S.alpha.data(), S.d_alpha.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), S.d_G.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    // per problem: rho and the objective in element order, the coefficients at full length
    std::vector<double> coef((size_t)P * nn, 0.0), rho(P), part;
    S.problems.assign(P, fsk_svm_cv_problem{});
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t np = probs[p].n;
        part.resize(np);
        const SvmFinish fin = svm_finish(S.alpha.data() + st_off[p], G.data() + st_off[p], y.data() + idx_off[p], np, probs[p].Cp, probs[p].Cn, part.data());
        for (uint32_t q = 0; q < np; ++q) coef[(size_t)p * nn + idx[idx_off[p] + q]] = part[q];
        rho[p] = fin.rho;
        fsk_svm_cv_problem& o = S.problems[p];
        o.n_rows = np;
        o.iterations = status[p].iter;
        o.gap = status[p].gmax - status[p].gmin;
        o.objective = fin.objective;
        o.rho = fin.rho;
        o.C = Cs[p / F];
        o.n_sv = fin.n_sv;
        o.n_bsv = fin.n_bsv;
        o.converged = status[p].converged;
        o.fold = (int32_t)(p % F);
    }
    FSK_HIP(hipMemcpyAsync(S.d_coef.p, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_rho.p, rho.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, e->stream));
    {
        const dim3 grid((nn + 3) / 4, nC);
        const double *diag = src.diag, *dc = S.d_coef.p, *dr = S.d_rho.p;
        const int32_t* df = S.d_fold.p;
        double* out = S.d_oof.p;
        svm_on_source(src, [=](auto* K) -> int {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_decision_oof<SrcOf<decltype(K)>>), grid, dim3(256), 0, e->stream, K, diag, dc, dr, df, F, nn, out);
            return FSK_OK;
        });
    }
    S.oof.resize((size_t)nC * nn);
    FSK_HIP(hipMemcpyAsync(S.oof.data(), S.d_oof.p, S.oof.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    S.scores.assign(nC, fsk_svm_cv_score{});
    for (uint32_t c = 0; c < nC; ++c) {
        S.scores[c].C = Cs[c];
        cv_metrics(S.oof.data() + (size_t)c * nn, labels, n, &S.scores[c].auc, &S.scores[c].accuracy);
    }
    S.idx.swap(idx);
    S.st_off.swap(st_off);
    S.idx_off.swap(idx_off);
    S.info = fsk_svm_cv_info{};
    S.info.n = n;
    S.info.n_folds = n_folds;
    S.info.n_C = n_C;
    S.info.form = form;
    S.info.launches = launches;
    S.info.ms = now_ms() - t0;
    S.valid = true;
    return FSK_OK;
}

// LIBSVM's sigmoid_predict, oriented to P(y = +1): both branches, so that neither exp overflows
double platt_predict(double f, double A, double B) {
    const double fApB = f * A + B;
    if (fApB >= 0) return std::exp(-fApB) / (1.0 + std::exp(-fApB));
    return 1.0 / (1.0 + std::exp(fApB));
}

// LIBSVM's sigmoid_train, operation for operation (this file is built without contraction: a * b + c is two roundings)
void platt_fit(const double* dec, const int32_t* labels, int64_t l, fsk_svm_platt_info* out) {
    double prior1 = 0, prior0 = 0;
    for (int64_t i = 0; i < l; ++i) {
        if (labels[i] > 0) prior1 += 1; else prior0 += 1;
    }
    const int max_iter = 100;
    const double min_step = 1e-10, sigma = 1e-12, eps = 1e-5;
    const double hiTarget = (prior1 + 1.0) / (prior1 + 2.0), loTarget = 1 / (prior0 + 2.0);
    std::vector<double> t((size_t)l);
    double A = 0.0, B = std::log((prior0 + 1.0) / (prior1 + 1.0)), fval = 0.0;
    for (int64_t i = 0; i < l; ++i) {
        t[i] = labels[i] > 0 ? hiTarget : loTarget;
        const double fApB = dec[i] * A + B;
        if (fApB >= 0) fval += t[i] * fApB + std::log(1 + std::exp(-fApB));
        else fval += (t[i] - 1) * fApB + std::log(1 + std::exp(fApB));
    }
    int iter = 0, status = 1;
    for (; iter < max_iter; ++iter) {
        double h11 = sigma, h22 = sigma, h21 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int64_t i = 0; i < l; ++i) {
            const double fApB = dec[i] * A + B;
            double p, q;
            if (fApB >= 0) {
                p = std::exp(-fApB) / (1.0 + std::exp(-fApB));
                q = 1.0 / (1.0 + std::exp(-fApB));
            } else {
                p = 1.0 / (1.0 + std::exp(fApB));
                q = std::exp(fApB) / (1.0 + std::exp(fApB));
            }
            const double d2 = p * q;
            h11 += dec[i] * dec[i] * d2;
            h22 += d2;
            h21 += dec[i] * d2;
            const double d1 = t[i] - p;
            g1 += dec[i] * d1;
            g2 += d1;
        }
        if (std::fabs(g1) < eps && std::fabs(g2) < eps) { status = 0; break; }
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det;
        const double dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double stepsize = 1;
        while (stepsize >= min_step) {
            const double newA = A + stepsize * dA, newB = B + stepsize * dB;
            double newf = 0.0;
            for (int64_t i = 0; i < l; ++i) {
                const double fApB = dec[i] * newA + newB;
                if (fApB >= 0) newf += t[i] * fApB + std::log(1 + std::exp(-fApB));
                else newf += (t[i] - 1) * fApB + std::log(1 + std::exp(fApB));
            }
            if (newf < fval + 0.0001 * stepsize * gd) {
                A = newA; B = newB; fval = newf;
                break;
            }
            stepsize = stepsize / 2.0;
        }
        if (stepsize < min_step) { status = 2; break; }
    }
    *out = fsk_svm_platt_info{};
    out->A = A; out->B = B;
    out->iterations = iter;
    out->status = status;
}

int calibration_ready(fsk_engine* e, const char* call) {
    int rc = model_of_kind(e, MODEL_SVC, call);
    if (rc) return rc;
    if (!e->svm.cal.valid || !e->svm.platt_valid) return e->fail(FSK_ESTATE, "no calibration: call fsk_svm_calibrate on the model first");
    return FSK_OK;
}

// ---- epsilon-SVR: the iteration over twin elements (fsk_kernels_svm.h) ---------------------------------------------------------
// One problem of n rows, 2n elements, in the two forms of solve(): the form is chosen by the caller from 2n.
template <typename SrcT>
int solve_svr(fsk_engine* e, const SrcT* K, const double* diag, uint32_t n, double C, double eps, int64_t max_iter, int form, uint32_t chunk,
              const SvmRecords& R, uint32_t n_wg, fsk::SvmRecB* status, int64_t* launches) {
    double *alpha = e->svm.d_alpha.p, *G = e->svm.d_G.p, *krow = e->svm.d_krow.p;
    if (form == 1) {
        const uint32_t nt = std::min<uint32_t>(fsk::SVM_WG_THREADS, (n + 63u) & ~63u);
        const size_t lds = fsk::svr_wg_lds(n, nt);
        if (n > (uint32_t)fsk::SVR_WG_ROWS * nt || lds > 160 * 1024) return e->fail(FSK_EUNSUPPORTED, "k_svr_wg needs %zu bytes of LDS for %u rows", lds, n);
        FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_svr_wg<SrcT>, lds));
        return svm_poll(e, R.rb, status, 1, [=] {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_wg<SrcT>), dim3(1), dim3(nt), lds, e->stream, K, diag, n, C, eps, (long long)max_iter, chunk, alpha, G,
                       R.rb);
            ++*launches;
        });
    }
    return svm_poll(e, R.rb, status, 1, [=] {
        for (uint32_t c = 0; c < chunk; ++c) {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_select_i<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, C, alpha, G,
                       (const double*)krow, (const fsk::SvmRecB*)R.rb, R.ra, R.ci, (const fsk::SvmCandJ*)R.cj, n_wg);
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_select_j<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, C, eps,
                       (long long)max_iter, (const double*)alpha, (const double*)G, krow, R.rb, (const fsk::SvmRecA*)R.ra,
                       (const fsk::SvmCandI*)R.ci, R.cj, n_wg);
            *launches += 2;
        }
    });
}

template <typename SrcT>
int solve_svr_batch(fsk_engine* e, const SrcT* K, const double* diag, const SvmBatch& B, double eps, int64_t max_iter, int form, uint32_t chunk,
                    fsk::SvmRecB* status, int64_t* launches) {
    if (form == 1) {
        const uint32_t nt = std::min<uint32_t>(fsk::SVM_WG_THREADS, (B.max_n + 63u) & ~63u);
        const size_t lds = fsk::svr_wg_lds(B.max_n, nt);
        if (B.max_n > (uint32_t)fsk::SVR_WG_ROWS * nt || lds > 160 * 1024)
            return e->fail(FSK_EUNSUPPORTED, "k_svr_wg_batch needs %zu bytes of LDS for %u rows", lds, B.max_n);
        FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_svr_wg_batch<SrcT>, lds));
        return svm_poll(e, B.rb, status, B.P, [=] {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_wg_batch<SrcT>), dim3(B.P), dim3(nt), lds, e->stream, K, diag, B.probs, B.idx, eps,
                       (long long)max_iter, chunk, B.alpha, B.G, B.rb);
            ++*launches;
        });
    }
    return svm_poll(e, B.rb, status, B.P, [=] {
        for (uint32_t c = 0; c < chunk; ++c) {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_select_i_batch<SrcT>), dim3(B.max_wg, B.P), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag,
                       B.probs, B.idx, B.alpha, B.G, (const double*)B.krow, (const fsk::SvmRecB*)B.rb, B.ra, B.ci, (const fsk::SvmCandJ*)B.cj);
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svr_select_j_batch<SrcT>), dim3(B.max_wg, B.P), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag,
                       B.probs, B.idx, eps, (long long)max_iter, (const double*)B.alpha, (const double*)B.G, B.krow, B.rb,
                       (const fsk::SvmRecA*)B.ra, (const fsk::SvmCandI*)B.ci, B.cj);
            *launches += 2;
        }
    });
}

// The start of a solve: G = p, p_e = epsilon - z_e for e < n and p_{e+n} = epsilon + z_e, one rounding each (alpha = 0)
void svr_start(const double* z, uint32_t n, double epsilon, double* p) {
    for (uint32_t t = 0; t < n; ++t) { p[t] = epsilon - z[t]; p[n + t] = epsilon + z[t]; }
}

// The finish of a solve as LIBSVM's: calculate_rho over the 2n elements in element order (y = +1 below n, -1 from n on, one
// box C), the objective 1/2 sum alpha_e (G_e + p_e) in element order, coef[t] = alpha_t - alpha*_t; n_sv counts coef != 0,
// n_bsv |coef| >= C
SvmFinish svr_finish(const double* alpha, const double* G, const double* p, uint32_t n, double C, double* coef) {
    double ub = HUGE_VAL, lb = -HUGE_VAL, sum_free = 0.0, obj = 0.0;
    int64_t n_free = 0, n_sv = 0, n_bsv = 0;
    for (uint32_t e = 0; e < 2 * n; ++e) {
        const bool up = e < n;
        const double a = alpha[e], yG = up ? G[e] : -G[e];
        if (a >= C) {
            if (!up) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else if (a <= 0.0) {
            if (up) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else {
            ++n_free;
            sum_free += yG;
        }
        obj += a * (G[e] + p[e]);
    }
    for (uint32_t t = 0; t < n; ++t) {
        coef[t] = alpha[t] - alpha[n + t];
        n_sv += coef[t] != 0.0;
        n_bsv += std::fabs(coef[t]) >= C;
    }
    return {n_free > 0 ? sum_free / (double)n_free : (ub + lb) / 2.0, obj / 2.0, n_sv, n_bsv};
}

// what fsk_svr_train and fsk_svr_cv check alike
int svr_check_problem(fsk_engine* e, const double* targets, const char* null_text, int64_t n, double eps) {
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (!targets) return e->fail(FSK_EINVAL, "%s", null_text);
    if (n != e->n_train) return e->fail(FSK_EINVAL, "%lld targets for %lld training sequences", (long long)n, (long long)e->n_train);
    if (n < 2) return e->fail(FSK_EINVAL, "%lld training sequences: a regression needs at least 2", (long long)n);
    if (!(eps > 0.0) || !std::isfinite(eps)) return e->fail(FSK_EINVAL, "eps must be a positive finite number");
    for (int64_t t = 0; t < n; ++t)
        if (!std::isfinite(targets[t])) return e->fail(FSK_EINVAL, "target %lld is not a finite number", (long long)t);
    return FSK_OK;
}

// mse, mae, r2 and Pearson's r of one grid point: plain sums in row order (the order include/fastsk_amd.h states)
void svr_metrics(const double* oof, const double* z, int64_t n, fsk_svr_cv_score* s) {
    double sz = 0.0, so = 0.0;
    for (int64_t t = 0; t < n; ++t) { sz += z[t]; so += oof[t]; }
    const double zm = sz / (double)n, om = so / (double)n;
    double sse = 0.0, sae = 0.0, sst = 0.0, soo = 0.0, szo = 0.0;
    for (int64_t t = 0; t < n; ++t) {
        const double d = oof[t] - z[t], dz = z[t] - zm, dq = oof[t] - om;
        sse += d * d;
        sae += std::fabs(d);
        sst += dz * dz;
        soo += dq * dq;
        szo += dq * dz;
    }
    s->mse = sse / (double)n;
    s->mae = sae / (double)n;
    s->r2 = 1.0 - sse / sst;
    s->r = szo / std::sqrt(soo * sst);
}

int svr_cv_ready(fsk_engine* e) {
    if (!e->finalized || !e->svm.svr_cv.valid) return e->fail(FSK_ESTATE, "no cross-validation: call fsk_svr_cv on a finalized result first");
    return FSK_OK;
}

// fsk_svr_cv: cv_run's plan with the grid (C, epsilon) — problem p = (c n_eps + q) n_folds + f, the folds' row lists shared,
// a start of G and a box of its own each — on the twin-element batch kernels. A refused call leaves the earlier result.
int svr_cv_run(fsk_engine* e, const double* z, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C, const double* epsilons,
               int32_t n_eps, double eps, int64_t max_iter) {
    const double t0 = now_ms();
    SvmCvState& S = e->svm.svr_cv;
    if (n_folds < 2) return e->fail(FSK_EINVAL, "n_folds is %d: at least 2 folds", n_folds);
    if (n_C < 1) return e->fail(FSK_EINVAL, "n_C is %d: at least one value of C", n_C);
    if (n_eps < 1) return e->fail(FSK_EINVAL, "n_eps is %d: at least one value of epsilon", n_eps);
    { int rcc = svr_check_problem(e, fold && Cs && epsilons ? z : nullptr, "null targets, fold, Cs or epsilons", n, eps); if (rcc) return rcc; }
    if ((int64_t)n_C * n_eps * n_folds > FSK_SVM_CV_MAX_PROBLEMS)
        return e->fail(FSK_EINVAL, "%d folds x %d values of C x %d of epsilon are more than %d problems", n_folds, n_C, n_eps, FSK_SVM_CV_MAX_PROBLEMS);
    for (int32_t c = 0; c < n_C; ++c)
        if (!(Cs[c] > 0.0) || !std::isfinite(Cs[c])) return e->fail(FSK_EINVAL, "C %d must be a positive finite number", c);
    for (int32_t q = 0; q < n_eps; ++q)
        if (!(epsilons[q] >= 0.0) || !std::isfinite(epsilons[q])) return e->fail(FSK_EINVAL, "epsilon %d must be a finite number >= 0", q);
    const uint32_t F = (uint32_t)n_folds, nG = (uint32_t)(n_C * n_eps), P = F * nG, nn = (uint32_t)n;
    std::vector<int64_t> rows(F, 0);
    for (int64_t t = 0; t < n; ++t) {
        if (fold[t] < 0 || fold[t] >= n_folds) return e->fail(FSK_EINVAL, "fold of row %lld is %d: folds are 0..%d", (long long)t, fold[t], n_folds - 1);
        ++rows[fold[t]];
    }
    for (uint32_t f = 0; f < F; ++f) {
        if (rows[f] == 0) return e->fail(FSK_EINVAL, "fold %u has no rows", f);
        if (n - rows[f] < 2) return e->fail(FSK_EINVAL, "fold %u leaves fewer than 2 training rows", f);
    }
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    std::vector<uint32_t> idx;
    std::vector<u64> fold_off(F), st_off(P), idx_off(P);
    idx.reserve((size_t)(F - 1) * nn);
    for (uint32_t f = 0; f < F; ++f) {
        fold_off[f] = idx.size();
        for (uint32_t t = 0; t < nn; ++t)
            if ((uint32_t)fold[t] != f) idx.push_back(t);
    }
    std::vector<fsk::SvmProb> probs(P);
    uint32_t max_n = 0, total_wg = 0;
    u64 total = 0;  // elements: 2 n_p a problem
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t f = p % F, np = (uint32_t)(n - rows[f]);
        probs[p].Cp = probs[p].Cn = Cs[p / F / (uint32_t)n_eps];
        probs[p].idx_off = idx_off[p] = fold_off[f];
        probs[p].st_off = st_off[p] = total;
        probs[p].n = np;
        probs[p].wg_off = total_wg;
        total += 2 * (u64)np;
        total_wg += (np + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS;
        max_n = std::max(max_n, np);
    }
    const int form = 2 * (int64_t)max_n <= e->tune.svm_wg_max ? 1 : 2;
    const uint32_t chunk = (uint32_t)e->tune.svm_chunk;

    const size_t rec_bytes = svm_batch_record_bytes(P, total_wg);
    FSK_HIP(S.d_alpha.reserve(total));
    FSK_HIP(S.d_G.reserve(total));
    if (form == 2) FSK_HIP(S.d_krow.reserve(total / 2));
    FSK_HIP(S.d_idx.reserve(idx.size()));
    FSK_HIP(S.d_prob.reserve((size_t)P * sizeof(fsk::SvmProb)));
    FSK_HIP(S.d_rec.reserve(rec_bytes));
    FSK_HIP(S.d_coef.reserve((size_t)P * nn));
    FSK_HIP(S.d_rho.reserve(P));
    FSK_HIP(S.d_fold.reserve(nn));
    FSK_HIP(S.d_oof.reserve((size_t)nG * nn));
    S.valid = false;  // (from here on the earlier result's buffers are written)

    SvmBatch B;
    B.P = P; B.max_n = max_n; B.max_wg = (max_n + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS; B.total_wg = total_wg;
    B.probs = reinterpret_cast<const fsk::SvmProb*>(S.d_prob.p);
    B.idx = S.d_idx.p; B.y = nullptr; B.alpha = S.d_alpha.p; B.G = S.d_G.p; B.krow = S.d_krow.p;
    B.rb = reinterpret_cast<fsk::SvmRecB*>(S.d_rec.p);
    B.ra = reinterpret_cast<fsk::SvmRecA*>(B.rb + P);
    B.ci = reinterpret_cast<fsk::SvmCandI*>(B.ra + P);
    B.cj = reinterpret_cast<fsk::SvmCandJ*>(B.ci + total_wg);

    // every problem's start of G: p of its rows' targets at its epsilon
    std::vector<double> pvec(total), G(total), zp;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t np = probs[p].n;
        zp.resize(np);
        for (uint32_t q = 0; q < np; ++q) zp[q] = z[idx[idx_off[p] + q]];
        svr_start(zp.data(), np, epsilons[(p / F) % (uint32_t)n_eps], pvec.data() + st_off[p]);
    }
    FSK_HIP(hipMemcpyAsync(S.d_prob.p, probs.data(), (size_t)P * sizeof(fsk::SvmProb), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_fold.p, fold, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_G.p, pvec.data(), total * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemsetAsync(S.d_alpha.p, 0, total * sizeof(double), e->stream));
    FSK_HIP(hipMemsetAsync(S.d_rec.p, 0, rec_bytes, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)

    std::vector<fsk::SvmRecB> status(P);
    int64_t launches = 0;
    const int rc = svm_on_source(src, [&](auto* K) { return solve_svr_batch(e, K, src.diag, B, eps, max_iter, form, chunk, status.data(), &launches); });
    if (rc) return rc;
    S.alpha.resize(total);
    FSK_HIP(hipMemcpyAsync(S.alpha.data(), S.d_alpha.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), S.d_G.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    std::vector<double> coef((size_t)P * nn, 0.0), rho(P), part;
    S.problems.assign(P, fsk_svm_cv_problem{});
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t np = probs[p].n;
        part.resize(np);
        const SvmFinish fin = svr_finish(S.alpha.data() + st_off[p], G.data() + st_off[p], pvec.data() + st_off[p], np, probs[p].Cp, part.data());
        for (uint32_t q = 0; q < np; ++q) coef[(size_t)p * nn + idx[idx_off[p] + q]] = part[q];
        rho[p] = fin.rho;
        fsk_svm_cv_problem& o = S.problems[p];
        o.n_rows = np;
        o.iterations = status[p].iter;
        o.gap = status[p].gmax - status[p].gmin;
        o.objective = fin.objective;
        o.rho = fin.rho;
        o.C = probs[p].Cp;
        o.reserved[0] = epsilons[(p / F) % (uint32_t)n_eps];
        o.n_sv = fin.n_sv;
        o.n_bsv = fin.n_bsv;
        o.converged = status[p].converged;
        o.fold = (int32_t)(p % F);
    }
    FSK_HIP(hipMemcpyAsync(S.d_coef.p, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_rho.p, rho.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, e->stream));
    {
        const dim3 grid((nn + 3) / 4, nG);  // (one grid point a blockIdx.y)
        const double *diag = src.diag, *dc = S.d_coef.p, *dr = S.d_rho.p;
        const int32_t* df = S.d_fold.p;
        double* out = S.d_oof.p;
        svm_on_source(src, [=](auto* K) -> int {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_decision_oof<SrcOf<decltype(K)>>), grid, dim3(256), 0, e->stream, K, diag, dc, dr, df, F, nn, out);
            return FSK_OK;
        });
    }
    S.oof.resize((size_t)nG * nn);
    FSK_HIP(hipMemcpyAsync(S.oof.data(), S.d_oof.p, S.oof.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    e->svm.svr_scores.assign(nG, fsk_svr_cv_score{});
    for (uint32_t g = 0; g < nG; ++g) {
        fsk_svr_cv_score& s = e->svm.svr_scores[g];
        s.C = Cs[g / (uint32_t)n_eps];
        s.epsilon = epsilons[g % (uint32_t)n_eps];
        svr_metrics(S.oof.data() + (size_t)g * nn, z, n, &s);
    }
    S.idx.swap(idx);
    S.st_off.swap(st_off);
    S.idx_off.swap(idx_off);
    S.info = fsk_svm_cv_info{};
    S.info.n = n;
    S.info.n_folds = n_folds;
    S.info.n_C = n_C;
    S.info.reserved0 = n_eps;
    S.info.form = form;
    S.info.launches = launches;
    S.info.ms = now_ms() - t0;
    S.valid = true;
    return FSK_OK;
}

// ---- one-vs-one multi-class C-SVC: the pairs of classes as one batch (fsk_svm_train_multiclass, fsk_svm_multiclass_cv) ---------
// The classes of a label vector: the distinct values ascending, every row's class index, the rows of each class (ascending),
// the weights by class index (1 where class_weight is null). What the train and the cross-validation check alike.
struct McClasses {
    std::vector<int32_t> classes;
    std::vector<uint32_t> cls;     // [n]
    std::vector<double> w;         // [k]
};
int mc_check(fsk_engine* e, const int32_t* labels, const char* null_text, int64_t n, double eps, const double* class_weight, McClasses* out) {
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (!labels) return e->fail(FSK_EINVAL, "%s", null_text);
    if (n != e->n_train) return e->fail(FSK_EINVAL, "%lld labels for %lld training sequences", (long long)n, (long long)e->n_train);
    if (!(eps > 0.0) || !std::isfinite(eps)) return e->fail(FSK_EINVAL, "eps must be a positive finite number");
    out->classes.assign(labels, labels + n);
    std::sort(out->classes.begin(), out->classes.end());
    out->classes.erase(std::unique(out->classes.begin(), out->classes.end()), out->classes.end());
    const size_t k = out->classes.size();
    if (k < 2) return e->fail(FSK_EINVAL, "only one class is present");
    if (k > FSK_SVM_MAX_CLASSES) return e->fail(FSK_EUNSUPPORTED, "%zu classes: at most %d", k, FSK_SVM_MAX_CLASSES);
    out->w.assign(k, 1.0);
    for (size_t c = 0; class_weight && c < k; ++c) {
        if (!(class_weight[c] > 0.0) || !std::isfinite(class_weight[c]))
            return e->fail(FSK_EINVAL, "the weight of class %d must be a positive finite number", out->classes[c]);
        out->w[c] = class_weight[c];
    }
    out->cls.resize((size_t)n);
    for (int64_t t = 0; t < n; ++t)
        out->cls[(size_t)t] = (uint32_t)(std::lower_bound(out->classes.begin(), out->classes.end(), labels[t]) - out->classes.begin());
    return FSK_OK;
}

// The batch of pair problems, solved and finished. In: probs with Cp, Cn, idx_off and n set (st_off and wg_off are set here), the
// row lists and their labels. The batch goes through solve_batch in the form cv_run would choose, every problem is finished by
// svm_finish; its coefficients (alpha y at the problem's own length, at st_off), rho, the problems and the lists stay on the
// device in M for the vote kernels. Out: alpha and the status records of every problem, what svm_finish returned.
struct McSolved {
    std::vector<double> alpha;
    std::vector<fsk::SvmRecB> status;
    std::vector<SvmFinish> fin;
    int form = 0;
    int64_t launches = 0;
};
int mc_solve(fsk_engine* e, SvmMcState& M, const SvmSource& src, std::vector<fsk::SvmProb>& probs, const std::vector<uint32_t>& idx,
             const std::vector<signed char>& y, double eps, int64_t max_iter, McSolved* out) {
    const uint32_t P = (uint32_t)probs.size();
    uint32_t max_n = 0, total_wg = 0;
    u64 total = 0;
    for (fsk::SvmProb& pr : probs) {
        pr.st_off = total;
        pr.wg_off = total_wg;
        total += pr.n;
        total_wg += (pr.n + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS;
        max_n = std::max(max_n, pr.n);
    }
    const int form = (int64_t)max_n <= e->tune.svm_wg_max ? 1 : 2;
    const uint32_t chunk = (uint32_t)e->tune.svm_chunk;
    const size_t rec_bytes = svm_batch_record_bytes(P, total_wg);
    FSK_HIP(M.d_alpha.reserve(total));
    FSK_HIP(M.d_G.reserve(total));
    if (form == 2) FSK_HIP(M.d_krow.reserve(total));
    FSK_HIP(M.d_coef.reserve(total));
    FSK_HIP(M.d_idx.reserve(idx.size()));
    FSK_HIP(M.d_y.reserve(y.size()));
    FSK_HIP(M.d_prob.reserve((size_t)P * sizeof(fsk::SvmProb)));
    FSK_HIP(M.d_rec.reserve(rec_bytes));
    FSK_HIP(M.d_rho.reserve(P));

    SvmBatch B;
    B.P = P; B.max_n = max_n; B.max_wg = (max_n + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS; B.total_wg = total_wg;
    B.probs = reinterpret_cast<const fsk::SvmProb*>(M.d_prob.p);
    B.idx = M.d_idx.p; B.y = M.d_y.p; B.alpha = M.d_alpha.p; B.G = M.d_G.p; B.krow = M.d_krow.p;
    B.rb = reinterpret_cast<fsk::SvmRecB*>(M.d_rec.p);
    B.ra = reinterpret_cast<fsk::SvmRecA*>(B.rb + P);
    B.ci = reinterpret_cast<fsk::SvmCandI*>(B.ra + P);
    B.cj = reinterpret_cast<fsk::SvmCandJ*>(B.ci + total_wg);

    std::vector<double> G(total, -1.0);
    FSK_HIP(hipMemcpyAsync(M.d_prob.p, probs.data(), (size_t)P * sizeof(fsk::SvmProb), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_idx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_y.p, y.data(), y.size(), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_G.p, G.data(), total * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemsetAsync(M.d_alpha.p, 0, total * sizeof(double), e->stream));
    FSK_HIP(hipMemsetAsync(M.d_rec.p, 0, rec_bytes, e->stream));  // iter = 0, nothing pending, nobody done
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)

    out->status.assign(P, fsk::SvmRecB{});
    out->launches = 0;
    out->form = form;
    const int rc = svm_on_source(src, [&](auto* K) { return solve_batch(e, K, src.diag, B, eps, max_iter, form, chunk, out->status.data(), &out->launches); });
    if (rc) return rc;
    out->alpha.resize(total);
    FSK_HIP(hipMemcpyAsync(out->alpha.data(), M.d_alpha.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), M.d_G.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    std::vector<double> coef(total), rho(P);
    out->fin.resize(P);
    for (uint32_t p = 0; p < P; ++p) {
        const fsk::SvmProb& pr = probs[p];
        out->fin[p] = svm_finish(out->alpha.data() + pr.st_off, G.data() + pr.st_off, y.data() + pr.idx_off, pr.n, pr.Cp, pr.Cn, coef.data() + pr.st_off);
        rho[p] = out->fin[p].rho;
    }
    FSK_HIP(hipMemcpyAsync(M.d_coef.p, coef.data(), total * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_rho.p, rho.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

// the classes and the pairs' (a | b << 16) for the vote, into M
int mc_upload_classes(fsk_engine* e, SvmMcState& M, const std::vector<int32_t>& classes) {
    const uint32_t k = (uint32_t)classes.size(), P = k * (k - 1) / 2;
    std::vector<uint32_t> ab;
    ab.reserve(P);
    for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = a + 1; b < k; ++b) ab.push_back(a | b << 16);
    FSK_HIP(M.d_ab.reserve(P));
    FSK_HIP(M.d_classes.reserve(k));
    FSK_HIP(hipMemcpyAsync(M.d_ab.p, ab.data(), (size_t)P * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_classes.p, classes.data(), (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    M.k = k;
    M.P = P;
    M.classes = classes;
    return FSK_OK;
}

// rows [r0, r1) under the model's pairs into device memory: dec [r1 - r0][P] and / or pred [r1 - r0]
int mc_launch_decision(fsk_engine* e, int64_t r0, int64_t r1, double* dec, int32_t* pred) {
    const SvmMcState& M = e->svm.mc;
    const uint32_t blocks = (uint32_t)((r1 - r0 + 3) / 4), a = (uint32_t)r0, b = (uint32_t)r1, P = M.P;
    SvmSource src;
    { int rc = svm_source(e, false, &src); if (rc) return rc; }
    const double *diag = src.diag, *coef = M.d_coef.p, *rho = M.d_rho.p;
    const fsk::SvmProb* probs = reinterpret_cast<const fsk::SvmProb*>(M.d_prob.p);
    const uint32_t *idx = M.d_idx.p, *ab = M.d_ab.p;
    const int32_t* classes = M.d_classes.p;
    return svm_on_source(src, [=](auto* K) -> int {
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_ovo_decision<SrcOf<decltype(K)>>), dim3(blocks), dim3(256), 0, e->stream, K, diag, probs, idx, coef, rho, ab,
                   classes, P, a, b, dec, pred);
        return FSK_OK;
    });
}

int mc_decision_args(fsk_engine* e, const char* call, int64_t r0, int64_t r1) {
    int rc = model_of_kind(e, MODEL_MC, call);
    if (rc) return rc;
    if (r0 < 0 || r1 > e->N || r0 > r1) return e->fail(FSK_EINVAL, "rows out of range");
    return FSK_OK;
}

int mc_cv_ready(fsk_engine* e) {
    if (!e->finalized || !e->svm.mc_cv.valid)
        return e->fail(FSK_ESTATE, "no cross-validation: call fsk_svm_multiclass_cv on a finalized result first");
    return FSK_OK;
}

// the rows of class a or b among `rows` of them (ascending), with y = +1 for a and -1 for b, appended to idx and y
template <typename Keep>
uint32_t mc_pair_list(const std::vector<uint32_t>& cls, uint32_t a, uint32_t b, Keep keep, std::vector<uint32_t>* idx, std::vector<signed char>* y) {
    uint32_t count = 0;
    for (uint32_t t = 0; t < (uint32_t)cls.size(); ++t)
        if ((cls[t] == a || cls[t] == b) && keep(t)) {
            idx->push_back(t);
            y->push_back(cls[t] == a ? (signed char)1 : (signed char)-1);
            ++count;
        }
    return count;
}

}  // namespace

extern "C" {

int fsk_svm_train_multiclass(fsk_engine* e, const int32_t* labels, int64_t n, double C, const double* class_weight, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    McClasses mcl;
    { int rcc = mc_check(e, labels, "null labels", n, eps, class_weight, &mcl); if (rcc) return rcc; }
    if (!(C > 0.0) || !std::isfinite(C)) return e->fail(FSK_EINVAL, "C must be a positive finite number");
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    const uint32_t k = (uint32_t)mcl.classes.size(), P = k * (k - 1) / 2;
    std::vector<uint32_t> idx;
    std::vector<signed char> y;
    idx.reserve((size_t)(k - 1) * (size_t)n);
    y.reserve((size_t)(k - 1) * (size_t)n);
    std::vector<fsk::SvmProb> probs;
    probs.reserve(P);
    for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = a + 1; b < k; ++b) {
            fsk::SvmProb pr{};
            pr.Cp = C * mcl.w[a];  // (each product once, one rounding)
            pr.Cn = C * mcl.w[b];
            pr.idx_off = idx.size();
            pr.n = mc_pair_list(mcl.cls, a, b, [](uint32_t) { return true; }, &idx, &y);
            probs.push_back(pr);
        }

    SvmState& S = e->svm;
    SvmMcState& M = S.mc;
    S.valid = false;  // (from here on the model slot's device state is written)
    S.cal.valid = S.platt_valid = M.cal_valid = false;  // (the calibration belonged to the model this one replaces)
    McSolved solved;
    { int rc = mc_solve(e, M, src, probs, idx, y, eps, max_iter, &solved); if (rc) return rc; }
    { int rc = mc_upload_classes(e, M, mcl.classes); if (rc) return rc; }

    std::vector<char> sv((size_t)n, 0);
    M.pairs.assign(P, fsk_svm_multiclass_pair{});
    for (uint32_t p = 0, a = 0; a < k; ++a)
        for (uint32_t b = a + 1; b < k; ++b, ++p) {
            const fsk::SvmProb& pr = probs[p];
            fsk_svm_multiclass_pair& o = M.pairs[p];
            o.class_a = mcl.classes[a];
            o.class_b = mcl.classes[b];
            o.n_rows = pr.n;
            o.iterations = solved.status[p].iter;
            o.gap = solved.status[p].gmax - solved.status[p].gmin;
            o.objective = solved.fin[p].objective;
            o.rho = solved.fin[p].rho;
            o.n_sv = solved.fin[p].n_sv;
            o.n_bsv = solved.fin[p].n_bsv;
            o.converged = solved.status[p].converged;
            for (uint32_t q = 0; q < pr.n; ++q)
                if (solved.alpha[pr.st_off + q] > 0.0) sv[idx[pr.idx_off + q]] = 1;
        }
    M.alpha.swap(solved.alpha);
    M.info = fsk_svm_multiclass_info{};
    M.info.k = (int32_t)k;
    M.info.n_pairs = (int32_t)P;
    M.info.form = solved.form;
    M.info.launches = solved.launches;
    M.info.n_sv = (int64_t)std::count(sv.begin(), sv.end(), (char)1);
    M.info.n_alpha = (int64_t)M.alpha.size();
    M.info.ms = now_ms() - t0;
    M.labels.assign(labels, labels + n);  // (what fsk_svm_multiclass_calibrate solves the folds with)
    M.w = mcl.w;
    M.weighted = class_weight != nullptr;
    M.C = C; M.eps = eps; M.max_iter = max_iter;
    S.model_kind = MODEL_MC;
    S.valid = true;
    return FSK_OK;
}

int fsk_svm_multiclass_get_model(fsk_engine* e, int32_t* classes, fsk_svm_multiclass_pair* pairs, double* alpha, fsk_svm_multiclass_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = model_of_kind(e, MODEL_MC, "fsk_svm_multiclass_get_model");
    if (rc) return rc;
    const SvmMcState& M = e->svm.mc;
    if (classes) memcpy(classes, M.classes.data(), M.classes.size() * sizeof(int32_t));
    if (pairs) memcpy(pairs, M.pairs.data(), M.pairs.size() * sizeof(fsk_svm_multiclass_pair));
    if (alpha) memcpy(alpha, M.alpha.data(), M.alpha.size() * sizeof(double));
    if (info) *info = M.info;
    return FSK_OK;
}

int fsk_svm_multiclass_decision(fsk_engine* e, int64_t r0, int64_t r1, double* dec, int32_t* pred) {
    if (!e) return FSK_EINVAL;
    int rc = mc_decision_args(e, "fsk_svm_multiclass_decision", r0, r1);
    if (rc || r0 == r1 || (!dec && !pred)) return rc;
    FSK_ON_DEVICE(e);
    SvmMcState& M = e->svm.mc;
    const size_t rows = (size_t)(r1 - r0);
    if (dec) FSK_HIP(M.d_dec.reserve(rows * M.P));
    if (pred) FSK_HIP(M.d_pred.reserve(rows));
    rc = mc_launch_decision(e, r0, r1, dec ? M.d_dec.p : nullptr, pred ? M.d_pred.p : nullptr);
    if (rc) return rc;
    if (dec) FSK_HIP(hipMemcpyAsync(dec, M.d_dec.p, rows * M.P * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (pred) FSK_HIP(hipMemcpyAsync(pred, M.d_pred.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    return FSK_OK;
}

int fsk_svm_multiclass_decision_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_dec, int32_t* device_pred) {
    if (!e) return FSK_EINVAL;
    int rc = mc_decision_args(e, "fsk_svm_multiclass_decision_device", r0, r1);
    if (rc || r0 == r1 || (!device_dec && !device_pred)) return rc;
    FSK_ON_DEVICE(e);
    rc = mc_launch_decision(e, r0, r1, device_dec, device_pred);
    if (rc) return rc;
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

}  // extern "C"

namespace {

// What fsk_svm_multiclass_cv and fsk_svm_multiclass_calibrate share — everything but where the batch is kept and what the
// out-of-fold launch writes: the checks, the (C, fold, pair) problems, the one batch solve. values = false: the out-of-fold
// LABELS of every C (k_svm_ovo_decision_oof), the scores and the problems' records into M. values = true (one C): the
// out-of-fold pair DECISIONS [n][P] (k_svm_ovo_values_oof) into *oof_values, and the form and launches into M.cv_info.
int mc_cv_run(fsk_engine* e, SvmMcState& M, bool values, std::vector<double>* oof_values, const int32_t* labels, int64_t n, const int32_t* fold,
              int32_t n_folds, const double* Cs, int32_t n_C, const double* class_weight, double eps, int64_t max_iter) {
    const double t0 = now_ms();
    if (n_folds < 2) return e->fail(FSK_EINVAL, "n_folds is %d: at least 2 folds", n_folds);
    if (n_C < 1) return e->fail(FSK_EINVAL, "n_C is %d: at least one value of C", n_C);  // (before the arrays: an empty Cs may be null)
    McClasses mcl;
    { int rcc = mc_check(e, fold && Cs ? labels : nullptr, "null labels, fold or Cs", n, eps, class_weight, &mcl); if (rcc) return rcc; }
    const uint32_t k = (uint32_t)mcl.classes.size(), P = k * (k - 1) / 2;
    if ((int64_t)n_C * n_folds * P > FSK_SVM_CV_MAX_PROBLEMS)
        return e->fail(FSK_EINVAL, "%d folds x %d values of C x %u pairs are more than %d problems", n_folds, n_C, P, FSK_SVM_CV_MAX_PROBLEMS);
    for (int32_t c = 0; c < n_C; ++c)
        if (!(Cs[c] > 0.0) || !std::isfinite(Cs[c])) return e->fail(FSK_EINVAL, "C %d must be a positive finite number", c);
    const uint32_t F = (uint32_t)n_folds, nC = (uint32_t)n_C, G = F * nC, nn = (uint32_t)n;
    std::vector<int64_t> rows(F, 0), of_class(k, 0), held((size_t)F * k, 0);
    for (int64_t t = 0; t < n; ++t) {
        if (fold[t] < 0 || fold[t] >= n_folds) return e->fail(FSK_EINVAL, "fold of row %lld is %d: folds are 0..%d", (long long)t, fold[t], n_folds - 1);
        ++rows[fold[t]];
        ++of_class[mcl.cls[(size_t)t]];
        ++held[(size_t)fold[t] * k + mcl.cls[(size_t)t]];
    }
    for (uint32_t f = 0; f < F; ++f) {
        if (rows[f] == 0) return e->fail(FSK_EINVAL, "fold %u has no rows", f);
        for (uint32_t c = 0; c < k; ++c)
            if (held[(size_t)f * k + c] == of_class[c])
                return e->fail(FSK_EINVAL, "class %d has no row among the training rows of fold %u", mcl.classes[c], f);
    }
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    // the lists of (f, pair) once, a problem for every (c, f, pair): p = (c F + f) P + pair
    std::vector<uint32_t> idx;
    std::vector<signed char> y;
    std::vector<u64> list_off((size_t)F * P);
    std::vector<uint32_t> list_n((size_t)F * P);
    for (uint32_t f = 0; f < F; ++f)
        for (uint32_t p = 0, a = 0; a < k; ++a)
            for (uint32_t b = a + 1; b < k; ++b, ++p) {
                list_off[(size_t)f * P + p] = idx.size();
                list_n[(size_t)f * P + p] = mc_pair_list(mcl.cls, a, b, [&](uint32_t t) { return (uint32_t)fold[t] != f; }, &idx, &y);
            }
    std::vector<fsk::SvmProb> probs((size_t)G * P);
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t p = 0, a = 0; a < k; ++a)
            for (uint32_t b = a + 1; b < k; ++b, ++p) {
                fsk::SvmProb& pr = probs[(size_t)g * P + p];
                pr = fsk::SvmProb{};
                pr.Cp = Cs[g / F] * mcl.w[a];  // (each product once, one rounding)
                pr.Cn = Cs[g / F] * mcl.w[b];
                pr.idx_off = list_off[(size_t)(g % F) * P + p];
                pr.n = list_n[(size_t)(g % F) * P + p];
            }

    FSK_HIP(M.d_fold.reserve(nn));
    if (values) FSK_HIP(M.d_dec.reserve((size_t)nn * P));
    else FSK_HIP(M.d_pred.reserve((size_t)nC * nn));
    M.valid = false;  // (from here on the earlier result's buffers are written)
    if (values) e->svm.mc.cal_valid = false;  // (and the calibration they belonged to is gone)
    McSolved solved;
    { int rc = mc_solve(e, M, src, probs, idx, y, eps, max_iter, &solved); if (rc) return rc; }
    { int rc = mc_upload_classes(e, M, mcl.classes); if (rc) return rc; }
    FSK_HIP(hipMemcpyAsync(M.d_fold.p, fold, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    if (values) {
        const double *diag = src.diag, *coef = M.d_coef.p, *rho = M.d_rho.p;
        const fsk::SvmProb* dp = reinterpret_cast<const fsk::SvmProb*>(M.d_prob.p);
        const uint32_t* di = M.d_idx.p;
        const int32_t* df = M.d_fold.p;
        double* out = M.d_dec.p;
        svm_on_source(src, [=](auto* K) -> int {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_ovo_values_oof<SrcOf<decltype(K)>>), dim3((nn + 3) / 4), dim3(256), 0, e->stream, K, diag, dp, di, coef,
                       rho, P, df, nn, out);
            return FSK_OK;
        });
        oof_values->resize((size_t)nn * P);
        FSK_HIP(hipMemcpyAsync(oof_values->data(), M.d_dec.p, oof_values->size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
        FSK_HIP(hipGetLastError());
        M.cv_info = fsk_svm_cv_info{};
        M.cv_info.n = n;
        M.cv_info.n_folds = n_folds;
        M.cv_info.n_C = n_C;
        M.cv_info.form = solved.form;
        M.cv_info.reserved0 = (int32_t)k;
        M.cv_info.launches = solved.launches;
        M.cv_info.ms = now_ms() - t0;
        M.valid = true;
        return FSK_OK;
    }
    {
        const dim3 grid((nn + 3) / 4, nC);
        const double *diag = src.diag, *coef = M.d_coef.p, *rho = M.d_rho.p;
        const fsk::SvmProb* dp = reinterpret_cast<const fsk::SvmProb*>(M.d_prob.p);
        const uint32_t *di = M.d_idx.p, *ab = M.d_ab.p;
        const int32_t *classes = M.d_classes.p, *df = M.d_fold.p;
        int32_t* out = M.d_pred.p;
        svm_on_source(src, [=](auto* K) -> int {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_ovo_decision_oof<SrcOf<decltype(K)>>), grid, dim3(256), 0, e->stream, K, diag, dp, di, coef, rho, ab,
                       classes, P, df, F, nn, out);
            return FSK_OK;
        });
    }
    M.oof.resize((size_t)nC * nn);
    FSK_HIP(hipMemcpyAsync(M.oof.data(), M.d_pred.p, M.oof.size() * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());

    M.scores.assign(nC, fsk_svm_cv_score{});
    for (uint32_t c = 0; c < nC; ++c) {
        int64_t right = 0;
        for (uint32_t t = 0; t < nn; ++t) right += M.oof[(size_t)c * nn + t] == labels[t];
        M.scores[c].C = Cs[c];
        M.scores[c].auc = NAN;  // (no AUC for more than two classes)
        M.scores[c].accuracy = (double)right / (double)n;
    }
    M.problems.assign((size_t)G * P, fsk_svm_cv_problem{});
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t p = 0, a = 0; a < k; ++a)
            for (uint32_t b = a + 1; b < k; ++b, ++p) {
                const size_t at = (size_t)g * P + p;
                fsk_svm_cv_problem& o = M.problems[at];
                o.n_rows = probs[at].n;
                o.iterations = solved.status[at].iter;
                o.gap = solved.status[at].gmax - solved.status[at].gmin;
                o.objective = solved.fin[at].objective;
                o.rho = solved.fin[at].rho;
                o.C = Cs[g / F];
                o.n_sv = solved.fin[at].n_sv;
                o.n_bsv = solved.fin[at].n_bsv;
                o.converged = solved.status[at].converged;
                o.fold = (int32_t)(g % F);
                o.reserved[0] = (double)mcl.classes[a];
                o.reserved[1] = (double)mcl.classes[b];
            }
    M.cv_info = fsk_svm_cv_info{};
    M.cv_info.n = n;
    M.cv_info.n_folds = n_folds;
    M.cv_info.n_C = n_C;
    M.cv_info.form = solved.form;
    M.cv_info.reserved0 = (int32_t)k;
    M.cv_info.launches = solved.launches;
    M.cv_info.ms = now_ms() - t0;
    M.valid = true;
    return FSK_OK;
}

// the sigmoids of the model's pairs onto the device, for k_svm_ovo_proba
int mc_upload_sigmoids(fsk_engine* e, SvmMcState& M) {
    std::vector<double> A(M.P), B(M.P);
    for (uint32_t p = 0; p < M.P; ++p) { A[p] = M.fits[p].A; B[p] = M.fits[p].B; }
    FSK_HIP(M.d_sigA.reserve(M.P));
    FSK_HIP(M.d_sigB.reserve(M.P));
    FSK_HIP(hipMemcpyAsync(M.d_sigA.p, A.data(), (size_t)M.P * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(M.d_sigB.p, B.data(), (size_t)M.P * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)
    return FSK_OK;
}

int mc_proba_args(fsk_engine* e, const char* call, int64_t r0, int64_t r1) {
    int rc = model_of_kind(e, MODEL_MC, call);
    if (rc) return rc;
    if (!e->svm.mc.cal_valid)
        return e->fail(FSK_ESTATE, "no calibration: call fsk_svm_multiclass_calibrate or fsk_svm_multiclass_set_calibration on the model first");
    if (r0 < 0 || r1 > e->N || r0 > r1) return e->fail(FSK_EINVAL, "rows out of range");
    return FSK_OK;
}

// rows [r0, r1) under the model's pairs and sigmoids into device memory: prob [r1 - r0][k], pred and iters [r1 - r0]
static_assert(4 * (FSK_SVM_MAX_CLASSES * (FSK_SVM_MAX_CLASSES - 1) / 2) * sizeof(double) <= 64 * 1024, "k_svm_ovo_proba's LDS: four waves of P doubles");
int mc_launch_proba(fsk_engine* e, int64_t r0, int64_t r1, double* prob, int32_t* pred, int32_t* iters) {
    const SvmMcState& M = e->svm.mc;
    const uint32_t blocks = (uint32_t)((r1 - r0 + 3) / 4), a = (uint32_t)r0, b = (uint32_t)r1, P = M.P, k = M.k;
    const size_t lds = (size_t)4 * P * sizeof(double);
    SvmSource src;
    { int rc = svm_source(e, false, &src); if (rc) return rc; }
    const double *diag = src.diag, *coef = M.d_coef.p, *rho = M.d_rho.p, *sA = M.d_sigA.p, *sB = M.d_sigB.p;
    const fsk::SvmProb* probs = reinterpret_cast<const fsk::SvmProb*>(M.d_prob.p);
    const uint32_t* idx = M.d_idx.p;
    const int32_t* classes = M.d_classes.p;
    return svm_on_source(src, [=](auto* K) -> int {
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_ovo_proba<SrcOf<decltype(K)>>), dim3(blocks), dim3(256), lds, e->stream, K, diag, probs, idx, coef, rho, sA,
                   sB, classes, k, P, a, b, prob, pred, iters);
        return FSK_OK;
    });
}

}  // namespace

extern "C" {

double fsk_exp_neg(double x) { return fsk::exp_neg(x); }

int fsk_svm_multiclass_cv(fsk_engine* e, const int32_t* labels, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
                          const double* class_weight, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    return mc_cv_run(e, e->svm.mc_cv, false, nullptr, labels, n, fold, n_folds, Cs, n_C, class_weight, eps, max_iter);
}

int fsk_svm_multiclass_calibrate(fsk_engine* e, const int32_t* fold, int32_t n_folds) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    int rc = model_of_kind(e, MODEL_MC, "fsk_svm_multiclass_calibrate");
    if (rc) return rc;
    SvmMcState& M = e->svm.mc;
    const std::vector<int32_t> labels = M.labels;  // (the model's own: what it was trained on)
    const std::vector<double> w = M.w;
    const double C = M.C;
    std::vector<double> oof;
    rc = mc_cv_run(e, e->svm.mc_cal, true, &oof, fold ? labels.data() : nullptr, (int64_t)labels.size(), fold, n_folds, &C, 1,
                   M.weighted ? w.data() : nullptr, M.eps, M.max_iter);
    if (rc) return rc;
    const SvmMcState& B = e->svm.mc_cal;
    const uint32_t k = M.k, P = M.P, nn = (uint32_t)labels.size();
    std::vector<fsk_svm_platt_info> fits(P);
    std::vector<double> dec;
    std::vector<int32_t> yy;
    for (uint32_t p = 0, a = 0; a < k; ++a)
        for (uint32_t b = a + 1; b < k; ++b, ++p) {
            dec.clear();
            yy.clear();
            for (uint32_t t = 0; t < nn; ++t)
                if (labels[t] == M.classes[a] || labels[t] == M.classes[b]) {
                    dec.push_back(oof[(size_t)t * P + p]);
                    yy.push_back(labels[t] == M.classes[a] ? 1 : -1);
                }
            platt_fit(dec.data(), yy.data(), (int64_t)dec.size(), &fits[p]);
            fits[p].n_folds = n_folds;
            fits[p].form = B.cv_info.form;
            fits[p].launches = B.cv_info.launches;
        }
    M.fits.swap(fits);
    M.cal_oof.swap(oof);
    FSK_ON_DEVICE(e);
    rc = mc_upload_sigmoids(e, M);
    if (rc) return rc;
    const double ms = now_ms() - t0;
    for (fsk_svm_platt_info& f : M.fits) f.ms = ms;
    M.cal_valid = true;
    return FSK_OK;
}

int fsk_svm_multiclass_get_calibration(fsk_engine* e, double* oof, fsk_svm_platt_info* fits) {
    if (!e) return FSK_EINVAL;
    int rc = mc_proba_args(e, "fsk_svm_multiclass_get_calibration", 0, 0);
    if (rc) return rc;
    const SvmMcState& M = e->svm.mc;
    if (oof && M.cal_oof.empty())
        return e->fail(FSK_ESTATE, "no out-of-fold decisions: the sigmoids were installed by fsk_svm_multiclass_set_calibration");
    if (oof) memcpy(oof, M.cal_oof.data(), M.cal_oof.size() * sizeof(double));
    if (fits) memcpy(fits, M.fits.data(), M.fits.size() * sizeof(fsk_svm_platt_info));
    return FSK_OK;
}

int fsk_svm_multiclass_set_calibration(fsk_engine* e, const double* A, const double* B) {
    if (!e) return FSK_EINVAL;
    int rc = model_of_kind(e, MODEL_MC, "fsk_svm_multiclass_set_calibration");
    if (rc) return rc;
    SvmMcState& M = e->svm.mc;
    if (!A || !B) return e->fail(FSK_EINVAL, "null A or B");
    for (uint32_t p = 0; p < M.P; ++p)
        if (!std::isfinite(A[p])) return e->fail(FSK_EINVAL, "A of pair %u must be a finite number", p);
    FSK_ON_DEVICE(e);
    M.cal_valid = false;
    M.fits.assign(M.P, fsk_svm_platt_info{});
    for (uint32_t p = 0; p < M.P; ++p) { M.fits[p].A = A[p]; M.fits[p].B = B[p]; }
    M.cal_oof.clear();
    rc = mc_upload_sigmoids(e, M);
    if (rc) return rc;
    M.cal_valid = true;
    return FSK_OK;
}

int fsk_svm_multiclass_proba(fsk_engine* e, int64_t r0, int64_t r1, double* prob, int32_t* pred, int32_t* iters) {
    if (!e) return FSK_EINVAL;
    int rc = mc_proba_args(e, "fsk_svm_multiclass_proba", r0, r1);
    if (rc || r0 == r1 || (!prob && !pred && !iters)) return rc;
    FSK_ON_DEVICE(e);
    SvmMcState& M = e->svm.mc;
    const size_t rows = (size_t)(r1 - r0);
    if (prob) FSK_HIP(M.d_proba.reserve(rows * M.k));
    if (pred) FSK_HIP(M.d_pred.reserve(rows));
    if (iters) FSK_HIP(M.d_iters.reserve(rows));
    rc = mc_launch_proba(e, r0, r1, prob ? M.d_proba.p : nullptr, pred ? M.d_pred.p : nullptr, iters ? M.d_iters.p : nullptr);
    if (rc) return rc;
    if (prob) FSK_HIP(hipMemcpyAsync(prob, M.d_proba.p, rows * M.k * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (pred) FSK_HIP(hipMemcpyAsync(pred, M.d_pred.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (iters) FSK_HIP(hipMemcpyAsync(iters, M.d_iters.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    return FSK_OK;
}

int fsk_svm_multiclass_proba_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_prob, int32_t* device_pred, int32_t* device_iters) {
    if (!e) return FSK_EINVAL;
    int rc = mc_proba_args(e, "fsk_svm_multiclass_proba_device", r0, r1);
    if (rc || r0 == r1 || (!device_prob && !device_pred && !device_iters)) return rc;
    FSK_ON_DEVICE(e);
    rc = mc_launch_proba(e, r0, r1, device_prob, device_pred, device_iters);
    if (rc) return rc;
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_svm_multiclass_cv_get(fsk_engine* e, int32_t* pred, fsk_svm_cv_score* scores, fsk_svm_cv_problem* problems, fsk_svm_cv_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = mc_cv_ready(e);
    if (rc) return rc;
    const SvmMcState& M = e->svm.mc_cv;
    if (pred) memcpy(pred, M.oof.data(), M.oof.size() * sizeof(int32_t));
    if (scores) memcpy(scores, M.scores.data(), M.scores.size() * sizeof(fsk_svm_cv_score));
    if (problems) memcpy(problems, M.problems.data(), M.problems.size() * sizeof(fsk_svm_cv_problem));
    if (info) *info = M.cv_info;
    return FSK_OK;
}

int fsk_svm_train(fsk_engine* e, const int32_t* labels, int64_t n, double C, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    int64_t n_pos = 0;
    { int rcc = svm_check_problem(e, labels, "null labels", n, eps, &n_pos); if (rcc) return rcc; }
    if (!(C > 0.0) || !std::isfinite(C)) return e->fail(FSK_EINVAL, "C must be a positive finite number");
    if (n_pos == 0 || n_pos == n) return e->fail(FSK_EINVAL, "only one class is present");
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    SvmState& S = e->svm;
    S.valid = false;
    S.cal.valid = S.platt_valid = S.mc.cal_valid = false;  // (the calibration belongs to the model)
    const double Cp = C * S.w_pos, Cn = C * S.w_neg;  // (each product once, one rounding)
    const uint32_t nn = (uint32_t)n;
    const int form = (int64_t)nn <= e->tune.svm_wg_max ? 1 : 2;
    const uint32_t chunk = (uint32_t)e->tune.svm_chunk;
    const uint32_t n_wg = (nn + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS;
    FSK_HIP(S.d_alpha.reserve(nn));
    FSK_HIP(S.d_G.reserve(nn));
    FSK_HIP(S.d_krow.reserve(nn));
    FSK_HIP(S.d_coef.reserve(nn));
    FSK_HIP(S.d_y.reserve(nn));
    FSK_HIP(S.d_rec.reserve(svm_record_bytes(n_wg)));
    const SvmRecords R = svm_records(S.d_rec.p, n_wg);

    S.y.resize(nn);
    for (uint32_t t = 0; t < nn; ++t) S.y[t] = (signed char)labels[t];
    S.alpha.assign(nn, 0.0);
    std::vector<double> G(nn, -1.0);
    FSK_HIP(hipMemcpyAsync(S.d_y.p, S.y.data(), nn, hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemcpyAsync(S.d_G.p, G.data(), (size_t)nn * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemsetAsync(S.d_alpha.p, 0, (size_t)nn * sizeof(double), e->stream));
    FSK_HIP(hipMemsetAsync(S.d_rec.p, 0, svm_record_bytes(n_wg), e->stream));  // iter = 0, nothing pending, not done
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)

    fsk::SvmRecB status{};
    int64_t launches = 0;
    const int rc = svm_on_source(src, [&](auto* K) { return solve(e, K, src.diag, nn, Cp, Cn, eps, max_iter, form, chunk, R, n_wg, &status, &launches); });
    if (rc) return rc;
    FSK_HIP(hipMemcpyAsync(S.alpha.data(), S.d_alpha.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), S.d_G.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    std::vector<double> coef(nn);
    const SvmFinish fin = svm_finish(S.alpha.data(), G.data(), S.y.data(), nn, Cp, Cn, coef.data());
    S.rho = fin.rho;
    S.C = C; S.eps = eps; S.max_iter = max_iter;
    FSK_HIP(hipMemcpyAsync(S.d_coef.p, coef.data(), (size_t)nn * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    S.info = fsk_svm_info{};
    S.info.iterations = status.iter;
    S.info.gap = status.gmax - status.gmin;
    S.info.objective = fin.objective;
    S.info.n_sv = fin.n_sv;
    S.info.n_bsv = fin.n_bsv;
    S.info.converged = status.converged;
    S.info.form = form;
    S.info.launches = launches;
    S.info.ms = now_ms() - t0;
    S.model_kind = MODEL_SVC;
    S.valid = true;
    return FSK_OK;
}

int fsk_svm_get_model(fsk_engine* e, double* alpha, double* rho, fsk_svm_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = model_of_kind(e, MODEL_SVC, "fsk_svm_get_model");
    if (rc) return rc;
    if (alpha) memcpy(alpha, e->svm.alpha.data(), e->svm.alpha.size() * sizeof(double));
    if (rho) *rho = e->svm.rho;
    if (info) *info = e->svm.info;
    return FSK_OK;
}

int fsk_svm_decision(fsk_engine* e, int64_t r0, int64_t r1, double* out) {
    if (!e) return FSK_EINVAL;
    int rc = decision_args(e, r0, r1, out);
    if (rc || r0 == r1) return rc;
    FSK_ON_DEVICE(e);
    FSK_HIP(e->svm.d_out.reserve((size_t)(r1 - r0)));
    rc = launch_decision(e, r0, r1, e->svm.d_out.p);
    if (rc) return rc;
    FSK_HIP(hipMemcpyAsync(out, e->svm.d_out.p, (size_t)(r1 - r0) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_svm_decision_device(fsk_engine* e, int64_t r0, int64_t r1, double* device_out) {
    if (!e) return FSK_EINVAL;
    int rc = decision_args(e, r0, r1, device_out);
    if (rc || r0 == r1) return rc;
    FSK_ON_DEVICE(e);
    rc = launch_decision(e, r0, r1, device_out);
    if (rc) return rc;
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_svm_cv(fsk_engine* e, const int32_t* labels, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
               double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    return cv_run(e, e->svm.cv, labels, n, fold, n_folds, Cs, n_C, eps, max_iter);
}

int fsk_svm_cv_get(fsk_engine* e, double* oof, fsk_svm_cv_score* scores, fsk_svm_cv_problem* problems, fsk_svm_cv_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = cv_ready(e);
    if (rc) return rc;
    const SvmCvState& S = e->svm.cv;
    if (oof) memcpy(oof, S.oof.data(), S.oof.size() * sizeof(double));
    if (scores) memcpy(scores, S.scores.data(), S.scores.size() * sizeof(fsk_svm_cv_score));
    if (problems) memcpy(problems, S.problems.data(), S.problems.size() * sizeof(fsk_svm_cv_problem));
    if (info) *info = S.info;
    return FSK_OK;
}

int fsk_svm_cv_get_alpha(fsk_engine* e, int32_t p, double* alpha) {
    if (!e) return FSK_EINVAL;
    int rc = cv_ready(e);
    if (rc) return rc;
    const SvmCvState& S = e->svm.cv;
    if (p < 0 || (size_t)p >= S.problems.size()) return e->fail(FSK_EINVAL, "problem %d of %zu", p, S.problems.size());
    if (!alpha) return e->fail(FSK_EINVAL, "null output");
    std::fill(alpha, alpha + S.info.n, 0.0);
    for (int64_t q = 0; q < S.problems[p].n_rows; ++q) alpha[S.idx[S.idx_off[p] + q]] = S.alpha[S.st_off[p] + q];
    return FSK_OK;
}

int fsk_svm_set_class_weights(fsk_engine* e, double w_pos, double w_neg) {
    if (!e) return FSK_EINVAL;
    if (!(w_pos > 0.0) || !std::isfinite(w_pos) || !(w_neg > 0.0) || !std::isfinite(w_neg))
        return e->fail(FSK_EINVAL, "class weights must be positive finite numbers");
    SvmState& S = e->svm;
    if (w_pos != S.w_pos || w_neg != S.w_neg) S.valid = S.cv.valid = S.cal.valid = S.platt_valid = false;  // (a model belongs to its weights)
    S.w_pos = w_pos;
    S.w_neg = w_neg;
    return FSK_OK;
}

int fsk_svm_get_class_weights(fsk_engine* e, double* w_pos, double* w_neg) {
    if (!e) return FSK_EINVAL;
    if (!w_pos || !w_neg) return e->fail(FSK_EINVAL, "null output");
    *w_pos = e->svm.w_pos;
    *w_neg = e->svm.w_neg;
    return FSK_OK;
}

int fsk_svm_platt_fit(const double* dec, const int32_t* labels, int64_t n, fsk_svm_platt_info* out) {
    if (!dec || !labels || !out || n < 1) return FSK_EINVAL;
    for (int64_t t = 0; t < n; ++t)
        if (labels[t] != 1 && labels[t] != -1) return FSK_EINVAL;
    platt_fit(dec, labels, n, out);
    return FSK_OK;
}

int fsk_svm_calibrate(fsk_engine* e, const int32_t* fold, int32_t n_folds) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    int rc = model_of_kind(e, MODEL_SVC, "fsk_svm_calibrate");
    if (rc) return rc;
    SvmState& S = e->svm;
    const std::vector<int32_t> labels(S.y.begin(), S.y.end());
    const double C = S.C;
    rc = cv_run(e, S.cal, labels.data(), (int64_t)labels.size(), fold, n_folds, &C, 1, S.eps, S.max_iter);
    if (rc) return rc;
    S.platt_valid = false;
    platt_fit(S.cal.oof.data(), labels.data(), (int64_t)labels.size(), &S.platt);
    S.platt.n_folds = n_folds;
    S.platt.form = S.cal.info.form;
    S.platt.launches = S.cal.info.launches;
    S.platt.ms = now_ms() - t0;
    S.platt_valid = true;
    return FSK_OK;
}

int fsk_svm_get_calibration(fsk_engine* e, double* oof, fsk_svm_platt_info* out) {
    if (!e) return FSK_EINVAL;
    int rc = calibration_ready(e, "fsk_svm_get_calibration");
    if (rc) return rc;
    if (oof) memcpy(oof, e->svm.cal.oof.data(), e->svm.cal.oof.size() * sizeof(double));
    if (out) *out = e->svm.platt;
    return FSK_OK;
}

int fsk_svm_proba(fsk_engine* e, int64_t r0, int64_t r1, double* out) {
    if (!e) return FSK_EINVAL;
    int rc = calibration_ready(e, "fsk_svm_proba");
    if (rc) return rc;
    rc = fsk_svm_decision(e, r0, r1, out);
    if (rc) return rc;
    for (int64_t r = 0; r < r1 - r0; ++r) out[r] = platt_predict(out[r], e->svm.platt.A, e->svm.platt.B);
    return FSK_OK;
}

int fsk_svr_train(fsk_engine* e, const double* targets, int64_t n, double C, double epsilon, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    { int rcc = svr_check_problem(e, targets, "null targets", n, eps); if (rcc) return rcc; }
    if (!(C > 0.0) || !std::isfinite(C)) return e->fail(FSK_EINVAL, "C must be a positive finite number");
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return e->fail(FSK_EINVAL, "epsilon must be a finite number >= 0");
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }
    SvmSource src;
    { int rcs = svm_source(e, true, &src); if (rcs) return rcs; }

    SvmState& S = e->svm;
    S.valid = false;
    S.cal.valid = S.platt_valid = S.mc.cal_valid = false;  // (the calibration belonged to the model this one replaces)
    const uint32_t nn = (uint32_t)n, m = 2 * nn;
    const int form = (int64_t)m <= e->tune.svm_wg_max ? 1 : 2;  // (the 2n elements against the workgroup's ceiling)
    const uint32_t chunk = (uint32_t)e->tune.svm_chunk;
    const uint32_t n_wg = (nn + fsk::SVM_THREADS - 1) / fsk::SVM_THREADS;
    FSK_HIP(S.d_alpha.reserve(m));
    FSK_HIP(S.d_G.reserve(m));
    FSK_HIP(S.d_krow.reserve(nn));
    FSK_HIP(S.d_coef.reserve(nn));
    FSK_HIP(S.d_rec.reserve(svm_record_bytes(n_wg)));
    const SvmRecords R = svm_records(S.d_rec.p, n_wg);

    std::vector<double> p(m), G(m);
    svr_start(targets, nn, epsilon, p.data());
    S.alpha.assign(m, 0.0);
    FSK_HIP(hipMemcpyAsync(S.d_G.p, p.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipMemsetAsync(S.d_alpha.p, 0, (size_t)m * sizeof(double), e->stream));
    FSK_HIP(hipMemsetAsync(S.d_rec.p, 0, svm_record_bytes(n_wg), e->stream));  // iter = 0, nothing pending, not done
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the host vectors above are pageable)

    fsk::SvmRecB status{};
    int64_t launches = 0;
    const int rc = svm_on_source(src, [&](auto* K) { return solve_svr(e, K, src.diag, nn, C, eps, max_iter, form, chunk, R, n_wg, &status, &launches); });
    if (rc) return rc;
    FSK_HIP(hipMemcpyAsync(S.alpha.data(), S.d_alpha.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), S.d_G.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    S.coef.resize(nn);
    const SvmFinish fin = svr_finish(S.alpha.data(), G.data(), p.data(), nn, C, S.coef.data());
    S.rho = fin.rho;
    S.C = C; S.eps = eps; S.max_iter = max_iter;
    FSK_HIP(hipMemcpyAsync(S.d_coef.p, S.coef.data(), (size_t)nn * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    S.info = fsk_svm_info{};
    S.info.iterations = status.iter;
    S.info.gap = status.gmax - status.gmin;
    S.info.objective = fin.objective;
    S.info.n_sv = fin.n_sv;
    S.info.n_bsv = fin.n_bsv;
    S.info.converged = status.converged;
    S.info.form = form;
    S.info.launches = launches;
    S.info.ms = now_ms() - t0;
    S.model_kind = MODEL_SVR;
    S.valid = true;
    return FSK_OK;
}

int fsk_svr_get_model(fsk_engine* e, double* alpha2, double* coef, double* rho, fsk_svm_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = model_of_kind(e, MODEL_SVR, "fsk_svr_get_model");
    if (rc) return rc;
    if (alpha2) memcpy(alpha2, e->svm.alpha.data(), e->svm.alpha.size() * sizeof(double));
    if (coef) memcpy(coef, e->svm.coef.data(), e->svm.coef.size() * sizeof(double));
    if (rho) *rho = e->svm.rho;
    if (info) *info = e->svm.info;
    return FSK_OK;
}

int fsk_svr_cv(fsk_engine* e, const double* targets, int64_t n, const int32_t* fold, int32_t n_folds, const double* Cs, int32_t n_C,
               const double* epsilons, int32_t n_eps, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    return svr_cv_run(e, targets, n, fold, n_folds, Cs, n_C, epsilons, n_eps, eps, max_iter);
}

int fsk_svr_cv_get(fsk_engine* e, double* oof, fsk_svr_cv_score* scores, fsk_svm_cv_problem* problems, fsk_svm_cv_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = svr_cv_ready(e);
    if (rc) return rc;
    const SvmCvState& S = e->svm.svr_cv;
    if (oof) memcpy(oof, S.oof.data(), S.oof.size() * sizeof(double));
    if (scores) memcpy(scores, e->svm.svr_scores.data(), e->svm.svr_scores.size() * sizeof(fsk_svr_cv_score));
    if (problems) memcpy(problems, S.problems.data(), S.problems.size() * sizeof(fsk_svm_cv_problem));
    if (info) *info = S.info;
    return FSK_OK;
}

}  // extern "C"
