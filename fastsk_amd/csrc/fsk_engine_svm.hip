// fsk_engine_svm.hip — the SVM stage on the resident result triangle: fsk_svm_train, fsk_svm_get_model, fsk_svm_decision(_device)
// of include/fastsk_amd.h. What FastSK::fit / FastSK::score do with LIBSVM on the host (fastsk.cpp:239-530), for the
// sequences of one compute call and without the kernel matrix ever leaving the device: the engine's consumer is an SVM, and
// the triangle it needs is 40 GB at 100,000 sequences.
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

// one workgroup, alpha / G / y in LDS: launches of up to `chunk` iterations until the status record says done
template <typename SrcT>
int solve_wg(fsk_engine* e, const SrcT* K, uint32_t n, double C, double eps, int64_t max_iter, uint32_t chunk, const SvmRecords& R,
             fsk::SvmRecB* status, int64_t* launches) {
    double *alpha = e->svm.d_alpha.p, *G = e->svm.d_G.p;  // (plain pointers: a launch takes its arguments by value)
    const signed char* y = e->svm.d_y.p;
    const double* diag = e->d_diag.p;
    fsk::SvmRecB* rb = R.rb;
    const uint32_t nt = std::min<uint32_t>(fsk::SVM_WG_THREADS, (n + 63u) & ~63u);
    const size_t lds = fsk::svm_wg_lds(n, nt);
    if (lds > 160 * 1024) return e->fail(FSK_EUNSUPPORTED, "k_svm_wg needs %zu bytes of LDS for %u rows", lds, n);
    FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_svm_wg<SrcT>, lds));
    for (;;) {
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_wg<SrcT>), dim3(1), dim3(nt), lds, e->stream, K, diag, n, C, eps, (long long)max_iter, chunk,
                   alpha, G, y, rb);
        ++*launches;
        FSK_HIP(hipMemcpyAsync(status, rb, sizeof *status, hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
        FSK_HIP(hipGetLastError());
        if (status->done) return FSK_OK;
    }
}

// two launches an iteration: `chunk` (A, B) pairs between two reads of the status record
template <typename SrcT>
int solve_two_launch(fsk_engine* e, const SrcT* K, uint32_t n, double C, double eps, int64_t max_iter, uint32_t chunk, const SvmRecords& R,
                     uint32_t n_wg, fsk::SvmRecB* status, int64_t* launches) {
    double *alpha = e->svm.d_alpha.p, *G = e->svm.d_G.p, *krow = e->svm.d_krow.p;  // (plain pointers: a launch takes its arguments by value)
    const signed char* y = e->svm.d_y.p;
    const double* diag = e->d_diag.p;
    fsk::SvmRecB* rb = R.rb;
    fsk::SvmRecA* ra = R.ra;
    fsk::SvmCandI* ci = R.ci;
    fsk::SvmCandJ* cj = R.cj;
    for (;;) {
        for (uint32_t c = 0; c < chunk; ++c) {
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_i<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, C, alpha, G, y,
                       (const double*)krow, (const fsk::SvmRecB*)rb, ra, ci, (const fsk::SvmCandJ*)cj, n_wg);
            FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_select_j<SrcT>), dim3(n_wg), dim3(fsk::SVM_THREADS), 0, e->stream, K, diag, n, C, eps,
                       (long long)max_iter, (const double*)alpha, (const double*)G, y, krow, rb, (const fsk::SvmRecA*)ra,
                       (const fsk::SvmCandI*)ci, cj, n_wg);
            *launches += 2;
        }
        FSK_HIP(hipMemcpyAsync(status, rb, sizeof *status, hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
        FSK_HIP(hipGetLastError());
        if (status->done) return FSK_OK;
    }
}

template <typename SrcT>
int solve(fsk_engine* e, const SrcT* K, uint32_t n, double C, double eps, int64_t max_iter, int form, uint32_t chunk, const SvmRecords& R,
          uint32_t n_wg, fsk::SvmRecB* status, int64_t* launches) {
    return form == 1 ? solve_wg<SrcT>(e, K, n, C, eps, max_iter, chunk, R, status, launches)
                     : solve_two_launch<SrcT>(e, K, n, C, eps, max_iter, chunk, R, n_wg, status, launches);
}

int model_ready(fsk_engine* e) {
    if (!e->finalized || !e->svm.valid) return e->fail(FSK_ESTATE, "no model: call fsk_svm_train on a finalized result first");
    return FSK_OK;
}

// the rows [r0, r1) into device memory at `dst`
int launch_decision(fsk_engine* e, int64_t r0, int64_t r1, double* dst) {
    const uint32_t blocks = (uint32_t)((r1 - r0 + 3) / 4), n_train = (uint32_t)e->n_train, a = (uint32_t)r0, b = (uint32_t)r1;
    const double *diag = e->d_diag.p, *coef = e->svm.d_coef.p, *Kf = e->d_Kf64.p;
    const u64* Ku = e->d_K;
    const double rho = e->svm.rho;
    if (e->result_f64)
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_decision<double>), dim3(blocks), dim3(256), 0, e->stream, Kf, diag, coef, n_train, a, b, rho, dst);
    else
        FSK_LAUNCH(HIP_KERNEL_NAME(fsk::k_svm_decision<u64>), dim3(blocks), dim3(256), 0, e->stream, Ku, diag, coef, n_train, a, b, rho, dst);
    return FSK_OK;
}

int decision_args(fsk_engine* e, int64_t r0, int64_t r1, const double* out) {
    int rc = model_ready(e);
    if (rc) return rc;
    if (r0 < 0 || r1 > e->N || r0 > r1) return e->fail(FSK_EINVAL, "rows out of range");
    if (r1 > r0 && !out) return e->fail(FSK_EINVAL, "null output");
    return FSK_OK;
}

}  // namespace

extern "C" {

int fsk_svm_train(fsk_engine* e, const int32_t* labels, int64_t n, double C, double eps, int64_t max_iter) {
    if (!e) return FSK_EINVAL;
    const double t0 = now_ms();
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (!labels) return e->fail(FSK_EINVAL, "null labels");
    if (n != e->n_train) return e->fail(FSK_EINVAL, "%lld labels for %lld training sequences", (long long)n, (long long)e->n_train);
    if (!(C > 0.0) || !std::isfinite(C)) return e->fail(FSK_EINVAL, "C must be a positive finite number");
    if (!(eps > 0.0) || !std::isfinite(eps)) return e->fail(FSK_EINVAL, "eps must be a positive finite number");
    int64_t n_pos = 0;
    for (int64_t t = 0; t < n; ++t) {
        if (labels[t] != 1 && labels[t] != -1) return e->fail(FSK_EINVAL, "label %lld is %d: labels must be -1 or +1", (long long)t, labels[t]);
        n_pos += labels[t] > 0;
    }
    if (n_pos == 0 || n_pos == n) return e->fail(FSK_EINVAL, "only one class is present");
    if (max_iter < 0) max_iter = SVM_DEFAULT_MAX_ITER;
    FSK_ON_DEVICE(e);
    { int rcz = materialise_zero(e); if (rcz) return rcz; }

    SvmState& S = e->svm;
    S.valid = false;
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
    const int rc = e->result_f64 ? solve<double>(e, e->d_Kf64.p, nn, C, eps, max_iter, form, chunk, R, n_wg, &status, &launches)
                                 : solve<u64>(e, e->d_K, nn, C, eps, max_iter, form, chunk, R, n_wg, &status, &launches);
    if (rc) return rc;
    FSK_HIP(hipMemcpyAsync(S.alpha.data(), S.d_alpha.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipMemcpyAsync(G.data(), S.d_G.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));

    // rho and the objective as LIBSVM's calculate_rho / calculate_objective_value, in index order
    double ub = HUGE_VAL, lb = -HUGE_VAL, sum_free = 0.0, obj = 0.0;
    int64_t n_free = 0, n_sv = 0, n_bsv = 0;
    std::vector<double> coef(nn);
    for (uint32_t t = 0; t < nn; ++t) {
        const double a = S.alpha[t], yG = S.y[t] > 0 ? G[t] : -G[t];
        if (a >= C) {
            if (S.y[t] < 0) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else if (a <= 0.0) {
            if (S.y[t] > 0) ub = std::min(ub, yG); else lb = std::max(lb, yG);
        } else {
            ++n_free;
            sum_free += yG;
        }
        obj += a * (G[t] - 1.0);
        n_sv += a > 0.0;
        n_bsv += a >= C;
        coef[t] = S.y[t] > 0 ? a : -a;
    }
    S.rho = n_free > 0 ? sum_free / (double)n_free : (ub + lb) / 2.0;
    FSK_HIP(hipMemcpyAsync(S.d_coef.p, coef.data(), (size_t)nn * sizeof(double), hipMemcpyHostToDevice, e->stream));
    FSK_HIP(hipStreamSynchronize(e->stream));
    S.info = fsk_svm_info{};
    S.info.iterations = status.iter;
    S.info.gap = status.gmax - status.gmin;
    S.info.objective = obj / 2.0;
    S.info.n_sv = n_sv;
    S.info.n_bsv = n_bsv;
    S.info.converged = status.converged;
    S.info.form = form;
    S.info.launches = launches;
    S.info.ms = now_ms() - t0;
    S.valid = true;
    return FSK_OK;
}

int fsk_svm_get_model(fsk_engine* e, double* alpha, double* rho, fsk_svm_info* info) {
    if (!e) return FSK_EINVAL;
    int rc = model_ready(e);
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

}  // extern "C"
