// fsk_engine_rows.hip — the rows kernel of include/fastsk_amd.h: fsk_rows_build, fsk_rows_get_block(_device), fsk_rows_get_info,
// fsk_svm_set_kernel / fsk_svm_get_kernel. L(r, c) = <K(r, train), K(c, train)> of the finalized result — the second-level
// kernel behind the reference's kernel_type = "linear" (fastsk.cpp:318-333) and upstream's LinearSVC on Ktr — as a packed fp64
// triangle with its raw diagonal: the layout the <double> instantiations of the SVM kernels read through normalised_cell, so
// the SVM stage runs on it unchanged. A translation unit of its own: nothing here reaches another kernel.
//
// A BUILD, N sequences of which n train (the one statement; DESIGN.md and tools/bench_rows_kernel.py refer to it).
// Multiply-adds: n for every cell with a train column, (n (n + 1) / 2 + (N - n) n) n, and (N - n) n for the diagonal of the test
// rows; N = n: n^2 (n + 1) / 2. Each is one fp64 multiply and one fp64 add, two instructions: the data sheet's 78.6 TFLOP/s of
// vector fp64 counts a fused multiply-add as two operations, so this form can issue 39.3 10^12 instructions a second, 19.6 10^12
// multiply-adds (derived, not measured). Bytes: the scratch is written once and holds n (n + 1) / 2 + (N - n) n doubles (16
// bytes a cell through the normalising pass: 8 read as u64 or fp64, 8 written); a tile of T x T cells reads 2 T n doubles of it
// (T n on the diagonal) and writes T^2, so the product moves about 16 n / T bytes a cell from L2 / HBM — 2 KB a cell at n =
// 16,000 and T = 128 against 16,000 multiply-adds: the product is bound by the fp64 issue rate and by the LDS reads (2 T / 16
// 8-byte reads a thread for (T / 16)^2 multiply-adds), not by memory.
#include "fsk_engine_internal.h"
#include "fsk_kernels_rows.h"

using namespace fsk_detail;

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int rows_ready(fsk_engine* e) {
    if (!e->finalized || !e->rows.valid) return e->fail(FSK_ESTATE, "no rows kernel: call fsk_rows_build on a finalized result first");
    return FSK_OK;
}

int block_args(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1) {
    int rc = rows_ready(e);
    if (rc) return rc;
    if (i0 < 0 || j0 < 0 || i1 > e->N || j1 > e->N || i0 > i1 || j0 > j1) return e->fail(FSK_EINVAL, "block out of range");
    return FSK_OK;
}

void launch_block(fsk_engine* e, u64 i0, u64 nr, u64 j0, u64 cols, int raw, double* dst) {
    const uint32_t blocks = (uint32_t)((nr * cols + 255) / 256);
    const double *L = e->rows.d_L.p, *diag = e->rows.d_diag.p;
    FSK_LAUNCH(fsk::k_rows_block, dim3(blocks), dim3(256), 0, e->stream, L, diag, i0, nr, j0, cols, raw, dst);
}

}  // namespace

int fsk_detail::rows_build(fsk_engine* e) {
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    if (e->rows.valid) return FSK_OK;
    const u64 n = (u64)e->n_train, N = (u64)e->N, nt = N - n;
    if (n < 1) return e->fail(FSK_EINVAL, "no training sequences");
    { int rcz = materialise_zero(e); if (rcz) return rcz; }

    RowsState& R = e->rows;
    R.drop();
    const u64 tri_cells = n * (n + 1) / 2, rect_off = (tri_cells + 1) & ~(u64)1, scratch_cells = rect_off + nt * n;
    const u64 L_cells = N * (N + 1) / 2;
    if (R.d_L.reserve((size_t)L_cells) != hipSuccess || R.d_diag.reserve((size_t)N) != hipSuccess) {
        (void)hipGetLastError();
        R.drop();
        return e->fail(FSK_ENOMEM, "cannot allocate the rows kernel: %llu bytes (%.1f GB) for %llu sequences on device %d",
                       (unsigned long long)((L_cells + N) * sizeof(double)), (double)(L_cells + N) * 8e-9, (unsigned long long)N, e->cfg.device);
    }
    DevBuf<double> scratch;  // (leaves with the build, whichever way it ends)
    if (scratch.reserve((size_t)scratch_cells) != hipSuccess) {
        (void)hipGetLastError();
        R.drop();
        return e->fail(FSK_ENOMEM, "cannot allocate the scratch of the rows kernel: %llu bytes (%.1f GB) for %llu train columns of %llu sequences on device %d",
                       (unsigned long long)(scratch_cells * sizeof(double)), (double)scratch_cells * 8e-9, (unsigned long long)n,
                       (unsigned long long)N, e->cfg.device);
    }

    // 1. the normalised cells with a train column, once: the train triangle by the streaming pass of fsk_get_triangle_device
    // (its first n (n + 1) / 2 cells are the train rows), the test rows' train columns by the block pass of fsk_get_block_device
    FSK_HIP(hipStreamSynchronize(e->stream));
    const double t0 = now_ms();
    const u64 chunk = (u64)1 << 33;
    for (u64 c0 = 0; c0 < tri_cells; c0 += chunk) {
        const int rc = launch_triangle(e, c0, std::min<u64>(chunk, tri_cells - c0), scratch.p + c0);
        if (rc) { R.drop(); return rc; }
    }
    if (nt > 0) {
        const int rc = fsk_get_block_device(e, (int64_t)n, (int64_t)N, 0, (int64_t)n, scratch.p + rect_off);
        if (rc) { R.drop(); return rc; }
    }
    FSK_HIP(hipStreamSynchronize(e->stream));
    const double t1 = now_ms();

    // 2. the product. The test rows of L are zero but for their train columns and their diagonal.
    if (nt > 0) FSK_HIP(hipMemsetAsync(R.d_L.p + tri_cells, 0, (size_t)(L_cells - tri_cells) * sizeof(double), e->stream));
    const fsk::RowsSrc src{scratch.p, scratch.p + rect_off, (uint32_t)n, (uint32_t)N};
    const uint32_t T = fsk::ROWS_TILE, ncb = (uint32_t)((n + T - 1) / T), nrb = (uint32_t)((N + T - 1) / T);
    double *Lp = R.d_L.p, *dp = R.d_diag.p;
    FSK_HIP(fsk_hw::allow_dynamic_lds(fsk::k_rows_syrk, fsk::ROWS_LDS_BYTES));
    FSK_LAUNCH(fsk::k_rows_syrk, dim3(ncb, nrb), dim3(fsk::ROWS_THREADS), fsk::ROWS_LDS_BYTES, e->stream, src, Lp, dp);
    if (nt > 0)
        FSK_LAUNCH(fsk::k_rows_diag, dim3((uint32_t)((nt + fsk::ROWS_THREADS - 1) / fsk::ROWS_THREADS)), dim3(fsk::ROWS_THREADS), 0, e->stream,
                   src, Lp, dp);
    FSK_HIP(hipStreamSynchronize(e->stream));
    FSK_HIP(hipGetLastError());
    const double t2 = now_ms();

    // (tiles at or below the diagonal with a column block below n)
    const u64 tiles = (u64)ncb * (ncb + 1) / 2 + (u64)(nrb - ncb) * ncb;
    R.info.n_train = (int64_t)n;
    R.info.n_seq = (int64_t)N;
    R.info.tile = fsk::ROWS_TILE;
    R.info.panel = fsk::ROWS_PANEL;
    R.info.tiles += (int64_t)tiles;
    R.info.builds += 1;
    R.info.scratch_bytes = (int64_t)(scratch_cells * sizeof(double));
    R.info.ms_scratch = t1 - t0;
    R.info.ms_product = t2 - t1;
    R.valid = true;
    return FSK_OK;
}

extern "C" {

int fsk_rows_build(fsk_engine* e) {
    if (!e) return FSK_EINVAL;
    if (!e->finalized) return e->fail(FSK_ESTATE, "no finalized kernel: call fsk_compute or fsk_finalize first");
    FSK_ON_DEVICE(e);
    return rows_build(e);
}

int fsk_rows_get_block(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t raw, double* out) {
    if (!e) return FSK_EINVAL;
    int rc = block_args(e, i0, i1, j0, j1);
    if (rc) return rc;
    const int64_t rows = i1 - i0, cols = j1 - j0;
    if (rows == 0 || cols == 0) return FSK_OK;
    if (!out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    const int64_t max_cells = (int64_t)32 << 20;  // 256 MB of doubles per staging round
    const int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(rows, max_cells / cols));
    FSK_HIP(e->d_stage.reserve((size_t)(rows_per * cols)));
    for (int64_t r = 0; r < rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, rows - r);
        launch_block(e, (u64)(i0 + r), (u64)nr, (u64)j0, (u64)cols, raw ? 1 : 0, e->d_stage.p);
        FSK_HIP(hipMemcpyAsync(out + r * cols, e->d_stage.p, (size_t)(nr * cols) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        FSK_HIP(hipStreamSynchronize(e->stream));
    }
    return FSK_OK;
}

int fsk_rows_get_block_device(fsk_engine* e, int64_t i0, int64_t i1, int64_t j0, int64_t j1, int32_t raw, double* device_out) {
    if (!e) return FSK_EINVAL;
    int rc = block_args(e, i0, i1, j0, j1);
    if (rc) return rc;
    const u64 rows = (u64)(i1 - i0), cols = (u64)(j1 - j0);
    if (rows == 0 || cols == 0) return FSK_OK;
    if (!device_out) return e->fail(FSK_EINVAL, "null output");
    FSK_ON_DEVICE(e);
    const u64 max_cells = (u64)1 << 31;  // grid.x limit: launch in row chunks
    const u64 rows_per = std::max<u64>(1, std::min<u64>(rows, max_cells / cols));
    for (u64 r = 0; r < rows; r += rows_per) launch_block(e, (u64)i0 + r, std::min(rows_per, rows - r), (u64)j0, cols, raw ? 1 : 0, device_out + r * cols);
    FSK_HIP(hipStreamSynchronize(e->stream));
    return FSK_OK;
}

int fsk_rows_get_info(fsk_engine* e, fsk_rows_info* out) {
    if (!e) return FSK_EINVAL;
    if (!out) return e->fail(FSK_EINVAL, "null output");
    *out = e->rows.info;
    out->tile = fsk::ROWS_TILE;
    out->panel = fsk::ROWS_PANEL;
    const bool there = e->finalized && e->rows.valid;
    out->resident_bytes = there ? (int64_t)((e->rows.d_L.cap + e->rows.d_diag.cap) * sizeof(double)) : 0;
    return FSK_OK;
}

int fsk_svm_set_kernel(fsk_engine* e, int32_t kind) {
    if (!e) return FSK_EINVAL;
    if (kind != FSK_SVM_KERNEL_RESULT && kind != FSK_SVM_KERNEL_ROWS) return e->fail(FSK_EINVAL, "kernel kind %d: FSK_SVM_KERNEL_RESULT (0) or FSK_SVM_KERNEL_ROWS (1)", kind);
    if (kind != e->svm.kernel) e->svm.valid = e->svm.cv.valid = e->svm.svr_cv.valid = e->svm.mc_cv.valid = false;  // (a model belongs to the kernel it was trained on)
    e->svm.kernel = kind;
    return FSK_OK;
}

int fsk_svm_get_kernel(fsk_engine* e, int32_t* kind) {
    if (!e) return FSK_EINVAL;
    if (!kind) return e->fail(FSK_EINVAL, "null output");
    *kind = e->svm.kernel;
    return FSK_OK;
}

}  // extern "C"
