// fsk_kernels_svm.h — a C-SVC dual solver and its decision values on the RESIDENT result triangle (fsk_svm_train,
// fsk_svm_decision), the pairs' decision values and the vote of a one-vs-one multi-class model (k_svm_ovo_decision), its class
// probabilities by pairwise coupling (k_svm_ovo_proba), and the same solver over the twin elements of an epsilon-SVR (fsk_svr_train, fsk_svr_cv: the last section). Included by fsk_engine_svm.hip only.
//
// The kernel is cosine-normalised: every K(t,t) is 1, the whole matrix is on the device, so the solver is SMO with LIBSVM's
// second-order working-set selection and nothing else — no row cache, no shrinking. A row of Q is read where it lies: cells
// tri_index(i, 0..i) (contiguous) and tri_index(t, i), t > i (one cell a triangle row), each through normalised_cell, i.e. the
// very IEEE values the getters hand out, from whichever triangle the result is (u64 counts, fp64 of variance mode).
//
// The arithmetic of one iteration is fixed to the operation (tests restate it in numpy and compare bit for bit). With
// y in {-1, +1}, alpha = 0 and G = -1 at the start, v_t = -y_t G_t, and the box of row t C_t = Cp where y_t > 0, Cn where
// y_t < 0 (fsk_svm_set_class_weights: Cp = C w_pos, Cn = C w_neg, each rounded once on the host; two kernel arguments, chosen
// by y in registers — with equal weights every C_t is the one C and C_i - C_j is 0.0):
//   1. I_up = {y > 0, alpha < C_t} u {y < 0, alpha > 0}, I_low = {y > 0, alpha > 0} u {y < 0, alpha < C_t};
//      i = argmax v over I_up, Gmax = v_i, Gmin = min v over I_low; stop when Gmax - Gmin <= eps (then: at max_iter);
//   2. b_t = Gmax - v_t, a_t = K_ii + K_tt - 2 K_it = 2 - 2 K_it (TAU where <= 0): j = argmin over I_low, b_t > 0, of -(b_t b_t) / a_t;
//   3. the two-variable step and its clipping to [0, C_i] x [0, C_j] as in LIBSVM's Solver::Solve (svm_step);
//   4. G_t = G_t + ((Q_it dalpha_i) + (Q_jt dalpha_j)), Q_it = y_i y_t K_it.
// Every tie goes to the lowest index: (value, index) compared lexicographically is associative, so neither the shape of a
// reduction tree nor the grid shows in the result. Products and sums are the __d*_rn forms: no contraction.
#pragma once
#include "fsk_common.h"
#include "fsk_exp_neg.h"

namespace fsk {

constexpr double SVM_TAU = 1e-12;
constexpr int SVM_NONE = 0x7fffffff;     // index of "no candidate": loses every tie
constexpr int SVM_WG_THREADS = 1024;     // k_svm_wg: one workgroup
constexpr int SVM_WG_ITEMS = 8;          // ... of at most this many elements a thread (8192 = svm_wg_max's ceiling)
constexpr int SVM_PART = 32;             // second level of a workgroup's reductions

// What the launches of one solve hand each other (device memory). rec_b: written by launch B (k_svm_select_j) and by
// k_svm_wg, read by launch A and the host. rec_a: written by launch A (k_svm_select_i), read by launch B. No launch reads a
// record that one of its own workgroups writes.
struct SvmRecB {
    long long iter;          // two-variable steps taken so far
    double gmax, gmin;       // of the last selection
    double ai, Gi;           // alpha_i, G_i before the pending step
    int i, yi;
    int done, converged;     // done: stop test met (converged = 1) or max_iter reached (converged = 0)
    int pending, pad;        // a step (i chosen, j's candidates reduced per workgroup) waits for launch A
};
struct SvmRecA {
    long long iter;
    int done, pad;           // 1: launch B has said done; 2: launch A found no j candidate, launch B is to say done
};
struct SvmCandI {            // a workgroup's share of step 1
    double vmax, vmin;
    int imax, pad;
};
struct SvmCandJ {            // a workgroup's share of step 2, with what the step needs of j
    double obj, aj, Gj, Kij;
    int j, yj;
};

// cell (a, b) of the symmetric normalised matrix, either order
template <typename SrcT>
__device__ __forceinline__ double svm_cell(const SrcT* K, const double* diag, uint32_t a, uint32_t b) {
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const double x = (double)K[tri_index(hi, lo)];
    return normalised_cell(x, diag[hi], diag[lo], hi == lo);
}

__device__ __forceinline__ double svm_inf() { return __builtin_huge_val(); }
__device__ __forceinline__ double svm_box(int y, double Cp, double Cn) { return y > 0 ? Cp : Cn; }  // C_t
// (a set tests alpha against one box only: I_up that of the positives, I_low that of the negatives)
__device__ __forceinline__ bool svm_in_up(int y, double a, double Cp) { return y > 0 ? a < Cp : a > 0.0; }
__device__ __forceinline__ bool svm_in_low(int y, double a, double Cn) { return y > 0 ? a > 0.0 : a < Cn; }
__device__ __forceinline__ double svm_v(int y, double G) { return y > 0 ? -G : G; }
// (value, index) orders: the larger value / the smaller value first, then the lower index
__device__ __forceinline__ bool svm_better_max(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ bool svm_better_min(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }
// step 2 for one element that lies in I_low: its objective, or "none" (b <= 0)
__device__ __forceinline__ bool svm_j_objective(double gmax, double v, double kit, double* obj) {
    const double b = __dsub_rn(gmax, v);
    if (!(b > 0.0)) return false;
    double a = __dsub_rn(2.0, __dmul_rn(2.0, kit));
    if (a <= 0.0) a = SVM_TAU;
    *obj = -__ddiv_rn(__dmul_rn(b, b), a);
    return true;
}

// Step 3: LIBSVM's Solver::Solve for one pair with Q_ii = Q_jj = 1, C_i and C_j by class; Qij = y_i y_j K_ij. ai, aj: in the
// old values, out the new ones.
__device__ __forceinline__ void svm_step(int yi, int yj, double Kij, double Gi, double Gj, double Cp, double Cn, double* ai, double* aj) {
    const double Qij = yi == yj ? Kij : -Kij;
    double a_i = *ai, a_j = *aj;
    if (yi != yj) {
        // (two classes: C_j is the other box, and C_i - C_j is Cp - Cn or its exact negative — one subtraction that does not
        // depend on the pair, so it stays out of the step's chain)
        const double dPN = __dsub_rn(Cp, Cn);
        const double Ci = yi > 0 ? Cp : Cn, Cj = yi > 0 ? Cn : Cp, dC = yi > 0 ? dPN : -dPN;
        double quad = __dadd_rn(2.0, __dmul_rn(2.0, Qij));
        if (quad <= 0.0) quad = SVM_TAU;
        const double delta = __ddiv_rn(__dsub_rn(-Gi, Gj), quad);
        const double diff = __dsub_rn(a_i, a_j);
        a_i = __dadd_rn(a_i, delta);
        a_j = __dadd_rn(a_j, delta);
        if (diff > 0.0) {
            if (a_j < 0.0) { a_j = 0.0; a_i = diff; }
        } else {
            if (a_i < 0.0) { a_i = 0.0; a_j = -diff; }
        }
        if (diff > dC) {  // (C_i - C_j; 0.0 with equal weights)
            if (a_i > Ci) { a_i = Ci; a_j = __dsub_rn(Ci, diff); }
        } else {
            if (a_j > Cj) { a_j = Cj; a_i = __dadd_rn(Cj, diff); }
        }
    } else {
        const double C = svm_box(yi, Cp, Cn);  // (one class: C_i = C_j)
        double quad = __dsub_rn(2.0, __dmul_rn(2.0, Qij));
        if (quad <= 0.0) quad = SVM_TAU;
        const double delta = __ddiv_rn(__dsub_rn(Gi, Gj), quad);
        const double sum = __dadd_rn(a_i, a_j);
        a_i = __dsub_rn(a_i, delta);
        a_j = __dadd_rn(a_j, delta);
        if (sum > C) {
            if (a_i > C) { a_i = C; a_j = __dsub_rn(sum, C); }
        } else {
            if (a_j < 0.0) { a_j = 0.0; a_i = sum; }
        }
        if (sum > C) {
            if (a_j > C) { a_j = C; a_i = __dsub_rn(sum, C); }
        } else {
            if (a_i < 0.0) { a_i = 0.0; a_j = sum; }
        }
    }
    *ai = a_i;
    *aj = a_j;
}

// step 4 for one element
__device__ __forceinline__ double svm_new_G(double G, int yt, int yi, int yj, double kit, double kjt, double dai, double daj) {
    const double qit = yi == yt ? kit : -kit, qjt = yj == yt ? kjt : -kjt;
    return __dadd_rn(G, __dadd_rn(__dmul_rn(qit, dai), __dmul_rn(qjt, daj)));
}

// A workgroup's reduction of one (value, index, tag) a thread, in two levels through LDS (blockDim.x a multiple of 64, at most
// 1024): thread s < 32 takes entries s, s + 32, ... (consecutive lanes read consecutive entries), then every thread takes
// the 32 partials (broadcast reads). MAX: the larger value wins, else the smaller; ties to the lower index. Every thread
// returns the same winner. Two barriers; the arrays may be written again right after the call (the next call's first
// barrier separates its level-two writes from this call's level-two reads).
struct SvmRed {
    double* v;   // [blockDim.x]
    int* i;      // [blockDim.x]
    int* w;      // [blockDim.x]  a tag that travels with the winner
    double* pv;  // [SVM_PART]
    int* pi;
    int* pw;
};
template <bool MAX>
__device__ __forceinline__ void svm_reduce(const SvmRed& r, double* v, int* i, int* w) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    r.v[tid] = *v; r.i[tid] = *i; r.w[tid] = *w;
    __syncthreads();
    if (tid < (uint32_t)SVM_PART) {
        double bv = r.v[tid];
        int bi = r.i[tid], bw = r.w[tid];
        for (uint32_t q = tid + SVM_PART; q < nt; q += SVM_PART) {
            const double x = r.v[q];
            const int xi = r.i[q];
            if (MAX ? svm_better_max(x, xi, bv, bi) : svm_better_min(x, xi, bv, bi)) { bv = x; bi = xi; bw = r.w[q]; }
        }
        r.pv[tid] = bv; r.pi[tid] = bi; r.pw[tid] = bw;
    }
    __syncthreads();
    double bv = r.pv[0];
    int bi = r.pi[0], bw = r.pw[0];
#pragma unroll 4
    for (int q = 1; q < SVM_PART; ++q) {
        const double x = r.pv[q];
        const int xi = r.pi[q];
        if (MAX ? svm_better_max(x, xi, bv, bi) : svm_better_min(x, xi, bv, bi)) { bv = x; bi = xi; bw = r.pw[q]; }
    }
    *v = bv; *i = bi; *w = bw;
}

// LDS of k_svm_wg for n elements and nt threads, in bytes (the host sizes the launch with it)
__host__ __device__ inline size_t svm_wg_lds(uint32_t n, uint32_t nt) {
    const size_t n8 = ((size_t)n + 7) & ~(size_t)7;
    return n8 * 17 + (size_t)nt * 16 + (size_t)SVM_PART * 16;
}

// =============================================================================================
// ROW MAPS. A problem is n elements; rows(e) is the row of the triangle that element e stands for. The single solve is the
// whole training set (element e is row e), a problem of a batch is a strictly ascending list of training rows (fsk_svm_cv),
// so the lowest element is the lowest row and every tie falls as in the single solve on the sub-matrix. The iterations below
// are written once over the map: each kernel is an instantiation with one of the two, there is no run-time "batch or not".
// KEPT: whether the workgroup form keeps the rows it read in step 2 for step 4 (a list's are loads; e is e again for nothing).
struct SvmRowsAll {
    static constexpr bool KEPT = false;
    __device__ __forceinline__ uint32_t operator()(uint32_t e) const { return e; }
};
struct SvmRowsList {
    static constexpr bool KEPT = true;
    const uint32_t* idx;
    __device__ __forceinline__ uint32_t operator()(uint32_t e) const { return idx[e]; }
};

// =============================================================================================
// ONE WORKGROUP (n <= svm_wg_max <= 8192): alpha, G and y live in LDS (17 bytes an element: 139,264 bytes at 8192, beside
// 17 KB of reduction scratch — one workgroup may take all 160 KiB of a CU), up to `chunk` iterations a launch. The state is
// loaded from and written back to device memory around them, so no launch runs unbounded. Element e belongs to thread
// e mod blockDim.x, which alone writes its alpha and G. Seven barriers an iteration (two a reduction, one before the writes).
template <typename SrcT, typename Rows>
__device__ __forceinline__ void svm_wg_iterations(unsigned char* smem, const SrcT* K, const double* diag, const Rows rows, uint32_t n, double Cp,
                                                  double Cn, double eps, long long max_iter, uint32_t chunk, double* alpha, double* G,
                                                  const signed char* y, SvmRecB* rec) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const size_t n8 = ((size_t)n + 7) & ~(size_t)7;
    double* sA = reinterpret_cast<double*>(smem);
    double* sG = sA + n8;
    SvmRed red;
    red.v = sG + n8;
    red.pv = red.v + nt;
    red.i = reinterpret_cast<int*>(red.pv + SVM_PART);
    red.w = red.i + nt;
    red.pi = red.w + nt;
    red.pw = red.pi + SVM_PART;
    signed char* sY = reinterpret_cast<signed char*>(red.pw + SVM_PART);

    for (uint32_t e = tid; e < n; e += nt) { sA[e] = alpha[e]; sG[e] = G[e]; sY[e] = y[e]; }
    long long iter = rec->iter;
    double gmax = rec->gmax, gmin = rec->gmin;
    int done = 0, converged = 0;
    __syncthreads();

    for (uint32_t c = 0; c < chunk; ++c) {
        // ---- 1. i, Gmax, Gmin
        double vmax = -svm_inf(), vmin = svm_inf();
        int imax = SVM_NONE, none = 0;
        for (uint32_t e = tid; e < n; e += nt) {
            const int ye = sY[e];
            const double a = sA[e], v = svm_v(ye, sG[e]);
            if (svm_in_up(ye, a, Cp) && svm_better_max(v, (int)e, vmax, imax)) { vmax = v; imax = (int)e; }
            if (svm_in_low(ye, a, Cn) && v < vmin) vmin = v;
        }
        svm_reduce<true>(red, &vmax, &imax, &none);
        int at = 0;
        svm_reduce<false>(red, &vmin, &at, &none);
        gmax = vmax; gmin = vmin;
        if (__dsub_rn(gmax, gmin) <= eps) { done = 1; converged = 1; break; }
        if (iter >= max_iter) { done = 1; break; }
        const uint32_t i = (uint32_t)imax, ri = rows(i);
        // ---- 2. j (row i, and the elements' rows where they are kept, stay in registers for step 4)
        double kit[SVM_WG_ITEMS];
        uint32_t row[SVM_WG_ITEMS];
        double obj = svm_inf();
        int j = SVM_NONE;
#pragma unroll
        for (int q = 0; q < SVM_WG_ITEMS; ++q) {
            const uint32_t e = tid + (uint32_t)q * nt;
            kit[q] = 0.0;
            if constexpr (Rows::KEPT) row[q] = 0;
            if (e < n) {
                const uint32_t r = rows(e);
                if constexpr (Rows::KEPT) row[q] = r;
                kit[q] = svm_cell(K, diag, ri, r);
                const int ye = sY[e];
                double o;
                if (svm_in_low(ye, sA[e], Cn) && svm_j_objective(gmax, svm_v(ye, sG[e]), kit[q], &o) && svm_better_min(o, (int)e, obj, j)) { obj = o; j = (int)e; }
            }
        }
        svm_reduce<false>(red, &obj, &j, &none);
        // no candidate (LIBSVM's Gmin_idx == -1; only cells that are not numbers — a result with a zero diagonal — get here,
        // a NaN objective wins no comparison): the solve ends, not converged, the step not taken
        if (j == SVM_NONE) { done = 1; break; }
        // ---- 3. the step, by every thread alike
        const uint32_t rj = rows((uint32_t)j);
        const int yi = sY[i], yj = sY[j];
        const double ai0 = sA[i], aj0 = sA[j], Gi = sG[i], Gj = sG[j];
        double ai = ai0, aj = aj0;
        svm_step(yi, yj, svm_cell(K, diag, ri, rj), Gi, Gj, Cp, Cn, &ai, &aj);
        const double dai = __dsub_rn(ai, ai0), daj = __dsub_rn(aj, aj0);
        __syncthreads();  // (everybody has read alpha and G of i and j)
        // ---- 4. G, alpha
#pragma unroll
        for (int q = 0; q < SVM_WG_ITEMS; ++q) {
            const uint32_t e = tid + (uint32_t)q * nt;
            if (e < n) {
                uint32_t r = e;
                if constexpr (Rows::KEPT) r = row[q];
                sG[e] = svm_new_G(sG[e], sY[e], yi, yj, kit[q], svm_cell(K, diag, rj, r), dai, daj);
                if (e == i) sA[e] = ai;
                if (e == (uint32_t)j) sA[e] = aj;
            }
        }
        ++iter;
    }
    __syncthreads();
    for (uint32_t e = tid; e < n; e += nt) { alpha[e] = sA[e]; G[e] = sG[e]; }
    if (tid == 0) {
        rec->iter = iter; rec->gmax = gmax; rec->gmin = gmin;
        rec->done = done; rec->converged = converged; rec->pending = 0;
    }
}

template <typename SrcT>
__global__ __launch_bounds__(SVM_WG_THREADS) void k_svm_wg(const SrcT* K, const double* diag, uint32_t n, double Cp, double Cn, double eps,
                                                           long long max_iter, uint32_t chunk, double* alpha, double* G,
                                                           const signed char* y, SvmRecB* rec) {
    FSK_DYN_SHARED(unsigned char, smem);
    svm_wg_iterations(smem, K, diag, SvmRowsAll{}, n, Cp, Cn, eps, max_iter, chunk, alpha, G, y, rec);
}

// =============================================================================================
// TWO LAUNCHES AN ITERATION (any n): 256 threads a workgroup, one element a thread, no barrier across workgroups — what one
// launch's workgroups tell each other travels through device memory to the NEXT launch, where every workgroup reduces the
// per-workgroup candidates again (the same winner everywhere: the order is total).
constexpr int SVM_THREADS = 256;

// LAUNCH A: finish the pending step — j from the workgroups' candidates, the scalar step, this workgroup's slice of G, alpha
// of i and j by the workgroups that hold them — then this workgroup's share of the next step 1.
template <typename SrcT, typename Rows>
__device__ __forceinline__ void svm_select_i(const SrcT* K, const double* diag, const Rows rows, uint32_t n, double Cp, double Cn, double* alpha,
                                             double* G, const signed char* y, const double* krow, const SvmRecB* rb, SvmRecA* ra,
                                             SvmCandI* cand_i, const SvmCandJ* cand_j, uint32_t n_wg) {
    __shared__ double s_v[SVM_THREADS], s_pv[SVM_PART];
    __shared__ int s_i[SVM_THREADS], s_w[SVM_THREADS], s_pi[SVM_PART], s_pw[SVM_PART];
    const SvmRed red{s_v, s_i, s_w, s_pv, s_pi, s_pw};
    const uint32_t tid = threadIdx.x, t = blockIdx.x * SVM_THREADS + tid;
    if (rb->done) {
        if (blockIdx.x == 0 && tid == 0) { ra->iter = rb->iter; ra->done = 1; }
        return;
    }
    long long iter = rb->iter;
    const bool mine = t < n;
    const int yt = mine ? (int)y[t] : 1;
    double a = mine ? alpha[t] : 0.0, g = mine ? G[t] : 0.0;
    if (rb->pending) {
        double obj = svm_inf();
        int j = SVM_NONE, w = 0;
        for (uint32_t q = tid; q < n_wg; q += SVM_THREADS) {
            const double o = cand_j[q].obj;
            const int oj = cand_j[q].j;
            if (svm_better_min(o, oj, obj, j)) { obj = o; j = oj; w = (int)q; }
        }
        svm_reduce<false>(red, &obj, &j, &w);
        if (j == SVM_NONE) {  // no workgroup had a candidate: the solve ends here (launch B turns done = 2 into the host's done flag)
            if (blockIdx.x == 0 && tid == 0) { ra->iter = iter; ra->done = 2; }
            return;
        }
        const SvmCandJ cj = cand_j[w];
        const int i = rb->i, yi = rb->yi;
        double ai = rb->ai, aj = cj.aj;
        svm_step(yi, cj.yj, cj.Kij, rb->Gi, cj.Gj, Cp, Cn, &ai, &aj);
        const double dai = __dsub_rn(ai, rb->ai), daj = __dsub_rn(aj, cj.aj);
        if (mine) {
            g = svm_new_G(g, yt, yi, cj.yj, krow[t], svm_cell(K, diag, rows((uint32_t)j), rows(t)), dai, daj);
            G[t] = g;
            if (t == (uint32_t)i) { a = ai; alpha[t] = a; }
            if (t == (uint32_t)j) { a = aj; alpha[t] = a; }
        }
        ++iter;
    }
    const double v = svm_v(yt, g);
    double vmax = -svm_inf(), vmin = svm_inf();
    int imax = SVM_NONE, none = 0, at = 0;
    if (mine && svm_in_up(yt, a, Cp)) { vmax = v; imax = (int)t; }
    if (mine && svm_in_low(yt, a, Cn)) vmin = v;
    svm_reduce<true>(red, &vmax, &imax, &none);
    svm_reduce<false>(red, &vmin, &at, &none);
    if (tid == 0) {
        cand_i[blockIdx.x].vmax = vmax; cand_i[blockIdx.x].vmin = vmin; cand_i[blockIdx.x].imax = imax;
        if (blockIdx.x == 0) { ra->iter = iter; ra->done = 0; }
    }
}

// LAUNCH B: i, Gmax and Gmin from the workgroups' candidates; the stop tests; row i (kept in krow for launch A), this
// workgroup's candidate for j.
template <typename SrcT, typename Rows>
__device__ __forceinline__ void svm_select_j(const SrcT* K, const double* diag, const Rows rows, uint32_t n, double Cp, double Cn, double eps,
                                             long long max_iter, const double* alpha, const double* G, const signed char* y, double* krow,
                                             SvmRecB* rb, const SvmRecA* ra, const SvmCandI* cand_i, SvmCandJ* cand_j, uint32_t n_wg) {
    __shared__ double s_v[SVM_THREADS], s_pv[SVM_PART];
    __shared__ int s_i[SVM_THREADS], s_w[SVM_THREADS], s_pi[SVM_PART], s_pw[SVM_PART];
    const SvmRed red{s_v, s_i, s_w, s_pv, s_pi, s_pw};
    const uint32_t tid = threadIdx.x, t = blockIdx.x * SVM_THREADS + tid;
    if (ra->done) {
        // 2: launch A found no j candidate — the end of the solve, not converged (gmax, gmin stay those of the last selection)
        if (ra->done == 2 && blockIdx.x == 0 && tid == 0) { rb->iter = ra->iter; rb->done = 1; rb->converged = 0; rb->pending = 0; }
        return;
    }
    const long long iter = ra->iter;
    double vmax = -svm_inf(), vmin = svm_inf();
    int imax = SVM_NONE, none = 0, at = 0;
    for (uint32_t q = tid; q < n_wg; q += SVM_THREADS) {
        const double x = cand_i[q].vmax, m = cand_i[q].vmin;
        const int xi = cand_i[q].imax;
        if (svm_better_max(x, xi, vmax, imax)) { vmax = x; imax = xi; }
        if (m < vmin) vmin = m;
    }
    svm_reduce<true>(red, &vmax, &imax, &none);
    svm_reduce<false>(red, &vmin, &at, &none);
    const bool converged = __dsub_rn(vmax, vmin) <= eps;
    if (converged || iter >= max_iter) {
        if (blockIdx.x == 0 && tid == 0) {
            rb->iter = iter; rb->gmax = vmax; rb->gmin = vmin;
            rb->done = 1; rb->converged = converged ? 1 : 0; rb->pending = 0;
        }
        return;
    }
    const uint32_t i = (uint32_t)imax;
    double obj = svm_inf(), kit = 0.0, a = 0.0, g = 0.0;
    int j = SVM_NONE, yt = 1;
    if (t < n) {
        kit = svm_cell(K, diag, rows(i), rows(t));
        krow[t] = kit;
        yt = (int)y[t]; a = alpha[t]; g = G[t];
        double o;
        if (svm_in_low(yt, a, Cn) && svm_j_objective(vmax, svm_v(yt, g), kit, &o) && svm_better_min(o, (int)t, obj, j)) { obj = o; j = (int)t; }
    }
    svm_reduce<false>(red, &obj, &j, &none);
    if (j == SVM_NONE) {
        if (tid == 0) { cand_j[blockIdx.x].obj = svm_inf(); cand_j[blockIdx.x].j = SVM_NONE; }
    } else if (t == (uint32_t)j) {
        SvmCandJ c;
        c.obj = obj; c.aj = a; c.Gj = g; c.Kij = kit; c.j = j; c.yj = yt;
        cand_j[blockIdx.x] = c;
    }
    if (blockIdx.x == 0 && tid == 0) {
        rb->iter = iter; rb->gmax = vmax; rb->gmin = vmin;
        rb->ai = alpha[i]; rb->Gi = G[i]; rb->i = (int)i; rb->yi = (int)y[i];
        rb->done = 0; rb->converged = 0; rb->pending = 1;
    }
}

template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svm_select_i(const SrcT* K, const double* diag, uint32_t n, double Cp, double Cn, double* alpha,
                                                              double* G, const signed char* y, const double* krow,
                                                              const SvmRecB* rb, SvmRecA* ra, SvmCandI* cand_i,
                                                              const SvmCandJ* cand_j, uint32_t n_wg) {
    svm_select_i(K, diag, SvmRowsAll{}, n, Cp, Cn, alpha, G, y, krow, rb, ra, cand_i, cand_j, n_wg);
}

template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svm_select_j(const SrcT* K, const double* diag, uint32_t n, double Cp, double Cn, double eps,
                                                              long long max_iter, const double* alpha, const double* G,
                                                              const signed char* y, double* krow, SvmRecB* rb, const SvmRecA* ra,
                                                              const SvmCandI* cand_i, SvmCandJ* cand_j, uint32_t n_wg) {
    svm_select_j(K, diag, SvmRowsAll{}, n, Cp, Cn, eps, max_iter, alpha, G, y, krow, rb, ra, cand_i, cand_j, n_wg);
}

// =============================================================================================
// DECISION VALUES: out[r - r0] = sum_{i < n_train} coef_i K(r, i) - rho for rows [r0, r1) of the N-set, coef = alpha y. One
// wave a row: a test row's train columns are contiguous in the triangle, a train row reads tri_index(r, 0..r) and then one
// cell a triangle row. Never a test x test cell. A lane sums its columns (lane, lane + 64, ...) in order, then the wave's
// lanes by xor shuffles; columns whose coefficient is zero are not read.
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_decision(const SrcT* K, const double* diag, const double* coef, uint32_t n_train,
                                                      uint32_t r0, uint32_t r1, double rho, double* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = r0 + blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = r < r1;  // (a dead wave still takes part in nothing: shuffles are per wave)
    double acc = 0.0;
    if (live)
        for (uint32_t i = lane; i < n_train; i += 64u) {
            const double c = coef[i];
            if (c != 0.0) acc = __dadd_rn(acc, __dmul_rn(c, svm_cell(K, diag, r, i)));
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, d));
    if (live && lane == 0) out[r - r0] = __dsub_rn(acc, rho);
}

// =============================================================================================
// A BATCH OF PROBLEMS ON ONE TRIANGLE (fsk_svm_cv: folds x values of C). Problem p is n of the training rows, a strictly
// ascending list (SvmRowsList), with labels and Cp, Cn of its own. Its kernels are the iterations above instantiated over
// that list, with the problem as one more grid dimension: what is written here is what is theirs alone — which problem a
// workgroup serves, the workgroups that have nothing to do, the problem's slices of the batch's arrays. The single-problem
// kernels keep their names, arguments and launches; the two sets share source, not a run-time mode.
struct SvmProb {
    double Cp, Cn;               // the boxes of its rows of label +1 / -1
    unsigned long long idx_off;  // idx and y of the problem start here (the problems of one fold share them)
    unsigned long long st_off;   // alpha, G and the kept row of the problem start here
    uint32_t n;                  // elements
    uint32_t wg_off;             // two-launch form: the first of its ceil(n / 256) candidate slots
};

// One workgroup a problem (blockIdx.x), alpha, G and y of ITS problem in LDS laid out as in k_svm_wg for its own n; the launch's
// LDS and thread count are those of the largest problem (n <= 8 blockDim.x for every problem of the launch). A workgroup
// whose record says done returns before it touches anything: the alpha and G of a finished problem are written once.
template <typename SrcT>
__global__ __launch_bounds__(SVM_WG_THREADS) void k_svm_wg_batch(const SrcT* K, const double* diag, const SvmProb* probs,
                                                                 const uint32_t* idx_all, const signed char* y_all, double eps,
                                                                 long long max_iter, uint32_t chunk, double* alpha_all, double* G_all,
                                                                 SvmRecB* recs) {
    FSK_DYN_SHARED(unsigned char, smem);
    SvmRecB* rec = recs + blockIdx.x;
    if (rec->done) return;  // (the whole workgroup: nobody writes the record before the end of the launch)
    const SvmProb pr = probs[blockIdx.x];
    svm_wg_iterations(smem, K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, pr.Cn, eps, max_iter, chunk, alpha_all + pr.st_off,
                      G_all + pr.st_off, y_all + pr.idx_off, rec);
}

// The two launches with the problem in blockIdx.y: the grid is (the largest problem's workgroups, problems), and a workgroup
// beyond its own problem's ceil(n / 256) returns at once — it writes no candidate slot and no reduction reads one of its
// (every reduction runs over the problem's own count). Records, candidate slots, the kept row, alpha and G are the
// problem's own, so "no launch reads a record that one of its own workgroups writes" holds problem by problem.
template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svm_select_i_batch(const SrcT* K, const double* diag, const SvmProb* probs,
                                                                    const uint32_t* idx_all, const signed char* y_all, double* alpha_all,
                                                                    double* G_all, const double* krow_all, const SvmRecB* rbs, SvmRecA* ras,
                                                                    SvmCandI* cand_i_all, const SvmCandJ* cand_j_all) {
    const SvmProb pr = probs[blockIdx.y];
    const uint32_t n_wg = (pr.n + SVM_THREADS - 1) / SVM_THREADS;
    if (blockIdx.x >= n_wg) return;
    svm_select_i(K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, pr.Cn, alpha_all + pr.st_off, G_all + pr.st_off, y_all + pr.idx_off,
                 krow_all + pr.st_off, rbs + blockIdx.y, ras + blockIdx.y, cand_i_all + pr.wg_off, cand_j_all + pr.wg_off, n_wg);
}

template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svm_select_j_batch(const SrcT* K, const double* diag, const SvmProb* probs,
                                                                    const uint32_t* idx_all, const signed char* y_all, double eps,
                                                                    long long max_iter, const double* alpha_all, const double* G_all,
                                                                    double* krow_all, SvmRecB* rbs, const SvmRecA* ras,
                                                                    const SvmCandI* cand_i_all, SvmCandJ* cand_j_all) {
    const SvmProb pr = probs[blockIdx.y];
    const uint32_t n_wg = (pr.n + SVM_THREADS - 1) / SVM_THREADS;
    if (blockIdx.x >= n_wg) return;
    svm_select_j(K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, pr.Cn, eps, max_iter, alpha_all + pr.st_off, G_all + pr.st_off,
                 y_all + pr.idx_off, krow_all + pr.st_off, rbs + blockIdx.y, ras + blockIdx.y, cand_i_all + pr.wg_off, cand_j_all + pr.wg_off,
                 n_wg);
}

// OUT-OF-FOLD DECISION VALUES: for the value of C blockIdx.y and training row t, out[c][t] = sum_i coef_p[i] K(t, i) - rho_p
// with p = c n_folds + fold[t], the one problem of that C which did not train on t. coef_p is alpha y at full length
// (n_train, zero at the problem's held-out rows), so the sum and its order are those of k_svm_decision: one wave a row, a
// lane its columns lane, lane + 64, ... in order, zero coefficients skipped, then the xor shuffles. Train x train cells only.
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_decision_oof(const SrcT* K, const double* diag, const double* coef, const double* rho,
                                                          const int32_t* fold, uint32_t n_folds, uint32_t n_train, double* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t < n_train;
    const uint32_t p = blockIdx.y * n_folds + (live ? (uint32_t)fold[t] : 0u);
    const double* cp = coef + (size_t)p * n_train;
    double acc = 0.0;
    if (live)
        for (uint32_t i = lane; i < n_train; i += 64u) {
            const double c = cp[i];
            if (c != 0.0) acc = __dadd_rn(acc, __dmul_rn(c, svm_cell(K, diag, t, i)));
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, d));
    if (live && lane == 0) out[(size_t)blockIdx.y * n_train + t] = __dsub_rn(acc, rho[p]);
}

// =============================================================================================
// ONE-VS-ONE: THE PAIRS' DECISION VALUES AND THE VOTE OF ONE ROW (fsk_svm_multiclass_decision, fsk_svm_multiclass_cv). One wave
// a row r of the N-set, as k_svm_decision. For every pair p of the P = k (k - 1) / 2 in turn the wave computes
//   dec_p(r) = sum_q coef_p[q] K(r, idx_p[q]) - rho_p
// over the pair's OWN row list (the SvmProb of its solve: idx at idx_off, coef = alpha y at st_off, both at the pair's
// length n_p): a lane takes the positions lane, lane + 64, ... of the list in order, one __dmul_rn and one __dadd_rn a term,
// zero coefficients skipped with their cell; then the six xor-shuffle stages (every lane ends with the same sum: a + b is
// b + a to the bit) and __dsub_rn of rho_p — the summation of k_svm_decision over a list. Cells through svm_cell: r may be a
// train or a test row, a list holds train rows only, so no test x test cell is read.
// WHAT A ROW READS: sum_p n_p = (k - 1) n_train coefficients (every training row is in k - 1 lists) and as many row numbers
// where the coefficient is not zero, and the cells of the non-zero ones — a cell once for every pair it is a support vector
// of, not once a row.
// THE VOTE (LIBSVM's): dec_p > 0 gives class a a vote, anything else (a NaN too) class b. Lane c counts class c (k <= 64), in a
// register: no scratch, no LDS. The winner goes over the lanes by xor shuffles of (votes, lane), the lower lane among equals.
// THE LAUNCH: 256 threads, a wave a SIMD, no LDS and no barrier (the waves share nothing), so occupancy is the registers' alone.
// The P values of a row are held one a lane — pair p by lane p mod 64 — and written 64 at a time: consecutive lanes, consecutive
// doubles of the row-major [rows][P] array.
template <typename SrcT>
__device__ __forceinline__ void svm_ovo_row(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                            const double* coef_all, const double* rho, const uint32_t* ab, const int32_t* classes,
                                            uint32_t P, uint32_t r, bool live, double* dec_row, int32_t* pred_out) {
    const uint32_t lane = threadIdx.x & 63u;
    int votes = 0;
    double keep = 0.0;
    for (uint32_t p = 0; p < P; ++p) {
        const SvmProb pr = probs[p];
        const uint32_t* idx = idx_all + pr.idx_off;
        const double* coef = coef_all + pr.st_off;
        double acc = 0.0;
        if (live)
            for (uint32_t q = lane; q < pr.n; q += 64u) {
                const double c = coef[q];
                if (c != 0.0) acc = __dadd_rn(acc, __dmul_rn(c, svm_cell(K, diag, r, idx[q])));
            }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, d));
        const double v = __dsub_rn(acc, rho[p]);
        const uint32_t w = ab[p], winner = v > 0.0 ? (w & 0xffffu) : (w >> 16);
        votes += lane == winner;
        if ((p & 63u) == lane) keep = v;
        if (((p & 63u) == 63u || p + 1 == P) && live && dec_row && lane <= (p & 63u)) dec_row[(p & ~63u) + lane] = keep;
    }
    int best = (int)lane;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int ov = __shfl_xor(votes, d), ob = __shfl_xor(best, d);
        if (ov > votes || (ov == votes && ob < best)) { votes = ov; best = ob; }
    }
    if (live && pred_out && lane == 0) *pred_out = classes[best];
}

// rows [r0, r1) of the N-set under the model's P pairs: dec [r1 - r0][P] and / or pred [r1 - r0], either may be null
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_ovo_decision(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                                          const double* coef_all, const double* rho, const uint32_t* ab,
                                                          const int32_t* classes, uint32_t P, uint32_t r0, uint32_t r1, double* dec,
                                                          int32_t* pred) {
    const uint32_t r = r0 + blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = r < r1;  // (a dead wave reads and writes nothing: shuffles are per wave)
    const size_t at = live ? (size_t)(r - r0) : 0;
    svm_ovo_row(K, diag, probs, idx_all, coef_all, rho, ab, classes, P, r, live, dec ? dec + at * P : nullptr, pred ? pred + at : nullptr);
}

// OUT OF FOLD: for the value of C blockIdx.y and training row t the pairs' models are those of the problem group
// (c n_folds + fold[t]) — problems (c n_folds + fold[t]) P + p, none of which trained on t — as k_svm_decision_oof picks the
// one problem of the binary case. pred [n_C][n_train]; train x train cells only.
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_ovo_decision_oof(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                                              const double* coef_all, const double* rho, const uint32_t* ab,
                                                              const int32_t* classes, uint32_t P, const int32_t* fold, uint32_t n_folds,
                                                              uint32_t n_train, int32_t* pred) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    const bool live = t < n_train;
    const size_t g = (size_t)blockIdx.y * n_folds + (live ? (uint32_t)fold[t] : 0u);
    svm_ovo_row(K, diag, probs + g * P, idx_all, coef_all, rho + g * P, ab, classes, P, t, live, (double*)nullptr,
                pred + (size_t)blockIdx.y * n_train + (live ? t : 0u));
}

// =============================================================================================
// ONE-VS-ONE: CLASS PROBABILITIES OF ONE ROW (fsk_svm_multiclass_calibrate, fsk_svm_multiclass_proba). LIBSVM's
// svm_predict_probability on the device: the pairs' decision values, a sigmoid a pair, and Wu, Lin and Weng's second method
// (multiclass_probability) over the k classes, one wave a row.
//
// svm_ovo_pair is the inner sum of svm_ovo_row restated as a function of its own — the same operations in the same order, so
// the same bits (the tests hold both to one restatement). svm_ovo_row keeps its own text: calling this function from it changed
// the register allocation and the schedule of k_svm_ovo_decision (54 instead of 55 VGPRs), and that kernel is to stay what it is.
// A wave of these kernels is alive as a whole or not at all (a dead wave returns at once), so there is no `live` here.
template <typename SrcT>
__device__ __forceinline__ double svm_ovo_pair(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                               const double* coef_all, const double* rho, uint32_t p, uint32_t r) {
    const uint32_t lane = threadIdx.x & 63u;
    const SvmProb pr = probs[p];
    const uint32_t* idx = idx_all + pr.idx_off;
    const double* coef = coef_all + pr.st_off;
    double acc = 0.0;
    for (uint32_t q = lane; q < pr.n; q += 64u) {
        const double c = coef[q];
        if (c != 0.0) acc = __dadd_rn(acc, __dmul_rn(c, svm_cell(K, diag, r, idx[q])));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, d));
    return __dsub_rn(acc, rho[p]);
}

// OUT OF FOLD, THE VALUES: dec [n_train][P], row t under the P problems of fold[t] (problems fold[t] P + p: one value of C).
// What k_svm_ovo_decision_oof computes and does not keep; the stores are those of svm_ovo_row, 64 values at a time.
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_ovo_values_oof(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                                            const double* coef_all, const double* rho, uint32_t P, const int32_t* fold,
                                                            uint32_t n_train, double* dec) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (t >= n_train) return;  // (the whole wave)
    const size_t g = (size_t)(uint32_t)fold[t] * P;
    double* dec_row = dec + (size_t)t * P;
    double keep = 0.0;
    for (uint32_t p = 0; p < P; ++p) {
        const double v = svm_ovo_pair(K, diag, probs + g, idx_all, coef_all, rho + g, p, t);
        if ((p & 63u) == lane) keep = v;
        if (((p & 63u) == 63u || p + 1 == P) && lane <= (p & 63u)) dec_row[(p & ~63u) + lane] = keep;
    }
}

// LIBSVM's sigmoid_predict and the clamp of svm_predict_probability: fApB = v A + B in two roundings; the exponential is
// fsk::exp_neg, whose argument is never positive on either branch; min(max(s, 1e-7), 1 - 1e-7) with LIBSVM's own comparisons,
// so a NaN becomes 1e-7 as it does there.
__device__ __forceinline__ double svm_pair_prob(double v, double A, double B) {
    const double fApB = __dadd_rn(__dmul_rn(v, A), B);
    double s;
    if (fApB >= 0.0) {
        const double e = exp_neg(-fApB);
        s = __ddiv_rn(e, __dadd_rn(1.0, e));
    } else {
        s = __ddiv_rn(1.0, __dadd_rn(1.0, exp_neg(fApB)));
    }
    constexpr double lo = 1e-7, hi = 1 - 1e-7;
    const double x = s > lo ? s : lo;
    return x < hi ? x : hi;
}

// the lanes of a wave meet: LDS written by one lane above is read by another below
__device__ __forceinline__ void svm_wave_sync() {
#ifdef FSK_EMU
    (void)__shfl(0, 0);  // (the emulator's lanes are fibers that meet at collectives only)
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}

// rows [r0, r1) under the model's P pairs and their sigmoids (sigA, sigB [P]): prob [r1 - r0][k], pred [r1 - r0] (the class of
// the largest probability, the lowest class among equals), iters [r1 - r0] (the coupling's iterations; 0 for k = 2); each may be
// null. 256 threads, a wave a row, a wave a SIMD.
// 1. The pair loop: v = dec_p(r) (svm_ovo_pair), x = svm_pair_prob(v, A_p, B_p) in every lane; r[a][b] = x is kept in the
//    wave's OWN slice of LDS, rp[p] (8 P bytes a wave, 64,512 bytes a workgroup at 64 classes; written 64 pairs at a time),
//    r[b][a] = 1 - x is formed where it is read (one rounding, as LIBSVM's stored value). No barrier: no wave reads another's.
// 2. k = 2: p = (x, 1 - x). Otherwise lane t owns class t and the wave runs multiclass_probability operation for operation:
//    Q[t][t] = sum_{j != t} r[j][t]^2 in ascending j (a register); Q[t][j] = -(r[j][t] r[t][j]) is formed from LDS where it is
//    used (the product commutes, so Q[t][j] and Q[j][t] are one value); p = 1 / k, eps = 0.005 / k, at most max(100, k)
//    iterations of
//      Qp[t] = sum_j Q[t][j] p[j] in ascending j from 0.0 (p[j] by a shuffle from lane j);
//      pQp = sum_t p[t] Qp[t] in ascending t, every lane the same scalar (the products by shuffles);
//      max_t |Qp[t] - pQp| by xor shuffles (a maximum does not depend on the order); stop when it is < eps;
//      for t = 0 .. k - 1 in turn: diff = (-Qp[t] + pQp) / Q[t][t], p[t] += diff,
//        pQp = (pQp + diff (diff Q[t][t] + 2 Qp[t])) / (1 + diff) / (1 + diff), and in every lane j
//        Qp[j] = (Qp[j] + diff Q[t][j]) / (1 + diff), p[j] /= (1 + diff).
//    One rounding an operation, divisions by __ddiv_rn. Lanes k .. 63 take part in the shuffles and hold nothing.
template <typename SrcT>
__global__ __launch_bounds__(256) void k_svm_ovo_proba(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                                       const double* coef_all, const double* rho, const double* sigA, const double* sigB,
                                                       const int32_t* classes, uint32_t k, uint32_t P, uint32_t r0, uint32_t r1,
                                                       double* prob, int32_t* pred, int32_t* iters) {
    FSK_DYN_SHARED(double, lds);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t r = r0 + blockIdx.x * 4u + wave;
    if (r >= r1) return;  // (the whole wave: a dead wave reads and writes nothing)
    const size_t at = (size_t)(r - r0);
    double* rp = lds + (size_t)wave * P;
    double keep = 0.0;
    for (uint32_t p = 0; p < P; ++p) {
        const double v = svm_ovo_pair(K, diag, probs, idx_all, coef_all, rho, p, r);
        const double x = svm_pair_prob(v, sigA[p], sigB[p]);
        if ((p & 63u) == lane) keep = x;
        if (((p & 63u) == 63u || p + 1 == P) && lane <= (p & 63u)) rp[(p & ~63u) + lane] = keep;
    }
    svm_wave_sync();

    const bool mine = lane < k;  // (this lane owns a class)
    double pr_t = 0.0;
    int iter = 0;
    if (k == 2) {
        const double x = rp[0];
        pr_t = lane == 0 ? x : __dsub_rn(1.0, x);
    } else {
        // r[i][j], i != j, from the pair (min, max) at a (2k - a - 1) / 2 + (b - a - 1)
        auto rij = [&](uint32_t i, uint32_t j) -> double {
            const uint32_t a = i < j ? i : j, b = i < j ? j : i;
            const double x = rp[a * (2u * k - a - 1u) / 2u + (b - a - 1u)];
            return i < j ? x : __dsub_rn(1.0, x);
        };
        auto q_of = [&](uint32_t t, uint32_t j, double qtt) -> double {  // Q[t][j] seen from lane j (or t): the diagonal is qtt
            return t == j ? qtt : -__dmul_rn(rij(j, t), rij(t, j));
        };
        double Qtt = 0.0;
        if (mine)
            for (uint32_t j = 0; j < k; ++j)
                if (j != lane) {
                    const double x = rij(j, lane);
                    Qtt = __dadd_rn(Qtt, __dmul_rn(x, x));
                }
        const double kd = (double)k, eps = __ddiv_rn(0.005, kd);
        const int max_iter = k > 100u ? (int)k : 100;
        double Qp = 0.0;
        pr_t = __ddiv_rn(1.0, kd);
        for (; iter < max_iter; ++iter) {
            double q = 0.0;
            for (uint32_t j = 0; j < k; ++j) {
                const double pj = __shfl(pr_t, (int)j);
                if (mine) q = __dadd_rn(q, __dmul_rn(q_of(lane, j, Qtt), pj));
            }
            Qp = q;
            const double prod = __dmul_rn(pr_t, Qp);
            double pQp = 0.0;
            for (uint32_t t = 0; t < k; ++t) pQp = __dadd_rn(pQp, __shfl(prod, (int)t));
            double err = mine ? fabs(__dsub_rn(Qp, pQp)) : 0.0;
            err = err > 0.0 ? err : 0.0;  // (LIBSVM's `error > max_error` from 0 never takes a NaN)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double o = __shfl_xor(err, d);
                err = o > err ? o : err;
            }
            if (err < eps) break;
            for (uint32_t t = 0; t < k; ++t) {
                const double Qp_t = __shfl(Qp, (int)t), Qtt_t = __shfl(Qtt, (int)t);
                const double diff = __ddiv_rn(__dadd_rn(-Qp_t, pQp), Qtt_t), d1 = __dadd_rn(1.0, diff);
                if (lane == t) pr_t = __dadd_rn(pr_t, diff);
                pQp = __ddiv_rn(__ddiv_rn(__dadd_rn(pQp, __dmul_rn(diff, __dadd_rn(__dmul_rn(diff, Qtt_t), __dmul_rn(2.0, Qp_t)))), d1), d1);
                if (mine) {
                    Qp = __ddiv_rn(__dadd_rn(Qp, __dmul_rn(diff, q_of(t, lane, Qtt))), d1);
                    pr_t = __ddiv_rn(pr_t, d1);
                }
            }
        }
    }
    if (prob && mine) prob[at * k + lane] = pr_t;
    if (iters && lane == 0) iters[at] = iter;
    double best_p = mine ? pr_t : -svm_inf();
    int best = (int)lane;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double op = __shfl_xor(best_p, d);
        const int ob = __shfl_xor(best, d);
        if (op > best_p || (op == best_p && ob < best)) { best_p = op; best = ob; }
    }
    if (pred && lane == 0) pred[at] = classes[best];
}

// =============================================================================================
// EPSILON-SVR: THE ITERATION OVER TWIN ELEMENTS (fsk_svr_train, fsk_svr_cv). LIBSVM solves the regression with the same
// Solver over 2n variables: element e < n is alpha_e with y = +1, element e + n is alpha*_e with y = -1, both stand for
// kernel row e (rows(e) in a batch), Q(e, f) = y_e y_f K(e mod n, f mod n), one box C for all, alpha = 0 and G = p at the
// start (the host forms p). Steps 1-4 and their functions are the ones above with Cp = Cn = C; ties go to the lowest element
// in [0, 2n). What is written here is the mapping: a thread owns BOTH twins of a row, so a cell svm_cell(K, diag, ri, r)
// read in step 2 serves the element and its twin and is kept for step 4 of both, and so is row j's — the kernel rows an
// iteration reads are those of an n-row C-SVC solve, not of a 2n-row one. The sign follows from the half: no y is loaded.
// The kernels are instantiations of their own; the C-SVC kernels above carry no "regression or not".
constexpr int SVR_WG_ROWS = 4;           // k_svr_wg: rows a thread at most (4096 rows = 8192 elements = svm_wg_max's ceiling)

// LDS of k_svr_wg for n rows and nt threads: alpha and G of the 2n elements (16 bytes an element: 147,968 bytes at 4096 rows
// and 1024 threads, below svm_wg_lds(8192, 1024))
__host__ __device__ inline size_t svr_wg_lds(uint32_t n, uint32_t nt) {
    const size_t m8 = (2 * (size_t)n + 7) & ~(size_t)7;
    return m8 * 16 + (size_t)nt * 16 + (size_t)SVM_PART * 16;
}

// steps 1 and 2 for the two elements of one row: the better candidate of the pair into the thread's running one
__device__ __forceinline__ void svr_pair_i(uint32_t r, uint32_t n, double C, double a_up, double g_up, double a_dn, double g_dn, double* vmax,
                                           int* imax, double* vmin) {
    const double vu = svm_v(1, g_up), vd = svm_v(-1, g_dn);
    if (svm_in_up(1, a_up, C) && svm_better_max(vu, (int)r, *vmax, *imax)) { *vmax = vu; *imax = (int)r; }
    if (svm_in_up(-1, a_dn, C) && svm_better_max(vd, (int)(r + n), *vmax, *imax)) { *vmax = vd; *imax = (int)(r + n); }
    if (svm_in_low(1, a_up, C) && vu < *vmin) *vmin = vu;
    if (svm_in_low(-1, a_dn, C) && vd < *vmin) *vmin = vd;
}
__device__ __forceinline__ void svr_pair_j(uint32_t r, uint32_t n, double C, double gmax, double kit, double a_up, double g_up, double a_dn,
                                           double g_dn, double* obj, int* j) {
    double o;
    if (svm_in_low(1, a_up, C) && svm_j_objective(gmax, svm_v(1, g_up), kit, &o) && svm_better_min(o, (int)r, *obj, *j)) { *obj = o; *j = (int)r; }
    if (svm_in_low(-1, a_dn, C) && svm_j_objective(gmax, svm_v(-1, g_dn), kit, &o) && svm_better_min(o, (int)(r + n), *obj, *j)) { *obj = o; *j = (int)(r + n); }
}

// ONE WORKGROUP (2n <= svm_wg_max): alpha and G of the 2n elements in LDS, element e at [e]. Thread tid owns rows
// tid + q blockDim.x, q < 4, and both elements of each; it alone writes their alpha and G. Barriers as in svm_wg_iterations.
template <typename SrcT, typename Rows>
__device__ __forceinline__ void svr_wg_iterations(unsigned char* smem, const SrcT* K, const double* diag, const Rows rows, uint32_t n, double C,
                                                  double eps, long long max_iter, uint32_t chunk, double* alpha, double* G, SvmRecB* rec) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x, m = 2 * n;
    const size_t m8 = ((size_t)m + 7) & ~(size_t)7;
    double* sA = reinterpret_cast<double*>(smem);
    double* sG = sA + m8;
    SvmRed red;
    red.v = sG + m8;
    red.pv = red.v + nt;
    red.i = reinterpret_cast<int*>(red.pv + SVM_PART);
    red.w = red.i + nt;
    red.pi = red.w + nt;
    red.pw = red.pi + SVM_PART;

    for (uint32_t e = tid; e < m; e += nt) { sA[e] = alpha[e]; sG[e] = G[e]; }
    long long iter = rec->iter;
    double gmax = rec->gmax, gmin = rec->gmin;
    int done = 0, converged = 0;
    __syncthreads();

    for (uint32_t c = 0; c < chunk; ++c) {
        // ---- 1. i, Gmax, Gmin
        double vmax = -svm_inf(), vmin = svm_inf();
        int imax = SVM_NONE, none = 0;
        for (uint32_t r = tid; r < n; r += nt) svr_pair_i(r, n, C, sA[r], sG[r], sA[r + n], sG[r + n], &vmax, &imax, &vmin);
        svm_reduce<true>(red, &vmax, &imax, &none);
        int at = 0;
        svm_reduce<false>(red, &vmin, &at, &none);
        gmax = vmax; gmin = vmin;
        if (__dsub_rn(gmax, gmin) <= eps) { done = 1; converged = 1; break; }
        if (iter >= max_iter) { done = 1; break; }
        const uint32_t i = (uint32_t)imax, ri = rows(i < n ? i : i - n);
        // ---- 2. j (one cell a row for both twins, kept with the row's number for step 4)
        double kit[SVR_WG_ROWS];
        uint32_t row[SVR_WG_ROWS];
        double obj = svm_inf();
        int j = SVM_NONE;
#pragma unroll
        for (int q = 0; q < SVR_WG_ROWS; ++q) {
            const uint32_t r = tid + (uint32_t)q * nt;
            kit[q] = 0.0;
            if constexpr (Rows::KEPT) row[q] = 0;
            if (r < n) {
                const uint32_t rr = rows(r);
                if constexpr (Rows::KEPT) row[q] = rr;
                kit[q] = svm_cell(K, diag, ri, rr);
                svr_pair_j(r, n, C, gmax, kit[q], sA[r], sG[r], sA[r + n], sG[r + n], &obj, &j);
            }
        }
        svm_reduce<false>(red, &obj, &j, &none);
        if (j == SVM_NONE) { done = 1; break; }  // (as in svm_wg_iterations: cells that are not numbers)
        // ---- 3. the step, by every thread alike
        const uint32_t rj = rows((uint32_t)j < n ? (uint32_t)j : (uint32_t)j - n);
        const int yi = i < n ? 1 : -1, yj = (uint32_t)j < n ? 1 : -1;
        const double ai0 = sA[i], aj0 = sA[j], Gi = sG[i], Gj = sG[j];
        double ai = ai0, aj = aj0;
        svm_step(yi, yj, svm_cell(K, diag, ri, rj), Gi, Gj, C, C, &ai, &aj);
        const double dai = __dsub_rn(ai, ai0), daj = __dsub_rn(aj, aj0);
        __syncthreads();  // (everybody has read alpha and G of i and j)
        // ---- 4. G of both twins from the two cells of the row, alpha
#pragma unroll
        for (int q = 0; q < SVR_WG_ROWS; ++q) {
            const uint32_t r = tid + (uint32_t)q * nt;
            if (r < n) {
                uint32_t rr = r;
                if constexpr (Rows::KEPT) rr = row[q];
                const double kjt = svm_cell(K, diag, rj, rr);
                sG[r] = svm_new_G(sG[r], 1, yi, yj, kit[q], kjt, dai, daj);
                sG[r + n] = svm_new_G(sG[r + n], -1, yi, yj, kit[q], kjt, dai, daj);
                if (r == i) sA[r] = ai;
                if (r + n == i) sA[r + n] = ai;
                if (r == (uint32_t)j) sA[r] = aj;
                if (r + n == (uint32_t)j) sA[r + n] = aj;
            }
        }
        ++iter;
    }
    __syncthreads();
    for (uint32_t e = tid; e < m; e += nt) { alpha[e] = sA[e]; G[e] = sG[e]; }
    if (tid == 0) {
        rec->iter = iter; rec->gmax = gmax; rec->gmin = gmin;
        rec->done = done; rec->converged = converged; rec->pending = 0;
    }
}

// TWO LAUNCHES AN ITERATION: one ROW a thread, both twins; alpha and G have 2n entries, the kept row n; the candidate slots
// stay one a workgroup (n_wg = ceil(n / 256)): a thread hands in the better of its two elements. Records as above, i and j
// element numbers in [0, 2n).
template <typename SrcT, typename Rows>
__device__ __forceinline__ void svr_select_i(const SrcT* K, const double* diag, const Rows rows, uint32_t n, double C, double* alpha, double* G,
                                             const double* krow, const SvmRecB* rb, SvmRecA* ra, SvmCandI* cand_i, const SvmCandJ* cand_j,
                                             uint32_t n_wg) {
    __shared__ double s_v[SVM_THREADS], s_pv[SVM_PART];
    __shared__ int s_i[SVM_THREADS], s_w[SVM_THREADS], s_pi[SVM_PART], s_pw[SVM_PART];
    const SvmRed red{s_v, s_i, s_w, s_pv, s_pi, s_pw};
    const uint32_t tid = threadIdx.x, t = blockIdx.x * SVM_THREADS + tid;
    if (rb->done) {
        if (blockIdx.x == 0 && tid == 0) { ra->iter = rb->iter; ra->done = 1; }
        return;
    }
    long long iter = rb->iter;
    const bool mine = t < n;
    double a_up = mine ? alpha[t] : 0.0, g_up = mine ? G[t] : 0.0, a_dn = mine ? alpha[t + n] : 0.0, g_dn = mine ? G[t + n] : 0.0;
    if (rb->pending) {
        double obj = svm_inf();
        int j = SVM_NONE, w = 0;
        for (uint32_t q = tid; q < n_wg; q += SVM_THREADS) {
            const double o = cand_j[q].obj;
            const int oj = cand_j[q].j;
            if (svm_better_min(o, oj, obj, j)) { obj = o; j = oj; w = (int)q; }
        }
        svm_reduce<false>(red, &obj, &j, &w);
        if (j == SVM_NONE) {
            if (blockIdx.x == 0 && tid == 0) { ra->iter = iter; ra->done = 2; }
            return;
        }
        const SvmCandJ cj = cand_j[w];
        const int i = rb->i, yi = rb->yi;
        double ai = rb->ai, aj = cj.aj;
        svm_step(yi, cj.yj, cj.Kij, rb->Gi, cj.Gj, C, C, &ai, &aj);
        const double dai = __dsub_rn(ai, rb->ai), daj = __dsub_rn(aj, cj.aj);
        if (mine) {
            const uint32_t rj = rows((uint32_t)j < n ? (uint32_t)j : (uint32_t)j - n);
            const double kit = krow[t], kjt = svm_cell(K, diag, rj, rows(t));
            g_up = svm_new_G(g_up, 1, yi, cj.yj, kit, kjt, dai, daj);
            g_dn = svm_new_G(g_dn, -1, yi, cj.yj, kit, kjt, dai, daj);
            G[t] = g_up;
            G[t + n] = g_dn;
            if (t == (uint32_t)i) { a_up = ai; alpha[t] = ai; }
            if (t + n == (uint32_t)i) { a_dn = ai; alpha[t + n] = ai; }
            if (t == (uint32_t)j) { a_up = aj; alpha[t] = aj; }
            if (t + n == (uint32_t)j) { a_dn = aj; alpha[t + n] = aj; }
        }
        ++iter;
    }
    double vmax = -svm_inf(), vmin = svm_inf();
    int imax = SVM_NONE, none = 0, at = 0;
    if (mine) svr_pair_i(t, n, C, a_up, g_up, a_dn, g_dn, &vmax, &imax, &vmin);
    svm_reduce<true>(red, &vmax, &imax, &none);
    svm_reduce<false>(red, &vmin, &at, &none);
    if (tid == 0) {
        cand_i[blockIdx.x].vmax = vmax; cand_i[blockIdx.x].vmin = vmin; cand_i[blockIdx.x].imax = imax;
        if (blockIdx.x == 0) { ra->iter = iter; ra->done = 0; }
    }
}

template <typename SrcT, typename Rows>
__device__ __forceinline__ void svr_select_j(const SrcT* K, const double* diag, const Rows rows, uint32_t n, double C, double eps, long long max_iter,
                                             const double* alpha, const double* G, double* krow, SvmRecB* rb, const SvmRecA* ra,
                                             const SvmCandI* cand_i, SvmCandJ* cand_j, uint32_t n_wg) {
    __shared__ double s_v[SVM_THREADS], s_pv[SVM_PART];
    __shared__ int s_i[SVM_THREADS], s_w[SVM_THREADS], s_pi[SVM_PART], s_pw[SVM_PART];
    const SvmRed red{s_v, s_i, s_w, s_pv, s_pi, s_pw};
    const uint32_t tid = threadIdx.x, t = blockIdx.x * SVM_THREADS + tid;
    if (ra->done) {
        if (ra->done == 2 && blockIdx.x == 0 && tid == 0) { rb->iter = ra->iter; rb->done = 1; rb->converged = 0; rb->pending = 0; }
        return;
    }
    const long long iter = ra->iter;
    double vmax = -svm_inf(), vmin = svm_inf();
    int imax = SVM_NONE, none = 0, at = 0;
    for (uint32_t q = tid; q < n_wg; q += SVM_THREADS) {
        const double x = cand_i[q].vmax, m = cand_i[q].vmin;
        const int xi = cand_i[q].imax;
        if (svm_better_max(x, xi, vmax, imax)) { vmax = x; imax = xi; }
        if (m < vmin) vmin = m;
    }
    svm_reduce<true>(red, &vmax, &imax, &none);
    svm_reduce<false>(red, &vmin, &at, &none);
    const bool converged = __dsub_rn(vmax, vmin) <= eps;
    if (converged || iter >= max_iter) {
        if (blockIdx.x == 0 && tid == 0) {
            rb->iter = iter; rb->gmax = vmax; rb->gmin = vmin;
            rb->done = 1; rb->converged = converged ? 1 : 0; rb->pending = 0;
        }
        return;
    }
    const uint32_t i = (uint32_t)imax;
    double obj = svm_inf(), kit = 0.0, a_up = 0.0, g_up = 0.0, a_dn = 0.0, g_dn = 0.0;
    int j = SVM_NONE;
    if (t < n) {
        kit = svm_cell(K, diag, rows(i < n ? i : i - n), rows(t));
        krow[t] = kit;
        a_up = alpha[t]; g_up = G[t]; a_dn = alpha[t + n]; g_dn = G[t + n];
        svr_pair_j(t, n, C, vmax, kit, a_up, g_up, a_dn, g_dn, &obj, &j);
    }
    const int mine_j = j;  // (this thread's better element, before the reduction)
    svm_reduce<false>(red, &obj, &j, &none);
    if (j == SVM_NONE) {
        if (tid == 0) { cand_j[blockIdx.x].obj = svm_inf(); cand_j[blockIdx.x].j = SVM_NONE; }
    } else if (mine_j == j) {
        const bool up = (uint32_t)j < n;
        SvmCandJ c;
        c.obj = obj; c.aj = up ? a_up : a_dn; c.Gj = up ? g_up : g_dn; c.Kij = kit; c.j = j; c.yj = up ? 1 : -1;
        cand_j[blockIdx.x] = c;
    }
    if (blockIdx.x == 0 && tid == 0) {
        rb->iter = iter; rb->gmax = vmax; rb->gmin = vmin;
        rb->ai = alpha[i]; rb->Gi = G[i]; rb->i = (int)i; rb->yi = i < n ? 1 : -1;
        rb->done = 0; rb->converged = 0; rb->pending = 1;
    }
}

// the single solve: the whole training set
template <typename SrcT>
__global__ __launch_bounds__(SVM_WG_THREADS) void k_svr_wg(const SrcT* K, const double* diag, uint32_t n, double C, double eps, long long max_iter,
                                                           uint32_t chunk, double* alpha, double* G, SvmRecB* rec) {
    FSK_DYN_SHARED(unsigned char, smem);
    svr_wg_iterations(smem, K, diag, SvmRowsAll{}, n, C, eps, max_iter, chunk, alpha, G, rec);
}
template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svr_select_i(const SrcT* K, const double* diag, uint32_t n, double C, double* alpha, double* G,
                                                              const double* krow, const SvmRecB* rb, SvmRecA* ra, SvmCandI* cand_i,
                                                              const SvmCandJ* cand_j, uint32_t n_wg) {
    svr_select_i(K, diag, SvmRowsAll{}, n, C, alpha, G, krow, rb, ra, cand_i, cand_j, n_wg);
}
template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svr_select_j(const SrcT* K, const double* diag, uint32_t n, double C, double eps, long long max_iter,
                                                              const double* alpha, const double* G, double* krow, SvmRecB* rb,
                                                              const SvmRecA* ra, const SvmCandI* cand_i, SvmCandJ* cand_j, uint32_t n_wg) {
    svr_select_j(K, diag, SvmRowsAll{}, n, C, eps, max_iter, alpha, G, krow, rb, ra, cand_i, cand_j, n_wg);
}

// the batch (fsk_svr_cv): SvmProb with n ROWS, Cp the box, st_off the start of the problem's 2n alpha and G (its kept row
// starts at st_off / 2), wg_off the first of its ceil(n / 256) candidate slots. Grids and early returns as in the C-SVC batch.
template <typename SrcT>
__global__ __launch_bounds__(SVM_WG_THREADS) void k_svr_wg_batch(const SrcT* K, const double* diag, const SvmProb* probs, const uint32_t* idx_all,
                                                                 double eps, long long max_iter, uint32_t chunk, double* alpha_all,
                                                                 double* G_all, SvmRecB* recs) {
    FSK_DYN_SHARED(unsigned char, smem);
    SvmRecB* rec = recs + blockIdx.x;
    if (rec->done) return;
    const SvmProb pr = probs[blockIdx.x];
    svr_wg_iterations(smem, K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, eps, max_iter, chunk, alpha_all + pr.st_off, G_all + pr.st_off,
                      rec);
}
template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svr_select_i_batch(const SrcT* K, const double* diag, const SvmProb* probs,
                                                                    const uint32_t* idx_all, double* alpha_all, double* G_all,
                                                                    const double* krow_all, const SvmRecB* rbs, SvmRecA* ras,
                                                                    SvmCandI* cand_i_all, const SvmCandJ* cand_j_all) {
    const SvmProb pr = probs[blockIdx.y];
    const uint32_t n_wg = (pr.n + SVM_THREADS - 1) / SVM_THREADS;
    if (blockIdx.x >= n_wg) return;
    svr_select_i(K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, alpha_all + pr.st_off, G_all + pr.st_off, krow_all + pr.st_off / 2,
                 rbs + blockIdx.y, ras + blockIdx.y, cand_i_all + pr.wg_off, cand_j_all + pr.wg_off, n_wg);
}
template <typename SrcT>
__global__ __launch_bounds__(SVM_THREADS) void k_svr_select_j_batch(const SrcT* K, const double* diag, const SvmProb* probs,
                                                                    const uint32_t* idx_all, double eps, long long max_iter,
                                                                    const double* alpha_all, const double* G_all, double* krow_all,
                                                                    SvmRecB* rbs, const SvmRecA* ras, const SvmCandI* cand_i_all,
                                                                    SvmCandJ* cand_j_all) {
    const SvmProb pr = probs[blockIdx.y];
    const uint32_t n_wg = (pr.n + SVM_THREADS - 1) / SVM_THREADS;
    if (blockIdx.x >= n_wg) return;
    svr_select_j(K, diag, SvmRowsList{idx_all + pr.idx_off}, pr.n, pr.Cp, eps, max_iter, alpha_all + pr.st_off, G_all + pr.st_off,
                 krow_all + pr.st_off / 2, rbs + blockIdx.y, ras + blockIdx.y, cand_i_all + pr.wg_off, cand_j_all + pr.wg_off, n_wg);
}

}  // namespace fsk
