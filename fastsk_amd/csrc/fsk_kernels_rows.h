// fsk_kernels_rows.h — the rows kernel (fsk_rows_build): the second-level kernel L(r, c) = <K(r, train), K(c, train)> of the
// finalized result, the "empirical kernel map" behind the reference's kernel_type = "linear" (fastsk.cpp:318-333: LIBSVM is
// handed the rows of the kernel matrix as feature vectors). Included by fsk_engine_rows.hip only.
//
// The definition is fixed to the operation (tests restate it in numpy and compare bit for bit). With n = n_train and A(r, i)
// the normalised cell (r, i) of the result — the IEEE value fsk_get_block returns —
//   L(r, c) = ((...((A(r,0) A(c,0)) + A(r,1) A(c,1)) + ...) + A(r,n-1) A(c,n-1)):
// one accumulator a cell, summed in ascending i, every product and every sum rounded once (__dmul_rn, __dadd_rn, no
// contraction). So there is no split over i, no tree, no wave reduction, no FMA and no MFMA anywhere below: a thread's loop
// over i ascends through the panels in order, and that is all that keeps the definition.
//
// A lies in an fp64 scratch the existing normalising passes wrote once: the train x train triangle (cell (r, i <= r) at
// tri_index(r, i)) and the test x train rectangle (row r >= n at (r - n) n). A panel of P consecutive i meets that storage in
// three regimes, per T-row block (uniform over the workgroup):
//   1  wholly left of the block's diagonal, or a block of test rows: contiguous in i within a row;
//   2  wholly beyond it: A(r, i) = tri(i, r), contiguous in r for fixed i;
//   0  straddling it, or the short last panel: element by element.
// Both contiguous regimes move 16 bytes a lane: a row (a column) starts at any multiple of 8 bytes, so a lane takes the
// ALIGNED pair k of its run — elements 2k - off and 2k - off + 1, off the parity of the run's first address — and the one or
// two single elements at the run's ends travel as 8 bytes.
//
// LDS image of a panel: [row][ROWS_PITCH] doubles, PITCH = P + 2 = 18 (36 dwords). Thread (ty, tx) of the 16 x 16 workgroup
// owns rows ty + 16 a and columns tx + 16 b of the tile, a, b < T / 16: its 8-byte reads of one i go to dword addresses
// 36 row + 2 i, and 36 tx mod 64 is a different multiple of 4 for each of the 16 tx, so the 32 lanes one ds_read_b64 cycle
// serves (16 tx, two ty: the ty side is a broadcast of two addresses 36 dwords apart) never share a bank. Writes of regime 1
// and 0 are contiguous along a row; those of regime 2 stride by two rows (72 dwords: four lanes a bank): T P / 256 stores a
// thread and panel beside 2 (T / 16) P reads.
#pragma once
#include "fsk_common.h"

namespace fsk {

constexpr int ROWS_TILE = FSK_ROWS_TILE;  // T: 64 or 128 (profiles/rows_kernel.json has both; 64, the faster at N = n = 8000, is built)
constexpr int ROWS_PANEL = FSK_ROWS_PANEL; // P
constexpr int ROWS_PITCH = ROWS_PANEL + 2;
constexpr int ROWS_THREADS = 256;
static_assert((ROWS_TILE == 64 || ROWS_TILE == 128) && ROWS_PANEL == 16, "the register block is T / 16 square; the slot tables assume P = 16");

// the scratch: tri = the train x train triangle, rect = rows n.. of the train columns; both 16-byte aligned
struct RowsSrc {
    const double* tri;
    const double* rect;
    uint32_t n, N;
};

// A(r, i), r < N, i < n
__device__ __forceinline__ double rows_cell(const RowsSrc& S, uint32_t r, uint32_t i) {
    if (r >= S.n) return S.rect[(u64)(r - S.n) * S.n + i];
    return r >= i ? S.tri[tri_index(r, i)] : S.tri[tri_index(i, r)];
}

__device__ __forceinline__ int rows_regime(uint32_t R0, uint32_t i0, uint32_t n) {
    if (i0 + ROWS_PANEL > n) return 0;                      // the short last panel
    if (R0 >= n || i0 + ROWS_PANEL - 1 <= R0) return 1;     // every train row of the block has the panel at or left of its diagonal
    if (R0 + ROWS_TILE - 1 <= i0) return 2;                 // every row of the block lies at or above the panel's first column
    return 0;
}

// Slots of the two contiguous regimes: a run of E elements has E / 2 + 1 aligned pairs at most.
constexpr int ROWS_SLOTS1 = ROWS_TILE * (ROWS_PANEL / 2 + 1);       // (row, pair of i)
constexpr int ROWS_SLOTS2 = ROWS_PANEL * (ROWS_TILE / 2 + 1);       // (i, pair of rows)
constexpr int ROWS_NS = (ROWS_SLOTS1 + ROWS_THREADS - 1) / ROWS_THREADS;   // double2 registers a thread stages an operand in
static_assert(ROWS_SLOTS2 <= ROWS_NS * ROWS_THREADS && ROWS_TILE * ROWS_PANEL <= 2 * ROWS_NS * ROWS_THREADS, "staging registers");

// an aligned pair of a run that starts at p (element 0) and has E elements: elements e0 = 2k - off and e0 + 1; those outside
// [0, E) read as zero and are never stored
__device__ __forceinline__ double2 rows_pair(const double* p, int e0, int E) {
    double2 v;
    if (e0 >= 0 && e0 + 1 < E) {
        v = *reinterpret_cast<const double2*>(p + e0);
    } else {
        v.x = e0 >= 0 && e0 < E ? p[e0] : 0.0;
        v.y = e0 + 1 >= 0 && e0 + 1 < E ? p[e0 + 1] : 0.0;
    }
    return v;
}
__device__ __forceinline__ int rows_parity(const double* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1u); }

// The two contiguous regimes are one loop over RUNS: regime 1 has T runs (the rows) of P elements, regime 2 has P runs (the
// columns i) of T elements; run q starts at cell (a0 + q, b0) of the scratch — (R0 + q, i0), or (i0 + q, R0) read through the
// symmetry — and lands in LDS at q sq + e se.
struct RowsRuns {
    uint32_t a0, b0;      // first cell of run 0
    int E, pairs;         // elements a run; aligned pairs a run at most (E / 2 + 1)
    uint32_t slots;       // runs x pairs
    int sq, se;           // LDS strides of a run and of an element
};
__device__ __forceinline__ RowsRuns rows_runs(uint32_t R0, uint32_t i0, int regime) {
    RowsRuns r;
    if (regime == 1) r = RowsRuns{R0, i0, ROWS_PANEL, ROWS_PANEL / 2 + 1, (uint32_t)ROWS_SLOTS1, ROWS_PITCH, 1};
    else r = RowsRuns{i0, R0, ROWS_TILE, ROWS_TILE / 2 + 1, (uint32_t)ROWS_SLOTS2, 1, ROWS_PITCH};
    return r;
}
__device__ __forceinline__ void rows_slot(int regime, uint32_t slot, uint32_t* q, uint32_t* k) {   // (divisions by constants)
    const uint32_t q1 = slot / (ROWS_PANEL / 2 + 1), q2 = slot / (ROWS_TILE / 2 + 1);
    *q = regime == 1 ? q1 : q2;
    *k = regime == 1 ? slot - q1 * (ROWS_PANEL / 2 + 1) : slot - q2 * (ROWS_TILE / 2 + 1);
}

// global -> registers: panel [i0, i0 + P) of rows [R0, R0 + T). Returns the parities of the runs of this thread's slots
// (bit s: slot s), which rows_put needs again.
__device__ __forceinline__ uint32_t rows_fetch(const RowsSrc& S, uint32_t R0, uint32_t i0, int regime, double2* stg) {
    const uint32_t tid = threadIdx.x;
    uint32_t offs = 0;
    if (regime != 0) {
        const RowsRuns U = rows_runs(R0, i0, regime);
#pragma unroll
        for (int s = 0; s < ROWS_NS; ++s) {
            const uint32_t slot = tid + (uint32_t)s * ROWS_THREADS;
            double2 v;
            v.x = v.y = 0.0;
            uint32_t q, k;
            rows_slot(regime, slot, &q, &k);
            const uint32_t a = U.a0 + q;   // (regime 2: a = i0 + q < n; regime 1: a row, which may lie past N in the last block)
            if (slot < U.slots && a < S.N) {
                const double* p = a >= S.n ? S.rect + (u64)(a - S.n) * S.n + U.b0 : S.tri + tri_index(a, U.b0);
                const int off = rows_parity(p);
                offs |= (uint32_t)off << s;
                v = rows_pair(p, 2 * (int)k - off, U.E);
            }
            stg[s] = v;
        }
    } else {
#pragma unroll
        for (int s = 0; s < ROWS_TILE * ROWS_PANEL / ROWS_THREADS; ++s) {   // (two elements a staging register)
            const uint32_t el = tid + (uint32_t)s * ROWS_THREADS, row = el / ROWS_PANEL, ii = el % ROWS_PANEL;
            const uint32_t r = R0 + row, i = i0 + ii;
            const double v = r < S.N && i < S.n ? rows_cell(S, r, i) : 0.0;
            if (s & 1) stg[s >> 1].y = v; else stg[s >> 1].x = v;
        }
    }
    return offs;
}

// registers -> the LDS image [row][ROWS_PITCH]
__device__ __forceinline__ void rows_put(double* lds, int regime, const double2* stg, uint32_t offs) {
    const uint32_t tid = threadIdx.x;
    if (regime != 0) {
        const RowsRuns U = rows_runs(0, 0, regime);
#pragma unroll
        for (int s = 0; s < ROWS_NS; ++s) {
            const uint32_t slot = tid + (uint32_t)s * ROWS_THREADS;
            uint32_t q, k;
            rows_slot(regime, slot, &q, &k);
            if (slot < U.slots) {
                const int off = (int)((offs >> s) & 1u), e0 = 2 * (int)k - off;
                double* dst = lds + (int)q * U.sq;
                if (regime == 1 && off == 0 && e0 + 1 < U.E) {
                    *reinterpret_cast<double2*>(dst + e0) = stg[s];   // (e0 even, the pitch even: 16-byte aligned)
                } else {
                    if (e0 >= 0 && e0 < U.E) dst[e0 * U.se] = stg[s].x;
                    if (e0 + 1 < U.E) dst[(e0 + 1) * U.se] = stg[s].y;
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < ROWS_TILE * ROWS_PANEL / ROWS_THREADS; ++s) {
            const uint32_t el = tid + (uint32_t)s * ROWS_THREADS, row = el / ROWS_PANEL, ii = el % ROWS_PANEL;
            lds[row * ROWS_PITCH + ii] = (s & 1) ? stg[s >> 1].y : stg[s >> 1].x;
        }
    }
}

// One workgroup a T x T tile of L: grid (column blocks below n, row blocks); a tile above the diagonal returns at once.
// L: the packed triangle of N (N + 1) / 2 cells; diag[r] = L(r, r) of the train rows comes from the diagonal tiles.
constexpr int ROWS_R = ROWS_TILE / 16;
constexpr int ROWS_IMAGE = ROWS_TILE * ROWS_PITCH;
constexpr size_t ROWS_LDS_BYTES = (size_t)4 * ROWS_IMAGE * sizeof(double);
// Registers: the accumulators are (T / 16)^2 doubles — 32 VGPRs at T = 64, 128 at T = 128 —, but the compiler keeps the address
// arithmetic of both staged operands in flight beside them: at T = 64 it takes 232 VGPRs unbounded, spills 32 dwords a lane
// when held to 168 (three waves a SIMD) and 82 when held to 128 (four). The second launch bound picks the occupancy that
// measured fastest (fsk_common.h: three waves at T = 64); the spills sit in the staging code, not in the loop over i.
__global__ __launch_bounds__(ROWS_THREADS, FSK_ROWS_WAVES) void k_rows_syrk(RowsSrc S, double* __restrict__ L, double* __restrict__ diag) {
    const uint32_t tc = blockIdx.x, tr = blockIdx.y;
    if (tc > tr) return;
    FSK_DYN_SHARED(double, lds_all);   // [buffer][row / column operand][ROWS_IMAGE]: ROWS_LDS_BYTES (over 64 KiB at T = 128)
    const uint32_t R0 = tr * ROWS_TILE, C0 = tc * ROWS_TILE, n = S.n;
    const bool same = tr == tc;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t n_panels = (n + ROWS_PANEL - 1) / ROWS_PANEL;

    double acc[ROWS_R][ROWS_R];
#pragma unroll
    for (int a = 0; a < ROWS_R; ++a)
#pragma unroll
        for (int b = 0; b < ROWS_R; ++b) acc[a][b] = -0.0;
    // (-0 + x = x for every x, signed zeros included: the first product enters the sum unchanged, as the definition has it)

    double2 sa[ROWS_NS], sb[ROWS_NS];
    uint32_t oa = 0, ob = 0;
    int ra = rows_regime(R0, 0, n), rb = rows_regime(C0, 0, n);
    oa = rows_fetch(S, R0, 0, ra, sa);
    if (!same) ob = rows_fetch(S, C0, 0, rb, sb);
    rows_put(lds_all, ra, sa, oa);
    if (!same) rows_put(lds_all + ROWS_IMAGE, rb, sb, ob);
    __syncthreads();

    for (uint32_t p = 0; p < n_panels; ++p) {
        const uint32_t buf = p & 1u, i1 = (p + 1) * ROWS_PANEL;
        const bool more = p + 1 < n_panels;
        if (more) {
            ra = rows_regime(R0, i1, n);
            oa = rows_fetch(S, R0, i1, ra, sa);
            if (!same) {
                rb = rows_regime(C0, i1, n);
                ob = rows_fetch(S, C0, i1, rb, sb);
            }
        }
        const double* As = lds_all + 2 * buf * ROWS_IMAGE + ty * ROWS_PITCH;
        const double* Bs = lds_all + (2 * buf + (same ? 0u : 1u)) * ROWS_IMAGE + tx * ROWS_PITCH;
        const uint32_t plen = n - p * ROWS_PANEL < (uint32_t)ROWS_PANEL ? n - p * ROWS_PANEL : (uint32_t)ROWS_PANEL;
        if (plen == (uint32_t)ROWS_PANEL) {
#pragma unroll 2
            for (int ii = 0; ii < ROWS_PANEL; ++ii) {
                double a[ROWS_R], b[ROWS_R];
#pragma unroll
                for (int q = 0; q < ROWS_R; ++q) {
                    a[q] = As[q * 16 * ROWS_PITCH + ii];
                    b[q] = Bs[q * 16 * ROWS_PITCH + ii];
                }
#pragma unroll
                for (int qa = 0; qa < ROWS_R; ++qa)
#pragma unroll
                    for (int qb = 0; qb < ROWS_R; ++qb) acc[qa][qb] = __dadd_rn(acc[qa][qb], __dmul_rn(a[qa], b[qb]));
            }
        } else {
            for (uint32_t ii = 0; ii < plen; ++ii) {
                double a[ROWS_R], b[ROWS_R];
#pragma unroll
                for (int q = 0; q < ROWS_R; ++q) {
                    a[q] = As[q * 16 * ROWS_PITCH + ii];
                    b[q] = Bs[q * 16 * ROWS_PITCH + ii];
                }
#pragma unroll
                for (int qa = 0; qa < ROWS_R; ++qa)
#pragma unroll
                    for (int qb = 0; qb < ROWS_R; ++qb) acc[qa][qb] = __dadd_rn(acc[qa][qb], __dmul_rn(a[qa], b[qb]));
            }
        }
        if (more) {
            rows_put(lds_all + 2 * (buf ^ 1u) * ROWS_IMAGE, ra, sa, oa);
            if (!same) rows_put(lds_all + (2 * (buf ^ 1u) + 1) * ROWS_IMAGE, rb, sb, ob);
        }
        __syncthreads();   // the panel just written is whole; the one just read may be written in the next trip
    }

#pragma unroll
    for (int qa = 0; qa < ROWS_R; ++qa) {
        const uint32_t r = R0 + ty + 16u * qa;
#pragma unroll
        for (int qb = 0; qb < ROWS_R; ++qb) {
            const uint32_t c = C0 + tx + 16u * qb;
            if (r < S.N && c < n && c <= r) {
                L[tri_index(r, c)] = acc[qa][qb];
                if (r == c) diag[r] = acc[qa][qb];
            }
        }
    }
}

// L(r, r) of the test rows: one thread a row, one accumulator, ascending i. 256 rows a workgroup; a panel of the rectangle
// (contiguous in i) goes through LDS transposed, so that the global reads stay coalesced. Pitch P + 1: thread = row reads
// its 16 values at 17 row + ii, 34 dwords a row — the 32 lanes of a ds_read_b64 cycle fall on different bank pairs.
__global__ __launch_bounds__(ROWS_THREADS) void k_rows_diag(RowsSrc S, double* __restrict__ L, double* __restrict__ diag) {
    __shared__ double lds[ROWS_THREADS * (ROWS_PANEL + 1)];
    const uint32_t n = S.n, n_test = S.N - n, row0 = blockIdx.x * ROWS_THREADS, tid = threadIdx.x;
    double acc = -0.0;   // (as in k_rows_syrk)
    for (uint32_t i0 = 0; i0 < n; i0 += ROWS_PANEL) {
        __syncthreads();   // (the previous panel has been read)
#pragma unroll
        for (int s = 0; s < ROWS_PANEL; ++s) {
            const uint32_t el = tid + (uint32_t)s * ROWS_THREADS, row = el / ROWS_PANEL, ii = el % ROWS_PANEL;
            const uint32_t t = row0 + row, i = i0 + ii;
            lds[row * (ROWS_PANEL + 1) + ii] = t < n_test && i < n ? S.rect[(u64)t * n + i] : 0.0;
        }
        __syncthreads();
        const uint32_t plen = n - i0 < (uint32_t)ROWS_PANEL ? n - i0 : (uint32_t)ROWS_PANEL;
        for (uint32_t ii = 0; ii < plen; ++ii) {
            const double a = lds[tid * (ROWS_PANEL + 1) + ii];
            acc = __dadd_rn(acc, __dmul_rn(a, a));
        }
    }
    const uint32_t t = row0 + tid;
    if (t < n_test) {
        const u64 r = (u64)n + t;
        L[tri_index(r, r)] = acc;
        diag[r] = acc;
    }
}

// cells [i0, i0 + rows) x [j0, j0 + cols) of the symmetric matrix: raw L, or K2 = normalised_cell(L(r,c), L(r,r), L(c,c))
__global__ __launch_bounds__(256) void k_rows_block(const double* L, const double* diag, u64 i0, u64 rows, u64 j0, u64 cols, int raw,
                                                    double* out) {
    const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
    if (c >= rows * cols) return;
    const u64 i = i0 + c / cols, j = j0 + c % cols;
    const u64 a = i > j ? i : j, b = i > j ? j : i;
    const double x = L[tri_index(a, b)];
    out[c] = raw ? x : normalised_cell(x, diag[a], diag[b], a == b);
}

}  // namespace fsk
