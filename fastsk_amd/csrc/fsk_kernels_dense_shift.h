// fsk_kernels_dense_shift.h — DENSE dataflow, shift classes: the kept-position sets of a call that differ only by a
// translation t of all kept positions form chains of consecutive shifts. The k-mer that window w shows under shift t is the
// k-mer at absolute start w + t under shift 0, so from shift t to t + 1 a sequence's count vector loses the key of its first
// window under t (delta) and gains the key of its last window under t + 1 (sigma):
//     c_{t+1} = c_t + d_t,  d_t = e(sigma_t) - e(delta_t)
//     G_{t+1}(i, j) = G_t(i, j) + [c_{t+1,i}(sigma_j) - c_{t+1,i}(delta_j)] + [c_{t,j}(sigma_i) - c_{t,j}(delta_i)]
//     sum_{t = t0..t1} G_t = n G_{t0} + sum_{u = t0}^{t1 - 1} (t1 - u) (G_{u+1} - G_u),  n = t1 - t0 + 1
// One weighted Gram product per chain (k_dense_tile_shift, fsk_engine_dense_shift.hip) and four nibble lookups a cell and
// further shift (k_dense_shift_fix) in the count panels k_dense_count writes anyway. k_dense_edge_keys writes the two keys.
// Included by fsk_engine_dense_shift.hip only.
#pragma once
#include "fsk_common.h"

namespace fsk {

// the sequence (0..63) that sits at dword `p` of a panel row: inverse of panel_slot
__device__ __forceinline__ uint32_t panel_seq(uint32_t p) { return (p >> 2) + 16u * (p & 3u); }

// The edge keys of every (sequence, derived step): delta = the key of the first window under the step's lower combination,
// sigma = the key of the last window under its upper one, k_dense_count's key formula (ranks 0..sigma-1, the first kept position
// most significant; at most 256 keys on this path: a byte each). A sequence without a window gets 0 | 0, which contributes
// nothing. keys[step][panel][dword of the panel row] = delta | sigma << 8: the order of the count panels' rows.
// steps[2 s] = upper slot << 16 | lower slot. grid = (panels, ceil(n_steps / 4)), block = 256 (lane = sequence, wave = step).
__global__ __launch_bounds__(256) void k_dense_edge_keys(SeqView S, int g, int k, uint32_t sigma, const uint8_t* combo_pos, const uint32_t* steps,
                                                         uint32_t n_steps, uint32_t np_seq, uint16_t* keys) {
    const uint32_t r = threadIdx.x & 63u, step = blockIdx.y * 4u + (threadIdx.x >> 6), panel = blockIdx.x;
    if (step >= n_steps) return;
    const uint32_t seq = panel * PANEL + r;
    const uint32_t sl = steps[2u * step], up = sl >> 16, lo = sl & 0xffffu;
    uint32_t kd = 0, ks = 0;
    if (seq < S.n_seq) {
        const uint32_t len = S.len[seq], wbase = S.wstart[seq];
        if (len >= (uint32_t)g) {
            const uint32_t last = len - (uint32_t)g;
            for (int c = 0; c < k; ++c) {
                kd = kd * sigma + fetch_sym(S.words, wbase, (uint32_t)combo_pos[(size_t)lo * k + c], S.bits);
                ks = ks * sigma + fetch_sym(S.words, wbase, last + (uint32_t)combo_pos[(size_t)up * k + c], S.bits);
            }
        }
    }
    keys[(size_t)step * np_seq + panel * PANEL + panel_slot(r)] = (uint16_t)(kd | (ks << 8));
}

// K += sum over the derived steps of weight x (G_{u+1} - G_u), one workgroup a 128 x 128 tile (the tile kernel's XCD-aware
// table), 512 threads (eight waves of 2 x 16 + 2 x 16 sums a lane: 64 KB of LDS are two workgroups a CU, four waves a SIMD).
// Per step the whole panels (Vq8 <= 32 dword rows) of the tile's row side under the UPPER slot and of its column side under
// the LOWER slot are staged by the tile kernel's direct-to-LDS loads, double buffered: 2 x 32 KB.
//
// A lookup c_i(key_j) gathers dword row key_j >> 3 of sequence i. With the tile kernel's lane layout (a lane = 8 rows x 8
// columns) the 16 lanes of a row group would read 16 different rows of the same four banks. So here a LANE is a SEQUENCE and
// the key is WAVE-UNIFORM (v_readlane), which makes every lookup one conflict-free ds_read_b32 of a 256-byte panel row:
//   row term     c_{u+1,i}(sigma_j) - c_{u+1,i}(delta_j): lane = row i (dword `lane` of panels A0 and A1), wave w owns the 16
//                columns at dwords 16 w .. 16 w + 15 of the tile's 128, whose keys it broadcasts one by one   -> accR[2][16]
//   column term  c_{u,j}(sigma_i) - c_{u,j}(delta_i): lane = column j (panels B0, B1), wave w owns 16 rows  -> accC[2][16]
// Two 32-register int32 sums a lane; at the end accR crosses LDS (skewed by the row, conflict-free both ways) into accC's
// layout, whose flush — a lane a column — adds 512 contiguous bytes of K a wave instruction: one signed 64-bit atomic add per
// non-zero cell with j <= i < N (K is u64: two's-complement wrap-around makes the final sum exact).
//
// Counts above 15: where a (panel, slot) of the step has a flagged row mask, the step runs a second, workgroup-uniform pass
// with the hi planes staged over the buffer just used (an unflagged panel's hi plane is zero) and 16 x the weight. The host guarantees (2 maxW + 32) x sum of weights < 2^31.
//
// Every load the compiler can see (step table, keys, row masks) is issued one step ahead, BEFORE the direct-to-LDS loads of the
// next stage, and first used — through a v_mov the compiler cannot see through — right after the explicit wait that ends a
// step: a wait the compiler places for one of its own registers would otherwise wait for the whole next stage as well.
__global__ __launch_bounds__(512, 4) void k_dense_shift_fix(const uint32_t* C4, const uint32_t* C4H, const uint32_t* rowmask, const uint32_t* tile_tab,
                                                            const uint32_t* steps, uint32_t n_steps, const uint16_t* keys, uint32_t np_seq,
                                                            int n_slots, uint32_t Vq8, uint32_t N, u64* K) {
    constexpr int ROWS = 32;                  // dword rows a panel has at most on this path
    constexpr int HALF = ROWS * PANEL;        // dwords of one staged panel
    constexpr int PBUF = 4 * HALF;            // dwords per stage buffer: A0 A1 B0 B1
    constexpr int QW = 16;                    // columns (row term) and rows (column term) a wave owns
    __shared__ __attribute__((aligned(1024))) uint32_t P[2 * PBUF];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tile = tile_tab[blockIdx.x];
    const uint32_t ti = tile >> 16, tj = tile & 0xffffu;
    const size_t slot_stride = (size_t)Vq8 * PANEL;
    const size_t panel_stride = (size_t)n_slots * slot_stride;

    int accR[2][QW], accC[2][QW];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < QW; ++q) accR[h][q] = accC[h][q] = 0;

    const fsk_hw::lds_addr_t lds_wave = fsk_hw::lds_address(P) + w * 1024u;
    auto load_stage = [&](const uint32_t* plane, int buf, uint32_t sl) {
        const uint32_t up = sl >> 16, lo = sl & 0xffffu;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t panel = (q < 2 ? ti : tj) * 2u + (uint32_t)(q & 1);
            const uint32_t* src = plane + panel * panel_stride + (size_t)(q < 2 ? up : lo) * slot_stride;
            // (eight waves land 4 rows each: all 32 rows of the panel in one load; the rows past Vq8 read as zero)
            fsk_hw::panel_rows_to_lds(src, Vq8 * PANEL * 4u, lds_wave + (uint32_t)(buf * PBUF + q * HALF) * 4u, tid * 16u);
        }
    };
    // a step's keys of this lane's four sequences (A0 | A1 << 16, B0 | B1 << 16) and whether it has rows with counts above 15
    auto load_meta = [&](uint32_t s, uint32_t sl, uint32_t& kA, uint32_t& kB, uint32_t& fl) {
        const uint16_t* ks = keys + (size_t)s * np_seq;
        kA = (uint32_t)ks[ti * TILE + lane] | (uint32_t)ks[ti * TILE + PANEL + lane] << 16;
        kB = (uint32_t)ks[tj * TILE + lane] | (uint32_t)ks[tj * TILE + PANEL + lane] << 16;
        const uint32_t up = sl >> 16, lo = sl & 0xffffu;  // (Vq8 <= 32: one mask word a (panel, slot))
        const uint32_t mA = rowmask[(size_t)(ti * 2u) * n_slots + up] | rowmask[(size_t)(ti * 2u + 1u) * n_slots + up];
        const uint32_t mB = rowmask[(size_t)(tj * 2u) * n_slots + lo] | rowmask[(size_t)(tj * 2u + 1u) * n_slots + lo];
        fl = mA | mB;
    };
    // four lookups a (sequence of this lane, broadcast key pair kk = delta | sigma << 8) in the two panels at p0 and p0 + stride
    auto edge = [&](const uint32_t* p0, size_t stride, uint32_t kk, int mul, int& a0, int& a1) {
        const uint32_t kd = kk & 255u, ks = (kk >> 8) & 255u;
        const uint32_t* rd = p0 + (kd >> 3) * PANEL + lane;
        const uint32_t* rs = p0 + (ks >> 3) * PANEL + lane;
        const uint32_t shd = (kd & 7u) * 4u, shs = (ks & 7u) * 4u;
        a0 += ((int)((rs[0] >> shs) & 15u) - (int)((rd[0] >> shd) & 15u)) * mul;
        a1 += ((int)((rs[stride] >> shs) & 15u) - (int)((rd[stride] >> shd) & 15u)) * mul;
    };

    // the compiler-visible loads run one step ahead (step table: two)
    uint32_t sl_cur = steps[0], wt_cur = steps[1];
    uint32_t sl_nxt = n_steps > 1u ? steps[2] : 0u, wt_nxt = n_steps > 1u ? steps[3] : 0u;
    uint32_t kA_n, kB_n, fl_n;
    load_meta(0u, sl_cur, kA_n, kB_n, fl_n);
    uint32_t sl_n2 = 0u, wt_n2 = 0u;
    int buf = 0;
    load_stage(C4, 0, (uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(sl_cur)));
    fsk_hw::wait_panel_rows();
    __syncthreads();
    const uint32_t lsel = (w & 3u) * (uint32_t)QW, hsh = (w >> 2) * 16u;
    for (uint32_t s = 0; s < n_steps; ++s) {
        const uint32_t kA = fsk_hw::vgpr_copy(kA_n), kB = fsk_hw::vgpr_copy(kB_n);
        const uint32_t fl = (uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(fl_n));
        const uint32_t sl = (uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(sl_cur));
        const int wt = (int)((uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(wt_cur)) & 255u);
        if (s + 1u < n_steps) {
            const uint32_t sn = (uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(sl_nxt));
            if (s + 2u < n_steps) {
                sl_n2 = steps[2u * (s + 2u)];
                wt_n2 = steps[2u * (s + 2u) + 1u];
            }
            load_meta(s + 1u, sn, kA_n, kB_n, fl_n);
            load_stage(C4, buf ^ 1, sn);  // in flight under the lookups
        }
        const uint32_t* pb = P + buf * PBUF;
        auto lookups = [&](int mul) {
#pragma unroll
            for (int q = 0; q < QW; ++q) {  // row term: the keys of this wave's 16 columns
                const uint32_t kk = (fsk_hw::readlane(kB, lsel + (uint32_t)q) >> hsh) & 0xffffu;
                edge(pb, (size_t)HALF, kk, mul, accR[0][q], accR[1][q]);
                if ((q & 3) == 3) asm volatile("" ::: "memory");  // (eight lookups in flight, not all of them: registers)
            }
#pragma unroll
            for (int q = 0; q < QW; ++q) {  // column term: the keys of this wave's 16 rows
                const uint32_t kk = (fsk_hw::readlane(kA, lsel + (uint32_t)q) >> hsh) & 0xffffu;
                edge(pb + 2 * HALF, (size_t)HALF, kk, mul, accC[0][q], accC[1][q]);
                if ((q & 3) == 3) asm volatile("" ::: "memory");
            }
        };
        lookups(wt);
        if (fl != 0u) {  // the hi planes over the buffer just used, at 16 x the weight
            __syncthreads();  // everyone is done with the lo planes
            load_stage(C4H, buf, sl);
            fsk_hw::wait_panel_rows();
            __syncthreads();
            lookups(16 * wt);
        }
        fsk_hw::wait_panel_rows();  // this wave's part of the next stage has landed (and every load of this trip)
        __syncthreads();            // ... everyone's has, and everyone is done with the current buffer
        sl_cur = sl_nxt; wt_cur = wt_nxt;
        sl_nxt = sl_n2; wt_nxt = wt_n2;
        buf ^= 1;
    }
    // accR -> LDS as tile[row dword][(column dword + row dword) mod 128] -> added in accC's layout
    int* const T = reinterpret_cast<int*>(P);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            const uint32_t i = (uint32_t)h * PANEL + lane, j = w * (uint32_t)QW + (uint32_t)q;
            T[i * TILE + ((j + i) & (TILE - 1u))] = accR[h][q];
        }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t jd = (uint32_t)h * PANEL + lane;
        const u64 j = (u64)tj * TILE + (uint32_t)h * PANEL + panel_seq(lane);
#pragma unroll
        for (int q = 0; q < QW; ++q) {
            const uint32_t id = w * (uint32_t)QW + (uint32_t)q;
            const u64 i = (u64)ti * TILE + (id >> 6) * PANEL + panel_seq(id & 63u);
            const int v = accC[h][q] + T[id * TILE + ((jd + id) & (TILE - 1u))];
            if (i < N && j <= i && v != 0) atomicAdd(&K[tri_index(i, j)], (u64)(long long)v);
        }
    }
}

}  // namespace fsk
