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
//
// The corrections have two forms. k_dense_shift_fix reads the count panels as k_dense_count wrote them (a dword = 8 keys of one
// sequence): one nibble a 32-bit LDS read. k_dense_shift_packed (the default, tuning dense_shift_packed) reads KEY-MAJOR planes
// (k_dense_keymajor: a dword = one key of 8 sequences): eight cells a read, summed with byte-parallel arithmetic.
#pragma once
#include "fsk_bytesel.h"
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

// ---- key-major planes and the packed corrections ------------------------------------------------------------------------
// A key-major plane holds, per (tile side = panel pair, slot), [key][16 dwords]: dword t of a key is the 4-bit counts of the 8
// sequences tile_index(t, 0..7) of the tile side (nibble n = tile_index(t, n): the 8 rows, or columns, of the tile kernel's lane
// group t), so a lane that owns an 8 x 8 block of cells gets a key's counts of its 8 rows or columns in ONE dword. Inside a
// key's 64 bytes dword t sits at t ^ km_swizzle(key): the lookups of a wave go to per-lane keys, and without the swizzle two
// keys of equal parity would meet in the same banks whatever the lane groups are.
__device__ __forceinline__ uint32_t km_swizzle(uint32_t key) { return ((key >> 1) & 3u) << 2; }
// byte offset of dword t of `key` inside a staged plane = km_offset(key) ^ 4 t
__device__ __forceinline__ uint32_t km_offset(uint32_t key) { return key << 6 | km_swizzle(key) << 2; }

// Panels -> key-major: thread = (panel pair, slot, dword row of 8 keys, lane group t). The four dwords a lane group owns in a
// panel row are adjacent (panel_slot), so a thread reads 16 bytes of each of the pair's panels and writes the 8 x 8 nibble
// transpose: 8 dwords, one a key. grid = ceil(pairs * slots * Vq8 * 16 / 256), block = 256. `plane` = the lo or the hi plane.
__global__ __launch_bounds__(256) void k_dense_keymajor(const uint32_t* plane, uint32_t n_pairs, int n_slots, uint32_t Vq8, uint32_t* KM) {
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t t = (uint32_t)id & 15u;
    size_t rest = id >> 4;
    const uint32_t row = (uint32_t)(rest % Vq8);
    rest /= Vq8;
    const uint32_t slot = (uint32_t)(rest % (uint32_t)n_slots);
    const size_t pair = rest / (uint32_t)n_slots;
    if (pair >= n_pairs) return;
    const size_t slot_stride = (size_t)Vq8 * PANEL, panel_stride = (size_t)n_slots * slot_stride;
    const uint32_t* src = plane + 2u * pair * panel_stride + slot * slot_stride + (size_t)row * PANEL + 4u * t;
    const uint4 a = *reinterpret_cast<const uint4*>(src), b = *reinterpret_cast<const uint4*>(src + panel_stride);
    const uint32_t in[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};  // sequence tile_index(t, n), keys 8 row .. 8 row + 7
    uint32_t* out = KM + (pair * (size_t)n_slots + slot) * ((size_t)Vq8 * 128u);
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t n = 0; n < 8u; ++n) v |= ((in[n] >> (4u * q)) & 15u) << (4u * n);
        const uint32_t key = row * 8u + q;
        out[key * 16u + (t ^ km_swizzle(key))] = v;
    }
}

// The edge keys as the packed kernel wants them: offs[q] = km_offset(delta) | km_offset(sigma) << 16 of keys[q] (14 bits each).
__global__ __launch_bounds__(256) void k_dense_edge_offs(const uint16_t* keys, size_t n, uint32_t* offs) {
    const size_t q = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const uint32_t kk = keys[q];
    offs[q] = km_offset(kk & 255u) | km_offset(kk >> 8) << 16;
}

// k_dense_shift_fix's work — same tile table, same masks, same store-then-add contract, same step table — from key-major
// planes: one workgroup a 128 x 128 tile, 256 threads, a lane = the tile kernel's 8 x 8 block of cells (row group tr, column
// group tc; register (er, ec) = cell (tile_index(tr, er), tile_index(tc, ec))), 64 int32 sums. Per step the key-major plane of
// the tile's row side under the UPPER slot (A) and of its column side under the LOWER slot (B) are staged by direct-to-LDS
// loads, double buffered: 2 x 32 KB, two workgroups a CU.
//   row term     c_{u+1,i}(sigma_j) - c_{u+1,i}(delta_j) for the lane's column ec: dwords tr of A[sigma_j], A[delta_j]: 8 rows
//   column term  c_{u,j}(sigma_i) - c_{u,j}(delta_i) for the lane's row er: dwords tc of B[sigma_i], B[delta_i]: 8 columns
// Keys are per lane. A wave is 8 row groups x 8 column groups, a 32-lane LDS service group 4 x 8: four (eight) keys of 8 (4)
// adjacent dwords, which km_swizzle spreads over the banks by the keys' low three bits.
//
// Two waves a SIMD (a form of 512 threads with 8 x 4 cells a lane and four waves a SIMD was built and measured: more waves, more
// instructions a cell, slower: profiles/dense_shift_waves_ab.txt). A wave of this kernel is parked at a wait or the barrier for a
// third of its cycles, so the step is written for few stops and few instructions:
//   - the 32 lookups stay in flight: the 16 of the row term are issued before anything is used, the column term's 16 while the
//     row term is worked on, and each group of 8 is waited for once, with a count (fsk_hw::first_use): 4 waits a step;
//   - the step table and the row masks of the NEXT step are loaded behind the step's last lookup (they are uniform; a scalar
//     load in flight shares the LDS reads' counter, returns out of order and turns every wait for an LDS read into a drain);
//   - ~d & m is one three-input bit operation and R + (s & m) + (~d & m) one v_add3_u32 (the mask lives in a register: the
//     instructions take no literal), and the two offsets of a key pair leave their dword, with the lane's term and the stage's
//     base, by one fsk_hw::xor_word each;
//   - a byte leaves for its int32 sum once a BATCH of steps, not once a step (below).
//
// Byte-parallel sums (m = 0x0f0f0f0f): (s & m) + (~d & m) holds four differences + 15, each in [0, 30], no borrow between bytes;
// the odd nibbles the same after >> 4. Weights are prefix sums, not multiplies: inside a chain
// sum_u (t1 - u) D_u = sum_r R_r with R_r = sum_{u <= r} D_u, and R stays packed in bytes (R += D': the R of step r of a chain
// lies in [0, 30 (r + 1)] — a byte for the 8 steps dense_shift_plan cuts chains to). R restarts where a step's lower slot is a
// chain base. The sum over r stays in bytes as well: Q += R every step (two adds a lookup pair), and only where the step's weight
// word carries bit 8 — "unpack after this step", one scalar branch a step — every byte of Q is added to its int32 sum
// (fsk_hw::add_byte, 128 a lane) and Q starts again. The host sets the flag by the bound (dense_shift_unpack_flags: 30 (r + 1) a
// step against a byte's 255, on the step before the one that would pass it and on the last step); Q does not restart at a chain
// base, so a batch may span chains: 125 unpacks for the 330 steps of the headline plan. Tuning dense_shift_batch = 0 flags every
// step. The bias, 15 (r + 1) a term and step, is 30 x the sum of the launch's weights a cell (`bias`), taken off at the flush.
//
// Counts above 15: a step runs a second, workgroup-uniform pass when the row mask of EITHER side is set, and that pass reads the
// key-major HI planes of BOTH sides, staged over the buffer just used, nibble by nibble at 16 x the step's weight (exact, and
// rare). The unflagged side contributes nothing: k_dense_count writes every hi plane, an unflagged panel's as zeros, and
// k_dense_keymajor transposes the hi plane unconditionally, so its key-major form is zero too. The key offsets are loaded one step
// ahead, as in k_dense_shift_fix. The flush adds, per wave instruction, 8 runs of 8 adjacent cells of K.
//
// INPLACE (tuning dense_shift_inplace, the default): where step s + 1 continues the chain of step s and neither step is flagged,
// its planes are not staged but MADE in LDS from the ones step s looked up, by the identity at the head of this file:
//   A holds c_up(s)  and becomes c_up(s + 1) = c_up(s) + e(sigma) - e(delta) with the keys of step s + 1 of the tile's 128 rows,
//   B holds c_lo(s)  and becomes c_lo(s + 1) = c_up(s) = c_lo(s) + e(sigma) - e(delta) with the keys of step s of its 128 columns.
// Thread q < 128 owns row-side position q, thread 128 + q column-side position q: one dword of `offs`, and two atomic adds of
// 1 << 4 e (the second negated) on LDS dwords off ^ 4 t, for position p = 64 h + 4 t + x = nibble e = 4 h + x of dword t — up to 8
// positions share a dword. A position whose two offsets are equal adds nothing (sigma = delta; a padded row or a sequence without
// a window: 0 | 0, whose zero plane stays zero). A nibble never leaves [0, 15]: both steps are unflagged, so every count of the four
// planes is below 16. A barrier ends the lookups, the next ends the updates. A chain's first step, a flagged step and the step
// behind a flagged one (whose buffer the hi planes took) are staged as before; the planes in memory are never written. The step
// table runs three steps ahead and the masks two, so that a step knows at its head whether the next one is flagged.
//
// AHEAD (tuning dense_shift_ahead, the default; a schedule of the in-place form): vmcnt retires in order, so a stage stays in
// flight only as long as NO younger vector load is waited for — and above every step loads its offsets, its table words and its
// masks, and ends in vmcnt(0). Here a step inside a chain issues no vector memory load at all, and the chain's first step stages
// the NEXT chain's start under the whole chain. The host hands over a chain table in place of the step table (`steps`; its
// length in `n_bases`: fsk_engine_dense_shift.hip, dense_shift_chain_table), two words a chain, from which every step's slot
// word, weight, unpack flag and masks follow; 64 descriptors sit in a VGPR pair, one chain a lane, and are read with v_readlane.
// LDS: the two 32 KB stage buffers and, behind them, a ring of two 8 KB halves of key offsets (8 steps x 256 positions): 80 KB,
// two workgroups a CU. At a chain's first step, in this order: the next chain's row masks (one word a lane, lane 4 r + x), then
// its first planes into the buffer the chain does not use (it is made in place in the other), then the offsets of all its steps
// into the ring half the chain does not read — wave w lands the 1 KB of steps w and w + 4. Inside the chain the lane's 16 offsets
// are four ds_read_b128 of the chain's ring half (eight lanes share an address) and the update's offset one ds_read_b32, one
// step ahead as before; the first offsets of a chain are read behind its predecessor's last barrier.
//
// What orders the prefetch (D = any LDS location a direct-to-LDS load of the prefetch writes: the idle buffer, the idle ring half):
//   - the overwrite of D after its last read: D was last read by the lookups (the buffer), the offset reads and the update's read
//     (the ring half) of the PREVIOUS chain, all in front of that chain's closing __syncthreads(); the loads are issued behind it.
//   - every read of D after the load: the chain's LAST step ends in fsk_hw::wait_panel_rows() — vmcnt(0): this wave's loads have
//     landed, with the mask words, which are older — and __syncthreads(): every wave's have. The next chain's first lookups, its
//     first ring reads and the ballot over the masks all follow that barrier. A chain of one step has its first step for its last:
//     the prefetch has one step of cover, as every stage had before.
//   - the barriers in between — the end of a step that is not the chain's last, and the one behind the in-place update — are
//     fsk_hw::barrier_lds_only(): lgkmcnt(0) and s_barrier, no fence. They order the lookups, the ds_add updates and the ring reads
//     of the CURRENT buffer and ring half, which no load in flight writes; __syncthreads() there would drain vmcnt and with it
//     the prefetch.
//   - a flagged step: the hi pass stages over the buffer just used and the step behind it is staged into the OTHER buffer, over
//     the prefetch, as before (`lost`: nothing is prefetched when the chain's second step is staged already). A wave waits for
//     its own part of the prefetch (vmcnt(0)) before it issues the replacement — the same wave writes the same 1 KB pieces, so
//     the replacement lands last — and that step, like every staged step, ends in vmcnt(0) + __syncthreads(). While `lost` is set
//     the chain's last step stages the next chain's start at its head, under its lookups: the schedule above. The ring is not
//     touched by any of this and is always prefetched.
// Every compiler-visible load (descriptors at every 64th chain, masks once a chain) is issued in front of the prefetch and first
// used, through a v_mov the compiler cannot see through, behind the chain's closing wait.
//
// STRAIGHT (tuning dense_shift_straight, the default; a form of the ahead schedule's loop): the loop runs over CHAINS, and what a
// chain needs is decided once, at its head, from the ballot over its masks. A chain none of whose steps meets a count above 15 on
// either side of the tile — all but about 2 % of the (tile, chain) pairs of random DNA — is: the prefetch; then per step the ring
// reads of the next step, the lookups, the unpack on bit 0 of the chain's unpack bits; between steps barrier_lds_only, the two
// ds_add, barrier_lds_only; the closing wait. It carries the steps left, the ring position and the unpack bits, and neither slot
// words nor a weight nor flags nor the first / middle / last ladder of the step loop. Any other chain runs that loop's body step by
// step around the SAME lookup block (one in the kernel: a form with the clean chains in a loop of their own beside the step loop
// held two and spilled 157 VGPRs). In this loop the next step's offsets are read from the ring INTO the registers of this step's,
// right behind the step's last lookup is issued (behind the hi pass where a step has one, which looks up again): the step loop's
// second set of 16 offset registers and its 16 v_mov a step are gone, and the read is a barrier pair ahead of its first use.
// What orders the prefetch across clean -> flagged -> clean:
//   - both kinds issue it at the chain's head, behind the previous chain's closing __syncthreads(), into the buffer and the ring
//     half that chain read last; both end in wait_panel_rows() + __syncthreads() and read what it landed behind them. Inside a
//     clean chain no barrier drains vmcnt and nothing is staged, so the first two points above hold as they stand.
//   - a flagged chain may stage over the prefetched buffer; `lost` is that chain's own — cleared at every chain's head — and under
//     it the chain's last step stages the next start before the same closing wait. Whichever way they came, `buf` holds a chain's
//     first planes at its head, which is all the next chain, clean or not, relies on. The ring half is never staged over.
//   - a chain whose first step is flagged stages its second step at the head, in the prefetch's place, behind a wait for the
//     ring loads just issued (the step loop skips that wait at a first step; here the step inside the chain is not kept).
template <bool INPLACE, bool AHEAD = false, bool STRAIGHT = false>
__global__ __launch_bounds__(256, 2) void k_dense_shift_packed(const uint32_t* KM, const uint32_t* KMH, const uint32_t* rowmask, const uint32_t* tile_tab,
                                                               const uint32_t* steps, uint32_t n_steps, const uint32_t* offs, uint32_t np_seq,
                                                               int n_slots, uint32_t Vq8, uint32_t n_bases, uint32_t bias, uint32_t N, u64* K) {
    static_assert(INPLACE || !AHEAD, "the ahead schedule is a schedule of the in-place form");
    static_assert(AHEAD || !STRAIGHT, "the straight chains are a form of the ahead schedule's loop");
    constexpr uint32_t SIDE = 256u * 16u;  // dwords of one staged plane (256 keys at most on this path)
    constexpr uint32_t PBUF = 2u * SIDE;   // dwords per stage buffer: A B
    constexpr uint32_t RING = 8u * 256u;   // (ahead) dwords of one half of the offsets ring: 8 steps x 256 positions
    // (ahead: the two stage buffers and the two ring halves, 80 KB of static LDS; gfx950 has 160 KB a CU)
    __shared__ __attribute__((aligned(1024))) uint32_t P[AHEAD ? 2 * PBUF + 2 * RING : 2 * PBUF];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    // (the two masks in registers the compiler cannot see through, one of them scalar: see above)
    const uint32_t M4 = (uint32_t)__builtin_amdgcn_readfirstlane(fsk_hw::vgpr_copy(0x0f0f0f0fu));
    const uint32_t tr = (w >> 1) * 8u + (lane >> 3), tc = (w & 1u) * 8u + (lane & 7u);
    const uint32_t tile = tile_tab[blockIdx.x];
    const uint32_t ti = tile >> 16, tj = tile & 0xffffu;
    const size_t slot_stride = (size_t)Vq8 * 128u;
    const size_t pair_stride = (size_t)n_slots * slot_stride;
    const uint32_t side_bytes = Vq8 * 512u;

    // acc[er][ec]; R, Q[even / odd nibbles][ec (row term) or er (column term)]: the prefix sums, and their byte sums over a batch
    uint32_t acc[8][8], Rr[2][8], Rc[2][8], Qr[2][8], Qc[2][8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0u;
        Rr[0][a] = Rr[1][a] = Rc[0][a] = Rc[1][a] = 0u;
        Qr[0][a] = Qr[1][a] = Qc[0][a] = Qc[1][a] = 0u;
    }

    const fsk_hw::lds_addr_t lds_wave = fsk_hw::lds_address(P) + w * 1024u;
    auto load_stage = [&](const uint32_t* plane, uint32_t buf, uint32_t sl) {
        const uint32_t up = sl >> 16, lo = sl & 0xffffu;
#pragma unroll
        for (uint32_t side = 0; side < 2u; ++side) {
            const uint32_t* src = plane + (side == 0u ? ti : tj) * pair_stride + (size_t)(side == 0u ? up : lo) * slot_stride;
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)  // (four waves land 1 KB each: 64 keys a load; the keys past 8 Vq8 are never looked up)
                if (q * 4096u < side_bytes)
                    fsk_hw::panel_rows_to_lds(src, side_bytes, lds_wave + (buf * PBUF + side * SIDE + q * 1024u) * 4u, q * 4096u + tid * 16u);
        }
    };
    // a step's key offsets of this lane's 8 rows (oR) and 8 columns (oC)
    auto load_offs = [&](uint32_t s, uint4 (&oR)[2], uint4 (&oC)[2]) {
        const uint32_t* os = offs + (size_t)s * np_seq;
#pragma unroll
        for (uint32_t h = 0; h < 2u; ++h) {
            oR[h] = *reinterpret_cast<const uint4*>(os + ti * TILE + h * PANEL + 4u * tr);
            oC[h] = *reinterpret_cast<const uint4*>(os + tj * TILE + h * PANEL + 4u * tc);
        }
    };
    // whether a step has rows with counts above 15 on either side
    auto flagged = [&](uint32_t sl) {
        const uint32_t up = sl >> 16, lo = sl & 0xffffu;  // (Vq8 <= 32: one mask word a (panel, slot))
        const uint32_t mA = rowmask[(size_t)(ti * 2u) * n_slots + up] | rowmask[(size_t)(ti * 2u + 1u) * n_slots + up];
        const uint32_t mB = rowmask[(size_t)(tj * 2u) * n_slots + lo] | rowmask[(size_t)(tj * 2u + 1u) * n_slots + lo];
        return mA | mB;
    };
    auto lds_at = [&](uint32_t byte_off) { return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(P) + byte_off); };

    // (the step table runs two steps ahead and the masks one, both loaded at the END of a step and landed by its barrier)
    // (wt is the whole weight word: bits 0..7 the weight, bit 8 "unpack after this step")
    uint32_t sl, wt, fl, sn = 0u, wn = 0u;
    uint32_t s2 = 0u, w2 = 0u, fl_nx = 0u;  // (in place: the table entry of step s + 2 and the masks of step s + 1, at the head of step s)
    uint4 oR_n[2], oC_n[2];
    uint32_t buf = 0;
    // ---- the ahead schedule's state and loads (see the head comment). `steps` is the CHAIN table here and n_bases the number of
    // its chains: chain c has the descriptor (the first step's slot word, steps | first weight << 8 | unpack flags << 16), its
    // step r the slots (up0 + r) << 16 | (up0 + r - 1) and the weight wt0 - r (the host checks that the step table says so). A
    // step's words are kept by increments — a shift, an add — because the kernel is bound by what it issues.
    [[maybe_unused]] uint32_t* const ring = P + 2u * PBUF;
    [[maybe_unused]] uint32_t cb = 0u, dv0 = 0u, dv1 = 0u;    // the descriptors of chains cb .. cb + 63, one a lane
    [[maybe_unused]] uint32_t c = 0u, r = 0u, rem = 0u;       // the chain, the step inside it, the steps it still has (this one included)
    [[maybe_unused]] uint32_t n0 = 0u, n1 = 0u, mk_n = 0u;    // the next chain's descriptor and row masks (lane 4 r + x: step r, A0 A1 B0 B1)
    [[maybe_unused]] uint32_t flw = 0u, wu = 0u, slq = 0u;    // nibble q: step r + q is flagged; bit q: step r + q unpacks; the slot word of step r + 1
    [[maybe_unused]] uint32_t half = 0u, rg = 0u;             // the chain's ring half, the dword of this step's offsets in the ring
    [[maybe_unused]] bool lost = false;                       // the other buffer does not (or will not) hold the next chain's first planes
    // chain (e0, e1) becomes the current one: its first step's words
    [[maybe_unused]] auto enter_chain = [&](uint32_t e0, uint32_t e1, uint32_t mk) {
        flw = (uint32_t)__ballot(fsk_hw::vgpr_copy(mk) != 0u);
        sl = e0;
        slq = ((e0 >> 16) + 1u) << 16 | (e0 >> 16);
        rem = e1 & 15u;
        wt = (e1 >> 8) & 255u;
        wu = e1 >> 16;
        r = 0u;
        rg = half * RING;
    };
    [[maybe_unused]] auto load_desc = [&]() {
        const uint32_t q = cb + lane < n_bases ? cb + lane : n_bases - 1u;
        dv0 = steps[2u * q];
        dv1 = steps[2u * q + 1u];
    };
    [[maybe_unused]] auto load_masks = [&](uint32_t e0, uint32_t e1) {
        const uint32_t mr = lane >> 2, x = lane & 3u, up0 = e0 >> 16;
        uint32_t m = 0u;
        if (mr < (e1 & 15u)) {
            const uint32_t slot = x < 2u ? up0 + mr : (mr == 0u ? (e0 & 0xffffu) : up0 + mr - 1u);
            m = rowmask[(size_t)((x < 2u ? ti : tj) * 2u + (x & 1u)) * n_slots + slot];
        }
        return m;
    };
    // a chain's key offsets into a ring half: wave w lands the 1 KB of steps w and w + 4 (the row side's 128 positions, then the
    // column side's)
    [[maybe_unused]] auto load_ring = [&](uint32_t hf, uint32_t s_first, uint32_t n) {
        const uint32_t ring_lane = lane < 32u ? (ti * TILE + 4u * lane) * 4u : (tj * TILE + 4u * (lane - 32u)) * 4u;
#pragma unroll
        for (uint32_t q = 0; q < 2u; ++q) {
            const uint32_t rr = w + 4u * q;
            if (rr < n)
                fsk_hw::panel_rows_to_lds(offs + (size_t)(s_first + rr) * np_seq, np_seq * 4u, fsk_hw::lds_address(ring) + (hf * RING + rr * 256u) * 4u,
                                          ring_lane);
        }
    };
    // a step's offsets of this lane's 8 rows and 8 columns from the ring, `at` = the step's dword there (eight lanes share an address)
    [[maybe_unused]] auto ring_offs = [&](uint32_t at, uint4 (&oR)[2], uint4 (&oC)[2]) {
        const uint32_t* q = ring + at;
#pragma unroll
        for (uint32_t hh = 0; hh < 2u; ++hh) {
            oR[hh] = *reinterpret_cast<const uint4*>(q + hh * PANEL + 4u * tr);
            oC[hh] = *reinterpret_cast<const uint4*>(q + TILE + hh * PANEL + 4u * tc);
        }
    };
    if constexpr (AHEAD) {
        load_desc();
        const uint32_t d0 = fsk_hw::readlane(dv0, 0u), d1 = fsk_hw::readlane(dv1, 0u);
        const uint32_t mk = load_masks(d0, d1);
        load_stage(KM, 0u, d0);
        load_ring(0u, 0u, d1 & 15u);
        fsk_hw::wait_panel_rows();
        __syncthreads();
        fl = 0u;
        enter_chain(d0, d1, mk);
        ring_offs(0u, oR_n, oC_n);
    } else {
        sl = steps[0]; wt = steps[1]; fl = flagged(sl);
        sn = n_steps > 1u ? steps[2] : 0u; wn = n_steps > 1u ? steps[3] : 0u;
        if constexpr (INPLACE) {
            if (n_steps > 2u) { s2 = steps[4]; w2 = steps[5]; }
            if (n_steps > 1u) fl_nx = flagged(sn);
        }
        load_offs(0u, oR_n, oC_n);
        load_stage(KM, 0u, sl);
        fsk_hw::wait_panel_rows();
        __syncthreads();
    }
    if constexpr (STRAIGHT) {
        // The loop over CHAINS. At a chain's head — enter_chain done, the first offsets read, `buf` holding its first planes
        // whichever way they came — the chain is clean (flw == 0: no step of it meets a count above 15 on either side of this
        // tile; 98 % of the (tile, chain) pairs of random DNA) or it is not, and that is decided once:
        //   head   the next chain's descriptor, masks, first planes and ring half, in the order above (the step loop's
        //          `first && has_next` block; in a clean chain `last || same` is known);
        //   body   a clean chain: the lookups with the ring reads of the next step behind the last of them, the unpack on bit 0 of wu, and
        //          between steps barrier_lds_only - the two ds_add - barrier_lds_only. It carries rem, rg and wu and nothing else: no slot
        //          words, no weight (the weights are prefix sums), no flags, no first / middle / last ladder;
        //          any other chain: the step loop's body below, step by step, in what it does (a staged step, the hi pass, `lost`,
        //          the late stage of the next start), around the same lookup block;
        //   tail   wait_panel_rows() + __syncthreads(), the buffer and the ring half change, the next chain is entered.
        // Both kinds issue the prefetch behind the previous chain's closing barrier and first read what it landed behind their
        // own closing wait and barrier, so the ordering argument above holds across clean -> flagged -> clean as it stands:
        // a clean chain leaves `buf ^ 1` and `half ^ 1` prefetched, a flagged one leaves `buf ^ 1` staged by its last step where
        // the prefetch was lost, and neither reads `lost` of the other: it is cleared at every chain's head.
        uint32_t s = 0u;  // the first step of the NEXT chain, from the chain's head on
        uint32_t xA = tr * 4u, xB = (tc * 4u) | (SIDE * 4u);  // (buf = 0; a staged plane's base is a multiple of 16 KB and a key offset has 14 bits)
        uint32_t oR[8], oC[8], dA[8], sA[8], dB[8], sB[8];
        auto read_A = [&](int e) { dA[e] = lds_at(fsk_hw::xor_word<0>(oC[e], xA)); sA[e] = lds_at(fsk_hw::xor_word<1>(oC[e], xA)); };
        auto read_B = [&](int e) { dB[e] = lds_at(fsk_hw::xor_word<0>(oR[e], xB)); sB[e] = lds_at(fsk_hw::xor_word<1>(oR[e], xB)); };
        auto row_term = [&](int e) {
            Rr[0][e] += (sA[e] & M4) + (~dA[e] & M4);
            Rr[1][e] += ((sA[e] >> 4) & M4) + (~(dA[e] >> 4) & M4);
            Qr[0][e] += Rr[0][e];
            Qr[1][e] += Rr[1][e];
        };
        auto col_term = [&](int e) {
            Rc[0][e] += (sB[e] & M4) + (~dB[e] & M4);
            Rc[1][e] += ((sB[e] >> 4) & M4) + (~(dB[e] >> 4) & M4);
            Qc[0][e] += Rc[0][e];
            Qc[1][e] += Rc[1][e];
        };
        // load_masks by arithmetic on lane constants (the slot of lane 4 r + x is up0 + r for A, up0 + r - 1 for B and the chain's
        // base slot for B at r = 0): written with selects, the lane conditions are hoisted in front of the loop as wave masks, two
        // SGPRs each, and the loop spills one
        const uint32_t mk_r = lane >> 2, mk_x = lane & 3u;
        const size_t mk_row = (size_t)((mk_x < 2u ? ti : tj) * 2u + (mk_x & 1u)) * n_slots;
        const uint32_t mk_add = mk_r - (mk_x >> 1), mk_base = fsk_hw::vgpr_copy(mk_x >= 2u && mk_r == 0u ? 1u : 0u);
        auto next_masks = [&](uint32_t e0, uint32_t e1) {
            const uint32_t up0 = e0 >> 16, slot = up0 + mk_add + mk_base * ((e0 & 0xffffu) + 1u - up0);
            uint32_t m = 0u;
            if (mk_r < (e1 & 15u)) m = rowmask[mk_row + slot];
            return m;
        };
        // a step's offsets from the ring into oR / oC (ring_offs without the registers of a step ahead)
        auto next_offs = [&](uint32_t at) {
            const uint32_t* q = ring + at;
#pragma unroll
            for (uint32_t hh = 0; hh < 2u; ++hh) {
                const uint4 a = *reinterpret_cast<const uint4*>(q + hh * PANEL + 4u * tr), b = *reinterpret_cast<const uint4*>(q + TILE + hh * PANEL + 4u * tc);
                oR[4 * hh] = a.x; oR[4 * hh + 1] = a.y; oR[4 * hh + 2] = a.z; oR[4 * hh + 3] = a.w;
                oC[4 * hh] = b.x; oC[4 * hh + 1] = b.y; oC[4 * hh + 2] = b.z; oC[4 * hh + 3] = b.w;
            }
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // (the first chain's first offsets were read above)
            oR[4 * h] = oR_n[h].x; oR[4 * h + 1] = oR_n[h].y; oR[4 * h + 2] = oR_n[h].z; oR[4 * h + 3] = oR_n[h].w;
            oC[4 * h] = oC_n[h].x; oC[4 * h + 1] = oC_n[h].y; oC[4 * h + 2] = oC_n[h].z; oC[4 * h + 3] = oC_n[h].w;
        }
        while (c < n_bases) {
            const uint32_t gen = flw;  // != 0: some step of the chain meets a count above 15 in this tile
            lost = false;
            if (c + 1u < n_bases) {
                if (c + 1u - cb >= 64u) {
                    cb = c;
                    load_desc();
                }
                n0 = fsk_hw::readlane(dv0, c + 1u - cb);
                n1 = fsk_hw::readlane(dv1, c + 1u - cb);
                mk_n = next_masks(n0, n1);
                s += rem;  // the next chain's first step
                if (rem == 1u || (flw & 255u) == 0u) load_stage(KM, buf ^ 1u, n0);
                else lost = true;  // (step 1 is about to be staged there)
                load_ring(half ^ 1u, s, n1 & 15u);
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) Rr[0][a] = Rr[1][a] = Rc[0][a] = Rc[1][a] = 0u;
            for (;;) {
                const bool last = rem == 1u;
                bool in_place = true;  // the next step's planes are made from this step's
                uint32_t uo_n = 0u;
                bool hi = false;  // the step meets a count above 15: the hi pass
                if (gen == 0u) {
                    if (!last) uo_n = ring[rg + (w < 2u ? 256u : (uint32_t)TILE) + (tid & 127u)];
                } else {
                    hi = (flw & 15u) != 0u;
                    in_place = (flw & 255u) == 0u;
                    if (!last) {
                        if (in_place) {
                            uo_n = ring[rg + (w < 2u ? 256u : (uint32_t)TILE) + (tid & 127u)];
                        } else {  // a flagged step, or the step behind one: staged, over the prefetch
                            lost = true;
                            fsk_hw::wait_panel_rows();  // (this wave's part of the prefetch has landed before its replacement is issued)
                            load_stage(KM, buf ^ 1u, ((sl >> 16) + 1u) << 16 | (sl >> 16));  // (the slot word of step r + 1)
                        }
                    } else if (lost && c + 1u < n_bases) {
                        load_stage(KM, buf ^ 1u, n0);  // the prefetch was lost: the next chain's start the old way, under this step's lookups
                    }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) read_A(e);
                fsk_hw::first_use(dA[0], sA[0], dA[1], sA[1], dA[2], sA[2], dA[3], sA[3]);
#pragma unroll
                for (int e = 0; e < 4; ++e) read_B(e);
#pragma unroll
                for (int e = 0; e < 4; ++e) row_term(e);
                fsk_hw::first_use(dA[4], sA[4], dA[5], sA[5], dA[6], sA[6], dA[7], sA[7]);
#pragma unroll
                for (int e = 4; e < 8; ++e) read_B(e);
                // the step's last lookup is issued: the next step's offsets land in the registers this step's leave (no copy a step;
                // a step with a hi pass looks up once more and reads them behind it)
                if (!last && !hi) next_offs(rg + 256u);
#pragma unroll
                for (int e = 4; e < 8; ++e) row_term(e);
                fsk_hw::first_use(dB[0], sB[0], dB[1], sB[1], dB[2], sB[2], dB[3], sB[3]);
#pragma unroll
                for (int e = 0; e < 4; ++e) col_term(e);
                fsk_hw::first_use(dB[4], sB[4], dB[5], sB[5], dB[6], sB[6], dB[7], sB[7]);
#pragma unroll
                for (int e = 4; e < 8; ++e) col_term(e);
                if ((wu & 1u) != 0u) {  // the batch ends behind this step: every byte of Q joins its int32 sum, and Q starts again
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        acc[0][e] = fsk_hw::add_byte<0>(acc[0][e], Qr[0][e]); acc[1][e] = fsk_hw::add_byte<0>(acc[1][e], Qr[1][e]);
                        acc[2][e] = fsk_hw::add_byte<1>(acc[2][e], Qr[0][e]); acc[3][e] = fsk_hw::add_byte<1>(acc[3][e], Qr[1][e]);
                        acc[4][e] = fsk_hw::add_byte<2>(acc[4][e], Qr[0][e]); acc[5][e] = fsk_hw::add_byte<2>(acc[5][e], Qr[1][e]);
                        acc[6][e] = fsk_hw::add_byte<3>(acc[6][e], Qr[0][e]); acc[7][e] = fsk_hw::add_byte<3>(acc[7][e], Qr[1][e]);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        acc[e][0] = fsk_hw::add_byte<0>(acc[e][0], Qc[0][e]); acc[e][1] = fsk_hw::add_byte<0>(acc[e][1], Qc[1][e]);
                        acc[e][2] = fsk_hw::add_byte<1>(acc[e][2], Qc[0][e]); acc[e][3] = fsk_hw::add_byte<1>(acc[e][3], Qc[1][e]);
                        acc[e][4] = fsk_hw::add_byte<2>(acc[e][4], Qc[0][e]); acc[e][5] = fsk_hw::add_byte<2>(acc[e][5], Qc[1][e]);
                        acc[e][6] = fsk_hw::add_byte<3>(acc[e][6], Qc[0][e]); acc[e][7] = fsk_hw::add_byte<3>(acc[e][7], Qc[1][e]);
                        Qr[0][e] = Qr[1][e] = Qc[0][e] = Qc[1][e] = 0u;
                    }
                }
                if (hi) {  // (a flagged chain only) the hi planes over the buffer just used, at 16 x the weight
                    __syncthreads();  // everyone is done with the lo planes
                    load_stage(KMH, buf, sl);
                    fsk_hw::wait_panel_rows();
                    __syncthreads();
                    const uint32_t mul = 16u * wt;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        read_A(e);
                        read_B(e);
#pragma unroll
                        for (int n = 0; n < 8; ++n) {
                            acc[n][e] += (((sA[e] >> (4 * n)) & 15u) - ((dA[e] >> (4 * n)) & 15u)) * mul;
                            acc[e][n] += (((sB[e] >> (4 * n)) & 15u) - ((dB[e] >> (4 * n)) & 15u)) * mul;
                        }
                    }
                    if (!last) next_offs(rg + 256u);
                }
                if (last) break;
                if (in_place) {
                    fsk_hw::barrier_lds_only();  // everyone is done with the lookups; the prefetch stays in flight
                    const uint32_t uo = fsk_hw::vgpr_copy(uo_n), od = uo & 0xffffu, os = uo >> 16;
                    if (od != os) {
                        const uint32_t p = tid & 127u, t4 = p & 0x3cu, e = (p >> 6) * 4u + (p & 3u);
                        const uint32_t base = buf * PBUF + (w >> 1) * SIDE, inc = 1u << (4u * e);
                        atomicAdd(&P[base + ((os ^ t4) >> 2)], inc);
                        atomicAdd(&P[base + ((od ^ t4) >> 2)], 0u - inc);
                    }
                    fsk_hw::barrier_lds_only();  // the planes of the next step are whole
                } else {
                    fsk_hw::wait_panel_rows();
                    __syncthreads();
                    buf ^= 1u;
                    xA ^= PBUF * 4u; xB ^= PBUF * 4u;
                }
                if (gen != 0u) {  // (the words a clean chain never reads)
                    sl = ((sl >> 16) + 1u) << 16 | (sl >> 16);
                    --wt; flw >>= 4;
                }
                --rem; wu >>= 1; rg += 256u;
            }
            fsk_hw::wait_panel_rows();  // the prefetch — planes, offsets, masks, descriptors — has landed
            __syncthreads();            // ... everyone's has, and everyone is done with this chain's buffer and ring half
            buf ^= 1u;
            xA ^= PBUF * 4u; xB ^= PBUF * 4u;
            if (c + 1u < n_bases) {
                half ^= 1u;
                enter_chain(n0, n1, mk_n);
                next_offs(rg);
            }
            ++c;
        }
    }
    for (uint32_t s = 0; !STRAIGHT && s < n_steps; ++s) {  // the loop over STEPS (every form but the straight one)
        uint32_t oR[8], oC[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            oR[4 * h] = fsk_hw::vgpr_copy(oR_n[h].x); oR[4 * h + 1] = fsk_hw::vgpr_copy(oR_n[h].y);
            oR[4 * h + 2] = fsk_hw::vgpr_copy(oR_n[h].z); oR[4 * h + 3] = fsk_hw::vgpr_copy(oR_n[h].w);
            oC[4 * h] = fsk_hw::vgpr_copy(oC_n[h].x); oC[4 * h + 1] = fsk_hw::vgpr_copy(oC_n[h].y);
            oC[4 * h + 2] = fsk_hw::vgpr_copy(oC_n[h].z); oC[4 * h + 3] = fsk_hw::vgpr_copy(oC_n[h].w);
        }
        // the next step's planes are made from this step's: it continues the chain, and neither step has a count above 15
        bool same;
        uint32_t uo_n = 0u;
        [[maybe_unused]] bool last = false;
        if constexpr (AHEAD) {
            // (wt: the weight in bits 0..7; bit 8, "unpack after this step", joins it here)
            const bool first = r == 0u, has_next = c + 1u < n_bases;
            last = rem == 1u;
            if (first) {
                lost = false;
                if (has_next) {  // the next chain's descriptor and masks: issued before its stage, retired with it at this chain's end
                    if (c + 1u - cb >= 64u) {
                        cb = c;
                        load_desc();
                    }
                    n0 = fsk_hw::readlane(dv0, c + 1u - cb);
                    n1 = fsk_hw::readlane(dv1, c + 1u - cb);
                    mk_n = load_masks(n0, n1);
                }
            }
            fl = flw & 15u;
            wt = (wt & 255u) | (wu & 1u) << 8;
            same = !last && (flw & 255u) == 0u;  // (the masks past the chain's end are zero)
            if (first && has_next) {  // the next chain's first planes into the idle buffer, its offsets into the idle ring half
                if (last || same) load_stage(KM, buf ^ 1u, n0);
                else lost = true;  // (step 1 is about to be staged there)
                load_ring(half ^ 1u, s + rem, n1 & 15u);
            }
            if (!last) {
                ring_offs(rg + 256u, oR_n, oC_n);
                if (same) {  // (thread q < 128: row-side position q, the keys of step r + 1; thread 128 + q: column-side position q, step r)
                    uo_n = ring[rg + (w < 2u ? 256u : (uint32_t)TILE) + (tid & 127u)];
                } else {  // a flagged step, or the step behind one: staged as before, over the prefetch
                    lost = true;
                    if (!first) fsk_hw::wait_panel_rows();  // (this wave's part of the prefetch has landed before its replacement is issued)
                    load_stage(KM, buf ^ 1u, slq);
                }
            } else if (lost && has_next) {
                load_stage(KM, buf ^ 1u, n0);  // the prefetch was lost: the next chain's start the old way, under this step's lookups
            }
        } else {
            same = INPLACE && s + 1u < n_steps && (sn & 0xffffu) >= n_bases && fl == 0u && fl_nx == 0u;
            if (s + 1u < n_steps) {
                load_offs(s + 1u, oR_n, oC_n);
                // (thread q < 128: row-side position q, the keys of step s + 1; thread 128 + q: column-side position q, the keys of step s)
                if (same) uo_n = offs[(size_t)(w < 2u ? s + 1u : s) * np_seq + (w < 2u ? ti : tj) * TILE + (tid & 127u)];
                else load_stage(KM, buf ^ 1u, sn);  // in flight under the lookups
            }
        }
        if (AHEAD ? r == 0u : (sl & 0xffffu) < n_bases) {  // a new chain: the prefix sums restart
#pragma unroll
            for (int a = 0; a < 8; ++a) Rr[0][a] = Rr[1][a] = Rc[0][a] = Rc[1][a] = 0u;
        }
        // (a staged plane's base inside P is a multiple of 16 KB and a key offset has 14 bits: the xor places it)
        const uint32_t baseA = buf * PBUF * 4u, baseB = baseA + SIDE * 4u;
        const uint32_t xA = (tr * 4u) | baseA, xB = (tc * 4u) | baseB;
        uint32_t dA[8], sA[8], dB[8], sB[8];  // the step's 32 lookups: A[delta], A[sigma] a column, B[delta], B[sigma] a row
        auto read_A = [&](int e) { dA[e] = lds_at(fsk_hw::xor_word<0>(oC[e], xA)); sA[e] = lds_at(fsk_hw::xor_word<1>(oC[e], xA)); };
        auto read_B = [&](int e) { dB[e] = lds_at(fsk_hw::xor_word<0>(oR[e], xB)); sB[e] = lds_at(fsk_hw::xor_word<1>(oR[e], xB)); };
        auto row_term = [&](int e) {  // column ec = e of this lane, its 8 rows
            Rr[0][e] += (sA[e] & M4) + (~dA[e] & M4);
            Rr[1][e] += ((sA[e] >> 4) & M4) + (~(dA[e] >> 4) & M4);
            Qr[0][e] += Rr[0][e];
            Qr[1][e] += Rr[1][e];
        };
        auto col_term = [&](int e) {  // row er = e of this lane, its 8 columns
            Rc[0][e] += (sB[e] & M4) + (~dB[e] & M4);
            Rc[1][e] += ((sB[e] >> 4) & M4) + (~(dB[e] >> 4) & M4);
            Qc[0][e] += Rc[0][e];
            Qc[1][e] += Rc[1][e];
        };
#pragma unroll
        for (int e = 0; e < 8; ++e) read_A(e);
        fsk_hw::first_use(dA[0], sA[0], dA[1], sA[1], dA[2], sA[2], dA[3], sA[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) read_B(e);
#pragma unroll
        for (int e = 0; e < 4; ++e) row_term(e);
        fsk_hw::first_use(dA[4], sA[4], dA[5], sA[5], dA[6], sA[6], dA[7], sA[7]);
#pragma unroll
        for (int e = 4; e < 8; ++e) read_B(e);
#pragma unroll
        for (int e = 4; e < 8; ++e) row_term(e);
        fsk_hw::first_use(dB[0], sB[0], dB[1], sB[1], dB[2], sB[2], dB[3], sB[3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) col_term(e);
        fsk_hw::first_use(dB[4], sB[4], dB[5], sB[5], dB[6], sB[6], dB[7], sB[7]);
#pragma unroll
        for (int e = 4; e < 8; ++e) col_term(e);
        if ((wt & 256u) != 0u) {  // the batch ends behind this step: every byte of Q joins its int32 sum, and Q starts again
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[0][e] = fsk_hw::add_byte<0>(acc[0][e], Qr[0][e]); acc[1][e] = fsk_hw::add_byte<0>(acc[1][e], Qr[1][e]);
                acc[2][e] = fsk_hw::add_byte<1>(acc[2][e], Qr[0][e]); acc[3][e] = fsk_hw::add_byte<1>(acc[3][e], Qr[1][e]);
                acc[4][e] = fsk_hw::add_byte<2>(acc[4][e], Qr[0][e]); acc[5][e] = fsk_hw::add_byte<2>(acc[5][e], Qr[1][e]);
                acc[6][e] = fsk_hw::add_byte<3>(acc[6][e], Qr[0][e]); acc[7][e] = fsk_hw::add_byte<3>(acc[7][e], Qr[1][e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[e][0] = fsk_hw::add_byte<0>(acc[e][0], Qc[0][e]); acc[e][1] = fsk_hw::add_byte<0>(acc[e][1], Qc[1][e]);
                acc[e][2] = fsk_hw::add_byte<1>(acc[e][2], Qc[0][e]); acc[e][3] = fsk_hw::add_byte<1>(acc[e][3], Qc[1][e]);
                acc[e][4] = fsk_hw::add_byte<2>(acc[e][4], Qc[0][e]); acc[e][5] = fsk_hw::add_byte<2>(acc[e][5], Qc[1][e]);
                acc[e][6] = fsk_hw::add_byte<3>(acc[e][6], Qc[0][e]); acc[e][7] = fsk_hw::add_byte<3>(acc[e][7], Qc[1][e]);
                Qr[0][e] = Qr[1][e] = Qc[0][e] = Qc[1][e] = 0u;
            }
        }
        if (fl != 0u) {  // the hi planes over the buffer just used, at 16 x the weight
            __syncthreads();  // everyone is done with the lo planes
            load_stage(KMH, buf, sl);
            fsk_hw::wait_panel_rows();
            __syncthreads();
            const uint32_t mul = 16u * (wt & 255u);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                read_A(e);
                read_B(e);
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    acc[n][e] += (((sA[e] >> (4 * n)) & 15u) - ((dA[e] >> (4 * n)) & 15u)) * mul;
                    acc[e][n] += (((sB[e] >> (4 * n)) & 15u) - ((dB[e] >> (4 * n)) & 15u)) * mul;
                }
            }
        }
        if constexpr (AHEAD) {
            if (last) {
                fsk_hw::wait_panel_rows();  // the prefetch — planes, offsets, masks, descriptors — has landed
                __syncthreads();            // ... everyone's has, and everyone is done with this chain's buffer and ring half
                buf ^= 1u;
                if (c + 1u < n_bases) {
                    half ^= 1u;
                    enter_chain(n0, n1, mk_n);
                    ring_offs(rg, oR_n, oC_n);
                }
                ++c;
            } else {
                if (same) {
                    fsk_hw::barrier_lds_only();  // everyone is done with the lookups; the prefetch stays in flight
                    const uint32_t uo = fsk_hw::vgpr_copy(uo_n), od = uo & 0xffffu, os = uo >> 16;
                    if (od != os) {
                        const uint32_t p = tid & 127u, t4 = p & 0x3cu, e = (p >> 6) * 4u + (p & 3u);
                        const uint32_t base = buf * PBUF + (w >> 1) * SIDE, inc = 1u << (4u * e);
                        atomicAdd(&P[base + ((os ^ t4) >> 2)], inc);
                        atomicAdd(&P[base + ((od ^ t4) >> 2)], 0u - inc);
                    }
                    fsk_hw::barrier_lds_only();  // the planes of step r + 1 are whole
                } else {
                    fsk_hw::wait_panel_rows();
                    __syncthreads();
                    buf ^= 1u;
                }
                sl = slq; slq += 0x10001u;
                --rem; --wt; wu >>= 1; flw >>= 4;
                ++r; rg += 256u;
            }
        } else {
            uint32_t fl_n = 0u, sl_n2 = 0u, wt_n2 = 0u;
            if constexpr (INPLACE) {  // the masks of step s + 2, the table entry of step s + 3
                if (s + 2u < n_steps) {
                    fl_n = flagged(s2);
                    if (s + 3u < n_steps) {
                        sl_n2 = steps[2u * (s + 3u)];
                        wt_n2 = steps[2u * (s + 3u) + 1u];
                    }
                }
            } else if (s + 1u < n_steps) {
                fl_n = flagged(sn);
                if (s + 2u < n_steps) {
                    sl_n2 = steps[2u * (s + 2u)];
                    wt_n2 = steps[2u * (s + 2u) + 1u];
                }
            }
            fsk_hw::wait_panel_rows();  // this wave's part of the next stage has landed (and every load of this trip)
            __syncthreads();            // ... everyone's has, and everyone is done with the current buffer
            if (same) {  // A: c_up(s) -> c_up(s + 1), B: c_lo(s) -> c_up(s): one nibble up and one down a position, where the keys differ
                const uint32_t uo = fsk_hw::vgpr_copy(uo_n), od = uo & 0xffffu, os = uo >> 16;
                if (od != os) {
                    const uint32_t p = tid & 127u, t4 = p & 0x3cu, e = (p >> 6) * 4u + (p & 3u);
                    const uint32_t base = buf * PBUF + (w >> 1) * SIDE, inc = 1u << (4u * e);
                    atomicAdd(&P[base + ((os ^ t4) >> 2)], inc);
                    atomicAdd(&P[base + ((od ^ t4) >> 2)], 0u - inc);
                }
                __syncthreads();  // the planes of step s + 1 are whole
            } else {
                buf ^= 1u;
            }
            if constexpr (INPLACE) {
                sl = sn; wt = wn; fl = fl_nx;
                sn = s2; wn = w2; fl_nx = fl_n;
                s2 = sl_n2; w2 = wt_n2;
            } else {
                sl = sn; wt = wn; fl = fl_n;
                sn = sl_n2; wn = wt_n2;
            }
        }
    }
#pragma unroll
    for (int er = 0; er < 8; ++er) {
        const u64 i = (u64)ti * TILE + tile_index(tr, (uint32_t)er);
#pragma unroll
        for (int ec = 0; ec < 8; ++ec) {
            const u64 j = (u64)tj * TILE + tile_index(tc, (uint32_t)ec);
            const int v = (int)(acc[er][ec] - bias);
            if (i < N && j <= i && v != 0) atomicAdd(&K[tri_index(i, j)], (u64)(long long)v);
        }
    }
}

}  // namespace fsk
