// fsk_tile_kernel_dma.inc — body of the tile kernel, the count panels staged by gfx950's direct-to-LDS
// buffer loads (`buffer_load_dwordx4 ... lds`). Included twice by fsk_kernels_dense.h:
//   k_dense_tile_dma          FSK_DMA_COMPACT 0  (the common case)
//   k_dense_tile_dma_compact  FSK_DMA_COMPACT 1  (key compaction: combo s has only ceil(vc[s]/8) dword rows)
// and twice more, in a translation unit of their own (fsk_engine_dense_small.hip, so that nothing about them reaches the
// register allocation of the two above), with FSK_DMA_STAGE32 1:
//   k_dense_tile_small / k_dense_tile_small_compact   small N, the combo range split over several workgroups a tile: a
//       workgroup's 128 x 128 partial sums leave as PLAIN 32-bit stores into a staging block of its own (one 1 KB store a
//       wave and register) instead of one 64-bit atomic a cell and split; k_dense_widen adds a tile's blocks into K.
// and once more, in fsk_engine_dense_shift.hip, with FSK_DMA_SHIFT 1:
//   k_dense_tile_shift   a group of chain bases of the shift-class plan, slots [slot0, slot0 + slots_per_split) of the n_slots
//       counted: every sum leaves multiplied by `weight`, the group's chain length, the product taken in 64 bits.
// and, there too, with FSK_DMA_SHIFT 2:
//   k_dense_tile_shift_all   every group of the plan in ONE launch, longest chains first: slots [0, slots_per_split) in one
//       pipeline, and where the slot crosses a group's end (`groups`: pairs {end slot, weight step}, a pair {~0, 0} behind the
//       last) the sums leave as (u64) sum x step WITHOUT being cleared: step_g = n_g - n_(g+1) (n past the last group = 0), so
//       a base of chain length n leaves n times in all. The first flush stores where the pass may, every later one adds. The
//       next stage's loads stay in flight under a flush; the sums hold all bases at once, which the caller's bound covers.
// Two plain functions rather than one template: instantiations of one template share register-
// allocation context on hipcc, and a second variant must not perturb the common one.
//
// Output-stationary tile accumulate. grid = (n_tiles, n_splits), block = 256 = 16 x 16 lanes;
// each lane owns 8 rows x 8 columns (interleaved by 16, see panel_slot) of a 128x128 tile of K.
// LDS holds the 4-bit count panels as they lie in HBM (8 keys per dword), each panel's rows
// contiguous: P[buffer][panel A0 A1 B0 B1][row][64 dwords]. A-fragment reads are 4 addresses per
// wave (broadcast), B-fragment reads are 16 consecutive 16-byte segments in each panel half:
// conflict-free ds_read_b128. Per dword row and lane: 4 x ds_read_b128 + 64 x v_dot8_u32_u4.
//   * no prefetch registers and no ds_write: each wave's load writes 1 KB (4 rows x 256 B of one
//     panel, contiguous in HBM and in LDS) straight into the stage buffer (M0 = LDS address);
//   * stages are DMA_ROWS = 16 dword rows, double buffered: the loads of stage s+1 are in flight
//     while stage s is multiplied; one barrier per stage (after `s_waitcnt vmcnt(0)`) publishes
//     the next buffer and retires the current one.
// 126 VGPRs (main loop unrolled by 2) and, with 1024 mask words, exactly 40 KB of LDS: 4 workgroups
// per CU, 4 waves per SIMD. The loads are inline asm: through the builtin the compiler would order
// every later ds_read behind them (it cannot tell the two buffers apart) and the overlap would be
// lost; the waits are therefore explicit.
//
// Counts are lo + 16*hi (two nibble planes). Every row is multiplied in its lo plane; the rare
// rows where some sequence of the four panels has hi != 0 (row masks from k_dense_count, OR-ed
// per tile into LDS) get the exact remainder 16*(lo.hi + hi.lo) + 256*hi.hi from the hi plane,
// fetched (MAXF rows per round) while the stage's lo plane is being multiplied. No divergence:
// the masks are workgroup-uniform.
//
// blockIdx.x -> tile through a host-built table (tile_tab[b] = ti << 16 | tj): the order is
// XCD-aware (blocks b, b+8, b+16, ... share an XCD and walk 8x8 super-tiles, so the ~128
// workgroups resident on one XCD stream 8+8 panel pairs out of its L2 instead of 1+64).
//
// The flush builds its 64-bit operand from a v_mov COPY of the accumulator (fsk_hw::vgpr_copy):
// written as (u64)acc, hipcc keeps every accumulator in the low half of a 64-bit register pair
// for the whole kernel (64 VGPRs of zeros).
#ifndef FSK_DMA_STAGE32
#define FSK_DMA_STAGE32 0
#endif
#ifndef FSK_DMA_SHIFT
#define FSK_DMA_SHIFT 0
#endif
__global__ __launch_bounds__(256, 4) void FSK_DMA_KERNEL(const uint32_t* C4, const uint32_t* C4H, const uint32_t* rowmask,
                                                        const uint32_t* tile_tab, int n_slots, uint32_t Vq8, uint32_t nst,
                                                        uint32_t N,
#if FSK_DMA_STAGE32
                                                        uint32_t* stage32,
#else
                                                        u64* K,
#endif
                                                        int slots_per_split, int store
#if FSK_DMA_COMPACT
                                                        , const uint16_t* vc
#endif
#if FSK_DMA_SHIFT == 1
                                                        , int slot0, uint32_t weight
#elif FSK_DMA_SHIFT == 2
                                                        , const uint32_t* groups
#endif
) {
    constexpr int MAXF = 4;           // flagged rows whose hi plane is fetched per round
#if FSK_DMA_COMPACT
    constexpr int MASK_WORDS = 960;   // LDS words of per-(combo, 32-row block) row masks; the last 64 of the 1024: rows per combo
    constexpr int ROW_SLOTS = 64;
#else
    constexpr int MASK_WORDS = 1024;  // LDS words of per-(combo, 32-row block) row masks
#endif
    constexpr int DMA_ROWS = 16;
    constexpr int PBUF = 4 * DMA_ROWS * PANEL;  // dwords per stage buffer
    __shared__ __attribute__((aligned(1024))) uint32_t P[2 * PBUF + 2 * MAXF * TILE];
    __shared__ uint32_t smask[1024];
    uint32_t* const AsH = P + 2 * PBUF;
    uint32_t* const BsH = P + 2 * PBUF + MAXF * TILE;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const uint32_t tile = tile_tab[blockIdx.x];
    const uint32_t ti = tile >> 16, tj = tile & 0xffffu;
#if FSK_DMA_SHIFT == 1
    const int s0 = slot0;
#elif FSK_DMA_SHIFT == 2
    const int s0 = 0;
#else
    const int s0 = blockIdx.y * slots_per_split;
#endif
    const int s1 = s0 + slots_per_split < n_slots ? s0 + slots_per_split : n_slots;
#if !FSK_DMA_STAGE32
    if (s0 >= s1) return;
#endif
    const size_t slot_stride = (size_t)Vq8 * PANEL;
    const size_t panel_stride = (size_t)n_slots * slot_stride;

    uint32_t acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0u;

#define FSK_PANEL_OF(which) (((which) < 2u ? ti : tj) * 2u + ((which) & 1u))
    // the lane's byte offset inside a panel's 16 rows: row tid/16, 16-byte column tid%16
    const uint32_t lane_off_b = (((uint32_t)tid >> 4) * PANEL + ((uint32_t)tid & 15u) * 4u) * 4u;
    // LDS byte address of this wave's 1 KB slice of buffer 0, panel 0 (uniform within the wave)
    const fsk_hw::lds_addr_t lds_wave = fsk_hw::lds_address(P) + (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6) * 1024u;
    auto load_stage = [&](int buf, int slot, uint32_t kq0, uint32_t rows) {
        const size_t so = (size_t)slot * slot_stride + (size_t)kq0 * PANEL;  // uniform
        const uint32_t left = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rows - kq0));  // (into the scalar descriptor)
        const uint32_t bytes = (left < (uint32_t)DMA_ROWS ? left : (uint32_t)DMA_ROWS) * PANEL * 4u;  // rows of the stage that exist
#pragma unroll
        for (int w = 0; w < 4; ++w)
            fsk_hw::panel_rows_to_lds(C4 + FSK_PANEL_OF((uint32_t)w) * panel_stride + so, bytes,
                                      lds_wave + (uint32_t)(buf * PBUF + w * DMA_ROWS * PANEL) * 4u, lane_off_b);
    };
    auto wait_loads = [&]() { fsk_hw::wait_panel_rows(); };
    auto fetch_hi = [&](int slot, uint32_t kq0, uint32_t m) -> uint4 {
        const uint32_t f = (uint32_t)tid >> 6;
        for (uint32_t q = 0; q < f; ++q) m &= m - 1u;
        uint4 h = make_uint4(0u, 0u, 0u, 0u);
        if (m) {
            const uint32_t row = kq0 + (uint32_t)__ffs((int)m) - 1u;
            const uint32_t within = (uint32_t)tid & 63u, which = within >> 4, r4 = within & 15u;
            h = *reinterpret_cast<const uint4*>(C4H + FSK_PANEL_OF(which) * panel_stride + (size_t)slot * slot_stride +
                                                (size_t)row * PANEL + r4 * 4u);
        }
        return h;
    };
    auto park_hi = [&](const uint4& h) {
        const uint32_t f = (uint32_t)tid >> 6, within = (uint32_t)tid & 63u, which = within >> 4, r4 = within & 15u;
        uint32_t* dst = (which < 2 ? AsH : BsH) + f * TILE + (which & 1u) * PANEL + r4 * 4u;
        *reinterpret_cast<uint4*>(dst) = h;
    };
#if FSK_DMA_COMPACT
    // exact remainder of one flagged row r of the stage in buffer `pb`, hi plane in AsH/BsH[f]. Data with a rare
    // symbol has many flagged rows (runs of 'n', repeats): the masks are kept per tile side and only the terms
    // that can be non-zero are computed — three small passes of one dot8 + one shift-add per cell, usually one
    // of them.
    auto fix_row = [&](const uint32_t* pb, uint32_t r, uint32_t f, bool hasA, bool hasB) {
        auto frag = [&](const uint32_t* p0, const uint32_t* p1, int t, uint32_t (&v)[8]) {
            const uint4 x0 = *reinterpret_cast<const uint4*>(&p0[t * 4]);
            const uint4 x1 = *reinterpret_cast<const uint4*>(&p1[t * 4]);
            v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        };
        const uint32_t* alo = pb + r * PANEL;
        const uint32_t* blo = pb + 2 * DMA_ROWS * PANEL + r * PANEL;
        uint32_t p[8], q[8];
        if (hasA) {  // 16 * hi_i * lo_j
            frag(&AsH[f * TILE], &AsH[f * TILE + PANEL], ty, p);
            frag(blo, blo + DMA_ROWS * PANEL, tx, q);
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] += __builtin_amdgcn_udot8(p[a], q[b], 0u, false) << 4;
        }
        if (hasB) {  // 16 * lo_i * hi_j
            frag(alo, alo + DMA_ROWS * PANEL, ty, p);
            frag(&BsH[f * TILE], &BsH[f * TILE + PANEL], tx, q);
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] += __builtin_amdgcn_udot8(p[a], q[b], 0u, false) << 4;
        }
        if (hasA && hasB) {  // 256 * hi_i * hi_j
            frag(&AsH[f * TILE], &AsH[f * TILE + PANEL], ty, p);
            frag(&BsH[f * TILE], &BsH[f * TILE + PANEL], tx, q);
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] += __builtin_amdgcn_udot8(p[a], q[b], 0u, false) << 8;
        }
    };
#else
    // exact remainder of one flagged row r of the stage in buffer `pb`, hi plane in AsH/BsH[f]
    auto fix_row = [&](const uint32_t* pb, uint32_t r, uint32_t f, bool, bool) {
        const uint4 b0 = *reinterpret_cast<const uint4*>(&pb[2 * DMA_ROWS * PANEL + r * PANEL + tx * 4]);
        const uint4 b1 = *reinterpret_cast<const uint4*>(&pb[3 * DMA_ROWS * PANEL + r * PANEL + tx * 4]);
        const uint4 d0 = *reinterpret_cast<const uint4*>(&BsH[f * TILE + tx * 4]);
        const uint4 d1 = *reinterpret_cast<const uint4*>(&BsH[f * TILE + PANEL + tx * 4]);
        const uint32_t blo[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        const uint32_t bhi[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const uint32_t alo = pb[(a >> 2) * DMA_ROWS * PANEL + r * PANEL + ty * 4 + (a & 3)];
            const uint32_t ahi = AsH[f * TILE + (a >> 2) * PANEL + ty * 4 + (a & 3)];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                uint32_t t = __builtin_amdgcn_udot8(alo, bhi[b], 0u, false);
                t = __builtin_amdgcn_udot8(ahi, blo[b], t, false);
                const uint32_t u = __builtin_amdgcn_udot8(ahi, bhi[b], 0u, false);
                acc[a][b] += 16u * t + 256u * u;
            }
        }
    };
#endif

#if FSK_DMA_COMPACT
    constexpr uint32_t MW = 2u;  // mask words per (combo, 32-row block): A side, B side
    int chunk_slots = (int)(MASK_WORDS / (MW * nst)) > 0 ? (int)(MASK_WORDS / (MW * nst)) : 1;
    if (chunk_slots > ROW_SLOTS) chunk_slots = ROW_SLOTS;
    // dword rows combo `sl` of the current chunk really has (its compacted keys), staged next to the masks
#define FSK_ROWS_OF(sl) smask[MASK_WORDS + (uint32_t)((sl) - c0)]
#else
    const int chunk_slots = (int)(MASK_WORDS / nst) > 0 ? (int)(MASK_WORDS / nst) : 1;
#define FSK_ROWS_OF(sl) Vq8
#endif
#if FSK_DMA_SHIFT == 2
    // The group at hand: its end slot and weight step (workgroup-uniform; the table ends with {~0, 0}), whether its flush is
    // the tile's first. The mask chunks below know nothing of the groups: a group's end may fall inside a chunk.
    int g_end = __builtin_amdgcn_readfirstlane((int)groups[0]);
    uint32_t g_step = (uint32_t)__builtin_amdgcn_readfirstlane((int)groups[1]);
    int g_at = 0;
    // The sums leave multiplied by `step` and stay. Row and column indices are made from an opaque copy of the thread index
    // HERE: made from `tid` they are loop-invariant, the compiler hoists all sixteen in front of the pipeline and the 64 sums
    // no longer fit beside them (23 spilled registers, 88 bytes of scratch a lane).
    auto flush_group = [&](uint32_t step, bool st) {
        const uint32_t t = fsk_hw::vgpr_copy((uint32_t)tid);
        const uint32_t fy = t >> 4, fx = t & 15u;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const u64 i = (u64)ti * TILE + tile_index(fy, (uint32_t)a);
            if (i >= N) continue;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const u64 j = (u64)tj * TILE + tile_index(fx, (uint32_t)b);
                // st (workgroup-uniform): the tile's first flush of a pass that may store writes every cell j <= i, zeros too
                if (j <= i && (st || acc[a][b] != 0u)) {
                    const uint32_t lo = fsk_hw::vgpr_copy(acc[a][b]);  // a copy: see the header
                    if (st) K[tri_index(i, j)] = (u64)lo * step;
                    else atomicAdd(&K[tri_index(i, j)], (u64)lo * step);
                }
            }
        }
    };
#endif
    for (int c0 = s0; c0 < s1; c0 += chunk_slots) {
        const int c1 = c0 + chunk_slots < s1 ? c0 + chunk_slots : s1;
        __syncthreads();  // the previous chunk's masks and stage buffers are no longer read
        for (uint32_t i = tid; i < (uint32_t)(c1 - c0) * nst; i += 256) {
            const uint32_t sl = (uint32_t)c0 + i / nst, st = i % nst;
            const size_t a = ((size_t)(ti * 2u) * n_slots + sl) * nst + st, b = ((size_t)(tj * 2u) * n_slots + sl) * nst + st;
            const size_t np = (size_t)n_slots * nst;
#if FSK_DMA_COMPACT
            smask[2u * i] = rowmask[a] | rowmask[a + np];       // rows where an A-side (row) sequence has hi != 0
            smask[2u * i + 1u] = rowmask[b] | rowmask[b + np];  // same for the B side (columns)
#else
            smask[i] = rowmask[a] | rowmask[a + np] | rowmask[b] | rowmask[b + np];
#endif
        }
#if FSK_DMA_COMPACT
        if (tid < c1 - c0) smask[MASK_WORDS + tid] = ((uint32_t)vc[c0 + tid] + 7u) >> 3;
        __syncthreads();
#endif
        int slot = c0;
#if FSK_DMA_COMPACT
        while (slot < c1 && FSK_ROWS_OF(slot) == 0u) ++slot;  // a combo none of whose keys occurs
        if (slot >= c1) continue;
#endif
        uint32_t kq0 = 0;
        int buf = 0;
        load_stage(buf, slot, kq0, FSK_ROWS_OF(slot));
        wait_loads();
        __syncthreads();  // masks staged, first stage landed
        while (slot < c1) {
            const uint32_t rows_s = __builtin_amdgcn_readfirstlane(FSK_ROWS_OF(slot));
            // next stage: the rest of this combo's rows, else the next combo
            int nslot = slot;
            uint32_t nkq0 = kq0 + DMA_ROWS;
            if (nkq0 >= rows_s) {
                nslot = slot + 1;
                nkq0 = 0;
#if FSK_DMA_COMPACT
                while (nslot < c1 && FSK_ROWS_OF(nslot) == 0u) ++nslot;
#endif
            }
            // rows of this stage with hi != 0 somewhere (workgroup-uniform): 16 bits of the 32-row mask word
#if FSK_DMA_COMPACT
            const uint32_t mi = 2u * ((uint32_t)(slot - c0) * nst + (kq0 >> 5));
            const uint32_t maskA = (__builtin_amdgcn_readfirstlane(smask[mi]) >> (kq0 & 16u)) & 0xffffu;
            const uint32_t maskB = (__builtin_amdgcn_readfirstlane(smask[mi + 1u]) >> (kq0 & 16u)) & 0xffffu;
            const uint32_t mask = maskA | maskB;
#else
            const uint32_t mword = __builtin_amdgcn_readfirstlane(smask[(uint32_t)(slot - c0) * nst + (kq0 >> 5)]);
            const uint32_t mask = (mword >> (kq0 & 16u)) & 0xffffu;
#endif
            uint4 hreg = make_uint4(0u, 0u, 0u, 0u);
            if (mask) hreg = fetch_hi(slot, kq0, mask);
            // (after the compiler's own loads of this trip: it cannot see the asm loads, and a wait it
            // places for one of its registers would otherwise wait for the whole next stage as well)
            if (nslot < c1) load_stage(buf ^ 1, nslot, nkq0, FSK_ROWS_OF(nslot));  // in flight under the dot products
            const uint32_t rows_left = rows_s - kq0;
            const int nkq = rows_left < (uint32_t)DMA_ROWS ? (int)rows_left : DMA_ROWS;
            const uint32_t* pb = P + buf * PBUF;
#pragma unroll 2
            for (int kq = 0; kq < nkq; ++kq) {
                const uint4 a0 = *reinterpret_cast<const uint4*>(&pb[kq * PANEL + ty * 4]);
                const uint4 a1 = *reinterpret_cast<const uint4*>(&pb[DMA_ROWS * PANEL + kq * PANEL + ty * 4]);
                const uint4 b0 = *reinterpret_cast<const uint4*>(&pb[2 * DMA_ROWS * PANEL + kq * PANEL + tx * 4]);
                const uint4 b1 = *reinterpret_cast<const uint4*>(&pb[3 * DMA_ROWS * PANEL + kq * PANEL + tx * 4]);
                const uint32_t av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const uint32_t bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) acc[a][b] = __builtin_amdgcn_udot8(av[a], bv[b], acc[a][b], false);
            }
            if (mask) {  // rows with counts above 15 in some sequence: add the exact remainder
                uint32_t m = mask;
                bool first = true;
                while (m) {  // MAXF rows per round
                    if (!first) {
                        hreg = fetch_hi(slot, kq0, m);
                        __syncthreads();  // the previous round's rows have been consumed
                    }
                    park_hi(hreg);
                    __syncthreads();
                    for (uint32_t f = 0; f < (uint32_t)MAXF && m; ++f) {
                        const uint32_t r = (uint32_t)__ffs((int)m) - 1u;
#if FSK_DMA_COMPACT
                        fix_row(pb, r, f, (maskA >> r) & 1u, (maskB >> r) & 1u);
#else
                        fix_row(pb, r, f, true, true);
#endif
                        m &= m - 1u;
                    }
                    first = false;
                }
            }
#if FSK_DMA_SHIFT == 2
            // The group's last stage has been multiplied: flush under the next stage's loads. A lane is the only writer of its
            // cells in this launch, and its store of a cell is ordered before its own later add to it by the vmcnt(0) of
            // wait_loads() just below: stores and atomics count into vmcnt like the loads, so that wait — which every stage
            // has, and the last stage of a chunk too — is passed only when this flush has been acknowledged.
            if (nslot != slot && nslot == g_end) {
                flush_group(g_step, store != 0 && g_at == 0);
                ++g_at;
                g_end = __builtin_amdgcn_readfirstlane((int)groups[2 * g_at]);
                g_step = (uint32_t)__builtin_amdgcn_readfirstlane((int)groups[2 * g_at + 1]);
            }
#endif
            wait_loads();     // this wave's part of the next stage has landed
            __syncthreads();  // ... everyone's has, and everyone is done with the current buffer
            slot = nslot;
            kq0 = nkq0;
            buf ^= 1;
        }
    }
#undef FSK_PANEL_OF
#undef FSK_ROWS_OF
#if FSK_DMA_STAGE32
    // the workgroup's block of the staging buffer: [split][tile][register a * 8 + b][thread] — a wave's store of one register is
    // 256 contiguous bytes; every cell of the block is written (zeros too: the buffer is never cleared)
    {
        uint32_t* blk = stage32 + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(TILE * TILE);
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) blk[(a * 8 + b) * 256 + tid] = acc[a][b];
    }
#elif FSK_DMA_SHIFT != 2
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const u64 i = (u64)ti * TILE + tile_index((uint32_t)ty, (uint32_t)a);
        if (i >= N) continue;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 j = (u64)tj * TILE + tile_index((uint32_t)tx, (uint32_t)b);
            // store != 0 (workgroup-uniform): these rows of K were reset but not yet zeroed and this
            // workgroup is the only writer of its cells in this launch, so the sums (zeros included)
            // are stored, not added: the pass needs no 8 N^2/2-byte fill in front of it.
            if (j <= i && (store || acc[a][b] != 0u)) {
                const uint32_t lo = fsk_hw::vgpr_copy(acc[a][b]);  // a copy: see the header
#if FSK_DMA_SHIFT == 1
                if (store) K[tri_index(i, j)] = (u64)lo * weight;
                else atomicAdd(&K[tri_index(i, j)], (u64)lo * weight);
#else
                if (store) K[tri_index(i, j)] = (u64)lo;
                else atomicAdd(&K[tri_index(i, j)], (u64)lo);
#endif
            }
        }
    }
#endif
}
