// fsk_engine_dense_shift.hip — the DENSE dataflow by shift classes (the headline, config 5: 495 combinations of g = 12, k = 4
// are 165 shapes at up to nine shifts): one weighted Gram product per chain of consecutive shifts and the other members by
// edge lookups (fsk_kernels_dense_shift.h has the identity). The reference work it stands for is the same as
// fsk_engine_dense.hip's: cntsrtna + countAndUpdateTri per combo (shared.cpp:156-191, 268-333).
//
//   dense_shift_plan   host arithmetic on the kept positions: shapes -> chains -> slot order (chain bases first, grouped by
//                      chain length), the groups of the base launch, the derived steps. Cached by the combination list.
//   k_dense_edge_keys  the two keys of every (sequence, derived step), once per counted list
//   k_dense_tile_shift_all  the body of the headline kernel (fsk_tile_kernel_dma.inc, FSK_DMA_SHIFT 2) over the chain bases in
//                      ONE launch (tuning dense_shift_one_launch; by default from 16384 tiles): the groups of equal chain
//                      length run longest first in one pipeline, and at a group's end the sums leave as (u64) sum x (the
//                      length minus the next group's) without being cleared, so a base of length n has left n times at the
//                      end. A tile's first flush stores when the pass may (every cell j <= i, zeros included), the later
//                      ones add their non-zero cells. The flush makes its row and column indices from an opaque copy of the
//                      thread index: made from threadIdx they are hoisted in front of the pipeline and spill (128 VGPRs and
//                      88 bytes of scratch a lane; 122 and none as written).
//   k_dense_tile_shift the same body (FSK_DMA_SHIFT 1) as one launch per group, whose sums leave as (u64) sum x n: where the
//                      one launch does not run (dense_shift_one_launch = -1, the shift path forced below 16384 tiles, a plan
//                      whose group was cut at by_overflow slots)
//   k_dense_keymajor   the count panels once more per counted list as key-major planes (a dword = one key of 8 sequences)
//   k_dense_shift_packed  the derived steps from those planes, eight cells an LDS read (tuning dense_shift_packed); by default
//                      by the ahead schedule (tuning dense_shift_ahead), which reads dense_shift_chain_table's chain table
//   k_dense_shift_fix  the derived steps from the count panels themselves: dense_shift_packed = -1, and whenever the key-major
//                      planes do not fit
//
// A translation unit of its own, like fsk_engine_dense_small.hip: nothing here can reach the register allocation of
// k_dense_tile_dma / k_dense_tile_dma_compact.
#include "fsk_engine_internal.h"
#include "fsk_kernels_dense_shift.h"

#include <map>

using namespace fsk_detail;

namespace fsk {

#define FSK_DMA_SHIFT 1
#define FSK_DMA_KERNEL k_dense_tile_shift
#define FSK_DMA_COMPACT 0
#include "fsk_tile_kernel_dma.inc"
#undef FSK_DMA_KERNEL
#undef FSK_DMA_SHIFT

#define FSK_DMA_SHIFT 2
#define FSK_DMA_KERNEL k_dense_tile_shift_all
#include "fsk_tile_kernel_dma.inc"
#undef FSK_DMA_KERNEL
#undef FSK_DMA_COMPACT
#undef FSK_DMA_SHIFT

}  // namespace fsk

namespace fsk_detail {

// The plan of a combination list. Combinations are grouped by shape (kept positions minus the first), sorted by shift inside
// a shape and cut into chains of consecutive shifts: a list with gaps, in any order or with a repeated id simply gives
// shorter chains, a chain of one is a plain slot of weight 1. max_chain != 0 (the packed corrections: their prefix sums are
// bytes) cuts a chain after that many members: a longer class becomes two chains, one more product. Returns whether the shift
// path can run the list: some chain has a derived step, and the correction sums stay inside int32.
bool dense_shift_plan(fsk_engine* e, const int32_t* combos, int n, u64 by_overflow, uint32_t max_chain) {
    ShiftPlan& p = e->shift;
    if (!(p.by_overflow == by_overflow && p.max_chain == max_chain && (int)p.combos.size() == n && std::equal(combos, combos + n, p.combos.begin()))) {
        p = ShiftPlan();
        p.combos.assign(combos, combos + n);
        p.by_overflow = by_overflow;
        p.max_chain = max_chain;
        const int k = e->k;
        std::map<std::vector<uint8_t>, std::vector<std::pair<int, int>>> shapes;  // shape -> (shift, place in the list)
        for (int q = 0; q < n; ++q) {
            const uint8_t* pos = &e->all_pos[(size_t)combos[q] * k];
            std::vector<uint8_t> shape(pos, pos + k);
            for (auto& x : shape) x = (uint8_t)(x - pos[0]);
            shapes[shape].push_back({(int)pos[0], q});
        }
        std::vector<std::vector<int>> chains;
        for (auto& kv : shapes) {
            auto& v = kv.second;
            std::stable_sort(v.begin(), v.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
            for (size_t i = 0; i < v.size(); ++i) {
                if (i == 0 || v[i].first != v[i - 1].first + 1 || (max_chain != 0u && chains.back().size() >= max_chain)) chains.emplace_back();
                chains.back().push_back(v[i].second);
            }
        }
        std::stable_sort(chains.begin(), chains.end(), [](const std::vector<int>& a, const std::vector<int>& b) { return a.size() > b.size(); });
        p.n_bases = (uint32_t)chains.size();
        p.order.resize((size_t)n);
        uint32_t derived = p.n_bases;
        size_t group_begin = 0;
        for (size_t c = 0; c < chains.size(); ++c) {
            const std::vector<int>& ch = chains[c];
            const uint32_t len = (uint32_t)ch.size();
            p.order[c] = ch[0];
            // groups of equal chain length, of at most by_overflow slots (u32 sums; the product by the length is taken in 64 bits)
            if (c == 0 || chains[c - 1].size() != ch.size() || (u64)(c - group_begin) >= by_overflow) {
                p.groups.push_back(0u);
                p.groups.push_back(len);
                group_begin = c;
            }
            p.groups[p.groups.size() - 2] = (uint32_t)c + 1u;  // the group's end slot
            uint32_t lower = (uint32_t)c;
            for (uint32_t u = 1; u < len; ++u) {  // step u - 1 -> u of the chain, weight (len - 1) - (u - 1)
                const uint32_t upper = derived++;
                p.order[upper] = ch[u];
                p.steps.push_back(upper << 16 | lower);
                p.steps.push_back(len - u);
                p.wsum += len - u;
                lower = upper;
            }
        }
        // the one launch over all groups: the sums are not cleared at a group's end, so group g leaves multiplied by its chain
        // length minus the next group's (the last by its own) and a base of length n has left n times at the end. Lengths
        // fall strictly from group to group unless a group was cut at by_overflow slots: then the table stays empty.
        bool falling = true;
        for (size_t gi = 2; gi + 1 < p.groups.size(); gi += 2) falling = falling && p.groups[gi + 1] < p.groups[gi - 1];
        if (falling) {
            for (size_t gi = 0; gi + 1 < p.groups.size(); gi += 2) {
                p.group_steps.push_back(p.groups[gi]);
                p.group_steps.push_back(p.groups[gi + 1] - (gi + 3 < p.groups.size() ? p.groups[gi + 3] : 0u));
            }
            p.group_steps.push_back(0xffffffffu);
            p.group_steps.push_back(0u);
        }
    }
    // (the + 32 is k_dense_shift_fix's bias a cell and unit of weight; k_dense_shift_packed's is 30, for which the bound is
    // slightly conservative)
    return !p.steps.empty() && n <= 32768 && ((u64)2 * e->maxW + 32) * p.wsum < ((u64)1 << 31);
}

// Bit 8 of a step's weight word: "unpack after this step" (k_dense_shift_packed adds the prefix sums of a batch of steps byte
// to byte and hands the bytes to its int32 sums where the flag stands; every reader masks the weight with & 255). Set by the
// bound alone: the step at position r (0-based) of its chain adds at most 30 (r + 1) to a byte, the table is walked in order
// with the running bound, and the flag goes on the step before the one that would pass 255 — a batch may span chains — and on
// the last step. Chains are cut at nine members, so one step is at most 240 and the walk never fails (a plan with uncut chains
// runs k_dense_shift_fix only, which masks the flags off). batch = false: on every step. The flags are a schedule, not part of
// the plan: they go into the uploaded copy only.
static void dense_shift_unpack_flags(std::vector<uint32_t>& steps, uint32_t n_bases, bool batch) {
    const size_t n_steps = steps.size() / 2;
    uint32_t r = 0, bound = 0;
    for (size_t s = 0; s < n_steps; ++s) {
        r = (steps[2 * s] & 0xffffu) < n_bases ? 0u : r + 1u;
        const uint32_t add = 30u * (r + 1u);
        if (s > 0 && (!batch || bound + add > 255u)) {
            steps[2 * s - 1] |= 256u;
            bound = 0;
        }
        bound += add;
    }
    if (n_steps > 0) steps[2 * n_steps - 1] |= 256u;
}

// The chain table of the ahead schedule (k_dense_shift_packed<true, true>), from the uploaded copy of the step table: two words
// a chain that has steps, {the first step's slot word, steps | first weight << 8 | the steps' unpack flags << 16}. The kernel
// makes every further step's slots and weight from them, which holds for the tables dense_shift_plan writes — a chain's upper
// slots are consecutive, a step's lower slot is the upper of the step before, the weights fall by one — and is checked here
// step by step: a table of another make returns empty, and the parent's schedule runs. Like the flags, a schedule and not
// part of the plan.
static std::vector<uint32_t> dense_shift_chain_table(const std::vector<uint32_t>& steps, uint32_t n_bases) {
    std::vector<uint32_t> t;
    const size_t n_steps = steps.size() / 2;
    size_t s = 0;
    while (s < n_steps) {
        const uint32_t sl0 = steps[2 * s], up0 = sl0 >> 16, wt0 = steps[2 * s + 1] & 255u;
        if ((sl0 & 0xffffu) >= n_bases) return {};
        uint32_t len = 0, flags = 0;
        for (; s + len < n_steps && (len == 0 || (steps[2 * (s + len)] & 0xffffu) >= n_bases); ++len) {
            const uint32_t sl = steps[2 * (s + len)], wt = steps[2 * (s + len) + 1];
            if (len > 0 && sl != ((up0 + len) << 16 | (up0 + len - 1u))) return {};
            if (len >= 8 || wt0 < len || (wt & 255u) != wt0 - len || up0 + len > 0xffffu) return {};
            flags |= ((wt >> 8) & 1u) << len;
        }
        t.push_back(sl0);
        t.push_back(len | wt0 << 8 | flags << 16);
        s += len;
    }
    return t;
}

// the plan's tables on the device, and the edge keys of the list just counted (chunk_pos: its kept positions in slot order)
int dense_shift_edge_keys(fsk_engine* e, const uint8_t* chunk_pos, uint32_t panels_pad) {
    ShiftPlan& p = e->shift;
    const uint32_t n_steps = (uint32_t)(p.steps.size() / 2), np_seq = panels_pad * fsk::PANEL;
    std::vector<uint32_t> steps = p.steps;
    dense_shift_unpack_flags(steps, p.n_bases, e->tune.dense_shift_batch != 0);
    const std::vector<uint32_t> chain_tab = dense_shift_chain_table(steps, p.n_bases);
    // the step table, the one launch's group table behind it, the ahead schedule's chain table behind that
    FSK_HIP(e->d_shift_steps.reserve(p.steps.size() + p.group_steps.size() + chain_tab.size()));
    FSK_HIP(e->d_edge_keys.reserve((size_t)n_steps * np_seq));
    FSK_HIP(hipMemcpyAsync(e->d_shift_steps.p, steps.data(), steps.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    if (!p.group_steps.empty())
        FSK_HIP(hipMemcpyAsync(e->d_shift_steps.p + p.steps.size(), p.group_steps.data(), p.group_steps.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               e->stream));
    if (!chain_tab.empty())
        FSK_HIP(hipMemcpyAsync(e->d_shift_steps.p + p.steps.size() + p.group_steps.size(), chain_tab.data(), chain_tab.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, e->stream));
    e->ld.shift_chains = (uint32_t)(chain_tab.size() / 2);
    FSK_LAUNCH(fsk::k_dense_edge_keys, dim3(panels_pad, (n_steps + 3u) / 4u), dim3(256), 0, e->stream, e->view(), e->cfg.g, e->k, e->sigma, chunk_pos,
               (const uint32_t*)e->d_shift_steps.p, n_steps, np_seq, e->d_edge_keys.p);
    FSK_HIP(hipStreamSynchronize(e->stream));  // (the plan's vectors are pageable memory)
    e->st.launches += 1;
    return FSK_OK;
}

// The key-major planes of the list just counted, and the edge keys as offsets into them: what k_dense_shift_packed reads. They
// stay with the panels (row bands reuse them). Leaves e->ld.shift_packed false, and the corrections to k_dense_shift_fix, when the
// tuning says so, the plan's chains are not cut to the packed kernel's eight steps, or the planes do not fit: never an error.
// A call that wanted the packed kernel and did not get it says so under trace=1 (the slower kernel otherwise shows only as
// three launches fewer in fsk_stats.launches). Memory is asked about only when the buffers have to grow; a growth may take half
// of what is free then, because the results (the normalised triangle of fsk_finalize) are still to be allocated.
int dense_shift_keymajor(fsk_engine* e, uint32_t panels_pad, int nb, uint32_t Vq8) {
    const ShiftPlan& p = e->shift;
    e->ld.shift_packed = false;
    if (e->tune.dense_shift_packed < 0 || p.max_chain != SHIFT_PACKED_CHAIN) return FSK_OK;
    const size_t plane = (size_t)panels_pad * Vq8 * fsk::PANEL * (size_t)nb;  // dwords: as many as a plane of the panels
    const size_t n_keys = (p.steps.size() / 2) * (size_t)panels_pad * fsk::PANEL;
    const size_t want = (2 * plane + n_keys) * sizeof(uint32_t);
    const char* why = nullptr;
    if (e->tune.dense_shift_plane_kb > 0 && want > (size_t)e->tune.dense_shift_plane_kb * 1024) why = "over the dense_shift_plane_kb cap";
    const size_t grow = (std::max(plane, e->d_KM.cap) - e->d_KM.cap + std::max(plane, e->d_KMH.cap) - e->d_KMH.cap +
                         std::max(n_keys, e->d_edge_offs.cap) - e->d_edge_offs.cap) * sizeof(uint32_t);
    if (!why && grow > 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        if (grow > free_b / 2) why = "more than half of the free device memory";
        else if (e->d_KM.reserve(plane) != hipSuccess || e->d_KMH.reserve(plane) != hipSuccess || e->d_edge_offs.reserve(n_keys) != hipSuccess) {
            (void)hipGetLastError();
            e->d_KM.release(); e->d_KMH.release(); e->d_edge_offs.release();
            why = "hipMalloc failed";
        }
    }
    if (why) {
        if (e->trace())
            fprintf(stderr, "[fsk] dense shift classes: the key-major planes (%.1f MB) do not fit, %s: k_dense_shift_fix runs the corrections\n",
                    (double)want / 1e6, why);
        return FSK_OK;
    }
    const uint32_t n_pairs = panels_pad / 2u;
    const uint32_t kgrid = (uint32_t)(((size_t)n_pairs * nb * Vq8 * 16u + 255u) / 256u);
    FSK_LAUNCH(fsk::k_dense_keymajor, dim3(kgrid), dim3(256), 0, e->stream, (const uint32_t*)e->d_C4.p, n_pairs, nb, Vq8, e->d_KM.p);
    FSK_LAUNCH(fsk::k_dense_keymajor, dim3(kgrid), dim3(256), 0, e->stream, (const uint32_t*)e->d_C4H.p, n_pairs, nb, Vq8, e->d_KMH.p);
    FSK_LAUNCH(fsk::k_dense_edge_offs, dim3((uint32_t)((n_keys + 255u) / 256u)), dim3(256), 0, e->stream, (const uint16_t*)e->d_edge_keys.p, n_keys,
               e->d_edge_offs.p);
    e->st.launches += 3;
    e->ld.shift_packed = true;
    return FSK_OK;
}

// the tile pass of accumulate_dense: the weighted base products, then the corrections
int dense_shift_tiles(fsk_engine* e, u64 n_tiles, int nb, uint32_t Vq8, uint32_t nst, u64* K, int store, uint32_t panels_pad) {
    const ShiftPlan& p = e->shift;
    // One launch over all groups (tuning dense_shift_one_launch), from the size at which the shift path runs by its own default
    // rule. Its u32 sums hold all bases at once, n_bases * maxW^2 < 2^32: the path's condition chunk == n says the whole list,
    // and so its bases, fit by_overflow = (2^32 - 1) / maxW^2 slots. A plan with a group cut at by_overflow slots has no table.
    const bool one_launch = !p.group_steps.empty() && (e->tune.dense_shift_one_launch > 0 ||
                                                       (e->tune.dense_shift_one_launch == 0 && e->tune.tile_splits == 0 && n_tiles >= 16384));
    int base_launches = 1;
    if (one_launch) {
        FSK_LAUNCH(fsk::k_dense_tile_shift_all, dim3((uint32_t)n_tiles, 1), dim3(256), 0, e->stream, (const uint32_t*)e->d_C4.p,
                   (const uint32_t*)e->d_C4H.p, (const uint32_t*)e->d_rowmask.p, (const uint32_t*)e->d_tiletab.p, nb, Vq8, nst, (uint32_t)e->N, K,
                   (int)p.n_bases, store, (const uint32_t*)e->d_shift_steps.p + p.steps.size());
    } else {
        base_launches = (int)(p.groups.size() / 2);
        int slot0 = 0;
        for (size_t gi = 0; gi + 1 < p.groups.size(); gi += 2) {  // {end slot, chain length}
            const int end = (int)p.groups[gi];
            FSK_LAUNCH(fsk::k_dense_tile_shift, dim3((uint32_t)n_tiles, 1), dim3(256), 0, e->stream, (const uint32_t*)e->d_C4.p,
                       (const uint32_t*)e->d_C4H.p, (const uint32_t*)e->d_rowmask.p, (const uint32_t*)e->d_tiletab.p, nb, Vq8, nst, (uint32_t)e->N, K,
                       end - slot0, gi == 0 ? store : 0, slot0, p.groups[gi + 1]);
            slot0 = end;
        }
    }
    if (e->ld.shift_packed) {
        // the ahead schedule (tuning dense_shift_ahead) is a schedule of the in-place form and needs the chain table
        const bool ahead = e->tune.dense_shift_inplace != 0 && e->tune.dense_shift_ahead != 0 && e->ld.shift_chains > 0;
        // the straight chains (tuning dense_shift_straight) are a form of the ahead schedule's step loop
        const bool straight = ahead && e->tune.dense_shift_straight != 0;
        const auto k_packed = straight ? fsk::k_dense_shift_packed<true, true, true>
                              : ahead  ? fsk::k_dense_shift_packed<true, true, false>
                                       : e->tune.dense_shift_inplace != 0 ? fsk::k_dense_shift_packed<true, false, false> : fsk::k_dense_shift_packed<false, false, false>;
        if (e->trace())
            fprintf(stderr, "[fsk] dense shift classes: the corrections by k_dense_shift_packed<%s>\n",
                    straight ? "true, true, true" : ahead ? "true, true, false" : e->tune.dense_shift_inplace != 0 ? "true, false, false" : "false, false, false");
        // (ahead: the chain table in the step table's place, its chains in n_bases' — the kernel makes the steps from them)
        FSK_LAUNCH(k_packed, dim3((uint32_t)n_tiles), dim3(256), 0, e->stream, (const uint32_t*)e->d_KM.p, (const uint32_t*)e->d_KMH.p,
                   (const uint32_t*)e->d_rowmask.p, (const uint32_t*)e->d_tiletab.p,
                   (const uint32_t*)e->d_shift_steps.p + (ahead ? p.steps.size() + p.group_steps.size() : 0), (uint32_t)(p.steps.size() / 2),
                   (const uint32_t*)e->d_edge_offs.p, panels_pad * fsk::PANEL, nb, Vq8, ahead ? e->ld.shift_chains : p.n_bases, (uint32_t)(30u * p.wsum), (uint32_t)e->N, K);
    } else {
        FSK_LAUNCH(fsk::k_dense_shift_fix, dim3((uint32_t)n_tiles), dim3(512), 0, e->stream, (const uint32_t*)e->d_C4.p, (const uint32_t*)e->d_C4H.p,
                   (const uint32_t*)e->d_rowmask.p, (const uint32_t*)e->d_tiletab.p, (const uint32_t*)e->d_shift_steps.p, (uint32_t)(p.steps.size() / 2),
                   (const uint16_t*)e->d_edge_keys.p, panels_pad * fsk::PANEL, nb, Vq8, (uint32_t)e->N, K);
    }
    e->st.launches += (int32_t)base_launches;  // (the base launches and the corrections; the caller counts one)
    return FSK_OK;
}

}  // namespace fsk_detail
