// fsk_load_plan.h — the host-only half of fsk_load_sequences: everything that follows from the tokens and the modes
// alone (lengths, window census, alphabet, word layout, the packed words), computed without a device and without an
// engine. fsk_engine.hip commits a finished plan: engine fields, reservations, uploads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace fsk_load {

// the modes as the engine stores them (complement map sorted by token, wildcards sorted, the centre-weight profile) and
// the caller's arrays: only tokens[offsets[0] .. offsets[n_train + n_test]) belong to the call
struct LoadInput {
    int g, k;
    const int32_t *rc_tokens, *rc_comps;
    size_t n_rc;
    const int32_t* wild_tokens;
    size_t n_wild;
    const uint8_t* cw;
    size_t n_cw;
    const int32_t* tokens;
    const int64_t* offsets;
    int64_t n_train, n_test;
};

struct LoadPlan {
    int code = 0;  // FSK_OK, or the FSK_E* code of the failure with its message
    std::string msg;
    int64_t N = 0, nfeat = 0, longest = 0, shortest = 0, most_valid = 0, total = 0, total_sym = 0;
    uint32_t sigma = 1;
    int bits = 2, key_symbits = 0;
    uint64_t V = 1;
    bool rc_on = false, wild_on = false, cw_on = false;
    uint64_t n_words = 0;         // packed words of all sequences (the staging holds four zero words more)
    uint32_t* staging = nullptr;  // the callback's buffer: [words + 4][wstart N][len N][fstart N + 1]
    std::vector<uint32_t> len32, fstart, wstart, nvalid, vstart, vbits, fwin;
    std::vector<uint16_t> comp_rank;
    std::vector<int64_t> sym_freq;
    std::vector<int32_t> distinct;
    double ms_census = 0, ms_pack = 0;  // host time up to the end of the window census / of the packing
};

// where the packed words and their three tables go: called once, with the number of 32-bit words needed, by the
// middle step of the packing team; nullptr fails the load with FSK_ENOMEM
using StagingAlloc = std::function<uint32_t*(size_t n_u32)>;

void make_load_plan(const LoadInput& in, const StagingAlloc& staging, LoadPlan& plan);

}  // namespace fsk_load
