// load_plan_check.cpp — TEST INFRASTRUCTURE: the load plan (fastsk_amd/csrc/fsk_load_plan.cpp) called without an engine, so
// that its raw indexing runs under the host sanitizers this program is linked with (tests/test_load_plan_host.py).
//   load_plan_check <case file> <plan file>
// case file, whitespace-separated integers: g k n_train n_test, then five counted lists (count first): the complement map
// as token complement pairs (sorted by token), the wildcards (sorted), the centre weights, the offsets, the tokens.
// plan file: one "name count values..." line a field. The staging is a vector of exactly the size asked for.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../fastsk_amd/csrc/fsk_load_plan.h"

template <typename T>
static std::vector<T> read_list(std::istream& in) {
    long long n = 0;
    in >> n;
    std::vector<T> v((size_t)n);
    for (T& x : v) { long long t = 0; in >> t; x = (T)t; }
    return v;
}

template <typename V>
static void put(std::ostream& out, const char* name, const V& v) {
    out << name << ' ' << v.size();
    for (const auto& x : v) out << ' ' << (long long)x;
    out << '\n';
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: load_plan_check <case file> <plan file>\n"); return 2; }
    std::ifstream in(argv[1]);
    fsk_load::LoadInput li;
    in >> li.g >> li.k >> li.n_train >> li.n_test;
    const std::vector<int32_t> rc = read_list<int32_t>(in), wild = read_list<int32_t>(in);
    const std::vector<uint8_t> cw = read_list<uint8_t>(in);
    const std::vector<int64_t> offsets = read_list<int64_t>(in);
    const std::vector<int32_t> tokens = read_list<int32_t>(in);
    if (!in || offsets.size() != (size_t)(li.n_train + li.n_test) + 1) { fprintf(stderr, "malformed case file\n"); return 2; }
    std::vector<int32_t> rc_tokens, rc_comps;
    for (size_t i = 0; i + 1 < rc.size(); i += 2) { rc_tokens.push_back(rc[i]); rc_comps.push_back(rc[i + 1]); }
    li.rc_tokens = rc_tokens.data(); li.rc_comps = rc_comps.data(); li.n_rc = rc_tokens.size();
    li.wild_tokens = wild.data(); li.n_wild = wild.size();
    li.cw = cw.data(); li.n_cw = cw.size();
    li.tokens = tokens.data(); li.offsets = offsets.data();

    std::vector<uint32_t> staging;
    int calls = 0;
    fsk_load::LoadPlan p;
    fsk_load::make_load_plan(li, [&](size_t n) { ++calls; staging.assign(n, 0xdeadbeefu); return staging.data(); }, p);
    if (calls > 1 || (p.code == 0 && (calls != 1 || p.staging != staging.data()))) { fprintf(stderr, "staging asked for %d times\n", calls); return 3; }

    std::ofstream out(argv[2]);
    out << "code " << p.code << "\nmsg " << p.msg << '\n';
    if (p.code == 0) {
        out << "scalars " << p.N << ' ' << p.nfeat << ' ' << p.longest << ' ' << p.shortest << ' ' << p.most_valid << ' ' << p.sigma << ' ' << p.bits
            << ' ' << p.V << ' ' << p.key_symbits << ' ' << p.total_sym << ' ' << p.total << ' ' << p.n_words << ' ' << p.rc_on << ' ' << p.wild_on << ' '
            << p.cw_on << '\n';
        put(out, "len32", p.len32); put(out, "fstart", p.fstart); put(out, "wstart", p.wstart); put(out, "nvalid", p.nvalid);
        put(out, "vstart", p.vstart); put(out, "vbits", p.vbits); put(out, "fwin", p.fwin); put(out, "comp_rank", p.comp_rank);
        put(out, "sym_freq", p.sym_freq); put(out, "distinct", p.distinct); put(out, "staging", staging);
    }
    return out ? 0 : 4;
}
