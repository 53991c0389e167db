// The host side of the linear-path merge plan (merge_host.hpp): fixed-set seeds, depth and type rules, totals, error texts.
#include "merge_host.hpp"

#include <stdexcept>

namespace ac {

static inline uint32_t number_of(int32_t e) { return e < 0 ? (uint32_t)(-(int64_t)e) : (uint32_t)e; }

void merge_seed_fixed(uint32_t n, const uint8_t* alive, const int32_t* path_ends, uint32_t n_seqs, std::vector<uint8_t>* seed) {
    seed->assign(n, 0);
    for (uint64_t i = 0; i < 2 * (uint64_t)n_seqs; i++) {
        const int32_t e = path_ends[i];
        const uint32_t u = number_of(e);
        const char* which = (i & 1) ? "last" : "first";
        if (u == 0 || u > n)
            throw std::runtime_error("path end: the " + std::string(which) + " entry of sequence " + std::to_string(i / 2) + " (" + std::to_string(e) +
                                     ") names no unitig: unitig numbers run from 1 to " + std::to_string(n));
        if (alive && !alive[u - 1])
            throw std::runtime_error("path end: the " + std::string(which) + " entry of sequence " + std::to_string(i / 2) + " (" + std::to_string(e) +
                                     ") names a unitig that is not alive");
        // first entry: + fixes the start, - the end; last entry: + fixes the end, - the start
        const bool start = ((i & 1) == 0) == (e > 0);
        (*seed)[u - 1] |= start ? MERGE_FIXED_START : MERGE_FIXED_END;
    }
}

double merge_path_depth(const int32_t* members, uint32_t n_members, const uint32_t* unitig_len, const double* depth, const uint32_t* fwd, const uint32_t* rev,
                        const uint8_t* type) {
    if (n_members == 0) return 0.0;
    const int32_t first = members[0];
    const uint32_t* counts = first > 0 ? fwd : rev;
    if (counts && counts[number_of(first) - 1]) return (double)counts[number_of(first) - 1];
    if (type)
        for (uint32_t i = 0; i < n_members; i++)
            if (type[number_of(members[i]) - 1] == MERGE_TYPE_ANCHOR) return depth ? depth[number_of(members[i]) - 1] : 0.0;
    // weighted_mean_depth (:519-526): the lengths summed as integers, the products one after the other in path order
    uint64_t total = 0;
    double depth_sum = 0.0;
    for (uint32_t i = 0; i < n_members; i++) {
        const uint32_t u = number_of(members[i]) - 1;
        total += unitig_len[u];
        depth_sum += (depth ? depth[u] : 0.0) * (double)unitig_len[u];
    }
    return depth_sum / (double)total;
}

uint8_t merge_path_type(const int32_t* members, uint32_t n_members, const uint8_t* type) {
    if (type)
        for (uint32_t i = 0; i < n_members; i++) {
            const uint8_t t = type[number_of(members[i]) - 1];
            if (t == MERGE_TYPE_ANCHOR || t == MERGE_TYPE_CONSENTIG) return MERGE_TYPE_CONSENTIG;
        }
    return MERGE_TYPE_OTHER;
}

void merge_finish(MergeResult* r, const uint32_t* unitig_len, const uint8_t* alive, const double* depth, const uint32_t* fwd, const uint32_t* rev, const uint8_t* type) {
    const uint32_t n = r->n_unitigs;
    if (r->chain_of.size() != n || r->fixed.size() != n) throw std::runtime_error("merge plan: the result arrays do not fit together");
    uint64_t at = 0, bases = 0;
    for (size_t c = 0; c < r->chains.size(); c++) {
        MergeChainRecord& rec = r->chains[c];
        if (rec.members < 2 || rec.member_off != at || rec.seq_off != bases || at + rec.members > r->members.size())
            throw std::runtime_error("merge plan: a chain record does not fit its member list");
        uint64_t len = 0;
        for (uint32_t i = 0; i < rec.members; i++) {
            const uint32_t u = number_of(r->members[at + i]);
            if (u == 0 || u > n || r->chain_of[u - 1] != c) throw std::runtime_error("merge plan: a member does not fit its chain");
            len += unitig_len[u - 1];
        }
        if (len != rec.length) throw std::runtime_error("merge plan: a chain's length is not the sum of its members'");
        rec.number = n + 1 + (uint32_t)c;
        rec.depth = merge_path_depth(r->members.data() + at, rec.members, unitig_len, depth, fwd, rev, type);
        rec.type = merge_path_type(r->members.data() + at, rec.members, type);
        at += rec.members; bases += rec.length;
    }
    if (at != r->members.size() || (!r->seq.empty() && r->seq.size() != bases)) throw std::runtime_error("merge plan: the member list or the sequences have the wrong size");
    r->alive = 0;
    for (uint32_t u = 0; u < n; u++) r->alive += !alive || alive[u];
    r->merged_unitigs = (uint32_t)at;
    r->unitigs_after = r->alive - r->merged_unitigs + (uint32_t)r->chains.size();
    r->bases_copied = r->seq.size();
}

std::string merge_duplicate_link_message(uint64_t index, int32_t a, int32_t b) {
    return "link " + std::to_string(index) + " (" + std::to_string(a) + " -> " + std::to_string(b) +
           ") is a duplicate: the merge plan needs the links among alive unitigs as a set";
}
std::string merge_unclosed_link_message(uint64_t index, int32_t a, int32_t b) {
    return "link " + std::to_string(index) + " (" + std::to_string(a) + " -> " + std::to_string(b) + ") has no reverse complement (" + std::to_string(-(int64_t)b) + " -> " +
           std::to_string(-(int64_t)a) + "): the merge plan needs a link set that is closed under reverse complement";
}

}  // namespace ac
