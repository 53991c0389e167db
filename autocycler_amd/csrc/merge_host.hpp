// The linear-path merge plan (merge_linear_paths, merge_path, get_merge_path_depth: graph_simplification.rs:315-371, 410-526) — the host
// side: the result as the C ABI hands it out, the seeds of the fixed sets from the path ends, the depth and type rules, the summary and
// the error texts.  Plain C++, no device code; the analysis itself is kernels_merge.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"

namespace ac {

// ac_merge_chain, field for field (the device writes members, length, member_off, seq_off and loop; merge_finish the rest)
struct MergeChainRecord {
    uint32_t number, members;
    uint64_t length, member_off, seq_off;
    double depth;
    uint8_t type, loop;
};
enum MergeFixedFlag { MERGE_FIXED_START = 1, MERGE_FIXED_END = 2 };
enum MergeUnitigType { MERGE_TYPE_OTHER = 0, MERGE_TYPE_ANCHOR = 1, MERGE_TYPE_CONSENTIG = 2, MERGE_TYPE_BRIDGE = 3 };
static const uint32_t MERGE_NOT_MERGED = 0xFFFFFFFFu;

struct MergeResult {
    uint32_t n_unitigs = 0;                   // the caller's n (alive or not) = the highest number
    std::vector<MergeChainRecord> chains;     // in the order the reference finds them
    std::vector<int32_t> members;             // signed numbers in path order, chain after chain
    std::vector<uint32_t> chain_of;           // n_unitigs; MERGE_NOT_MERGED
    std::vector<uint8_t> fixed;               // n_unitigs; MergeFixedFlag bits
    std::vector<uint8_t> seq;                 // merged sequences, addressed by seq_off (empty: none asked for)
    std::vector<Link> links;                  // the link set after the merge, ascending by (a, b)
    std::vector<uint32_t> fwd_positions, rev_positions;      // the histogram of a handle's path entries (empty: the caller's own counts)
    // filled by merge_finish
    uint32_t alive = 0, merged_unitigs = 0, unitigs_after = 0;
    uint64_t bases_copied = 0;
    // filled by the device driver
    uint64_t links_in = 0;        // how many links the plan was made from (a finished graph wants the same ones)
    StepStats stats;              // (the components' analysis inside it included)
    double seconds_copy = 0;      // of stats.seconds_device: the sequence kernel alone
};

// The seeds of get_fixed_unitig_starts_and_ends (:198-208): seed[u] gets MERGE_FIXED_START / MERGE_FIXED_END from the first and last entry
// of every path (path_ends: 2 * n_seqs signed numbers).  Throws std::runtime_error for an entry that names a dead or nonexistent unitig.
void merge_seed_fixed(uint32_t n_unitigs, const uint8_t* alive, const int32_t* path_ends, uint32_t n_seqs, std::vector<uint8_t>* seed);
// get_merge_path_depth (:501-526) of one chain: members in path order; fwd / rev: position counts per unitig or null
double merge_path_depth(const int32_t* members, uint32_t n_members, const uint32_t* unitig_len, const double* depth, const uint32_t* fwd, const uint32_t* rev,
                        const uint8_t* type);
// merge_path's type rule (:439-441)
uint8_t merge_path_type(const int32_t* members, uint32_t n_members, const uint8_t* type);
// numbers, depths, types and the totals of a result whose arrays are filled; throws std::runtime_error when the arrays contradict each other
void merge_finish(MergeResult* r, const uint32_t* unitig_len, const uint8_t* alive, const double* depth, const uint32_t* fwd, const uint32_t* rev, const uint8_t* type);
// "link 7 (3 -> -4) is a duplicate ..." / "... has no reverse complement (4 -> -3) ..."
std::string merge_duplicate_link_message(uint64_t index, int32_t a, int32_t b);
std::string merge_unclosed_link_message(uint64_t index, int32_t a, int32_t b);

}  // namespace ac
