// `autocycler clean` (clean.rs:23-45 over unitig_graph.rs:588-721) — the host side: the input as the C ABI takes it, parse_tig_numbers, the
// checks on the two number lists, the literal sequential duplicate_unitig_by_number over the links the device gathered, the S-line colours
// of a GFA text as types, the result as the C ABI hands it out, its text and the error texts.  Plain C++, no device code; the edit itself is
// kernels_clean.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"

namespace ac {

// why a unitig is or is not in the cleaned graph (ac_cleaned_unitigs: reason; the AC_CLEAN_* values)
enum CleanReason {
    CLEAN_KEPT = 0,
    CLEAN_REMOVED = 1,             // named by remove
    CLEAN_DUPLICATED = 2,          // named by duplicate: its two copies stand in for it
    CLEAN_LOW_DEPTH = 3,           // remove_low_depth_unitigs took it
    CLEAN_KEPT_DEAD_END = 4,       // depth not above min_depth, but taking it would have left a dead end: kept
    CLEAN_ABSENT = 5,              // not alive at entry
    CLEAN_REASONS = 6
};
static const uint32_t CLEAN_ROUNDS_PER_BATCH = 8;      // rounds of the low-depth step between two read-backs (even: the work lists alternate)

struct CleanInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const double* depth = nullptr;
    const uint8_t* type = nullptr; const uint8_t* alive = nullptr;
    const uint8_t* seq_bytes = nullptr; const uint64_t* seq_begin = nullptr; uint64_t seq_total = 0;
    const uint32_t* remove = nullptr; uint32_t n_remove = 0;            // ascending (parse_tig_numbers sorts)
    const uint32_t* duplicate = nullptr; uint32_t n_duplicate = 0;      // ascending
    bool has_min_depth = false; double min_depth = 0;
    std::string name = "the graph";                                     // what "<in_gfa> does not contain tig N" calls the input
};
struct CleanResult {
    uint32_t n_unitigs = 0, n_out = 0;              // the caller's n; n + 2 per duplicated unitig (copies a, b of duplicate[i]: n + 1 + 2 i, n + 2 + 2 i)
    std::vector<uint32_t> len, copy_of;             // n_out; copy_of: 0 for the originals
    std::vector<uint8_t> alive, type, reason;       // n_out
    std::vector<double> depth;                      // n_out: a copy has half its original's
    std::vector<uint64_t> seq_begin;                // n_out: a copy points at its original's bytes (empty: no sequences were given)
    std::vector<uint8_t> seq_all;                   // the caller's bytes, for the steps that follow (empty: none were given)
    std::vector<Link> links;                        // among alive unitigs, in get_links_for_gfa order; a multiset where a loop was duplicated
    uint64_t links_in = 0;
    uint32_t rounds = 0;                            // of the low-depth step
    uint64_t count[CLEAN_REASONS] = {0, 0, 0, 0, 0, 0};
    StepStats stats;
};

// parse_tig_numbers (clean.rs:142-149): spaces removed, split at ',', each piece a u32, sorted.  s == nullptr: the option is absent, an
// empty list.  Throws std::runtime_error("failed to parse '<piece>' as a node number").
std::vector<uint32_t> clean_parse_tig_numbers(const char* s);
// Null pointers, both-or-neither, n_unitigs within a signed number, the lists ascending, and check_tig_numbers_are_valid (:129-139) for
// remove, then duplicate: every number names a unitig that is alive at entry.  Throws std::runtime_error.
void clean_prepare(const CleanInput& in);
// duplicate_unitig_by_number (:594-668) for every number of in.duplicate in turn, literally, over `gathered`: the entries among the unitigs
// left after remove that have an end in the duplicate set, in input order.  Every entry the loop deletes or creates has an end in that set
// or in a copy, so nothing else is needed.  created: the entries create_link pushed that are still there at the end, in creation order.
// Throws std::runtime_error: a number that no longer exists, or "unitig N does not contain exactly two non-self links".
void clean_duplicate_edit(const CleanInput& in, const std::vector<Link>& gathered, std::vector<Link>* created);
// the result of a graph without unitigs
void clean_empty(CleanResult* r);
// seq_all and the counts per reason
void clean_finish(const CleanInput& in, CleanResult* r);
// Unitig::from_segment_line's type (unitig.rs:79-87) of every S line of a GFA text, in file order: MergeUnitigType values
std::vector<uint8_t> clean_gfa_types(const char* text, uint64_t len);
// save_gfa's text of the edited graph under its own numbers, before any merge: the alive originals ascending, then the alive copies; no P lines
std::string clean_gfa_string(const CleanResult& r, uint32_t k, bool use_other_colour);
std::string clean_unordered_link_message(uint64_t index, int32_t a, int32_t b, int32_t prev_a);
std::string clean_no_tig_message(const std::string& name, uint32_t tig);
std::string clean_gone_message(uint32_t tig);
std::string clean_not_two_links_message(uint32_t tig);

}  // namespace ac
