// apply_bridges with reduce_depths, delete_unitigs_not_connected_to_anchor and remove_zero_depth_unitigs (resolve.rs:223-282) — the host
// side: the input as the C ABI takes it, the checks on the bridge records before any kernel reads them, the numbering of the bridge
// unitigs, the layout of the device's work items, the result as the C ABI hands it out, 3_bridged.gfa's text and the error texts.  Plain
// C++, no device code; the edit itself is kernels_apply.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "finish_host.hpp"
#include "graph_types.hpp"

namespace ac {

// one bridge as ac_bridge describes it (the fields the edit reads)
struct ApplyBridgeIn { int32_t start, end; uint64_t best_off, first_distinct; uint32_t best_len, n_distinct, status; };
struct ApplyInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr;
    const double* depth = nullptr; const uint32_t* anchors = nullptr; uint32_t n_anchors = 0;
    const uint8_t* seq_bytes = nullptr; const uint64_t* seq_begin = nullptr; uint64_t seq_total = 0;
    const ApplyBridgeIn* bridges = nullptr; uint32_t n_bridges = 0; const uint8_t* apply = nullptr;      // apply[b] != 0: bridge b is applied
    const int32_t* best = nullptr; uint64_t n_best = 0;                                                 // the best-path pool
    const int32_t* dist_entries = nullptr; const uint64_t* dist_off = nullptr; const uint32_t* dist_mult = nullptr; uint64_t n_dist_paths = 0, n_dist_entries = 0;
    double bridge_depth = 0;
};
// an applied bridge as the kernels read it
struct ApplyRecord {
    int32_t start, end;
    uint32_t bridge;           // its index among the caller's bridges
    uint32_t unitig;           // the index of its new unitig (number n_unitigs + 1 + unitig), or 0xFFFFFFFF: a direct link
    uint64_t created_off;      // where its created entries begin behind the surviving ones
};
struct ApplyPlan {
    std::vector<ApplyRecord> records;               // the applied bridges in the caller's order (Bridge::cmp order)
    std::vector<uint32_t> bridge_of;                // per bridge unitig: the bridge
    std::vector<uint64_t> q_begin, q_best_off;      // per bridge unitig: its first member among all members (+ the end), its first entry in the pool
    std::vector<uint64_t> vis_begin, vis_src;       // per visited distinct path: its first work item (+ the end), its first entry in the pool
    std::vector<uint32_t> vis_mult, vis_bridge;     // ... its multiplicity, its bridge
    uint64_t n_created = 0, n_members = 0, n_visits = 0;
    uint32_t n_direct = 0;
};
struct ApplyResult {
    uint32_t n_unitigs = 0, n_total = 0;            // the caller's n; n + the bridge unitigs
    std::vector<uint32_t> len;                      // n_total
    std::vector<uint8_t> alive, type;               // n_total; MergeUnitigType
    std::vector<double> depth;                      // n_total: the reduced depths, bridge_depth for the bridge unitigs
    std::vector<uint32_t> bridge_of;                // n_total - n_unitigs
    std::vector<Link> links;                        // after the edit and the removals, in get_links_for_gfa order
    std::vector<uint8_t> bridge_seq;                // the bridge unitigs' sequences (empty: none were given)
    std::vector<uint64_t> bridge_seq_off;           // n_total - n_unitigs + 1
    // the original and the bridge sequences as one array for the steps that follow (empty: none were given)
    std::vector<uint8_t> seq_all; std::vector<uint64_t> seq_begin_all;
    uint32_t applied = 0, direct = 0;
    uint64_t removed_no_anchor = 0, removed_zero_depth = 0, alive_after = 0, links_in = 0, bases_copied = 0;
    StepStats stats, stats_components;              // stats: everything the call asked of the runtime, the components' analysis included
    double seconds_copy = 0;
};

// Everything about the bridge records that can be said before a kernel reads them; throws std::runtime_error with the texts below.  The path
// entries themselves are checked on the device.
void apply_prepare(const ApplyInput& in, ApplyPlan* plan);
// the result of a graph without unitigs
void apply_empty(ApplyResult* r);
// bridge_of, the counts, and seq_all / seq_begin_all
void apply_finish(const ApplyInput& in, const ApplyPlan& plan, ApplyResult* r);
// 3_bridged.gfa: the alive originals ascending, then the alive bridge unitigs, under their own numbers; no P lines
std::string apply_gfa_string(const ApplyResult& r, uint32_t k, bool use_other_colour);
std::string apply_bridge_name(uint32_t bridge, int32_t start, int32_t end);      // "bridge 3 (5 -> -7)"
std::string apply_conflict_message(uint32_t bridge_a, int32_t start_a, int32_t end_a, uint32_t bridge_b, int32_t start_b, int32_t end_b);
std::string apply_bad_entry_message(const ApplyPlan& plan, const ApplyInput& in, bool best, uint64_t at);
std::string apply_long_bridge_message(uint32_t bridge, uint64_t bytes);

}  // namespace ac
