// A finished graph: a merge plan applied — the S lines in graph.unitigs order after merge_path (graph_simplification.rs:410-485), optionally
// renumbered as renumber_unitigs does (unitig_graph.rs:295-315), the L lines in get_links_for_gfa order (:333-350), the P lines over the
// printed numbers, and the text of save_gfa (:317-360) — the host side: the result as the C ABI hands it out, the input checks (a NaN depth has
// no place in the reference's comparator), the consistency checks on what the device returned, the text and the error texts.  Plain C++, no
// device code; the order itself, the gather and the relabelling are kernels_finish.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"
#include "merge_host.hpp"

namespace ac {

// ac_finished_unitig, field for field (the device writes all of it)
struct FinishedUnitigRecord {
    uint32_t number, source;      // the printed number; where it comes from: an old number, or n_unitigs + 1 + chain index
    uint64_t length, seq_off;     // bytes; first byte in the gathered sequences
    double depth;
    uint8_t type;
};

struct FinishResult {
    uint32_t n_unitigs = 0, n_chains = 0;         // of the plan
    bool renumbered = false;
    std::vector<FinishedUnitigRecord> unitigs;    // in S-line order
    std::vector<uint8_t> seq;                     // the sequences in that order, back to back
    std::vector<uint32_t> new_of_old;             // n_unitigs + n_chains: the printed number of every source, 0 = gone
    std::vector<Link> links;                      // in L-line order, printed numbers
    std::vector<uint32_t> path_seq;               // the sequences of the P lines
    std::vector<uint64_t> path_off;               // path_seq.size() + 1
    std::vector<int32_t> path_entries;            // printed numbers
    uint64_t tie_items = 0;                       // unitigs whose place the radix keys (length, first 8 bytes, depth) left open
    StepStats stats;                              // filled by the device driver
    double seconds_gather = 0;                    // of stats.seconds_device: the sequence gather alone
};

// What the caller gave, checked before any kernel reads it.  Throws std::runtime_error with the texts below.  Returns the number of unitigs
// after the merge (alive and in no chain, plus the chains).
struct FinishArrays {
    uint32_t n_unitigs = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr; const double* depth = nullptr; const uint8_t* type = nullptr;
    const uint8_t* seq_bytes = nullptr; const uint64_t* seq_begin = nullptr; uint64_t n_links = 0;
};
uint64_t finish_check_inputs(const MergeResult& plan, const FinishArrays& in, bool renumber);
// the result of a graph without unitigs
void finish_empty(FinishResult* r, bool renumber);
// what the device returned against what the plan promised; throws std::runtime_error when they contradict each other
void finish_check_result(const FinishResult& r, const MergeResult& plan, uint64_t unitigs_after);
std::string finish_nan_depth_message(uint32_t number, bool chain);
std::string finish_bad_path_entry_message(uint64_t index, int32_t entry);

// save_gfa's text of a finished graph.  seq_id / seq_length / filename / header / cluster_tag: one per P line (cluster_tag may be null: no
// CL:i tag anywhere); n_meta must be the number of P lines.
struct FinishSeqMeta { uint16_t id; uint32_t length; std::string filename, header; uint32_t cluster; };
std::string finish_gfa_string(const FinishResult& r, uint32_t k, const std::vector<FinishSeqMeta>& meta, bool use_other_colour);

}  // namespace ac
