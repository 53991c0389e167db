// Sequence subsets of a graph (save_cluster_gfa cluster.rs:794-806, clean_up_graph trim.rs:260-269): which unitigs, position counts, links
// and path ends every cluster of sequences keeps — the host side: the label and offset checks, the per-cluster sequence lists and path ends
// (work that grows with the number of sequences only), the records, the densified arrays of one cluster, the error texts.  Plain C++, no
// device code; everything that grows with the path entries or the links is kernels_subset.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"

namespace ac {

// ac_subset_cluster, field for field
struct SubsetClusterRecord {
    uint32_t seqs, unitigs;             // kept sequences; alive unitigs
    uint64_t entries, links, length;    // path entries of the kept sequences; kept links; total length of the alive unitigs
};

// The kept sequences in the order their entries are laid out for the device: cluster after cluster, ascending index inside a cluster.
struct SubsetPlan {
    std::vector<uint32_t> kept_seq;       // the sequence's index
    std::vector<uint32_t> kept_label;     // its cluster, 1..n_clusters
    std::vector<uint64_t> kept_off;       // kept_seq.size() + 1: where its entries begin among the kept entries
    uint64_t kept_entries() const { return kept_off.empty() ? 0 : kept_off.back(); }
};

struct SubsetResult {
    uint32_t n_unitigs = 0, n_clusters = 0, n_seqs = 0;
    std::vector<SubsetClusterRecord> records;            // n_clusters
    std::vector<uint64_t> unitig_off;                    // n_clusters + 1
    std::vector<uint32_t> unitigs, positions;            // alive unitig numbers ascending per cluster; entries of the kept paths on each
    std::vector<uint64_t> length_at;                     // n_clusters + 1: total length of the alive unitigs of the clusters before
    std::vector<uint64_t> link_off;                      // n_clusters + 1
    std::vector<Link> links;                             // in the input's order per cluster
    std::vector<uint64_t> seq_off;                       // n_clusters + 1
    std::vector<uint32_t> seq_index;                     // kept sequences ascending per cluster
    std::vector<uint64_t> ends_off;                      // n_clusters + 1: in pairs
    std::vector<int32_t> path_ends;                      // first, last signed entry of every non-empty kept path
    uint64_t kept_entries = 0;
    StepStats stats;      // filled by the device driver
};

// Checks n_clusters, the labels and the offsets; fills the plan and, in the result, the sequence lists and path ends.  Throws
// std::runtime_error with the texts below.
void subset_prepare(uint32_t n_seqs, const int32_t* path_entries, const uint64_t* path_off, const uint16_t* cluster_of_seq, uint32_t n_clusters, SubsetPlan* plan,
                    SubsetResult* r);
// the result without any kept entry: every product empty (offsets all 0)
void subset_empty_products(SubsetResult* r);
// the records from the offsets; throws std::runtime_error when the arrays contradict each other
void subset_finish(SubsetResult* r, const SubsetPlan& plan);
// cluster c (1-based) as the argument arrays of ac_components_from_links / ac_merge_plan_from_links: n_unitigs entries each, any may be null
void subset_dense(const SubsetResult& r, uint32_t cluster, uint8_t* alive, uint32_t* fwd_positions, uint32_t* rev_positions, double* depth);
void subset_check_cluster(const SubsetResult& r, uint32_t cluster);
// where kept entry j lies: the sequence and the index within its path
void subset_locate(const SubsetPlan& plan, uint64_t j, uint32_t* seq, uint64_t* index);
std::string subset_bad_entry_message(uint32_t seq, uint64_t index, int32_t entry, uint32_t n_unitigs);
std::string subset_dead_entry_message(uint32_t seq, uint64_t index, int32_t entry);

// ---- the paths over the merged unitigs ----
struct MergedPathsResult {
    std::vector<uint32_t> seq_index;      // the cluster's kept sequences, ascending
    std::vector<uint64_t> path_off;       // seq_index.size() + 1
    std::vector<int32_t> entries;
    uint64_t entries_before = 0;
    StepStats stats;      // filled by the device driver
};
std::string merged_paths_inside_message(uint32_t seq, bool begins, int32_t entry, uint32_t chain_number);
std::string merged_paths_length_message(uint32_t seq);

}  // namespace ac
