// The host side of `autocycler cluster` after the tree (cluster.rs:497-661, 852-879, metrics.rs:123-187): generate_clusters, qc_clusters on
// the verdicts the device chain hands back, clustering_metrics, split_clusters, the accept walk of refine_auto_clusters, set_min_assemblies
// and the header parsing of Sequence::is_trusted / cluster_weight.  Plain C++ without the device runtime (compiled with -ffp-contract=off:
// every f64 operation is written out, one rounding each), so that tests/c_client/cluster_qc_host_check.cpp runs it alone, under sanitizers,
// with a plain loop in place of the device.  The device side is kernels_cluster_qc.inc.
//
// How the work is cut.  Every cluster of every clustering that refinement looks at is a node of the tree, and in the tree's left-first
// depth-first order the tips under a node are one contiguous range.  What depends on a node alone (size, median length, assembly count,
// trusted, `ones`, 2 * distance) is computed here, once per node, when a clustering first names it.  What depends on the matrix (is cluster x
// contained in cluster y) and the sequential chain over it run on the device, for all alternatives of a round at once: this file writes a
// ClusterQcPlan, the device (or the stand-in of the check program) answers one word per cluster of every alternative.
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "cluster_host.hpp"

namespace ac {

static const uint32_t CLUSTER_QC_NONE = 0xFFFFFFFFu;
enum : uint32_t { CLUSTER_QC_FAIL_MANUAL = 1, CLUSTER_QC_FAIL_ASSEMBLIES = 2, CLUSTER_QC_FAIL_CONTAINED = 4 };

struct ClusteringMetrics {      // metrics.rs:111-121
    uint32_t pass_cluster_count = 0, fail_cluster_count = 0, pass_contig_count = 0, fail_contig_count = 0;
    double pass_contig_fraction = 0, fail_contig_fraction = 0, cluster_balance_score = 0, cluster_tightness_score = 0, overall_clustering_score = 0;
};
struct ClusterQcItem {          // one cluster as the metrics see it, in reordered order
    uint32_t size, ones;        // ones: file names with exactly one sequence in the cluster
    double dist;                // max_pairwise_distance
    bool pass;
};
// clustering_metrics (cluster.rs:852-879) with the sums in ONE order: balance over c ascending, acc += (ones / F) * size, then / S; tightness
// over the passing c ascending, sum += (1 - sqrt(dist)) * size, then / (their total size); overall = (balance + tightness) / 2.
ClusteringMetrics cluster_metrics(const ClusterQcItem* items, uint32_t n, uint32_t n_assemblies);

// set_min_assemblies (cluster.rs:645-661) without a user's value: 1 for one assembly, else max(2, (F + 2) / 4)
uint32_t cluster_min_assemblies(uint32_t n_assemblies);
// the number of distinct values of assembly[0 .. n); throws unless they are exactly 0 .. F - 1
uint32_t cluster_assembly_count_checked(const uint32_t* assembly, uint32_t n);
// Sequence::is_trusted / Sequence::cluster_weight (sequence.rs:89-102) on a contig header
bool cluster_header_trusted(const std::string& header);
uint32_t cluster_header_weight(const std::string& header);
// assembly[i] = the index of filenames[i] by first appearance; returns the number of distinct names
uint32_t cluster_number_assemblies(const std::vector<std::string>& filenames, uint32_t* assembly);

struct ClusterSeqInputs {       // one entry per tip, in tip order
    const uint64_t* seq_len; const uint32_t* assembly; const uint32_t* cluster_weight; const uint8_t* trusted;
    uint32_t n, n_assemblies;
};
struct ClusterNodeFacts {
    uint32_t lo = 0, hi = 0;    // the node's tips in depth-first order
    uint64_t median = 0;        // median_usize of their lengths
    uint32_t assembly_count = 0;// cluster_assembly_count: per file name the largest weight, summed
    uint32_t ones = 0;
    uint8_t trusted = 0, known = 0;
    double dist = 0;            // 2 * distance
};
// The tree as the QC uses it: node ids, the depth-first tip order, every node's tip range, and the per-node facts (filled on demand).
struct ClusterQcIndex {
    const ClusterTree* t = nullptr;
    ClusterSeqInputs in{};
    std::vector<int32_t> node_of_id;       // 65536 entries, -1 = no such node
    std::vector<uint32_t> dfs_tip;         // depth-first position -> tip (row of the matrix)
    std::vector<uint32_t> lo, hi;          // per node
    std::vector<ClusterNodeFacts> facts;
    std::vector<uint32_t> scratch_max, scratch_count;      // per file name
    const ClusterNodeFacts& node(int32_t v);
};
// throws when the tree's tip count is not in.n
void cluster_qc_index(const ClusterTree& t, const ClusterSeqInputs& in, ClusterQcIndex* out);
// node indices of the ids; an id that is not in the tree, or a list that does not cover every tip exactly once (check_complete_coverage,
// cluster.rs:297-309: the reference panics), throws
std::vector<int32_t> cluster_qc_nodes_checked(const ClusterQcIndex& ix, const uint16_t* ids, uint32_t n);
// split_clusters (cluster.rs:311-335): per non-tip cluster the sorted list with that cluster replaced by its children, the lists sorted
std::vector<std::vector<uint16_t>> cluster_split_clusters(const ClusterTree& t, const std::vector<uint16_t>& clusters);

// ---- what goes to the device --------------------------------------------------------------------------------------------------------
struct ClusterQcEntity { uint32_t lo, hi, flags; };      // flags: 1 = trusted, 2 = too few assemblies (and not trusted)
struct ClusterQcAlt {
    uint32_t kpos;              // position (in the base order) of the cluster this alternative splits; NONE: the base clustering itself
    uint32_t ins0, ins1;        // the positions of the two children in the alternative's own order, ins0 < ins1
    uint32_t reserved;
    ClusterQcEntity child[2];   // child[0] is the one at ins0
};
// One evaluation: a base clustering in REORDERED order (median descending, then `tie` ascending) and alternatives that each replace one base
// cluster by its two children.  The clusters of alternative a, in ITS reordered order, are position j = 0 .. count(a) - 1:
//   j == ins0 -> child[0], j == ins1 -> child[1], else r = j - (j > ins0) - (j > ins1), base[r + (r >= kpos)].
// An entity is a base position b < n, or n + c for child c.  Whether x is contained in y (2 * contain > total) is one byte per ordered entity
// pair: base x, base y at x * n + y; with off = n * n + a * (4 n + 2): child c, base y at off + c * n + y; base x, child c at
// off + 2 n + c * n + x; child c in the other child at off + 4 n + c.  Diagonal entries and entries with the split cluster are never used.
struct ClusterQcPlan {
    uint32_t n = 0;
    std::vector<ClusterQcEntity> base;
    std::vector<ClusterQcAlt> alts;
    std::vector<int32_t> base_node;                       // host side: the node behind each base position
    std::vector<std::array<int32_t, 2>> child_node;       // ... behind child[0] / child[1] of every alternative
    uint32_t count(uint32_t a) const { return n + (alts[a].kpos != CLUSTER_QC_NONE ? 1u : 0u); }
    uint32_t stride() const { return n + 1; }
    uint64_t pair_entries() const { return (uint64_t)n * n + (uint64_t)alts.size() * (4ull * n + 2); }
    uint64_t pairs_counted() const;                       // the entries that are used
    uint32_t entity(uint32_t a, uint32_t j) const {
        const ClusterQcAlt& al = alts[a];
        if (j == al.ins0) return n;
        if (j == al.ins1) return n + 1;
        const uint32_t r = j - (j > al.ins0 ? 1u : 0u) - (j > al.ins1 ? 1u : 0u);
        return r + (r >= al.kpos ? 1u : 0u);
    }
    int32_t node_at(uint32_t a, uint32_t j) const { const uint32_t e = entity(a, j); return e < n ? base_node[e] : child_node[a][e - n]; }
};
// The answer: verdict[a * plan.stride() + j] for cluster j of alternative a = fail bits (2, 4) | (container's cluster number << 8).
using ClusterQcEvaluate = std::function<void(const ClusterQcPlan&, std::vector<uint32_t>*)>;

// ---- the result -----------------------------------------------------------------------------------------------------------------------
struct ClusterQcRecord {
    uint16_t node = 0, container = 0;
    uint32_t size = 0, assembly_count = 0, fail = 0, trusted = 0;
    uint64_t median = 0;
    double cluster_dist = 0;
};
struct ClusterQcResult {
    std::vector<uint16_t> nodes;               // the clusters' node ids as given or refined (ascending when refined or cut)
    std::vector<uint16_t> cluster_of_seq;      // per tip, the reordered cluster number
    std::vector<ClusterQcRecord> records;      // per reordered cluster
    ClusteringMetrics metrics;
    std::vector<uint32_t> round_alternatives;  // refine_auto_clusters: per round the number of alternatives,
    std::vector<double> scores;                // every alternative's overall score in walk order, round after round,
    std::vector<uint8_t> accepted;             // and whether it replaced the running best
    double start_score = 0;
    uint32_t evaluations = 0;
};
// qc_clusters (cluster.rs:511-570) on the caller's node list.  With manual clusters `evaluate` is never called.
void cluster_qc_nodes_host(ClusterQcIndex& ix, const uint16_t* cluster_nodes, uint32_t n_nodes, const uint16_t* manual, uint32_t n_manual,
                           uint32_t min_assemblies, const ClusterQcEvaluate& evaluate, ClusterQcResult* out);
// generate_clusters (cluster.rs:497-508): the cut, refine_auto_clusters (:607-630) when there are no manual clusters, the final qc_clusters
void cluster_generate_host(ClusterQcIndex& ix, double cutoff, const uint16_t* manual, uint32_t n_manual, uint32_t min_assemblies,
                           const ClusterQcEvaluate& evaluate, ClusterQcResult* out);

}  // namespace ac
