// The host side of `autocycler cluster` around the UPGMA merge loop (cluster.rs:195-546, 692-723): the tree from the merges, normalise_tree,
// the cutoff / manual clusters, the assignment of sequences to clusters with reorder_clusters, the containment counts and the Newick text.
// Plain C++ without the device runtime (compiled with -ffp-contract=off: every f64 operation is the reference's, one rounding each), so that
// tests/c_client/cluster_host_check.cpp runs it alone, under sanitizers.  The merge loop itself is kernels_cluster.inc.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace ac {

struct ClusterError : std::runtime_error { using std::runtime_error::runtime_error; };

struct ClusterNode {      // TreeNode (cluster.rs:195-201) with its children as indices into the tree's node array (-1 at a tip)
    uint16_t id;
    int32_t left, right;
    double distance;      // from this node to the tips
};
struct ClusterRowMerge {  // one pass of upgma's loop: rows (sequences in ascending id order) a < b, and the distance get_closest_pair compared
    uint32_t a, b;
    double distance;
};
struct ClusterMerge { uint16_t a, b; double distance; };      // the same with the clusters' ids
struct ClusterTree {
    std::vector<ClusterNode> nodes;      // a built tree: the tips in sequence order, then the internal nodes in merge order
    int32_t root = -1;
    std::vector<ClusterMerge> merges;    // (empty for a tree the caller supplied)
    std::vector<int32_t> post_order;     // every node after its children
    std::vector<int32_t> tips;           // node indices of the tips, ascending
};

// n == 0, ids that do not strictly ascend, or max id + n - 1 > 65535 (upgma's u16 node counter, cluster.rs:402/422, would overflow)
void cluster_check_ids(const uint16_t* ids, uint32_t n);
// upgma's tree (cluster.rs:399-457) from its n - 1 merges; normalise != 0: normalise_tree (:483-494) afterwards
void cluster_tree_from_merges(const uint16_t* ids, uint32_t n, const std::vector<ClusterRowMerge>& merges, bool normalise, ClusterTree* out);
// a caller's tree: checked to be one binary tree that holds every node once, with distinct ids
void cluster_tree_from_nodes(const ClusterNode* nodes, uint32_t n_nodes, int32_t root, ClusterTree* out);
// automatic_clustering (n_manual == 0) / manual_clustering (cluster.rs:219-271): node ids, ascending.  Nested manual clusters throw.
std::vector<uint16_t> cluster_cut(const ClusterTree& t, double cutoff, const uint16_t* manual, uint32_t n_manual);
// The first half of qc_clusters (cluster.rs:522-546): cluster k + 1 = the tips under node cluster_nodes[k] (a later node overrides an
// earlier one), then reorder_clusters (:882-903, median_usize misc.rs:423-430).  seq_len / cluster_of_seq: one entry per tip, in tip order;
// a tip under none of the nodes keeps 0.  cluster_dist[c - 1] = max_pairwise_distance (:208-217) of the node behind the REORDERED cluster c
// (-1 for a number no sequence carries any more).  Returns the number of clusters (the largest number in use).
uint32_t cluster_assign(const ClusterTree& t, const uint16_t* cluster_nodes, uint32_t n, const uint64_t* seq_len, uint16_t* cluster_of_seq,
                        double* cluster_dist);
// The two counts of cluster_is_contained_in_another (cluster.rs:705-717) for every ordered pair of different clusters (x, y) at
// [(x - 1) * n_clusters + (y - 1)]; asym = the S x S matrix of pairwise_contig_distances.  A sequence of cluster 0 takes no part.
void cluster_containment(const double* asym, uint32_t n, const uint16_t* cluster_of_seq, uint32_t n_clusters, double cutoff,
                         uint64_t* contain_count, uint64_t* total_count);
// tree_to_newick (cluster.rs:381-392); file_form: the line save_tree_to_newick writes (:363-378).  tip_names: one per tip in tip order, or
// NULL (the tip's id).
std::string cluster_newick(const ClusterTree& t, const char* const* tip_names, bool file_form);
// an f64 as Rust's `{}` prints it: the shortest digits that read back as the same value, never an exponent
std::string cluster_format_f64(double x);

}  // namespace ac
