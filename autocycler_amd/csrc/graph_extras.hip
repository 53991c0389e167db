// The neighbouring rows of SURVEY.md §8 (f): device end repair and pairwise contig distances (neighbours.inc), the round-trip verifier
// and device decompress (kernels_verify.inc); trim's path-overlap alignment (kernels_trim.inc); resolve's path distances (kernels_resolve.inc);
// cluster's UPGMA merge loop (kernels_cluster.inc) and the QC of its clusters (kernels_cluster_qc.inc); connected components and topology
// (kernels_components.inc); the linear-path merge plan (kernels_merge.inc); sequence subsets and the paths over merged unitigs (kernels_subset.inc);
// the finished graph after a merge: order, renumbering, L lines (kernels_finish.inc); resolve's apply_bridges with its removals (kernels_apply.inc);
// clean's removal, duplication and low-depth rounds (kernels_clean.inc); trim's slices, length check and exclusion feeding the subset stages
// (kernels_trim_apply.inc); combine's graph order, offsets, per-unitig end tests and L-line order over all clusters at once (kernels_combine.inc).
#include "graph_impl.hpp"

namespace ac {

#include "neighbours.inc"      // device end repair (f-1) and pairwise contig distances (f-3)
#include "kernels_verify.inc"  // ac_verify_graph: the round-trip verifier at scale (f-4)
#include "kernels_trim.inc"    // ac_trim_paths / ac_overlap_alignment: overlap_alignment of `autocycler trim`
#include "kernels_resolve.inc" // ac_path_distances / ac_resolve_bridges: global_alignment_distance of `autocycler resolve`
#include "kernels_cluster.inc" // ac_cluster_tree_build / ac_cluster_tree_from_distances: upgma of `autocycler cluster` (f-7)
#include "kernels_cluster_qc.inc" // ac_cluster_generate / ac_cluster_qc_nodes: qc_clusters for every alternative of a refinement round (f-8)
#include "kernels_components.inc" // ac_graph_components / ac_components_from_links: connected_components, circular loops, link_count, topology (f-9)
#include "kernels_merge.inc"   // ac_graph_merge_plan / ac_merge_plan_from_links: merge_linear_paths as a plan, with its products (f-10)
#include "kernels_subset.inc"  // ac_graph_subsets / ac_subsets_from_paths / ac_subsets_merged_paths: what each cluster of sequences keeps (f-11)
#include "kernels_trim_apply.inc" // ac_trim_apply / ac_graph_trim_apply / ac_graph_trim: trim's slices, exclusion and clean_up_graph's subset on resident entries (f-15)
#include "kernels_finish.inc"  // ac_merge_finish / ac_subsets_finish: the S-line order, renumber_unitigs, the L and P lines after a merge (f-12)
#include "kernels_apply.inc"   // ac_apply_bridges / ac_graph_resolve_apply: apply_bridges, reduce_depths and the two removals of `autocycler resolve` (f-13)
#include "kernels_clean.inc"   // ac_clean_graph / ac_graph_clean: remove, duplicate and remove_low_depth_unitigs of `autocycler clean` (f-14)
#include "kernels_combine.inc" // ac_combine_graphs / ac_combine_handles: load_clusters' order, combine_clusters' offsets, topology and get_links_for_gfa of `autocycler combine` (f-16)

}  // namespace ac
