"""ctypes binding of libautocycler_hip.so (include/autocycler_hip.h).

There is no Python or CPU implementation behind these calls: if the HIP library has not been built
(`python -c 'import __graft_entry__ as g; g.build()'` or `make -C autocycler_amd/csrc`) importing the
package still works, but any graph build raises HipLibraryMissing."""
import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libautocycler_hip.so"


class HipLibraryMissing(RuntimeError):
    pass


class AutocyclerError(RuntimeError):
    """The text the reference would hand to quit_with_error (misc.rs:131-137)."""


class SeqView(C.Structure):
    _fields_ = [("fwd", C.c_char_p), ("length", C.c_uint32), ("id", C.c_uint16)]


class Position(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("seq_id_and_strand", C.c_uint16)]


class Link(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32)]      # signed unitig numbers: +n forward strand, -n reverse (ABI 7)


class Stats(C.Structure):
    _fields_ = [("unitigs", C.c_uint32), ("links_one_way", C.c_uint64), ("total_length", C.c_uint64)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("h2d", "pack", "insert", "collect_sort", "degree", "segment", "minkey",
                                          "rank", "paths", "links", "seqs", "d2h", "total_device", "expand",
                                          "insert_kernel_ms")] + \
               [(n, C.c_uint64) for n in ("insert_positions", "table_capacity", "n_distinct", "n_path_entries")] + \
               [("simplify_passes", C.c_uint32), ("insert_launches", C.c_uint32), ("insert_real", C.c_uint64),
                ("analysis", C.c_double), ("finalize", C.c_double), ("n_candidates", C.c_uint32), ("n_levels", C.c_uint32),
                ("fragments", C.c_double), ("union_pack", C.c_double), ("union_insert", C.c_double),
                ("n_local_distinct", C.c_uint64), ("n_fragments", C.c_uint64), ("fragment_bytes", C.c_uint64),
                ("upload_device_ms", C.c_double), ("path_runs_copied", C.c_uint64), ("path_entries_walked", C.c_uint64), ("position_retries", C.c_uint64), ("n_candidates_owned", C.c_uint32),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("n_degrees_open", C.c_uint64), ("sort_retries", C.c_uint64), ("insert_rest_known", C.c_double), ("insert_rest_sampled", C.c_double), ("path_stretches", C.c_uint64),
                ("expand_sparse_sweeps", C.c_uint32), ("expand_sparse_start", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TrimSlice(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("status", "begin", "end", "trimmed_length")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TrimResult(C.Structure):
    _fields_ = [("start_end", TrimSlice), ("hairpin", TrimSlice), ("hairpin_start_trimmed", C.c_uint32), ("hairpin_end_trimmed", C.c_uint32)]

    def as_dict(self):
        return dict(start_end=self.start_end.as_dict(), hairpin=self.hairpin.as_dict(),
                    hairpin_start_trimmed=self.hairpin_start_trimmed, hairpin_end_trimmed=self.hairpin_end_trimmed)


class TrimSummary(C.Structure):
    _fields_ = [("size", C.c_uint64), ("c_se", C.c_uint32), ("c_hp", C.c_uint32), ("chosen", C.c_uint32), ("launches", C.c_uint32),
                ("cells", C.c_uint64), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class AlignmentPiece(C.Structure):
    _fields_ = [("a_unitig", C.c_int32), ("a_index", C.c_uint32), ("b_unitig", C.c_int32), ("b_index", C.c_uint32)]


ALIGN_GAP, ALIGN_NONE = 0, 0xFFFFFFFF


class Bridge(C.Structure):      # ac_bridge
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("depth", C.c_uint32), ("n_distinct", C.c_uint32), ("best_off", C.c_uint64),
                ("best_total", C.c_uint64), ("first_distinct", C.c_uint64), ("best_len", C.c_uint32), ("status", C.c_uint32),
                ("conflicting", C.c_uint32), ("culled", C.c_uint32), ("cull_rank", C.c_uint32), ("reserved", C.c_uint32)]


class ResolveSummary(C.Structure):
    _fields_ = [("size", C.c_uint64), ("jobs", C.c_uint64), ("jobs_not_launched", C.c_uint64), ("cells", C.c_uint64), ("largest_job_cells", C.c_uint64),
                ("launches", C.c_uint32), ("reserved", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n not in ("size", "reserved")}


class Component(C.Structure):      # ac_component
    _fields_ = [("first", C.c_uint32), ("unitigs", C.c_uint32), ("length", C.c_uint64), ("links_all", C.c_uint64), ("links_one_way", C.c_uint64),
                ("open_ends", C.c_uint32), ("marked", C.c_uint32), ("circular_loop", C.c_uint8)]


class ComponentsSummary(C.Structure):      # ac_components_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "unitigs", "components", "topology")] + \
               [(n, C.c_uint64) for n in ("links_all", "links_one_way", "total_length")] + \
               [("launches", C.c_uint32), ("read_backs", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class MergeChain(C.Structure):      # ac_merge_chain
    _fields_ = [("number", C.c_uint32), ("members", C.c_uint32), ("length", C.c_uint64), ("member_off", C.c_uint64), ("seq_off", C.c_uint64), ("depth", C.c_double),
                ("type", C.c_uint8), ("loop", C.c_uint8)]


class MergeSummary(C.Structure):      # ac_merge_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "chains", "merged_unitigs", "unitigs_after")] + [("links_after", C.c_uint64), ("bases_copied", C.c_uint64)] + \
               [("launches", C.c_uint32), ("read_backs", C.c_uint32), ("seconds_device", C.c_double), ("seconds_copy", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class SubsetCluster(C.Structure):      # ac_subset_cluster
    _fields_ = [("seqs", C.c_uint32), ("unitigs", C.c_uint32), ("entries", C.c_uint64), ("links", C.c_uint64), ("length", C.c_uint64)]


class SubsetsSummary(C.Structure):      # ac_subsets_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "clusters", "sequences_kept", "n_unitigs")] + [(n, C.c_uint64) for n in ("entries_kept", "unitigs", "links")] + \
               [("launches", C.c_uint32), ("read_backs", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class MergedPathsSummary(C.Structure):      # ac_merged_paths_summary
    _fields_ = [("size", C.c_uint32), ("sequences", C.c_uint32), ("entries_before", C.c_uint64), ("entries_after", C.c_uint64),
                ("launches", C.c_uint32), ("read_backs", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class FinishedUnitig(C.Structure):      # ac_finished_unitig
    _fields_ = [("number", C.c_uint32), ("source", C.c_uint32), ("length", C.c_uint64), ("seq_off", C.c_uint64), ("depth", C.c_double), ("type", C.c_uint8)]


class FinishedSummary(C.Structure):      # ac_finished_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "unitigs", "renumbered", "launches", "read_backs")] + \
               [(n, C.c_uint64) for n in ("links", "path_entries", "bases", "tie_items")] + [("seconds_device", C.c_double), ("seconds_gather", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class AppliedSummary(C.Structure):      # ac_applied_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "bridges_applied", "direct_links", "launches", "launches_components", "read_backs")] + \
               [(n, C.c_uint64) for n in ("removed_no_anchor", "removed_zero_depth", "links_in", "links_out", "bases_copied")] + \
               [("seconds_device", C.c_double), ("seconds_copy", C.c_double), ("seconds_components", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class CleanedSummary(C.Structure):      # ac_cleaned_summary
    _fields_ = [(n, C.c_uint32) for n in ("size", "unitigs_in", "unitigs_out", "rounds", "rounds_per_batch", "launches", "read_backs", "reserved")] + \
               [(n, C.c_uint64) for n in ("kept", "removed", "duplicated", "low_depth", "kept_dead_end", "absent", "links_in", "links_out")] + [("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n not in ("size", "reserved")}


class TrimmedRecord(C.Structure):      # ac_trimmed_record
    _fields_ = [("begin", C.c_uint32), ("end", C.c_uint32), ("length", C.c_uint64), ("trimmed", C.c_uint32), ("excluded", C.c_uint32)]


class TrimmedSummary(C.Structure):      # ac_trimmed_summary
    _fields_ = [("size", C.c_uint32), ("chosen", C.c_uint32), ("c_se", C.c_uint32), ("c_hp", C.c_uint32), ("sequences", C.c_uint32), ("trimmed", C.c_uint32),
                ("excluded", C.c_uint32), ("rejected", C.c_uint32), ("unitigs_in", C.c_uint32), ("unitigs_alive", C.c_uint32), ("launches", C.c_uint32),
                ("read_backs", C.c_uint32), ("median", C.c_uint64), ("mad", C.c_uint64), ("min_length", C.c_uint64), ("max_length", C.c_uint64),
                ("entries_kept", C.c_uint64), ("links", C.c_uint64), ("seconds_device", C.c_double), ("align_launches", C.c_uint32), ("reserved", C.c_uint32),
                ("align_cells", C.c_uint64), ("align_seconds_device", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("size", "reserved")}


class CombinedCluster(C.Structure):      # ac_combined_cluster
    _fields_ = [("input_index", C.c_uint32), ("unitigs", C.c_uint32), ("length", C.c_uint64), ("links", C.c_uint64), ("offset", C.c_uint64), ("max_number", C.c_uint32),
                ("topology", C.c_uint32), ("has_read_depth", C.c_uint32), ("reserved", C.c_uint32), ("read_depth", C.c_double)]


class CombinedUnitig(C.Structure):      # ac_combined_unitig
    _fields_ = [("graph", C.c_uint32), ("index", C.c_uint32), ("number", C.c_uint32), ("length", C.c_uint32), ("depth", C.c_double), ("read_depth", C.c_double),
                ("has_read_depth", C.c_uint8), ("flags", C.c_uint8), ("type", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class CombinedSummary(C.Structure):      # ac_combined_summary
    _fields_ = [("size", C.c_uint32), ("graphs", C.c_uint32), ("bases", C.c_uint64), ("unitigs", C.c_uint64), ("links", C.c_uint64), ("fully_resolved", C.c_uint32),
                ("with_reads", C.c_uint32), ("launches", C.c_uint32), ("read_backs", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}
        d["fully_resolved"], d["with_reads"] = bool(d["fully_resolved"]), bool(d["with_reads"])
        return d


class ClusterNode(C.Structure):      # ac_cluster_node
    _fields_ = [("id", C.c_uint16), ("left", C.c_int32), ("right", C.c_int32), ("distance", C.c_double)]


class ClusterMerge(C.Structure):      # ac_cluster_merge
    _fields_ = [("a", C.c_uint16), ("b", C.c_uint16), ("distance", C.c_double)]


class ClusterSummary(C.Structure):
    _fields_ = [("n_seqs", C.c_uint32), ("launches", C.c_uint32), ("rescans", C.c_uint64), ("compares", C.c_uint64), ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ClusterQcRecord(C.Structure):      # ac_cluster_qc_record
    _fields_ = [("node", C.c_uint16), ("container", C.c_uint16), ("size", C.c_uint32), ("assembly_count", C.c_uint32), ("fail", C.c_uint32),
                ("trusted", C.c_uint32), ("reserved", C.c_uint32), ("median_length", C.c_uint64), ("cluster_dist", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class ClusteringMetrics(C.Structure):      # ac_clustering_metrics
    _fields_ = [(n, C.c_uint32) for n in ("pass_cluster_count", "fail_cluster_count", "pass_contig_count", "fail_contig_count")] + \
               [(n, C.c_double) for n in ("pass_contig_fraction", "fail_contig_fraction", "cluster_balance_score", "cluster_tightness_score",
                                          "overall_clustering_score")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ClusterQcSummary(C.Structure):      # ac_cluster_qc_summary
    _fields_ = [(n, C.c_uint32) for n in ("n_seqs", "n_clusters", "rounds", "evaluations", "pair_batches", "launches", "readbacks", "reserved")] + \
               [(n, C.c_uint64) for n in ("alternatives", "node_pairs", "bytes_read_back")] + [("seconds", C.c_double), ("start_score", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class DepthGraph(C.Structure):      # ac_depth_graph
    _fields_ = [("seq_bytes", C.c_void_p), ("seq_begin", C.c_void_p), ("seq_len", C.c_void_p), ("n_unitigs", C.c_uint32),
                ("links", C.c_void_p), ("n_links", C.c_uint64)]


class DepthTotals(C.Structure):
    _fields_ = [("size", C.c_uint64)] + \
               [(n, C.c_uint64) for n in ("reads", "rejected_reads", "read_bases", "span_bases", "span_kmers", "hits", "distinct_kmers", "repeat_kmers",
                                          "table_slots")] + [("batches", C.c_uint32), ("launches", C.c_uint32), ("seconds_device", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int)      # ac_allreduce_fn

EXPORTS = ["ac_compress_build", "ac_compress_build_multi", "ac_multi_info_get", "ac_compress_build_device", "ac_pack_text", "ac_text_size", "ac_layout_text", "ac_kmer_count",
           "ac_stats_pre", "ac_stats_post", "ac_unitig_count", "ac_unitig", "ac_unitigs_bulk", "ac_paths_bulk", "ac_unitig_positions", "ac_links",
           "ac_path", "ac_timings_get", "ac_timings_get_sized", "ac_free", "ac_gfa_string", "ac_string_free", "ac_last_error",
           "ac_device_count", "ac_max_kmer", "ac_version", "ac_abi_version", "ac_set_host_side_device", "ac_source_hash", "ac_set_stage_timing", "ac_random_access_ceilings", "ac_random_access_ceilings_at", "ac_release_memory", "ac_end_repair_device", "ac_pairwise_distances", "ac_trim_paths", "ac_trim_path_slices", "ac_overlap_alignment", "ac_trim_max_unitigs", "ac_resolve_bridges", "ac_resolve_bridge_paths", "ac_path_distances", "ac_resolve_anchors", "ac_resolve_bridge_records", "ac_resolve_best_paths", "ac_resolve_distinct_paths", "ac_resolve_summary_get_sized", "ac_resolve_max_path", "ac_resolve_free", "ac_graph_components", "ac_components_from_links", "ac_components_records", "ac_components_of_unitig", "ac_components_members", "ac_components_unitig_flags", "ac_components_summary_get_sized", "ac_topology_name", "ac_components_free", "ac_graph_merge_plan", "ac_merge_plan_from_links", "ac_merge_chains", "ac_merge_members", "ac_merge_chain_of_unitig", "ac_merge_fixed_flags", "ac_merge_sequences", "ac_merge_links", "ac_merge_summary_get_sized", "ac_merge_free", "ac_graph_subsets", "ac_subsets_from_paths", "ac_subsets_records", "ac_subsets_unitigs", "ac_subsets_links", "ac_subsets_seqs", "ac_subsets_path_ends", "ac_subsets_dense", "ac_subsets_summary_get_sized", "ac_subsets_free", "ac_subsets_components", "ac_subsets_merge_plan", "ac_subsets_merged_paths", "ac_merged_paths_get", "ac_merged_paths_summary_get_sized", "ac_merged_paths_free", "ac_merge_finish", "ac_subsets_finish", "ac_finished_unitigs", "ac_finished_sequences", "ac_finished_new_of_old", "ac_finished_links", "ac_finished_paths", "ac_finished_summary_get_sized", "ac_finished_free", "ac_finished_gfa_string", "ac_finished_to_graph", "ac_apply_bridges", "ac_graph_resolve_apply", "ac_applied_unitigs", "ac_applied_bridge_of", "ac_applied_links", "ac_applied_bridge_sequences", "ac_applied_summary_get_sized", "ac_applied_free", "ac_applied_merge_plan", "ac_applied_finish", "ac_applied_gfa_string", "ac_resolve_graphs", "ac_clean_graph", "ac_graph_clean", "ac_cleaned_unitigs", "ac_cleaned_links", "ac_cleaned_summary_get_sized", "ac_cleaned_free", "ac_cleaned_merge_plan", "ac_cleaned_finish", "ac_cleaned_gfa_string", "ac_parse_tig_numbers", "ac_gfa_segment_types", "ac_clean_gfa", "ac_clean", "ac_trim_apply", "ac_graph_trim_apply", "ac_graph_trim", "ac_trimmed_records", "ac_trimmed_summary_get_sized", "ac_trimmed_free", "ac_trimmed_subsets", "ac_trimmed_finish", "ac_trimmed_yaml_string", "ac_trim_gfa", "ac_trim_dir", "ac_resolve_dir", "ac_combine_graphs", "ac_combine_handles", "ac_combined_clusters", "ac_combined_unitigs", "ac_combined_links", "ac_combined_summary_get_sized", "ac_combined_free", "ac_combined_gfa_string", "ac_combined_fasta_string", "ac_combined_yaml_string", "ac_combined_depth_lines", "ac_combine_gfas", "ac_combine", "ac_gfa2fasta_string", "ac_gfa2fasta", "ac_cluster_tree_build", "ac_cluster_tree_from_distances", "ac_cluster_tree_from_nodes", "ac_cluster_nodes", "ac_cluster_merges", "ac_cluster_summary_get_sized", "ac_cluster_free", "ac_cluster_max_seqs", "ac_cluster_cut", "ac_cluster_assign", "ac_cluster_containment", "ac_cluster_newick", "ac_cluster_generate", "ac_cluster_qc_nodes", "ac_cluster_qc_clusters", "ac_cluster_qc_assignment", "ac_cluster_qc_records", "ac_cluster_qc_metrics", "ac_cluster_qc_trace", "ac_cluster_qc_summary_get_sized", "ac_cluster_qc_free", "ac_cluster_min_assemblies", "ac_cluster_seq_inputs", "ac_depth_begin", "ac_depth_begin_handles", "ac_depth_add_reads", "ac_depth_add_fastq", "ac_depth_totals_get", "ac_depth_kmer_counts", "ac_depth_finish", "ac_depth_free", "ac_selftest_primitives", "ac_selftest_scan", "ac_selftest_radix", "ac_selftest_segments", "ac_selftest_sort_cmp", "ac_selftest_scan_pool", "ac_selftest_wave", "ac_selftest_fills", "ac_selftest_fill_order", "ac_selftest_readback", "ac_selftest_scalar_chain", "ac_selftest_arena", "ac_selftest_launch", "ac_selftest_atomics", "ac_selftest_side_order", "ac_selftest_event_ring", "ac_verify_graph", "ac_verify_graph_device", "ac_graph_from_gfa", "ac_graph_kmer_size", "ac_graph_seq_info", "ac_decompress_seq", "ac_decompress_device", "ac_decompress",
           "ac_shard_begin", "ac_shard_fragment_sizes", "ac_shard_fragments_export", "ac_shard_build_union", "ac_shard_fragment_packed_words", "ac_shard_fragments_export_packed", "ac_shard_build_union_packed",
           "ac_shard_unitig_count", "ac_shard_table_capacity", "ac_shard_bitmap_words", "ac_shard_bitmap_export", "ac_shard_build_novel", "ac_shard_sib_words", "ac_shard_sib_export", "ac_shard_degrees",
           "ac_shard_degree_bytes", "ac_multi_info_get_sized", "ac_shard_links_export", "ac_shard_links_import",
           "ac_shard_query_count", "ac_shard_query_key_words", "ac_shard_queries_export", "ac_shard_answer", "ac_shard_walk", "ac_shard_queries_route", "ac_shard_walk_routed", "ac_shard_local_distinct", "ac_shard_set_distinct_upper_bound", "ac_shard_distinct_count", "ac_shard_degrees_export", "ac_shard_build_graph", "ac_gfa_string_parts", "ac_shard_reduce_export", "ac_shard_reduce_import", "ac_shard_finish", "ac_shard_set_allreduce", "ac_device_copy",
           "ac_shard_path_entries", "ac_shard_paths_export", "ac_shard_free", "ac_graph_set_paths", "ac_graph_seq_count", "ac_path_counts",
           "ac_seqs_load", "ac_seqs_from_raw", "ac_seqs_count", "ac_seqs_assembly_count", "ac_seqs_views", "ac_seqs_get",
           "ac_seqs_repair_seconds", "ac_seqs_metrics_yaml", "ac_seqs_free", "ac_compress_seqs", "ac_compress_dir", "ac_compress_dir_multi"]

_libs = {}


def load_library(path=None):
    path = Path(path) if path else LIB_PATH
    key = str(path)
    if key in _libs:
        return _libs[key]
    if not path.exists():
        raise HipLibraryMissing(f"{path} not found: build the HIP extension first (make -C autocycler_amd/csrc). "
                                "There is no CPU fallback.")
    try:
        if os.environ.get("AC_NO_TORCH"):      # torch-free processes (tools/ab_knobs.py): the system HIP runtime is the only one
            raise ImportError
        # PyTorch bundles its own HIP runtime; when ours (/opt/rocm) is loaded first, torch later finds "no HIP GPUs".
        # Importing torch first makes the dynamic loader resolve our libamdhip64 dependency to the copy torch loaded.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(key)
    lib.ac_last_error.restype = C.c_char_p
    lib.ac_version.restype = C.c_char_p
    lib.ac_source_hash.restype = C.c_char_p
    lib.ac_kmer_count.restype = C.c_uint64
    lib.ac_kmer_count.argtypes = [C.c_void_p]
    lib.ac_stats_pre.restype = Stats
    lib.ac_stats_pre.argtypes = [C.c_void_p]
    lib.ac_stats_post.restype = Stats
    lib.ac_stats_post.argtypes = [C.c_void_p]
    lib.ac_unitig_count.restype = C.c_uint32
    lib.ac_unitig_count.argtypes = [C.c_void_p]
    lib.ac_max_kmer.restype = C.c_uint32
    lib.ac_text_size.restype = C.c_uint64
    lib.ac_free.argtypes = [C.c_void_p]
    lib.ac_string_free.argtypes = [C.c_void_p]
    lib.ac_unitig.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.ac_unitig_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.POINTER(Position)), C.POINTER(C.c_uint32)]
    lib.ac_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_path.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_uint32)]
    lib.ac_timings_get.argtypes = [C.c_void_p, C.POINTER(Timings)]
    lib.ac_shard_unitig_count.restype = C.c_uint32
    lib.ac_shard_unitig_count.argtypes = [C.c_void_p]
    lib.ac_shard_fragment_packed_words.restype = C.c_uint64
    lib.ac_shard_fragment_packed_words.argtypes = [C.c_void_p, C.c_uint64]
    lib.ac_shard_local_distinct.restype = C.c_uint64
    lib.ac_shard_local_distinct.argtypes = [C.c_void_p]
    lib.ac_shard_set_distinct_upper_bound.argtypes = [C.c_void_p, C.c_uint64]
    lib.ac_shard_set_distinct_upper_bound.restype = None
    lib.ac_shard_distinct_count.restype = C.c_uint64
    lib.ac_shard_distinct_count.argtypes = [C.c_void_p]
    lib.ac_shard_path_entries.restype = C.c_uint64
    lib.ac_shard_path_entries.argtypes = [C.c_void_p]
    lib.ac_shard_free.argtypes = [C.c_void_p]
    for name in ("ac_shard_table_capacity", "ac_shard_bitmap_words", "ac_shard_query_count", "ac_shard_sib_words", "ac_shard_degree_bytes"):
        getattr(lib, name).restype = C.c_uint64
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.ac_shard_query_key_words.restype = C.c_uint32
    lib.ac_shard_query_key_words.argtypes = [C.c_void_p]
    lib.ac_graph_seq_count.restype = C.c_uint32
    lib.ac_graph_seq_count.argtypes = [C.c_void_p]
    lib.ac_trim_max_unitigs.restype = C.c_uint32
    lib.ac_trim_max_unitigs.argtypes = []
    lib.ac_trim_paths.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.c_int, C.POINTER(TrimResult), C.POINTER(TrimSummary)]
    lib.ac_trim_path_slices.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_int,
                                        C.POINTER(TrimResult), C.POINTER(TrimSummary)]
    lib.ac_overlap_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_int, C.c_int,
                                         C.POINTER(AlignmentPiece), C.POINTER(C.c_uint32)]
    lib.ac_resolve_max_path.restype = C.c_uint32
    lib.ac_resolve_max_path.argtypes = []
    lib.ac_resolve_bridges.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_resolve_bridge_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_path_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    lib.ac_resolve_anchors.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
    lib.ac_resolve_bridge_records.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Bridge)), C.POINTER(C.c_uint32)]
    lib.ac_resolve_best_paths.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_uint64)]
    lib.ac_resolve_distinct_paths.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32)),
                                              C.POINTER(C.c_uint64)]
    lib.ac_resolve_summary_get_sized.restype = C.c_size_t
    lib.ac_resolve_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(ResolveSummary), C.c_size_t]
    lib.ac_resolve_free.argtypes = [C.c_void_p]
    lib.ac_resolve_free.restype = None
    lib.ac_graph_components.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_components_from_links.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_components_records.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Component)), C.POINTER(C.c_uint32)]
    lib.ac_components_of_unitig.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32))]
    lib.ac_components_members.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32))]
    lib.ac_components_unitig_flags.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
    lib.ac_components_summary_get_sized.restype = C.c_size_t
    lib.ac_components_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(ComponentsSummary), C.c_size_t]
    lib.ac_topology_name.restype = C.c_char_p
    lib.ac_topology_name.argtypes = [C.c_uint32]
    lib.ac_components_free.argtypes = [C.c_void_p]
    lib.ac_components_free.restype = None
    lib.ac_graph_merge_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_merge_plan_from_links.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_merge_chains.argtypes = [C.c_void_p, C.POINTER(C.POINTER(MergeChain)), C.POINTER(C.c_uint32)]
    lib.ac_merge_members.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_uint64)]
    lib.ac_merge_chain_of_unitig.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32))]
    lib.ac_merge_fixed_flags.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
    lib.ac_merge_sequences.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
    lib.ac_merge_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_merge_summary_get_sized.restype = C.c_size_t
    lib.ac_merge_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(MergeSummary), C.c_size_t]
    lib.ac_merge_free.argtypes = [C.c_void_p]
    lib.ac_merge_free.restype = None
    lib.ac_graph_subsets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_subsets_from_paths.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
                                          C.POINTER(C.c_void_p)]
    lib.ac_subsets_records.argtypes = [C.c_void_p, C.POINTER(C.POINTER(SubsetCluster)), C.POINTER(C.c_uint32)]
    lib.ac_subsets_unitigs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)),
                                       C.POINTER(C.POINTER(C.c_uint32))]
    lib.ac_subsets_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(Link))]
    lib.ac_subsets_seqs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32))]
    lib.ac_subsets_path_ends.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_int32))]
    lib.ac_subsets_dense.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ac_subsets_summary_get_sized.restype = C.c_size_t
    lib.ac_subsets_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(SubsetsSummary), C.c_size_t]
    lib.ac_subsets_free.argtypes = [C.c_void_p]
    lib.ac_subsets_free.restype = None
    lib.ac_subsets_components.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_subsets_merge_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_subsets_merged_paths.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_merged_paths_get.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_int32))]
    lib.ac_merged_paths_summary_get_sized.restype = C.c_size_t
    lib.ac_merged_paths_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(MergedPathsSummary), C.c_size_t]
    lib.ac_merged_paths_free.argtypes = [C.c_void_p]
    lib.ac_merged_paths_free.restype = None
    lib.ac_merge_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_subsets_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_finished_unitigs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(FinishedUnitig)), C.POINTER(C.c_uint32)]
    lib.ac_finished_sequences.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
    lib.ac_finished_new_of_old.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64)]
    lib.ac_finished_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_finished_paths.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_int32))]
    lib.ac_finished_summary_get_sized.restype = C.c_size_t
    lib.ac_finished_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(FinishedSummary), C.c_size_t]
    lib.ac_finished_free.argtypes = [C.c_void_p]
    lib.ac_finished_free.restype = None
    lib.ac_finished_gfa_string.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_finished_to_graph.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ac_cluster_max_seqs.restype = C.c_uint32
    lib.ac_cluster_max_seqs.argtypes = []
    lib.ac_cluster_tree_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ac_cluster_tree_from_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_apply_bridges.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_graph_resolve_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_applied_unitigs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_double)),
                                       C.POINTER(C.POINTER(C.c_uint8))]
    lib.ac_applied_bridge_of.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32)]
    lib.ac_applied_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_applied_bridge_sequences.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    lib.ac_applied_summary_get_sized.restype = C.c_size_t
    lib.ac_applied_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(AppliedSummary), C.c_size_t]
    lib.ac_applied_free.argtypes = [C.c_void_p]
    lib.ac_applied_free.restype = None
    lib.ac_applied_merge_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_applied_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_applied_gfa_string.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_clean_graph.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_uint32, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_graph_clean.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_cleaned_unitigs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_double)),
                                       C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8))]
    lib.ac_cleaned_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_cleaned_summary_get_sized.restype = C.c_size_t
    lib.ac_cleaned_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(CleanedSummary), C.c_size_t]
    lib.ac_cleaned_free.argtypes = [C.c_void_p]
    lib.ac_cleaned_free.restype = None
    lib.ac_cleaned_merge_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_cleaned_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_cleaned_gfa_string.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_parse_tig_numbers.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    lib.ac_gfa_segment_types.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    lib.ac_clean_gfa.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_clean.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int]
    lib.ac_trim_apply.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                  C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_graph_trim_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_graph_trim.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_trimmed_records.argtypes = [C.c_void_p, C.POINTER(C.POINTER(TrimmedRecord)), C.POINTER(C.c_uint32)]
    lib.ac_trimmed_summary_get_sized.restype = C.c_size_t
    lib.ac_trimmed_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(TrimmedSummary), C.c_size_t]
    lib.ac_trimmed_free.restype = None
    lib.ac_trimmed_free.argtypes = [C.c_void_p]
    lib.ac_trimmed_subsets.restype = C.c_void_p
    lib.ac_trimmed_subsets.argtypes = [C.c_void_p]
    lib.ac_trimmed_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_trimmed_yaml_string.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_trim_gfa.argtypes = [C.c_char_p, C.c_uint64, C.c_double, C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                C.POINTER(TrimmedSummary)]
    lib.ac_trim_dir.argtypes = [C.c_char_p, C.c_double, C.c_uint32, C.c_double, C.c_int]
    lib.ac_resolve_dir.argtypes = [C.c_char_p, C.c_int]
    lib.ac_combine_graphs.argtypes = [C.c_uint32] + [C.c_void_p] * 11 + [C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_combine_handles.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_combined_clusters.argtypes = [C.c_void_p, C.POINTER(C.POINTER(CombinedCluster)), C.POINTER(C.c_uint32)]
    lib.ac_combined_unitigs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(CombinedUnitig)), C.POINTER(C.c_uint64)]
    lib.ac_combined_links.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Link)), C.POINTER(C.c_uint64)]
    lib.ac_combined_summary_get_sized.restype = C.c_size_t
    lib.ac_combined_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(CombinedSummary), C.c_size_t]
    lib.ac_combined_free.argtypes = [C.c_void_p]
    lib.ac_combined_free.restype = None
    for f in (lib.ac_combined_gfa_string, lib.ac_combined_fasta_string, lib.ac_combined_yaml_string, lib.ac_combined_depth_lines):
        f.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.ac_combine_gfas.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(CombinedSummary)]
    lib.ac_combine.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_gfa2fasta_string.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ac_gfa2fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
    lib.ac_resolve_graphs.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    lib.ac_cluster_tree_from_nodes.argtypes = [C.POINTER(ClusterNode), C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ac_cluster_nodes.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ClusterNode)), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    lib.ac_cluster_merges.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ClusterMerge)), C.POINTER(C.c_uint32)]
    lib.ac_cluster_summary_get_sized.restype = C.c_size_t
    lib.ac_cluster_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(ClusterSummary), C.c_size_t]
    lib.ac_cluster_free.argtypes = [C.c_void_p]
    lib.ac_cluster_free.restype = None
    lib.ac_cluster_cut.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.ac_cluster_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.ac_cluster_containment.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    lib.ac_cluster_newick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    qc_in = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32]
    lib.ac_cluster_generate.argtypes = qc_in + [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_cluster_qc_nodes.argtypes = qc_in + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_cluster_qc_clusters.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.c_uint32)]
    lib.ac_cluster_qc_assignment.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.c_uint32)]
    lib.ac_cluster_qc_records.argtypes = [C.c_void_p, C.POINTER(C.POINTER(ClusterQcRecord)), C.POINTER(C.c_uint32)]
    lib.ac_cluster_qc_metrics.argtypes = [C.c_void_p, C.POINTER(ClusteringMetrics)]
    lib.ac_cluster_qc_trace.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_double)),
                                        C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
    lib.ac_cluster_qc_summary_get_sized.restype = C.c_size_t
    lib.ac_cluster_qc_summary_get_sized.argtypes = [C.c_void_p, C.POINTER(ClusterQcSummary), C.c_size_t]
    lib.ac_cluster_qc_free.argtypes = [C.c_void_p]
    lib.ac_cluster_qc_free.restype = None
    lib.ac_cluster_min_assemblies.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ac_cluster_seq_inputs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.ac_depth_begin.argtypes = [C.c_uint32, C.POINTER(DepthGraph), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_depth_begin_handles.argtypes = [C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    lib.ac_depth_add_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.ac_depth_add_fastq.argtypes = [C.c_void_p, C.c_char_p]
    lib.ac_depth_totals_get.argtypes = [C.c_void_p, C.POINTER(DepthTotals)]
    lib.ac_depth_kmer_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ac_depth_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ac_depth_free.argtypes = [C.c_void_p]
    lib.ac_depth_free.restype = None
    lib.ac_selftest_scan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ac_selftest_radix.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.ac_selftest_segments.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.ac_selftest_sort_cmp.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ac_selftest_scan_pool.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.ac_selftest_wave.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ac_selftest_fills.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ac_selftest_fill_order.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
    lib.ac_selftest_readback.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.ac_selftest_scalar_chain.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.ac_selftest_arena.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ac_selftest_launch.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.ac_selftest_atomics.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ac_selftest_side_order.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p]
    lib.ac_selftest_event_ring.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    _libs[key] = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise AutocyclerError(lib.ac_last_error().decode(errors="replace"))


class Graph:
    """Owning handle of an ac_graph (the final UnitigGraph after simplify_structure)."""

    def __init__(self, lib, handle, n_seqs):
        self._lib, self._h, self.n_seqs = lib, handle, n_seqs

    def close(self):
        if self._h:
            self._lib.ac_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def kmer_count(self):
        return self._lib.ac_kmer_count(self._h)

    def _stats(self, fn):
        s = fn(self._h)
        return dict(unitigs=s.unitigs, links=s.links_one_way, total_length=s.total_length)

    @property
    def stats_pre(self):
        return self._stats(self._lib.ac_stats_pre)

    @property
    def stats_post(self):
        return self._stats(self._lib.ac_stats_post)

    @property
    def unitig_count(self):
        return self._lib.ac_unitig_count(self._h)

    def unitig(self, idx):
        p, n, d = C.c_void_p(), C.c_uint32(), C.c_double()
        _check(self._lib, self._lib.ac_unitig(self._h, idx, C.byref(p), C.byref(n), C.byref(d)))
        return C.string_at(p.value, n.value), d.value

    def positions(self, idx, forward):
        p, n = C.POINTER(Position)(), C.c_uint32()
        _check(self._lib, self._lib.ac_unitig_positions(self._h, idx, 1 if forward else 0, C.byref(p), C.byref(n)))
        return [(p[i].seq_id_and_strand & 0x7FFF, bool(p[i].seq_id_and_strand & 0x8000), p[i].pos) for i in range(n.value)]

    def links(self):
        p, n = C.POINTER(Link)(), C.c_uint64()
        _check(self._lib, self._lib.ac_links(self._h, C.byref(p), C.byref(n)))
        return [(abs(p[i].a), p[i].a > 0, abs(p[i].b), p[i].b > 0) for i in range(n.value)]      # (unitig, forward?) pairs like UnitigStrand

    def path(self, seq_index):
        p, n = C.POINTER(C.c_int32)(), C.c_uint32()
        _check(self._lib, self._lib.ac_path(self._h, seq_index, C.byref(p), C.byref(n)))
        return p[:n.value]

    def bulk(self):
        """Zero-copy numpy views (valid while this handle lives): seq_bytes, seq_begin, seq_len, depth, links (structured: a, b — signed
        unitig numbers, negative = reverse strand), path_entries, path_off."""
        import numpy as np
        U = self.unitig_count
        sb, bg, ln, dp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib, self._lib.ac_unitigs_bulk(self._h, C.byref(sb), C.byref(bg), C.byref(ln), C.byref(dp)))
        view = lambda ptr, n, ct: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)) if n else np.zeros(0, dtype=ct)
        seq_begin = view(bg, U, C.c_uint64); seq_len = view(ln, U, C.c_uint32); depth = view(dp, U, C.c_double)
        total = int((seq_begin + seq_len).max()) if U else 0
        seq_bytes = view(sb, total, C.c_uint8)
        lp, n = C.POINTER(Link)(), C.c_uint64()
        _check(self._lib, self._lib.ac_links(self._h, C.byref(lp), C.byref(n)))
        ldt = np.dtype([("a", "<i4"), ("b", "<i4")])
        assert ldt.itemsize == C.sizeof(Link)
        links = np.frombuffer((C.c_uint8 * (n.value * C.sizeof(Link))).from_address(C.addressof(lp.contents)), dtype=ldt) if n.value else np.zeros(0, dtype=ldt)
        pe, po, ne = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_paths_bulk(self._h, C.byref(pe), C.byref(po), C.byref(ne)))
        S = self._lib.ac_graph_seq_count(self._h)
        return dict(seq_bytes=seq_bytes, seq_begin=seq_begin, seq_len=seq_len, depth=depth, links=links,
                    path_entries=view(pe, ne.value, C.c_int32), path_off=view(po, S + 1, C.c_uint64))

    def path_counts(self):
        n = self._lib.ac_graph_seq_count(self._h)
        out = (C.c_uint64 * n)()
        _check(self._lib, self._lib.ac_path_counts(self._h, out))
        return list(out)

    def decompress(self, seq_index):
        idv, ln = C.c_uint16(), C.c_uint32()
        _check(self._lib, self._lib.ac_graph_seq_info(self._h, C.c_uint32(seq_index), C.byref(idv), C.byref(ln), None, None))
        buf = C.create_string_buffer(ln.value)
        _check(self._lib, self._lib.ac_decompress_seq(self._h, C.c_uint32(seq_index), buf))
        return buf.raw

    def decompress_all(self, device=0):
        """reconstruct_original_sequences for every sequence at once, on the device (ac_decompress_device) -> list of bytes."""
        n = self._lib.ac_graph_seq_count(self._h)
        lens = []
        for i in range(n):
            ln = C.c_uint32()
            _check(self._lib, self._lib.ac_graph_seq_info(self._h, C.c_uint32(i), None, C.byref(ln), None, None))
            lens.append(ln.value)
        buf = C.create_string_buffer(max(sum(lens), 1))
        _check(self._lib, self._lib.ac_decompress_device(self._h, C.c_int(device), buf, C.c_uint64(sum(lens))))
        out, o = [], 0
        for ln in lens:
            out.append(buf.raw[o:o + ln]); o += ln
        return out

    def pairwise_distances(self, device=0):
        """cluster.rs:132-157 -> S x S list of lists (row a, column b)."""
        S = self._lib.ac_graph_seq_count(self._h)
        out = (C.c_double * (S * S))()
        _check(self._lib, self._lib.ac_pairwise_distances(self._h, C.c_int(device), out))
        return [[out[a * S + b] for b in range(S)] for a in range(S)]

    def trim_paths(self, min_identity=0.75, max_unitigs=5000, device=0):
        """The compute of `autocycler trim` (ac_trim_paths; the defaults are the reference's --min_identity / --max_unitigs): per sequence
        the slices [begin, end) of its path that start-end and hairpin trimming keep.  Returns (list of result dicts, summary dict)."""
        n = self._lib.ac_graph_seq_count(self._h)
        out = (TrimResult * max(n, 1))()
        sm = TrimSummary(size=C.sizeof(TrimSummary))
        _check(self._lib, self._lib.ac_trim_paths(self._h, min_identity, max_unitigs, device, out, C.byref(sm)))
        return [out[i].as_dict() for i in range(n)], sm.as_dict()

    def trim(self, min_identity=0.75, max_unitigs=5000, mad=5.0, device=0):
        """ac_graph_trim: trim.rs:45-49 on this graph — the alignments, choose_trim_type, the slices, exclude_outliers_in_length and the
        sequence subset of clean_up_graph — as a Trimmed (which keeps the graph alive)."""
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_graph_trim(self._h, min_identity, max_unitigs, mad, device, C.byref(h)))
        return Trimmed(self._lib, h, self.unitig_count, (self,))

    def trim_apply(self, results, chosen="auto", mad=5.0, device=0):
        """ac_graph_trim_apply: the same from a table of slices (trim_paths' list of dicts)."""
        res = _trim_results(results, self._lib.ac_graph_seq_count(self._h))
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_graph_trim_apply(self._h, res, TRIM_CHOOSE[chosen], mad, device, C.byref(h)))
        return Trimmed(self._lib, h, self.unitig_count, (self,))

    def resolve_bridges(self, device=0):
        """The compute of `autocycler resolve` up to the graph edits (ac_resolve_bridges) on this graph's paths, unitig lengths and
        headers.  Returns (anchors, bridges, summary) as resolve_bridge_paths does."""
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_resolve_bridges(self._h, device, C.byref(h)))
        return _resolve_result(self._lib, h)

    def resolve_apply(self, which="unique", device=0):
        """ac_graph_resolve_apply on the bridges ac_resolve_bridges finds on this graph: apply_bridges with reduce_depths and the two removals.
        which: "unique" (the bridges that do not conflict: the first pass) or "kept" (those cull_ambiguity kept: the final pass).  An Applied."""
        if which not in ("unique", "kept"):
            raise AutocyclerError('which: "unique" or "kept"')
        r, h = C.c_void_p(), C.c_void_p()
        _check(self._lib, self._lib.ac_resolve_bridges(self._h, device, C.byref(r)))
        try:
            _check(self._lib, self._lib.ac_graph_resolve_apply(self._h, r, Applied.UNIQUE if which == "unique" else Applied.KEPT, device, C.byref(h)))
        finally:
            self._lib.ac_resolve_free(r)
        return Applied(self._lib, h)

    def clean(self, remove=None, duplicate=None, min_depth=None, unitig_type=None, device=0):
        """ac_graph_clean: `autocycler clean`'s edit on this graph's links, lengths, depths and sequences.  remove / duplicate: the option's
        string ("3, 5") or a sequence of numbers; min_depth: a float or None; unitig_type: one type per unitig (gfa_segment_types of the text the
        graph was loaded from), None = every unitig Other.  A Cleaned."""
        import numpy as np
        rm, dp = _tig_numbers(self._lib, remove), _tig_numbers(self._lib, duplicate)
        ty = None if unitig_type is None else np.ascontiguousarray(np.asarray(unitig_type, dtype=np.uint8))
        if ty is not None and ty.shape != (self.unitig_count,):
            raise AutocyclerError(f"unitig_type: one entry per unitig expected ({self.unitig_count}), got shape {ty.shape}")
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_graph_clean(self._h, ptr(ty), ptr(rm), rm.shape[0], ptr(dp), dp.shape[0], 0 if min_depth is None else 1,
                                                   0.0 if min_depth is None else float(min_depth), device, C.byref(h)))
        return Cleaned(self._lib, h)

    def resolve_graphs(self, device=0):
        """ac_resolve_graphs: resolve.rs:44-67 on this graph -> (3_bridged.gfa, 4_merged.gfa, 5_final.gfa as bytes, cull count)"""
        outs, n = [C.c_void_p(), C.c_void_p(), C.c_void_p()], C.c_uint32()
        _check(self._lib, self._lib.ac_resolve_graphs(self._h, device, C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(n)))
        texts = [C.string_at(o.value) for o in outs]
        for o in outs:
            self._lib.ac_string_free(o)
        return texts[0], texts[1], texts[2], n.value

    def default_tip_names(self):
        """Sequence::string_for_newick (sequence.rs:77-87) per sequence: "{id}__{filename}__{contig_name}__{length}_bp", the contig
        name being the header up to its first space.  A built graph carries no file names or headers: both parts are empty."""
        names = []
        for i in range(self._lib.ac_graph_seq_count(self._h)):
            idv, ln, fn, hd = C.c_uint16(), C.c_uint32(), C.c_char_p(), C.c_char_p()
            _check(self._lib, self._lib.ac_graph_seq_info(self._h, C.c_uint32(i), C.byref(idv), C.byref(ln), C.byref(fn), C.byref(hd)))
            contig = (hd.value or b"").decode().split(" ")[0]
            names.append(f"{idv.value}__{(fn.value or b'').decode()}__{contig}__{ln.value}_bp")
        return names

    def cluster_inputs(self):
        """ac_cluster_seq_inputs: what ClusterTree.generate / qc take per sequence, from the file names and headers of a graph loaded from a
        GFA -> {"seq_len", "assembly", "cluster_weight", "trusted": one list each, "n_assemblies"}"""
        n = self._lib.ac_graph_seq_count(self._h)
        ln, asm, wt, tr, f = (C.c_uint64 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint8 * max(n, 1))(), C.c_uint32()
        _check(self._lib, self._lib.ac_cluster_seq_inputs(self._h, ln, asm, wt, tr, C.byref(f)))
        return {"seq_len": list(ln)[:n], "assembly": list(asm)[:n], "cluster_weight": list(wt)[:n], "trusted": list(tr)[:n], "n_assemblies": f.value}

    def cluster_tree(self, normalise=True, device=0, want_distances=False):
        """pairwise_contig_distances, make_symmetrical_distances and upgma (cluster.rs:132-192, 395-480) on this graph's paths, on the device
        in one go (ac_cluster_tree_build) -> ClusterTree, or (ClusterTree, S x S list of lists equal to pairwise_distances()) with
        want_distances.  The tree's default tip names are default_tip_names()."""
        S = self._lib.ac_graph_seq_count(self._h)
        out = (C.c_double * max(S * S, 1))() if want_distances else None
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_cluster_tree_build(self._h, 1 if normalise else 0, device, out, C.byref(h)))
        tree = ClusterTree(self._lib, h, self.default_tip_names())
        return (tree, [[out[a * S + b] for b in range(S)] for a in range(S)]) if want_distances else tree

    def verify(self, seqs, device=0):
        """ac_verify_graph: the round-trip verifier on the device (decompress identity, check_links, depth, renumber order, statistics).
        seqs: [(padded forward bytes, unpadded length, id)] as for compress_build.  Returns the report as a dict; report["failed"] == 0
        means the graph holds."""
        n = len(seqs)
        views = (SeqView * n)()
        keep = []
        for i, (fwd, length, sid) in enumerate(seqs):
            b = bytes(fwd); keep.append(b)
            views[i].fwd, views[i].length, views[i].id = b, length, sid
        rep = VerifyReport()
        _check(self._lib, self._lib.ac_verify_graph(self._h, views, C.c_uint32(n), C.c_int(device), C.byref(rep)))
        return rep.as_dict()

    def verify_device(self, d_text_ptr, n_text, off, lens, device=0):
        """The same against a text resident on the device (off / lens: ctypes arrays or sequences)."""
        n = len(lens)
        rep = VerifyReport()
        _check(self._lib, self._lib.ac_verify_graph_device(self._h, C.c_void_p(d_text_ptr), C.c_uint64(n_text), (C.c_uint64 * n)(*list(off)),
                                                           (C.c_uint32 * n)(*list(lens)), C.c_uint32(n), C.c_int(device), C.byref(rep)))
        return rep.as_dict()

    def timings(self):
        t = Timings()
        _check(self._lib, self._lib.ac_timings_get(self._h, C.byref(t)))
        return t.as_dict()

    def gfa(self, filenames, headers, parts=3):
        """parts: bit 0 = H, S, L lines; bit 1 = P lines (of the sequences this handle holds paths for)."""
        n = self.n_seqs
        fn = (C.c_char_p * n)(*[f.encode() for f in filenames])
        hd = (C.c_char_p * n)(*[h.encode() for h in headers])
        out, ln = C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_gfa_string_parts(self._h, C.c_int(parts), fn, hd, C.byref(out), C.byref(ln)))
        s = C.string_at(out.value, ln.value).decode()
        self._lib.ac_string_free(out)
        return s


def graph_from_gfa(gfa_text, lib_path=None):
    """UnitigGraph::from_gfa_lines for a compress-written GFA -> (Graph, filenames, headers)."""
    lib = load_library(lib_path)
    b = gfa_text.encode() if isinstance(gfa_text, str) else gfa_text
    h = C.c_void_p()
    _check(lib, lib.ac_graph_from_gfa(b, C.c_uint64(len(b)), C.byref(h)))
    n = lib.ac_graph_seq_count(h)
    g = Graph(lib, h, n)
    fns, hds = [], []
    for i in range(n):
        fn, hd = C.c_char_p(), C.c_char_p()
        _check(lib, lib.ac_graph_seq_info(h, C.c_uint32(i), None, None, C.byref(fn), C.byref(hd)))
        fns.append(fn.value.decode()); hds.append(hd.value.decode())
    return g, fns, hds


def max_trim_unitigs(lib_path=None):
    """ac_trim_max_unitigs: the largest min(max_unitigs, path length) the alignment kernels take."""
    return load_library(lib_path).ac_trim_max_unitigs()


def _weights_array(weights):
    """weights: a sequence (weights[u - 1] = length of unitig u) or a dict {unitig number: length} (absent numbers get no weight slot
    beyond the largest key; a path that names one of the holes aligns it with weight 0)."""
    if isinstance(weights, dict):
        m = max(weights) if weights else 0
        w = [0] * m
        for u, x in weights.items():
            w[u - 1] = x
        weights = w
    return (C.c_uint32 * max(len(weights), 1))(*weights), len(weights)


def overlap_alignment(path_a, path_b, weights, min_identity, max_unitigs, skip_diagonal, device=0, lib_path=None):
    """overlap_alignment (trim.rs:366-480) of two paths of signed unitig numbers on the device (ac_overlap_alignment).
    Returns the pieces as (a_unitig, a_index, b_unitig, b_index) tuples; a gap is (ALIGN_GAP, ALIGN_NONE); [] = no alignment."""
    lib = load_library(lib_path)
    if len(path_a) != len(path_b):
        raise AutocyclerError("the two paths differ in length")
    n = len(path_a)
    a = (C.c_int32 * max(n, 1))(*path_a); b = (C.c_int32 * max(n, 1))(*path_b)
    w, nw = _weights_array(weights)
    pieces = (AlignmentPiece * max(2 * min(n, max_unitigs), 1))()
    cnt = C.c_uint32()
    _check(lib, lib.ac_overlap_alignment(a, b, n, w, nw, min_identity, max_unitigs, 1 if skip_diagonal else 0, device, pieces, C.byref(cnt)))
    return [(pieces[i].a_unitig, pieces[i].a_index, pieces[i].b_unitig, pieces[i].b_index) for i in range(cnt.value)]


def trim_path_slices(paths, weights, min_identity=0.75, max_unitigs=5000, device=0, lib_path=None):
    """ac_trim_path_slices: Graph.trim_paths on caller-supplied paths (lists of signed unitig numbers).  Returns (results, summary)."""
    lib = load_library(lib_path)
    flat = [x for p in paths for x in p]
    off = [0]
    for p in paths:
        off.append(off[-1] + len(p))
    ent = (C.c_int32 * max(len(flat), 1))(*flat)
    offs = (C.c_uint64 * len(off))(*off)
    w, nw = _weights_array(weights)
    out = (TrimResult * max(len(paths), 1))()
    sm = TrimSummary(size=C.sizeof(TrimSummary))
    _check(lib, lib.ac_trim_path_slices(ent, offs, len(paths), w, nw, min_identity, max_unitigs, device, out, C.byref(sm)))
    return [out[i].as_dict() for i in range(len(paths))], sm.as_dict()


def _flat_paths(paths):
    flat = [x for p in paths for x in p]
    off = [0]
    for p in paths:
        off.append(off[-1] + len(p))
    return (C.c_int32 * max(len(flat), 1))(*flat), (C.c_uint64 * len(off))(*off)


def max_resolve_path(lib_path=None):
    """ac_resolve_max_path: the longest path a distance job takes."""
    return load_library(lib_path).ac_resolve_max_path()


def path_distances(paths, pairs, weights, device=0, lib_path=None):
    """global_alignment_distance (resolve.rs:387-418) on the device (ac_path_distances) for pairs (a, b) of indices into `paths` (lists of
    signed unitig numbers).  Returns (distances, statuses): status 2 = the two paths' weights add up to 2^32 or more, not computed."""
    lib = load_library(lib_path)
    ent, offs = _flat_paths(paths)
    n = len(pairs)
    pa = (C.c_uint32 * max(n, 1))(*[a for a, _ in pairs]); pb = (C.c_uint32 * max(n, 1))(*[b for _, b in pairs])
    w, nw = _weights_array(weights)
    dist = (C.c_uint32 * max(n, 1))(); status = (C.c_uint8 * max(n, 1))()
    _check(lib, lib.ac_path_distances(ent, offs, len(paths), pa, pb, n, w, nw, device, dist, status))
    return list(dist)[:n], list(status)[:n]


def _resolve_result(lib, h):
    try:
        ap, an = C.POINTER(C.c_uint32)(), C.c_uint32()
        _check(lib, lib.ac_resolve_anchors(h, C.byref(ap), C.byref(an)))
        anchors = ap[:an.value]
        bp, bn = C.POINTER(Bridge)(), C.c_uint32()
        _check(lib, lib.ac_resolve_bridge_records(h, C.byref(bp), C.byref(bn)))
        best, nbest = C.POINTER(C.c_int32)(), C.c_uint64()
        _check(lib, lib.ac_resolve_best_paths(h, C.byref(best), C.byref(nbest)))
        de, do, dm, dn = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        _check(lib, lib.ac_resolve_distinct_paths(h, C.byref(de), C.byref(do), C.byref(dm), C.byref(dn)))
        bridges = []
        for i in range(bn.value):
            b = bp[i]
            assert b.best_off + b.best_len <= nbest.value and b.first_distinct + b.n_distinct <= dn.value
            distinct = [(de[do[q]:do[q + 1]], dm[q]) for q in range(b.first_distinct, b.first_distinct + b.n_distinct)]
            bridges.append(dict(start=b.start, end=b.end, depth=b.depth, status=b.status,
                                best_path=best[b.best_off:b.best_off + b.best_len] if b.status == 0 else None,
                                best_total=b.best_total if b.status == 0 else None, distinct_paths=distinct,
                                conflicting=b.conflicting, culled=b.culled, cull_rank=b.cull_rank))
        sm = ResolveSummary()
        assert lib.ac_resolve_summary_get_sized(h, C.byref(sm), C.sizeof(ResolveSummary)) == C.sizeof(ResolveSummary)
        return anchors, bridges, sm.as_dict()
    finally:
        lib.ac_resolve_free(h)


def resolve_bridge_paths(paths, weights, consensus_weights=None, device=0, lib_path=None):
    """ac_resolve_bridge_paths: anchors, bridges (Bridge::cmp order) and a summary for the sequences' paths (lists of signed unitig
    numbers).  A bridge is a dict: start, end, depth, status (2: the reference's u32 arithmetic would overflow; best_path is None),
    best_path, best_total, distinct_paths [(path, multiplicity)], conflicting, culled, cull_rank (1-based; 0 = kept)."""
    lib = load_library(lib_path)
    ent, offs = _flat_paths(paths)
    w, nw = _weights_array(weights)
    cw = (C.c_uint32 * max(len(paths), 1))(*consensus_weights) if consensus_weights is not None else None
    h = C.c_void_p()
    _check(lib, lib.ac_resolve_bridge_paths(ent, offs, len(paths), cw, w, nw, device, C.byref(h)))
    return _resolve_result(lib, h)


class Components:
    """What ac_graph_components / ac_components_from_links found, copied out of the handle (numpy arrays):
    records        structured array, one per component in connected_components() order: first, unitigs, length, links_all, links_one_way,
                   open_ends, marked, circular_loop
    component_of   per unitig its component index; NOT_ALIVE for a unitig that is not alive
    member_off, members   component c = members[member_off[c] : member_off[c + 1]], unitig numbers ascending
    flags          per unitig: OPEN_START, OPEN_END, HAIRPIN_START, HAIRPIN_END, ISOLATED_CIRCULAR, ISOLATED_LINEAR
    summary        dict (unitigs = the alive ones, components, topology, links_all, links_one_way, total_length, launches, read_backs,
                   seconds_device); topology: the reference's string"""
    NOT_ALIVE = 0xFFFFFFFF
    OPEN_START, OPEN_END, HAIRPIN_START, HAIRPIN_END, ISOLATED_CIRCULAR, ISOLATED_LINEAR = 1, 2, 4, 8, 16, 32

    def __init__(self, lib, h, n_unitigs):
        import numpy as np
        try:
            dt = np.dtype([("first", "<u4"), ("unitigs", "<u4"), ("length", "<u8"), ("links_all", "<u8"), ("links_one_way", "<u8"),
                           ("open_ends", "<u4"), ("marked", "<u4"), ("circular_loop", "u1")], align=True)
            assert dt.itemsize == C.sizeof(Component)

            def take(ptr, n, dtype):
                dtype = np.dtype(dtype)
                return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype) if n else np.zeros(0, dtype=dtype)
            rp, rn = C.POINTER(Component)(), C.c_uint32()
            _check(lib, lib.ac_components_records(h, C.byref(rp), C.byref(rn)))
            self.records = take(rp, rn.value, dt)
            cp = C.POINTER(C.c_uint32)()
            _check(lib, lib.ac_components_of_unitig(h, C.byref(cp)))
            self.component_of = take(cp, n_unitigs, "<u4")
            op, mp = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
            _check(lib, lib.ac_components_members(h, C.byref(op), C.byref(mp)))
            self.member_off = take(op, rn.value + 1, "<u8")
            self.members = take(mp, int(self.member_off[-1]), "<u4")
            fp = C.POINTER(C.c_uint8)()
            _check(lib, lib.ac_components_unitig_flags(h, C.byref(fp)))
            self.flags = take(fp, n_unitigs, "u1")
            sm = ComponentsSummary()
            assert lib.ac_components_summary_get_sized(h, C.byref(sm), C.sizeof(ComponentsSummary)) == C.sizeof(ComponentsSummary) == sm.size
            self.summary = sm.as_dict()
            self.topology = lib.ac_topology_name(sm.topology).decode()
        finally:
            lib.ac_components_free(h)

    def components(self):
        """connected_components(): a list of ascending member lists"""
        off, m = self.member_off.tolist(), self.members.tolist()
        return [m[off[c]:off[c + 1]] for c in range(len(off) - 1)]

    def record_dicts(self):
        return [{k: int(r[k]) for k in self.records.dtype.names} for r in self.records]


def _bytes_per_unitig(values, n, what):
    """None, or one byte per unitig (any sequence of truth values, or a numpy array)"""
    if values is None:
        return None
    import numpy as np
    a = np.ascontiguousarray(np.asarray(values) != 0, dtype=np.uint8)
    if a.shape != (n,):
        raise AutocyclerError(f"{what}: one entry per unitig expected ({n}), got shape {a.shape}")
    return a


def graph_components(graph, marked=None, device=0, lib_path=None):
    """ac_graph_components: connected components, circular loops, link counts and topology of a Graph's links (one entry per L line) and
    unitig lengths.  marked: one truth value per unitig, counted per component.  lib_path is not needed: the graph knows its library."""
    lib = graph._lib
    n = graph.unitig_count
    mk = _bytes_per_unitig(marked, n, "marked")
    h = C.c_void_p()
    _check(lib, lib.ac_graph_components(graph._h, mk.ctypes.data if mk is not None else None, device, C.byref(h)))
    return Components(lib, h, n)


def components_from_links(n_unitigs, links, unitig_len=None, alive=None, marked=None, device=0, lib_path=None):
    """ac_components_from_links: the same on plain arrays.  links: (a, b) pairs of signed unitig numbers (a list, or an (m, 2) int32 numpy
    array) in L-line order; unitig_len[u - 1] = length of unitig u; alive: the unitigs that are still there (None = all) — one that is not
    is in no component and its links are ignored."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))
    ln = None
    if unitig_len is not None:
        ln = np.ascontiguousarray(np.asarray(unitig_len, dtype=np.uint32))
        if ln.shape != (n_unitigs,):
            raise AutocyclerError(f"unitig_len: one entry per unitig expected ({n_unitigs}), got shape {ln.shape}")
    al, mk = _bytes_per_unitig(alive, n_unitigs, "alive"), _bytes_per_unitig(marked, n_unitigs, "marked")
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_components_from_links(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(mk), device, C.byref(h)))
    return Components(lib, h, n_unitigs)


class MergePlan:
    """What ac_graph_merge_plan / ac_merge_plan_from_links found, copied out of the handle (numpy arrays):
    chains         structured array, one per chain in the order merge_linear_paths finds them: number, members, length, member_off, seq_off,
                   depth, type (OTHER or CONSENTIG), loop
    members        signed unitig numbers in path order: chain c = members[member_off : member_off + members]
    chain_of       per unitig its chain index; NOT_MERGED
    fixed          per unitig: FIXED_START, FIXED_END (after fix_circular_loops)
    sequences      the merged bytes: chain c = sequences[seq_off : seq_off + length] (empty when none were given or asked for)
    links          (m, 2) int32: the link set after the merge, ascending by (a, b) — a set, not get_links_for_gfa order
    summary        dict (chains, merged_unitigs, unitigs_after, links_after, bases_copied, launches, read_backs, seconds_device, seconds_copy)"""
    NOT_MERGED = 0xFFFFFFFF
    FIXED_START, FIXED_END = 1, 2
    OTHER, ANCHOR, CONSENTIG, BRIDGE = 0, 1, 2, 3

    def __init__(self, lib, h, n_unitigs, keep=False):
        import numpy as np
        self._lib, self._h = lib, None      # (keep: the handle lives on for Subsets.merged_paths, until close())
        try:
            dt = np.dtype([("number", "<u4"), ("members", "<u4"), ("length", "<u8"), ("member_off", "<u8"), ("seq_off", "<u8"), ("depth", "<f8"), ("type", "u1"),
                           ("loop", "u1")], align=True)
            assert dt.itemsize == C.sizeof(MergeChain)

            def take(ptr, n, dtype):
                dtype = np.dtype(dtype)
                return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype) if n else np.zeros(0, dtype=dtype)
            rp, rn = C.POINTER(MergeChain)(), C.c_uint32()
            _check(lib, lib.ac_merge_chains(h, C.byref(rp), C.byref(rn)))
            self.chains = take(rp, rn.value, dt)
            mp, mn = C.POINTER(C.c_int32)(), C.c_uint64()
            _check(lib, lib.ac_merge_members(h, C.byref(mp), C.byref(mn)))
            self.members = take(mp, mn.value, "<i4")
            cp = C.POINTER(C.c_uint32)()
            _check(lib, lib.ac_merge_chain_of_unitig(h, C.byref(cp)))
            self.chain_of = take(cp, n_unitigs, "<u4")
            fp = C.POINTER(C.c_uint8)()
            _check(lib, lib.ac_merge_fixed_flags(h, C.byref(fp)))
            self.fixed = take(fp, n_unitigs, "u1")
            sp, sn = C.POINTER(C.c_uint8)(), C.c_uint64()
            _check(lib, lib.ac_merge_sequences(h, C.byref(sp), C.byref(sn)))
            self.sequences = take(sp, sn.value, "u1")
            lp, ln = C.POINTER(Link)(), C.c_uint64()
            _check(lib, lib.ac_merge_links(h, C.byref(lp), C.byref(ln)))
            self.links = take(lp, 2 * ln.value, "<i4").reshape(-1, 2)
            sm = MergeSummary()
            assert lib.ac_merge_summary_get_sized(h, C.byref(sm), C.sizeof(MergeSummary)) == C.sizeof(MergeSummary) == sm.size
            self.summary = sm.as_dict()
            if keep:
                self._h, h = h, None
        finally:
            if h is not None:
                lib.ac_merge_free(h)

    def close(self):
        if self._h:
            self._lib.ac_merge_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def chain_members(self):
        """merge_paths: a list of lists of signed unitig numbers"""
        m = self.members.tolist()
        return [m[int(c["member_off"]):int(c["member_off"]) + int(c["members"])] for c in self.chains]

    def chain_sequences(self):
        b = self.sequences.tobytes()
        return [b[int(c["seq_off"]):int(c["seq_off"]) + int(c["length"])] for c in self.chains] if len(b) else []

    def chain_dicts(self):
        return [{k: (float(r[k]) if k == "depth" else int(r[k])) for k in self.chains.dtype.names} for r in self.chains]


def graph_merge_plan(graph, use_paths=True, with_sequences=True, device=0, lib_path=None):
    """ac_graph_merge_plan: what merge_linear_paths would do to a Graph, and its products.  use_paths: the path ends fix unitig ends and the
    position counts come from the paths (the reference's call with the graph's sequences); False: a call without sequences on a graph without
    positions.  lib_path is not needed: the graph knows its library."""
    lib = graph._lib
    h = C.c_void_p()
    _check(lib, lib.ac_graph_merge_plan(graph._h, int(bool(use_paths)), int(bool(with_sequences)), device, C.byref(h)))
    return MergePlan(lib, h, graph.unitig_count)


def merge_plan_from_links(n_unitigs, links, unitig_len, alive=None, path_ends=None, depth=None, fwd_positions=None, rev_positions=None, unitig_type=None,
                          sequences=None, device=0, lib_path=None, keep=False):
    """ac_merge_plan_from_links: the same on plain arrays (keep: the plan's handle stays open for merge_finish, until close()).  links: (a, b) pairs of signed unitig numbers, a set closed under reverse
    complement; path_ends: (first, last) signed entries per sequence; fwd_positions / rev_positions: position counts per unitig;
    unitig_type: MergePlan.OTHER / ANCHOR / CONSENTIG / BRIDGE per unitig; sequences: one bytes object per unitig (forward strand), or a
    tuple (all bytes as a uint8 array, the first byte of every unitig as a uint64 array)."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))

    def per_unitig(values, dtype, what):
        if values is None:
            return None
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
        if a.shape != (n_unitigs,):
            raise AutocyclerError(f"{what}: one entry per unitig expected ({n_unitigs}), got shape {a.shape}")
        return a
    ln, dp = per_unitig(unitig_len, np.uint32, "unitig_len"), per_unitig(depth, np.float64, "depth")
    fw, rv = per_unitig(fwd_positions, np.uint32, "fwd_positions"), per_unitig(rev_positions, np.uint32, "rev_positions")
    ty, al = per_unitig(unitig_type, np.uint8, "unitig_type"), _bytes_per_unitig(alive, n_unitigs, "alive")
    pe = np.ascontiguousarray(np.asarray(path_ends, dtype=np.int32).reshape(-1, 2)) if path_ends is not None else np.zeros((0, 2), dtype=np.int32)
    sb = sg = None
    if isinstance(sequences, tuple):      # (bytes of all forward sequences as a uint8 array, first byte per unitig as a uint64 array)
        sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), per_unitig(sequences[1], np.uint64, "sequences[1]")
    elif sequences is not None:
        if len(sequences) != n_unitigs:
            raise AutocyclerError(f"sequences: one entry per unitig expected ({n_unitigs}), got {len(sequences)}")
        sg = np.zeros(max(n_unitigs, 1), dtype=np.uint64)
        sg[1:n_unitigs] = np.cumsum([len(x) for x in sequences[:-1]], dtype=np.uint64) if n_unitigs > 1 else []
        sb = np.frombuffer(b"".join(bytes(x) for x in sequences) + b"\0", dtype=np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_merge_plan_from_links(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(pe), pe.shape[0], ptr(dp), ptr(fw), ptr(rv), ptr(ty),
                                             ptr(sb), ptr(sg), device, C.byref(h)))
    return MergePlan(lib, h, n_unitigs, keep=keep)


class MergedPaths:
    """What ac_subsets_merged_paths found, copied out of the handle: seq_index (the cluster's kept sequences, ascending), path_off, entries
    (sequence seq_index[i] = entries[path_off[i] : path_off[i + 1]], merged unitigs under their chain numbers), summary."""

    def __init__(self, lib, h, keep=False):
        import numpy as np
        self._lib, self._h = lib, None      # (keep: the handle lives on for Subsets.finish / merge_finish, until close())
        try:
            sp, sn, op, ep = C.POINTER(C.c_uint32)(), C.c_uint32(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)()
            _check(lib, lib.ac_merged_paths_get(h, C.byref(sp), C.byref(sn), C.byref(op), C.byref(ep)))
            self.seq_index = _take(sp, sn.value, "<u4")
            self.path_off = _take(op, sn.value + 1, "<u8")
            self.entries = _take(ep, int(self.path_off[-1]), "<i4")
            sm = MergedPathsSummary()
            assert lib.ac_merged_paths_summary_get_sized(h, C.byref(sm), C.sizeof(MergedPathsSummary)) == C.sizeof(MergedPathsSummary) == sm.size
            self.summary = sm.as_dict()
            if keep:
                self._h, h = h, None
        finally:
            if h is not None:
                lib.ac_merged_paths_free(h)

    def close(self):
        if self._h:
            self._lib.ac_merged_paths_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def paths(self):
        """{sequence index: list of signed numbers}"""
        off, e = self.path_off.tolist(), self.entries.tolist()
        return {int(s): e[off[i]:off[i + 1]] for i, s in enumerate(self.seq_index.tolist())}


def _take(ptr, n, dtype):
    import numpy as np
    dtype = np.dtype(dtype)
    return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype) if n else np.zeros(0, dtype=dtype)


class Subsets:
    """Owning handle of an ac_subsets: what every cluster of sequences (1..n_clusters; label 0 = dropped) keeps of a graph.  The arrays are
    copied out on construction; the handle stays for components / merge_plan / merged_paths until close().
    records        structured array, one per cluster: seqs, unitigs, entries, links, length
    unitigs(c)     the alive unitig numbers of cluster c, ascending
    positions(c)   (fwd_positions, rev_positions) of those unitigs: both the number of kept path entries that name the unitig
    links(c)       (m, 2) int32: the input's links with both ends alive in c, in the input's order
    seqs(c)        the kept sequence indices, ascending
    path_ends(c)   (k, 2) int32: first and last signed entry of every kept sequence with a non-empty path
    dense(c)       dict alive, fwd_positions, rev_positions, depth: n_unitigs entries each — the arguments of components_from_links /
                   merge_plan_from_links
    summary        dict (clusters, sequences_kept, n_unitigs, entries_kept, unitigs, links, launches, read_backs, seconds_device)"""

    def __init__(self, lib, h, n_unitigs, keepalive, owns=True):
        import numpy as np
        self._lib, self._h, self.n_unitigs, self._keepalive, self._owns = lib, h, n_unitigs, keepalive, owns
        dt = np.dtype([("seqs", "<u4"), ("unitigs", "<u4"), ("entries", "<u8"), ("links", "<u8"), ("length", "<u8")], align=True)
        assert dt.itemsize == C.sizeof(SubsetCluster)
        rp, rn = C.POINTER(SubsetCluster)(), C.c_uint32()
        _check(lib, lib.ac_subsets_records(h, C.byref(rp), C.byref(rn)))
        self.n_clusters = nc = rn.value
        self.records = _take(rp, nc, dt)
        op, up, fp, vp = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        _check(lib, lib.ac_subsets_unitigs(h, C.byref(op), C.byref(up), C.byref(fp), C.byref(vp)))
        self.unitig_off = _take(op, nc + 1, "<u8")
        total = int(self.unitig_off[-1])
        self._unitigs, self._fwd, self._rev = _take(up, total, "<u4"), _take(fp, total, "<u4"), _take(vp, total, "<u4")
        op, lp = C.POINTER(C.c_uint64)(), C.POINTER(Link)()
        _check(lib, lib.ac_subsets_links(h, C.byref(op), C.byref(lp)))
        self.link_off = _take(op, nc + 1, "<u8")
        self._links = _take(lp, 2 * int(self.link_off[-1]), "<i4").reshape(-1, 2)
        op, sp = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
        _check(lib, lib.ac_subsets_seqs(h, C.byref(op), C.byref(sp)))
        self.seq_off = _take(op, nc + 1, "<u8")
        self._seqs = _take(sp, int(self.seq_off[-1]), "<u4")
        op, ep = C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)()
        _check(lib, lib.ac_subsets_path_ends(h, C.byref(op), C.byref(ep)))
        self.ends_off = _take(op, nc + 1, "<u8")
        self._ends = _take(ep, 2 * int(self.ends_off[-1]), "<i4").reshape(-1, 2)
        sm = SubsetsSummary()
        assert lib.ac_subsets_summary_get_sized(h, C.byref(sm), C.sizeof(SubsetsSummary)) == C.sizeof(SubsetsSummary) == sm.size
        self.summary = sm.as_dict()

    def close(self):
        if self._h and self._owns:      # (a Trimmed's view is borrowed)
            self._lib.ac_subsets_free(self._h)
        self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _row(self, off, c):
        if not 1 <= c <= self.n_clusters:
            raise AutocyclerError(f"cluster {c} does not exist: clusters run from 1 to {self.n_clusters}")
        return slice(int(off[c - 1]), int(off[c]))

    def unitigs(self, c):
        return self._unitigs[self._row(self.unitig_off, c)]

    def positions(self, c):
        r = self._row(self.unitig_off, c)
        return self._fwd[r], self._rev[r]

    def links(self, c):
        return self._links[self._row(self.link_off, c)]

    def seqs(self, c):
        return self._seqs[self._row(self.seq_off, c)]

    def path_ends(self, c):
        return self._ends[self._row(self.ends_off, c)]

    def dense(self, c):
        import numpy as np
        n = self.n_unitigs
        alive, fwd, rev, depth = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.float64)
        ptr = lambda a: a.ctypes.data if a.size else None
        _check(self._lib, self._lib.ac_subsets_dense(self._h, c, ptr(alive), ptr(fwd), ptr(rev), ptr(depth)))
        return dict(alive=alive, fwd_positions=fwd, rev_positions=rev, depth=depth)

    def components(self, c, marked=None, device=0):
        """ac_subsets_components: Components of cluster c's graph"""
        mk = _bytes_per_unitig(marked, self.n_unitigs, "marked")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_subsets_components(self._h, c, mk.ctypes.data if mk is not None and mk.size else None, device, C.byref(h)))
        return Components(self._lib, h, self.n_unitigs)

    def merge_plan(self, c, with_sequences=True, sequences=None, device=0):
        """ac_subsets_merge_plan: the MergePlan of cluster c's graph (its handle stays alive for merged_paths; close() it or let it go).
        sequences: (all bytes as a uint8 array, the first byte of every unitig as a uint64 array) for an object made from plain arrays."""
        import numpy as np
        sb = sg = None
        if sequences is not None:
            sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), np.ascontiguousarray(sequences[1], dtype=np.uint64)
            if sg.shape != (self.n_unitigs,):
                raise AutocyclerError(f"sequences[1]: one entry per unitig expected ({self.n_unitigs}), got shape {sg.shape}")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_subsets_merge_plan(self._h, c, sb.ctypes.data if sb is not None else None, sg.ctypes.data if sg is not None else None,
                                                          int(bool(with_sequences)), device, C.byref(h)))
        return MergePlan(self._lib, h, self.n_unitigs, keep=True)

    def merged_paths(self, c, plan, device=0, keep=False):
        """ac_subsets_merged_paths: the paths of cluster c's sequences over the merged unitigs of `plan` (from merge_plan(c)).  keep: the
        handle stays open for finish()"""
        if getattr(plan, "_h", None) is None:
            raise AutocyclerError("merged_paths: the plan must come from Subsets.merge_plan and still be open")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_subsets_merged_paths(self._h, c, plan._h, device, C.byref(h)))
        return MergedPaths(self._lib, h, keep=keep)

    def finish(self, c, plan, merged_paths=None, renumber=False, sequences=None, device=0):
        """ac_subsets_finish: cluster c's graph after the merge of `plan` (from merge_plan(c)) as a Finished.  merged_paths: from
        merged_paths(c, plan, keep=True) for the P lines, or None; sequences as for merge_plan."""
        import numpy as np
        if getattr(plan, "_h", None) is None:
            raise AutocyclerError("finish: the plan must come from Subsets.merge_plan and still be open")
        if merged_paths is not None and getattr(merged_paths, "_h", None) is None:
            raise AutocyclerError("finish: the merged paths must come from Subsets.merged_paths(..., keep=True) and still be open")
        sb = sg = None
        if sequences is not None:
            sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), np.ascontiguousarray(sequences[1], dtype=np.uint64)
            if sg.shape != (self.n_unitigs,):
                raise AutocyclerError(f"sequences[1]: one entry per unitig expected ({self.n_unitigs}), got shape {sg.shape}")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_subsets_finish(self._h, c, plan._h, merged_paths._h if merged_paths is not None else None,
                                                      sb.ctypes.data if sb is not None else None, sg.ctypes.data if sg is not None else None,
                                                      1 if renumber else 0, device, C.byref(h)))
        return Finished(self._lib, h)


TRIM_CHOOSE = {"auto": 0, "none": 1, None: 1, "start_end": 2, "hairpin": 3}
TRIM_KINDS = {0: None, 1: "start_end", 2: "hairpin"}


def _trim_results(results, n_seqs):
    """a list of trim_paths' result dicts (or None) as an array of ac_trim_result"""
    if results is None:
        return None
    if len(results) != n_seqs:
        raise AutocyclerError(f"results: one per sequence expected ({n_seqs}), got {len(results)}")
    out = (TrimResult * max(n_seqs, 1))()
    for i, r in enumerate(results):
        for kind in ("start_end", "hairpin"):
            sl = getattr(out[i], kind)
            sl.status, sl.begin, sl.end, sl.trimmed_length = (r[kind][f] for f in ("status", "begin", "end", "trimmed_length"))
        out[i].hairpin_start_trimmed, out[i].hairpin_end_trimmed = r.get("hairpin_start_trimmed", 0), r.get("hairpin_end_trimmed", 0)
    return out


class Trimmed:
    """Owning handle of an ac_trimmed: a graph's sequences after choose_trim_type and exclude_outliers_in_length, and what they keep of it.
    records   structured array, one per input sequence: begin, end (the slice of its path that stays), length (new), trimmed, excluded
    summary   dict: chosen (None, "start_end", "hairpin"), c_se, c_hp, sequences, trimmed, excluded, rejected, unitigs_in, unitigs_alive,
              launches, read_backs, median, mad, min_length, max_length, entries_kept, links, seconds_device, align_*
    subsets   a Subsets view with one cluster that does not own: unitigs(1), links(1), merge_plan(1), ... as for any Subsets
    finish()  merge plan, merged paths and finish with renumbering in one call: a Finished
    yaml()    2_trimmed.yaml as bytes"""

    def __init__(self, lib, h, n_unitigs, keepalive):
        import numpy as np
        self._lib, self._h, self.n_unitigs, self._keepalive = lib, h, n_unitigs, keepalive
        dt = np.dtype([("begin", "<u4"), ("end", "<u4"), ("length", "<u8"), ("trimmed", "<u4"), ("excluded", "<u4")], align=True)
        assert dt.itemsize == C.sizeof(TrimmedRecord)
        rp, rn = C.POINTER(TrimmedRecord)(), C.c_uint32()
        _check(lib, lib.ac_trimmed_records(h, C.byref(rp), C.byref(rn)))
        self.records = _take(rp, rn.value, dt)
        sm = TrimmedSummary()
        assert lib.ac_trimmed_summary_get_sized(h, C.byref(sm), C.sizeof(TrimmedSummary)) == C.sizeof(TrimmedSummary) == sm.size
        self.summary = sm.as_dict()
        self.summary["chosen"] = TRIM_KINDS[sm.chosen]
        self.subsets = Subsets(lib, C.c_void_p(lib.ac_trimmed_subsets(h)), n_unitigs, None, owns=False)

    def close(self):
        if self._h:
            self.subsets._h = None      # (borrowed: it dies with this object)
            self._lib.ac_trimmed_free(self._h)
            self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def kept(self):
        """the indices of the sequences that stay, ascending"""
        return [i for i, x in enumerate(self.records["excluded"].tolist()) if not x]

    def finish(self, sequences=None, device=0):
        """ac_trimmed_finish.  sequences: (all bytes as a uint8 array, the first byte of every unitig as a uint64 array) for an object made
        from plain arrays; None on one made from a Graph."""
        import numpy as np
        sb = sg = None
        if sequences is not None:
            sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), np.ascontiguousarray(sequences[1], dtype=np.uint64)
            if sg.shape != (self.n_unitigs,):
                raise AutocyclerError(f"sequences[1]: one entry per unitig expected ({self.n_unitigs}), got shape {sg.shape}")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_trimmed_finish(self._h, sb.ctypes.data if sb is not None else None, sg.ctypes.data if sg is not None else None, device,
                                                      C.byref(h)))
        return Finished(self._lib, h)

    def yaml(self):
        out, n = C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_trimmed_yaml_string(self._h, C.byref(out), C.byref(n)))
        text = C.string_at(out.value, n.value)
        self._lib.ac_string_free(out)
        return text


def trim_apply(n_unitigs, links, unitig_len, paths, seq_lengths, results, chosen="auto", mad=5.0, alive=None, unitig_type=None, device=0, lib_path=None):
    """ac_trim_apply: trim's edit on plain arrays.  links, unitig_len, paths, alive as for subsets_from_paths; seq_lengths: one per sequence;
    results: trim_path_slices' list of dicts (None with chosen="none"); unitig_type: AC_UNITIG_* bytes or None."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))
    ln = np.ascontiguousarray(np.asarray(unitig_len, dtype=np.uint32))
    if ln.shape != (n_unitigs,):
        raise AutocyclerError(f"unitig_len: one entry per unitig expected ({n_unitigs}), got shape {ln.shape}")
    al, ty = _bytes_per_unitig(alive, n_unitigs, "alive"), _bytes_per_unitig(unitig_type, n_unitigs, "unitig_type")
    if isinstance(paths, tuple):
        ent, off = np.ascontiguousarray(paths[0], dtype=np.int32), np.ascontiguousarray(paths[1], dtype=np.uint64)
    else:
        ent = np.ascontiguousarray(np.fromiter((e for p in paths for e in p), dtype=np.int32))
        off = np.zeros(len(paths) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64) if len(paths) else []
    n_seqs = off.shape[0] - 1
    sl = np.ascontiguousarray(np.asarray(seq_lengths, dtype=np.uint32))
    if sl.shape != (n_seqs,):
        raise AutocyclerError(f"seq_lengths: one per sequence expected ({n_seqs}), got shape {sl.shape}")
    res = _trim_results(results, n_seqs)
    if ln.size == 0:
        ln = np.zeros(1, dtype=np.uint32)
    if sl.size == 0:
        sl = np.zeros(1, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_trim_apply(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(ty), ptr(ent), off.ctypes.data, ptr(sl), n_seqs, res, TRIM_CHOOSE[chosen],
                                  mad, device, C.byref(h)))
    return Trimmed(lib, h, n_unitigs, (la, ln, al, ty, ent, off, sl))


def trim_gfa(text, min_identity=0.75, max_unitigs=5000, mad=5.0, device=0, lib_path=None):
    """ac_trim_gfa: `autocycler trim` from the text of 1_untrimmed.gfa (segment numbers in any order) -> (2_trimmed.gfa as bytes,
    2_trimmed.yaml as bytes, summary dict)"""
    lib = load_library(lib_path)
    b = text.encode() if isinstance(text, str) else text
    gfa, n, yaml, sm = C.c_void_p(), C.c_uint64(), C.c_void_p(), TrimmedSummary()
    sm.size = C.sizeof(TrimmedSummary)
    _check(lib, lib.ac_trim_gfa(b, len(b), min_identity, max_unitigs, mad, device, C.byref(gfa), C.byref(n), C.byref(yaml), C.byref(sm)))
    out = C.string_at(gfa.value, n.value), C.string_at(yaml.value)
    lib.ac_string_free(gfa)
    lib.ac_string_free(yaml)
    d = sm.as_dict()
    d["chosen"] = TRIM_KINDS[sm.chosen]
    return out[0], out[1], d


def trim_dir(cluster_dir, min_identity=0.75, max_unitigs=5000, mad=5.0, device=0, lib_path=None):
    """ac_trim_dir: <cluster_dir>/1_untrimmed.gfa -> 2_trimmed.gfa, 2_trimmed.yaml"""
    lib = load_library(lib_path)
    _check(lib, lib.ac_trim_dir(str(cluster_dir).encode(), min_identity, max_unitigs, mad, device))


def resolve_dir(cluster_dir, device=0, lib_path=None):
    """ac_resolve_dir: <cluster_dir>/2_trimmed.gfa -> 3_bridged.gfa, 4_merged.gfa, 5_final.gfa"""
    lib = load_library(lib_path)
    _check(lib, lib.ac_resolve_dir(str(cluster_dir).encode(), device))


TOPOLOGY_NAMES = ("empty", "fragmented", "linear-open-open", "circular", "linear-hairpin-hairpin", "linear-open-hairpin", "other")      # AC_TOPOLOGY_*


class Combined:
    """Owning handle of an ac_combined: the clusters' graphs as `autocycler combine` (combine.rs:144-224) puts them together.  The records are
    copied out on construction; the handle stays for gfa(), fasta(), yaml() and depth_lines() until close().
    clusters   structured array, one per graph in output order: input_index, unitigs, length, links, offset, max_number, topology (an index into
               TOPOLOGY_NAMES), has_read_depth, read_depth
    unitigs    structured array, one per unitig in output order: graph, index, number (printed), length, depth (printed), read_depth,
               has_read_depth, flags (as Components.flags), type
    links      (m, 2) int32 of printed numbers, graph after graph, in get_links_for_gfa order
    summary    dict: graphs, bases, unitigs, links, fully_resolved, with_reads, launches, read_backs, seconds_device"""

    def __init__(self, lib, h):
        import numpy as np
        self._lib, self._h = lib, h
        cp, cn = C.POINTER(CombinedCluster)(), C.c_uint32()
        _check(lib, lib.ac_combined_clusters(h, C.byref(cp), C.byref(cn)))
        self.clusters = np.frombuffer(C.string_at(cp, cn.value * C.sizeof(CombinedCluster)), dtype=np.dtype(CombinedCluster)).copy()
        up, un = C.POINTER(CombinedUnitig)(), C.c_uint64()
        _check(lib, lib.ac_combined_unitigs(h, C.byref(up), C.byref(un)))
        self.unitigs = np.frombuffer(C.string_at(up, un.value * C.sizeof(CombinedUnitig)) if un.value else b"", dtype=np.dtype(CombinedUnitig)).copy()
        kp, kn = C.POINTER(Link)(), C.c_uint64()
        _check(lib, lib.ac_combined_links(h, C.byref(kp), C.byref(kn)))
        self.links = _take(kp, 2 * kn.value, "<i4").reshape(-1, 2)
        sm = CombinedSummary()
        assert lib.ac_combined_summary_get_sized(h, C.byref(sm), C.sizeof(CombinedSummary)) == C.sizeof(CombinedSummary) == sm.size
        self.summary = sm.as_dict()

    def close(self):
        if self._h:
            self._lib.ac_combined_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _text(self, f):
        out, n = C.c_void_p(), C.c_uint64()
        _check(self._lib, f(self._h, C.byref(out), C.byref(n)))
        text = C.string_at(out.value, n.value)
        self._lib.ac_string_free(out)
        return text

    def gfa(self):
        """ac_combined_gfa_string: consensus_assembly.gfa (bytes)"""
        return self._text(self._lib.ac_combined_gfa_string)

    def fasta(self):
        """ac_combined_fasta_string: consensus_assembly.fasta (bytes)"""
        return self._text(self._lib.ac_combined_fasta_string)

    def yaml(self):
        """ac_combined_yaml_string: consensus_assembly.yaml (bytes)"""
        return self._text(self._lib.ac_combined_yaml_string)

    def depth_lines(self):
        """ac_combined_depth_lines: what print_read_depths writes on stderr (bytes; empty without reads)"""
        return self._text(self._lib.ac_combined_depth_lines)


def _read_depth_lists(read_depths, sizes):
    """read depths as the entries take them.  read_depths: None, a ReadDepth (its depths(g) of every graph), or one sequence per graph of floats
    with None where there is no depth (what ReadDepth.depths returns).  -> (depth arrays, has arrays), one pair per graph, or (None, None)"""
    import numpy as np
    if read_depths is None:
        return None, None
    if isinstance(read_depths, ReadDepth):
        read_depths = [read_depths.depths(g) for g in range(len(sizes))]
    if len(read_depths) != len(sizes):
        raise AutocyclerError(f"read_depths: one entry per graph expected ({len(sizes)}), got {len(read_depths)}")
    rd, has = [], []
    for g, (v, n) in enumerate(zip(read_depths, sizes)):
        v = list(v)
        if len(v) != n:
            raise AutocyclerError(f"read_depths[{g}]: one entry per unitig expected ({n}), got {len(v)}")
        rd.append(np.array([0.0 if x is None else float(x) for x in v] + [0.0], dtype=np.float64))
        has.append(np.array([0 if x is None else 1 for x in v] + [0], dtype=np.uint8))
    return rd, has


def _pointer_list(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def combine_graphs(graphs, read_depths=None, device=0, lib_path=None):
    """ac_combine_graphs: `autocycler combine` on plain arrays.  graphs: one dict per graph with
    number (per unitig), len, links ((a, b) pairs of signed 1-based file-order indices within the graph, in L-line order) and optionally depth,
    type, seqs (one bytes object per unitig: needed for gfa() and fasta() only).  read_depths: see _read_depth_lists.  A Combined."""
    import numpy as np
    lib = load_library(lib_path)
    graphs = list(graphs)
    sizes = [len(g["number"]) for g in graphs]
    for g, n in zip(graphs, sizes):
        for key in ("len", "depth", "type"):
            if g.get(key) is not None and len(g[key]) != n:
                raise AutocyclerError(f"{key}: one entry per unitig expected ({n}), got {len(g[key])}")
    uoff = np.zeros(len(graphs) + 1, dtype=np.uint64); loff = np.zeros(len(graphs) + 1, dtype=np.uint64)

    def cat(key, dtype):
        parts = [np.asarray(g[key], dtype=dtype).reshape(-1) if g.get(key) is not None else np.zeros(n, dtype=dtype) for g, n in zip(graphs, sizes)]
        return np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, dtype=dtype)]))
    number, ln, depth, ty = cat("number", np.uint32), cat("len", np.uint32), cat("depth", np.float64), cat("type", np.uint8)
    link_arrays = [np.asarray(g.get("links", []), dtype=np.int32).reshape(-1, 2) for g in graphs]
    links = np.ascontiguousarray(np.concatenate(link_arrays + [np.zeros((1, 2), dtype=np.int32)]))
    if graphs:
        uoff[1:] = np.cumsum(sizes); loff[1:] = np.cumsum([a.shape[0] for a in link_arrays])
    rd, has = _read_depth_lists(read_depths, sizes)
    rd_all = np.ascontiguousarray(np.concatenate([a[:-1] for a in rd] + [np.zeros(1)])) if rd is not None else None
    has_all = np.ascontiguousarray(np.concatenate([a[:-1] for a in has] + [np.zeros(1, dtype=np.uint8)])) if has is not None else None
    sb = sg = None
    if graphs and all(g.get("seqs") is not None for g in graphs):
        seqs = [bytes(x) for g in graphs for x in g["seqs"]]
        if len(seqs) != sum(sizes):
            raise AutocyclerError("seqs: one entry per unitig expected")
        sg = np.zeros(len(seqs) + 1, dtype=np.uint64)
        sg[1:] = np.cumsum([len(x) for x in seqs])
        sb = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None else None
    h = C.c_void_p()
    _check(lib, lib.ac_combine_graphs(len(graphs), ptr(uoff), ptr(loff), ptr(number), ptr(ln), ptr(depth), ptr(ty), ptr(links), ptr(rd_all), ptr(has_all), ptr(sb), ptr(sg),
                                      device, C.byref(h)))
    return Combined(lib, h)


def combine_handles(graphs, types=None, read_depths=None, device=0, lib_path=None):
    """ac_combine_handles: the same on Graph handles (graph_from_gfa of each 5_final.gfa).  types: one uint8 array per graph (gfa_segment_types of
    its text) or None = Other.  A Combined."""
    import numpy as np
    lib = load_library(lib_path)
    graphs = list(graphs)
    sizes = [g.unitig_count for g in graphs]
    hs = (C.c_void_p * max(len(graphs), 1))(*[g._h for g in graphs])
    ty = None
    if types is not None:
        ty = [np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.uint8), np.zeros(1, dtype=np.uint8)])) for t in types]
        if [len(t) - 1 for t in ty] != sizes:
            raise AutocyclerError("types: one array per graph with one entry per unitig expected")
    rd, has = _read_depth_lists(read_depths, sizes)
    h = C.c_void_p()
    _check(lib, lib.ac_combine_handles(hs, len(graphs), _pointer_list(ty) if ty is not None else None, _pointer_list(rd) if rd is not None else None,
                                       _pointer_list(has) if has is not None else None, device, C.byref(h)))
    return Combined(lib, h)


def combine_gfas(texts, read_depths=None, device=0, lib_path=None):
    """ac_combine_gfas: from the texts of the clusters' GFAs -> (consensus_assembly.gfa, .fasta, .yaml as bytes, summary dict).  read_depths: see
    _read_depth_lists (per graph in S-line order)."""
    lib = load_library(lib_path)
    bs = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
    tp = (C.c_char_p * max(len(bs), 1))(*bs)
    tn = (C.c_uint64 * max(len(bs), 1))(*[len(b) for b in bs])
    sizes = [sum(1 for line in b.split(b"\n") if line.split(b"\t")[0] == b"S") for b in bs]
    rd, has = _read_depth_lists(read_depths, sizes)
    gfa, fasta, yaml = C.c_void_p(), C.c_void_p(), C.c_void_p()
    gn, fn, yn = C.c_uint64(), C.c_uint64(), C.c_uint64()
    sm = CombinedSummary()
    sm.size = C.sizeof(CombinedSummary)
    _check(lib, lib.ac_combine_gfas(tp, tn, len(bs), _pointer_list(rd) if rd is not None else None, _pointer_list(has) if has is not None else None, device,
                                    C.byref(gfa), C.byref(gn), C.byref(fasta), C.byref(fn), C.byref(yaml), C.byref(yn), C.byref(sm)))
    out = C.string_at(gfa.value, gn.value), C.string_at(fasta.value, fn.value), C.string_at(yaml.value, yn.value)
    for p in (gfa, fasta, yaml):
        lib.ac_string_free(p)
    return out[0], out[1], out[2], sm.as_dict()


def combine_dir(autocycler_dir, in_gfas, reads=(), depth_kmer=19, device=0, lib_path=None):
    """ac_combine: the whole command -> what it would print on stderr after the work (str): the depth lines, then the verdict"""
    lib = load_library(lib_path)
    gs = [os.fsencode(str(p)) for p in in_gfas]
    rs = [os.fsencode(str(p)) for p in reads]
    report = C.c_void_p()
    _check(lib, lib.ac_combine(os.fsencode(str(autocycler_dir)), (C.c_char_p * max(len(gs), 1))(*gs), len(gs), (C.c_char_p * max(len(rs), 1))(*rs) if rs else None, len(rs),
                               depth_kmer, device, C.byref(report)))
    text = C.string_at(report.value).decode()
    lib.ac_string_free(report)
    return text


def gfa2fasta(gfa_text, device=0, lib_path=None):
    """ac_gfa2fasta_string: `autocycler gfa2fasta` from a GFA text -> (FASTA as bytes, (circular, linear, other))"""
    lib = load_library(lib_path)
    b = gfa_text.encode() if isinstance(gfa_text, str) else gfa_text
    out, n, counts = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 3)()
    _check(lib, lib.ac_gfa2fasta_string(b, len(b), device, C.byref(out), C.byref(n), counts))
    text = C.string_at(out.value, n.value)
    lib.ac_string_free(out)
    return text, tuple(counts)


def gfa2fasta_file(in_gfa, out_fasta, device=0, lib_path=None):
    """ac_gfa2fasta: the command on files -> (circular, linear, other)"""
    lib = load_library(lib_path)
    counts = (C.c_uint64 * 3)()
    _check(lib, lib.ac_gfa2fasta(os.fsencode(str(in_gfa)), os.fsencode(str(out_fasta)), device, counts))
    return tuple(counts)


class Finished:
    """Owning handle of an ac_finished: a merge plan applied.  The arrays are copied out on construction; the handle stays for gfa() and
    to_graph() until close().
    unitigs        structured array in S-line order: number (as printed), source (an old number, or n_unitigs + 1 + chain index), length,
                   seq_off, depth, type
    sequences      the bytes in that order: unitig i = sequences[seq_off : seq_off + length]
    new_of_old     the printed number of every old number and chain number (n_unitigs + chains entries), 0 = gone
    links          (m, 2) int32 in L-line order (get_links_for_gfa after the merge), printed numbers
    path_seq, path_off, path_entries   the P lines (those of the MergedPaths it was made with), printed numbers
    summary        dict (unitigs, renumbered, launches, read_backs, links, path_entries, bases, tie_items, seconds_device, seconds_gather)"""

    def __init__(self, lib, h):
        import numpy as np
        self._lib, self._h = lib, h
        dt = np.dtype([("number", "<u4"), ("source", "<u4"), ("length", "<u8"), ("seq_off", "<u8"), ("depth", "<f8"), ("type", "u1")], align=True)
        assert dt.itemsize == C.sizeof(FinishedUnitig)
        up, un = C.POINTER(FinishedUnitig)(), C.c_uint32()
        _check(lib, lib.ac_finished_unitigs(h, C.byref(up), C.byref(un)))
        self.unitigs = _take(up, un.value, dt)
        sp, sn = C.POINTER(C.c_uint8)(), C.c_uint64()
        _check(lib, lib.ac_finished_sequences(h, C.byref(sp), C.byref(sn)))
        self.sequences = _take(sp, sn.value, "u1")
        np_, nn = C.POINTER(C.c_uint32)(), C.c_uint64()
        _check(lib, lib.ac_finished_new_of_old(h, C.byref(np_), C.byref(nn)))
        self.new_of_old = _take(np_, nn.value, "<u4")
        lp, ln = C.POINTER(Link)(), C.c_uint64()
        _check(lib, lib.ac_finished_links(h, C.byref(lp), C.byref(ln)))
        self.links = _take(lp, 2 * ln.value, "<i4").reshape(-1, 2)
        qp, qn, op, ep = C.POINTER(C.c_uint32)(), C.c_uint32(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int32)()
        _check(lib, lib.ac_finished_paths(h, C.byref(qp), C.byref(qn), C.byref(op), C.byref(ep)))
        self.path_seq = _take(qp, qn.value, "<u4")
        self.path_off = _take(op, qn.value + 1, "<u8")
        self.path_entries = _take(ep, int(self.path_off[-1]), "<i4")
        sm = FinishedSummary()
        assert lib.ac_finished_summary_get_sized(h, C.byref(sm), C.sizeof(FinishedSummary)) == C.sizeof(FinishedSummary) == sm.size
        self.summary = sm.as_dict()

    def close(self):
        if self._h:
            self._lib.ac_finished_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def unitig_sequences(self):
        b = self.sequences.tobytes()
        return [b[int(u["seq_off"]):int(u["seq_off"]) + int(u["length"])] for u in self.unitigs]

    def paths(self):
        """{sequence index: list of signed printed numbers}"""
        off, e = self.path_off.tolist(), self.path_entries.tolist()
        return {int(s): e[off[i]:off[i + 1]] for i, s in enumerate(self.path_seq.tolist())}

    def _meta(self, seq_ids, seq_lengths, filenames, headers, cluster_tags=None):
        import numpy as np
        n = len(self.path_seq)
        for what, v in (("seq_ids", seq_ids), ("seq_lengths", seq_lengths), ("filenames", filenames), ("headers", headers)):
            if len(v) != n:
                raise AutocyclerError(f"{what}: one entry per P line expected ({n}), got {len(v)}")
        ids, lens = np.ascontiguousarray(seq_ids, dtype=np.uint16), np.ascontiguousarray(seq_lengths, dtype=np.uint32)
        fns = (C.c_char_p * max(n, 1))(*[x.encode() for x in filenames])
        hds = (C.c_char_p * max(n, 1))(*[x.encode() for x in headers])
        tags = np.ascontiguousarray(cluster_tags, dtype=np.uint32) if cluster_tags is not None else None
        if tags is not None and tags.shape != (n,):
            raise AutocyclerError(f"cluster_tags: one entry per P line expected ({n}), got shape {tags.shape}")
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        return (ptr(ids), ptr(lens), fns, hds, ptr(tags)), (ids, lens, fns, hds, tags)

    def gfa(self, k, seq_ids=(), seq_lengths=(), filenames=(), headers=(), cluster_tags=None, use_other_colour=False):
        """ac_finished_gfa_string: save_gfa's text (bytes).  One id / length / filename / header (and cluster tag) per P line."""
        args, keep = self._meta(seq_ids, seq_lengths, filenames, headers, cluster_tags)
        out, n = C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_finished_gfa_string(self._h, k, *args, 1 if use_other_colour else 0, C.byref(out), C.byref(n)))
        text = C.string_at(out.value, n.value)
        self._lib.ac_string_free(out)
        return text

    def to_graph(self, k, seq_ids=(), seq_lengths=(), filenames=(), headers=()):
        """ac_finished_to_graph: an ordinary Graph (renumber = 1 and every type Other only)"""
        args, keep = self._meta(seq_ids, seq_lengths, filenames, headers)
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_finished_to_graph(self._h, k, *args[:4], C.byref(h)))
        return Graph(self._lib, h, self._lib.ac_graph_seq_count(h))


def merge_finish(plan, n_unitigs, links, unitig_len, alive=None, depth=None, unitig_type=None, sequences=None, paths=None, renumber=False, device=0, lib_path=None):
    """ac_merge_finish: the graph after the merge.  plan: a MergePlan whose handle is open (Subsets.merge_plan's); links, unitig_len, alive,
    depth, unitig_type: the arrays the plan was made from, the links in list order; sequences: (all bytes as a uint8 array, the first byte of
    every unitig as a uint64 array), or one bytes object per unitig; paths: a MergedPaths made with keep_handle, or None."""
    import numpy as np
    lib = load_library(lib_path)
    if getattr(plan, "_h", None) is None:
        raise AutocyclerError("merge_finish: the plan's handle must be open (merge_plan_from_links(..., keep=True) or Subsets.merge_plan)")
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))

    def per_unitig(values, dtype, what):
        if values is None:
            return None
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
        if a.shape != (n_unitigs,):
            raise AutocyclerError(f"{what}: one entry per unitig expected ({n_unitigs}), got shape {a.shape}")
        return a
    ln, dp, ty = per_unitig(unitig_len, np.uint32, "unitig_len"), per_unitig(depth, np.float64, "depth"), per_unitig(unitig_type, np.uint8, "unitig_type")
    al = _bytes_per_unitig(alive, n_unitigs, "alive")
    sb = sg = None
    if isinstance(sequences, tuple):
        sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), per_unitig(sequences[1], np.uint64, "sequences[1]")
    elif sequences is not None:
        if len(sequences) != n_unitigs:
            raise AutocyclerError(f"sequences: one entry per unitig expected ({n_unitigs}), got {len(sequences)}")
        sg = np.zeros(max(n_unitigs, 1), dtype=np.uint64)
        sg[1:n_unitigs] = np.cumsum([len(x) for x in sequences[:-1]], dtype=np.uint64) if n_unitigs > 1 else []
        sb = np.frombuffer(b"".join(bytes(x) for x in sequences) + b"\0", dtype=np.uint8)
    if ln is not None and ln.size == 0:
        ln = np.zeros(1, dtype=np.uint32)      # (n_unitigs == 0: the entry still wants a pointer)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_merge_finish(plan._h, n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(dp), ptr(ty), ptr(sb), ptr(sg),
                                    paths._h if paths is not None else None, 1 if renumber else 0, device, C.byref(h)))
    return Finished(lib, h)


class Applied:
    """Owning handle of an ac_applied: a graph after apply_bridges, reduce_depths and the two removals (resolve.rs:223-282).  The arrays are
    copied out on construction; the handle stays for merge_plan(), finish() and gfa() until close().
    n_unitigs, n_total   the caller's n; n + the bridge unitigs (unitig n_unitigs + 1 + i was made from bridge bridge_of[i])
    len, alive, depth, type   per unitig 1 .. n_total (type: MergePlan.OTHER / ANCHOR / BRIDGE)
    links          (m, 2) int32 in get_links_for_gfa order: the alive originals ascending, then the bridge unitigs
    bridge_sequences, bridge_seq_off   the bridge unitigs' bytes: unitig i = bridge_sequences[bridge_seq_off[i] : bridge_seq_off[i + 1]]
    summary        dict (bridges_applied, direct_links, launches, launches_components, read_backs, removed_no_anchor, removed_zero_depth,
                   links_in, links_out, bases_copied, seconds_device, seconds_copy, seconds_components)"""
    UNIQUE, KEPT = 0, 1

    def __init__(self, lib, h):
        self._lib, self._h = lib, h
        nt, lp, ap, dp, tp = C.c_uint32(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint8)()
        _check(lib, lib.ac_applied_unitigs(h, C.byref(nt), C.byref(lp), C.byref(ap), C.byref(dp), C.byref(tp)))
        self.n_total = nt.value
        self.len, self.alive, self.depth, self.type = _take(lp, nt.value, "<u4"), _take(ap, nt.value, "u1"), _take(dp, nt.value, "<f8"), _take(tp, nt.value, "u1")
        bp, bn = C.POINTER(C.c_uint32)(), C.c_uint32()
        _check(lib, lib.ac_applied_bridge_of(h, C.byref(bp), C.byref(bn)))
        self.bridge_of = _take(bp, bn.value, "<u4")
        self.n_unitigs = self.n_total - bn.value
        kp, kn = C.POINTER(Link)(), C.c_uint64()
        _check(lib, lib.ac_applied_links(h, C.byref(kp), C.byref(kn)))
        self.links = _take(kp, 2 * kn.value, "<i4").reshape(-1, 2)
        sp, op, sn = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)(), C.c_uint64()
        _check(lib, lib.ac_applied_bridge_sequences(h, C.byref(sp), C.byref(op), C.byref(sn)))
        self.bridge_sequences = _take(sp, sn.value, "u1")
        self.bridge_seq_off = _take(op, bn.value + 1, "<u8")
        sm = AppliedSummary()
        assert lib.ac_applied_summary_get_sized(h, C.byref(sm), C.sizeof(AppliedSummary)) == C.sizeof(AppliedSummary) == sm.size
        self.summary = sm.as_dict()

    def close(self):
        if self._h:
            self._lib.ac_applied_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bridge_unitig_sequences(self):
        b, off = self.bridge_sequences.tobytes(), self.bridge_seq_off.tolist()
        return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)] if len(b) else []

    def merge_plan(self, with_sequences=True, device=0):
        """ac_applied_merge_plan: merge_linear_paths(graph, &vec![]) after clear_positions; the plan's handle stays open for finish()"""
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_applied_merge_plan(self._h, int(bool(with_sequences)), device, C.byref(h)))
        return MergePlan(self._lib, h, self.n_total, keep=True)

    def finish(self, plan, renumber=True, device=0):
        """ac_applied_finish: the graph after that merge (renumber: renumber_unitigs), a Finished"""
        if getattr(plan, "_h", None) is None:
            raise AutocyclerError("Applied.finish: the plan's handle must be open (Applied.merge_plan)")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_applied_finish(self._h, plan._h, 1 if renumber else 0, device, C.byref(h)))
        return Finished(self._lib, h)

    def gfa(self, k, use_other_colour=False):
        """ac_applied_gfa_string: 3_bridged.gfa's text (bytes): the edited graph under its own numbers, no P lines"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_applied_gfa_string(self._h, k, 1 if use_other_colour else 0, C.byref(out), C.byref(n)))
        text = C.string_at(out.value, n.value)
        self._lib.ac_string_free(out)
        return text


def apply_bridges(n_unitigs, links, unitig_len, anchors, bridges, apply="unique", bridge_depth=1.0, alive=None, depth=None, sequences=None, device=0, lib_path=None):
    """ac_apply_bridges: apply_bridges with reduce_depths and the two removals on plain arrays.  links: (a, b) pairs of signed unitig numbers in
    list order, a set closed under reverse complement; anchors: ascending unitig numbers; bridges: the dicts resolve_bridge_paths returns, in
    its order (start, end, status, best_path, distinct_paths [(path, multiplicity)], conflicting, culled); apply: "unique" (not conflicting),
    "kept" (not culled) or one truth value per bridge; sequences: one bytes object per unitig, or (uint8 array, uint64 first bytes)."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))

    def per_unitig(values, dtype, what):
        if values is None:
            return None
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
        if a.shape != (n_unitigs,):
            raise AutocyclerError(f"{what}: one entry per unitig expected ({n_unitigs}), got shape {a.shape}")
        return a
    ln, dp, al = per_unitig(unitig_len, np.uint32, "unitig_len"), per_unitig(depth, np.float64, "depth"), _bytes_per_unitig(alive, n_unitigs, "alive")
    an = np.ascontiguousarray(np.asarray(anchors, dtype=np.uint32).reshape(-1))
    sb = sg = None
    if isinstance(sequences, tuple):
        sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), per_unitig(sequences[1], np.uint64, "sequences[1]")
    elif sequences is not None:
        if len(sequences) != n_unitigs:
            raise AutocyclerError(f"sequences: one entry per unitig expected ({n_unitigs}), got {len(sequences)}")
        sg = np.zeros(max(n_unitigs, 1), dtype=np.uint64)
        sg[1:n_unitigs] = np.cumsum([len(x) for x in sequences[:-1]], dtype=np.uint64) if n_unitigs > 1 else []
        sb = np.frombuffer(b"".join(bytes(x) for x in sequences) + b"\0", dtype=np.uint8)
    nb = len(bridges)
    recs = (Bridge * max(nb, 1))()
    best, dist, doff, mult = [], [], [0], []
    for i, b in enumerate(bridges):
        r = recs[i]
        r.start, r.end, r.status, r.conflicting, r.culled = b["start"], b["end"], b.get("status", 0), int(b.get("conflicting", 0)), int(b.get("culled", 0))
        bp = b.get("best_path") or []
        r.best_off, r.best_len = len(best), len(bp)
        best.extend(bp)
        r.first_distinct, r.n_distinct = len(mult), len(b.get("distinct_paths", ()))
        for path, m in b.get("distinct_paths", ()):
            dist.extend(path); doff.append(len(dist)); mult.append(m)
    if isinstance(apply, str):
        if apply not in ("unique", "kept"):
            raise AutocyclerError('apply: "unique", "kept" or one truth value per bridge')
        flags = [not b.get("conflicting", 0) if apply == "unique" else not b.get("culled", 0) for b in bridges]
    else:
        flags = [bool(x) for x in apply]
        if len(flags) != nb:
            raise AutocyclerError(f"apply: one entry per bridge expected ({nb}), got {len(flags)}")
    fl = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8).reshape(-1))
    ba, da = np.asarray(best, dtype=np.int32), np.asarray(dist, dtype=np.int32)
    oa, ma = np.asarray(doff, dtype=np.uint64), np.asarray(mult, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_apply_bridges(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(dp), ptr(an), an.shape[0], ptr(sb), ptr(sg), recs if nb else None, nb,
                                     ptr(ba), ba.shape[0], ptr(da), oa.ctypes.data, ptr(ma), ma.shape[0], ptr(fl), float(bridge_depth), device, C.byref(h)))
    return Applied(lib, h)


class Cleaned:
    """Owning handle of an ac_cleaned: a graph after the edits of `autocycler clean` (clean.rs:33-41), before its merge.  The arrays are copied
    out on construction; the handle stays for merge_plan(), finish() and gfa() until close().
    n_unitigs, n_out   the caller's n; n + 2 per duplication (copies a, b of the i-th duplicated number: n + 1 + 2 i, n + 2 + 2 i)
    len, alive, depth, type, copy_of, reason   per unitig 1 .. n_out (reason: Cleaned.KEPT / REMOVED / DUPLICATED / LOW_DEPTH / KEPT_DEAD_END / ABSENT)
    seq_begin      per unitig the first byte of its sequence in the caller's bytes (a copy: its original's), or None without sequences
    links          (m, 2) int32 in get_links_for_gfa order: the originals ascending, then the copies; a multiset after a duplicated loop
    summary        dict (unitigs_in, unitigs_out, rounds, rounds_per_batch, launches, read_backs, kept, removed, duplicated, low_depth,
                   kept_dead_end, absent, links_in, links_out, seconds_device)"""
    KEPT, REMOVED, DUPLICATED, LOW_DEPTH, KEPT_DEAD_END, ABSENT = range(6)

    def __init__(self, lib, h):
        self._lib, self._h = lib, h
        nt, lp, ap, dp, tp = C.c_uint32(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint8)()
        sp, cp, rp = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        _check(lib, lib.ac_cleaned_unitigs(h, C.byref(nt), C.byref(lp), C.byref(ap), C.byref(dp), C.byref(tp), C.byref(sp), C.byref(cp), C.byref(rp)))
        n = self.n_out = nt.value
        self.len, self.alive, self.depth, self.type = _take(lp, n, "<u4"), _take(ap, n, "u1"), _take(dp, n, "<f8"), _take(tp, n, "u1")
        self.copy_of, self.reason = _take(cp, n, "<u4"), _take(rp, n, "u1")
        self.seq_begin = _take(sp, n, "<u8") if sp else None
        kp, kn = C.POINTER(Link)(), C.c_uint64()
        _check(lib, lib.ac_cleaned_links(h, C.byref(kp), C.byref(kn)))
        self.links = _take(kp, 2 * kn.value, "<i4").reshape(-1, 2)
        sm = CleanedSummary()
        assert lib.ac_cleaned_summary_get_sized(h, C.byref(sm), C.sizeof(CleanedSummary)) == C.sizeof(CleanedSummary) == sm.size
        self.summary = sm.as_dict()
        self.n_unitigs = sm.unitigs_in

    def close(self):
        if self._h:
            self._lib.ac_cleaned_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def merge_plan(self, with_sequences=True, device=0):
        """ac_cleaned_merge_plan: merge_linear_paths(graph, &vec![]); the plan's handle stays open for finish().  Refused after a duplicated loop."""
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_cleaned_merge_plan(self._h, int(bool(with_sequences)), device, C.byref(h)))
        return MergePlan(self._lib, h, self.n_out, keep=True)

    def finish(self, plan, renumber=True, device=0):
        """ac_cleaned_finish: the graph after that merge (renumber: renumber_unitigs), a Finished"""
        if getattr(plan, "_h", None) is None:
            raise AutocyclerError("Cleaned.finish: the plan's handle must be open (Cleaned.merge_plan)")
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_cleaned_finish(self._h, plan._h, 1 if renumber else 0, device, C.byref(h)))
        return Finished(self._lib, h)

    def gfa(self, k, use_other_colour=True):
        """ac_cleaned_gfa_string: the edited graph under its own numbers, before the merge (bytes); no P lines"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(self._lib, self._lib.ac_cleaned_gfa_string(self._h, k, 1 if use_other_colour else 0, C.byref(out), C.byref(n)))
        text = C.string_at(out.value, n.value)
        self._lib.ac_string_free(out)
        return text


def parse_tig_numbers(text, lib_path=None):
    """ac_parse_tig_numbers: parse_tig_numbers of clean.rs — "4, 5,6" -> [4, 5, 6]; None -> []; a piece that is no u32 raises"""
    lib = load_library(lib_path)
    out, n = C.c_void_p(), C.c_uint32()
    _check(lib, lib.ac_parse_tig_numbers(None if text is None else text.encode(), C.byref(out), C.byref(n)))
    v = list((C.c_uint32 * n.value).from_address(out.value)) if n.value else []
    lib.ac_string_free(out)
    return v


def _tig_numbers(lib, numbers):
    """an option of clean as the ABI takes it: its string parsed by the library, or a sequence of numbers sorted as parse_tig_numbers sorts"""
    import numpy as np
    if numbers is None:
        return np.zeros(0, dtype=np.uint32)
    if isinstance(numbers, (str, bytes)):
        out, n = C.c_void_p(), C.c_uint32()
        _check(lib, lib.ac_parse_tig_numbers(numbers.encode() if isinstance(numbers, str) else numbers, C.byref(out), C.byref(n)))
        v = list((C.c_uint32 * n.value).from_address(out.value)) if n.value else []
        lib.ac_string_free(out)
        return np.asarray(v, dtype=np.uint32)
    return np.sort(np.ascontiguousarray(np.asarray(list(numbers), dtype=np.uint32).reshape(-1)))


def gfa_segment_types(gfa_text, lib_path=None):
    """ac_gfa_segment_types: the type of every S line of a GFA text from its CL:Z colour (MergePlan.OTHER / ANCHOR / CONSENTIG / BRIDGE), a uint8 array"""
    import numpy as np
    lib = load_library(lib_path)
    b = gfa_text.encode() if isinstance(gfa_text, str) else gfa_text
    out, n = C.c_void_p(), C.c_uint32()
    _check(lib, lib.ac_gfa_segment_types(b, len(b), C.byref(out), C.byref(n)))
    v = np.frombuffer(C.string_at(out.value, n.value), dtype=np.uint8).copy()
    lib.ac_string_free(out)
    return v


def clean_graph(n_unitigs, links, unitig_len, depth=None, unitig_type=None, alive=None, sequences=None, remove=None, duplicate=None, min_depth=None, device=0,
                lib_path=None):
    """ac_clean_graph: the edits of `autocycler clean` on plain arrays.  links: (a, b) pairs of signed unitig numbers in L-line order, a set closed
    under reverse complement; remove / duplicate: the option's string or a sequence of numbers; min_depth: a float or None; sequences: one bytes
    object per unitig, or (uint8 array, uint64 first bytes).  A Cleaned."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))

    def per_unitig(values, dtype, what):
        if values is None:
            return None
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype))
        if a.shape != (n_unitigs,):
            raise AutocyclerError(f"{what}: one entry per unitig expected ({n_unitigs}), got shape {a.shape}")
        return a
    ln, dp, ty = per_unitig(unitig_len, np.uint32, "unitig_len"), per_unitig(depth, np.float64, "depth"), per_unitig(unitig_type, np.uint8, "unitig_type")
    al = _bytes_per_unitig(alive, n_unitigs, "alive")
    sb = sg = None
    if isinstance(sequences, tuple):
        sb, sg = np.ascontiguousarray(sequences[0], dtype=np.uint8), per_unitig(sequences[1], np.uint64, "sequences[1]")
    elif sequences is not None:
        if len(sequences) != n_unitigs:
            raise AutocyclerError(f"sequences: one entry per unitig expected ({n_unitigs}), got {len(sequences)}")
        sg = np.zeros(max(n_unitigs, 1), dtype=np.uint64)
        sg[1:n_unitigs] = np.cumsum([len(x) for x in sequences[:-1]], dtype=np.uint64) if n_unitigs > 1 else []
        sb = np.frombuffer(b"".join(bytes(x) for x in sequences) + b"\0", dtype=np.uint8)
    rm, du = _tig_numbers(lib, remove), _tig_numbers(lib, duplicate)
    if ln is not None and ln.size == 0:
        ln = np.zeros(1, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_clean_graph(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(dp), ptr(ty), ptr(al), ptr(sb), ptr(sg), ptr(rm), rm.shape[0], ptr(du), du.shape[0],
                                   0 if min_depth is None else 1, 0.0 if min_depth is None else float(min_depth), device, C.byref(h)))
    return Cleaned(lib, h)


def clean_gfa(text, remove=None, duplicate=None, min_depth=None, device=0, lib_path=None):
    """ac_clean_gfa: `autocycler clean` from a GFA text to the cleaned GFA text (bytes).  remove / duplicate: the option's string, or None."""
    lib = load_library(lib_path)
    b = text.encode() if isinstance(text, str) else text
    out, n = C.c_void_p(), C.c_uint64()
    enc = lambda v: None if v is None else (v.encode() if isinstance(v, str) else ",".join(str(int(x)) for x in v).encode())
    _check(lib, lib.ac_clean_gfa(b, len(b), enc(remove), enc(duplicate), 0 if min_depth is None else 1, 0.0 if min_depth is None else float(min_depth), device,
                                 C.byref(out), C.byref(n)))
    res = C.string_at(out.value, n.value)
    lib.ac_string_free(out)
    return res


def graph_subsets(graph, cluster_of_seq, n_clusters=None, device=0, lib_path=None):
    """ac_graph_subsets: what every cluster keeps of a Graph's unitigs, links and paths.  cluster_of_seq: one label per sequence in path
    order, 0 = dropped; n_clusters: None = the highest label (at least 1).  The Subsets keeps the graph alive."""
    import numpy as np
    lib = graph._lib
    labels = np.ascontiguousarray(np.asarray(cluster_of_seq, dtype=np.uint16))
    n_seqs = lib.ac_graph_seq_count(graph._h)
    if labels.shape != (n_seqs,):
        raise AutocyclerError(f"cluster_of_seq: one label per sequence expected ({n_seqs}), got shape {labels.shape}")
    if n_clusters is None:
        n_clusters = max(1, int(labels.max())) if labels.size else 1
    h = C.c_void_p()
    _check(lib, lib.ac_graph_subsets(graph._h, labels.ctypes.data if labels.size else None, n_clusters, device, C.byref(h)))
    return Subsets(lib, h, graph.unitig_count, (graph,))


def subsets_from_paths(n_unitigs, links, unitig_len, paths, cluster_of_seq, n_clusters=None, alive=None, device=0, lib_path=None):
    """ac_subsets_from_paths: the same on plain arrays.  links: (a, b) pairs of signed unitig numbers in L-line order; paths: a list of lists
    of signed numbers, or a tuple (entries as an int32 array, offsets as a uint64 array of n_seqs + 1); alive: the unitigs that are still
    there (None = all)."""
    import numpy as np
    lib = load_library(lib_path)
    la = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1, 2))
    ln = np.ascontiguousarray(np.asarray(unitig_len, dtype=np.uint32))
    if ln.shape != (n_unitigs,):
        raise AutocyclerError(f"unitig_len: one entry per unitig expected ({n_unitigs}), got shape {ln.shape}")
    al = _bytes_per_unitig(alive, n_unitigs, "alive")
    if isinstance(paths, tuple):
        ent, off = np.ascontiguousarray(paths[0], dtype=np.int32), np.ascontiguousarray(paths[1], dtype=np.uint64)
    else:
        ent = np.ascontiguousarray(np.fromiter((e for p in paths for e in p), dtype=np.int32))
        off = np.zeros(len(paths) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64) if len(paths) else []
    n_seqs = off.shape[0] - 1
    labels = np.ascontiguousarray(np.asarray(cluster_of_seq, dtype=np.uint16))
    if labels.shape != (n_seqs,):
        raise AutocyclerError(f"cluster_of_seq: one label per sequence expected ({n_seqs}), got shape {labels.shape}")
    if n_clusters is None:
        n_clusters = max(1, int(labels.max())) if labels.size else 1
    if ln.size == 0:
        ln = np.zeros(1, dtype=np.uint32)      # (n_unitigs == 0: the entry still wants a pointer)
    if labels.size == 0:
        labels = np.zeros(1, dtype=np.uint16)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    h = C.c_void_p()
    _check(lib, lib.ac_subsets_from_paths(n_unitigs, ptr(la), la.shape[0], ptr(ln), ptr(al), ptr(ent), off.ctypes.data, n_seqs, ptr(labels), n_clusters, device,
                                          C.byref(h)))
    return Subsets(lib, h, n_unitigs, (la, ln, ent, off))


class ClusterTree:
    """Owning handle of an ac_cluster_tree: the UPGMA tree of `autocycler cluster` (cluster.rs:395-494) and the host functions on it."""

    def __init__(self, lib, handle, tip_names=None):
        self._lib, self._h, self.tip_names = lib, handle, tip_names

    def close(self):
        if self._h:
            self._lib.ac_cluster_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_nodes(cls, nodes, root, lib_path=None):
        """ac_cluster_tree_from_nodes: nodes = [(id, left index, right index, distance)], -1 / -1 at a tip; root = index of the root."""
        lib = load_library(lib_path)
        arr = (ClusterNode * max(len(nodes), 1))()
        for i, (nid, left, right, dist) in enumerate(nodes):
            arr[i].id, arr[i].left, arr[i].right, arr[i].distance = nid, left, right, dist
        h = C.c_void_p()
        _check(lib, lib.ac_cluster_tree_from_nodes(arr, len(nodes), root, C.byref(h)))
        return cls(lib, h)

    def _nodes(self):
        p, n, root = C.POINTER(ClusterNode)(), C.c_uint32(), C.c_int32()
        _check(self._lib, self._lib.ac_cluster_nodes(self._h, C.byref(p), C.byref(n), C.byref(root)))
        return [(p[i].id, p[i].left, p[i].right, p[i].distance) for i in range(n.value)], root.value

    @property
    def nodes(self):
        """[(id, left, right, distance)]: a built tree has its tips first, in sequence order, then the internal nodes in merge order"""
        return self._nodes()[0]

    @property
    def root(self):
        return self._nodes()[1]

    @property
    def merges(self):
        """[(a, b, distance)]: cluster ids a < b and the value get_closest_pair compared"""
        p, n = C.POINTER(ClusterMerge)(), C.c_uint32()
        _check(self._lib, self._lib.ac_cluster_merges(self._h, C.byref(p), C.byref(n)))
        return [(p[i].a, p[i].b, p[i].distance) for i in range(n.value)]

    @property
    def summary(self):
        sm = ClusterSummary()
        assert self._lib.ac_cluster_summary_get_sized(self._h, C.byref(sm), C.sizeof(ClusterSummary)) == C.sizeof(ClusterSummary)
        return sm.as_dict()

    def _n_tips(self):
        return sum(1 for n in self.nodes if n[1] < 0)

    def cut(self, cutoff, manual=()):
        """automatic_clustering (no manual clusters) or manual_clustering -> the clusters' node ids, ascending"""
        manual = list(manual)
        m = (C.c_uint16 * max(len(manual), 1))(*manual)
        out, n = (C.c_uint16 * self._n_tips())(), C.c_uint32()
        _check(self._lib, self._lib.ac_cluster_cut(self._h, cutoff, m, len(manual), out, C.byref(n)))
        return list(out)[:n.value]

    def assign(self, cluster_nodes, lengths):
        """ac_cluster_assign: (cluster per tip after reorder_clusters, cluster_dist per reordered cluster); lengths: one per tip"""
        cluster_nodes, lengths = list(cluster_nodes), list(lengths)
        n_tips = self._n_tips()
        if len(lengths) != n_tips:
            raise AutocyclerError(f"{len(lengths)} lengths for {n_tips} tips")
        cn = (C.c_uint16 * max(len(cluster_nodes), 1))(*cluster_nodes)
        ln = (C.c_uint64 * n_tips)(*lengths)
        of_seq, dist, nc = (C.c_uint16 * n_tips)(), (C.c_double * max(len(cluster_nodes), 1))(), C.c_uint32()
        _check(self._lib, self._lib.ac_cluster_assign(self._h, cn, len(cluster_nodes), ln, of_seq, dist, C.byref(nc)))
        return list(of_seq), list(dist)[:nc.value]

    def _qc_inputs(self, distances, seq_len, assembly, cluster_weight, trusted):
        ptr, n, keep = _double_matrix(distances)
        arrays = []
        for name, values, ctype in (("seq_len", seq_len, C.c_uint64), ("assembly", assembly, C.c_uint32), ("cluster_weight", cluster_weight, C.c_uint32),
                                    ("trusted", trusted, C.c_uint8)):
            values = [int(v) for v in values]
            if len(values) != n:
                raise AutocyclerError(f"{len(values)} entries of {name} for a matrix of {n} rows")
            arrays.append((ctype * max(n, 1))(*values))
        return ptr, n, keep, arrays

    def generate(self, distances, seq_len, assembly, cluster_weight, trusted, cutoff, min_assemblies, manual=(), device=0):
        """ac_cluster_generate: generate_clusters (cluster.rs:497-508) -> ClusterQC.  distances: the S x S asymmetric matrix (rows in tip
        order); the four lists: one entry per tip (Graph.cluster_inputs()); manual: node ids, or empty for the cut at `cutoff` refined by
        refine_auto_clusters."""
        ptr, n, _keep, (ln, asm, wt, tr) = self._qc_inputs(distances, seq_len, assembly, cluster_weight, trusted)
        manual = list(manual)
        m = (C.c_uint16 * max(len(manual), 1))(*manual)
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_cluster_generate(self._h, ptr, n, ln, asm, wt, tr, cutoff, min_assemblies, m, len(manual), device, C.byref(h)))
        return ClusterQC(self._lib, h)

    def qc(self, cluster_nodes, distances, seq_len, assembly, cluster_weight, trusted, cutoff, min_assemblies, manual=(), device=0):
        """ac_cluster_qc_nodes: qc_clusters (cluster.rs:511-570) and clustering_metrics on the given node list, without refinement -> ClusterQC"""
        ptr, n, _keep, (ln, asm, wt, tr) = self._qc_inputs(distances, seq_len, assembly, cluster_weight, trusted)
        manual, cluster_nodes = list(manual), list(cluster_nodes)
        m = (C.c_uint16 * max(len(manual), 1))(*manual)
        cn = (C.c_uint16 * max(len(cluster_nodes), 1))(*cluster_nodes)
        h = C.c_void_p()
        _check(self._lib, self._lib.ac_cluster_qc_nodes(self._h, ptr, n, ln, asm, wt, tr, cutoff, min_assemblies, cn, len(cluster_nodes), m, len(manual),
                                                        device, C.byref(h)))
        return ClusterQC(self._lib, h)

    def newick(self, names=None, file_form=False):
        """tree_to_newick, or with file_form the line save_tree_to_newick writes.  names: one per tip (default: the graph's
        default_tip_names(), or the ids for a tree that came from a matrix or from nodes)"""
        names = self.tip_names if names is None else names
        arr = None
        if names is not None:
            if len(names) != self._n_tips():
                raise AutocyclerError(f"{len(names)} names for {self._n_tips()} tips")
            arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
        out = C.c_void_p()
        _check(self._lib, self._lib.ac_cluster_newick(self._h, arr, 1 if file_form else 0, C.byref(out)))
        s = C.string_at(out.value).decode()
        self._lib.ac_string_free(out)
        return s


class ClusterQC:
    """The result of ClusterTree.generate / ClusterTree.qc (an ac_cluster_qc, read out once): clusters = the node ids; cluster_of_seq = the
    reordered cluster number per tip; records = one dict per reordered cluster (node, container, size, assembly_count, fail, trusted,
    median_length, cluster_dist; fail bits 1 = not in manual clusters, 2 = too few assemblies, 4 = contained); metrics = ClusteringMetrics;
    trace = per refinement round {"scores": [...], "accepted": [...]} in split_clusters' order; summary = the device schedule."""

    def __init__(self, lib, h):
        try:
            p16, n = C.POINTER(C.c_uint16)(), C.c_uint32()
            _check(lib, lib.ac_cluster_qc_clusters(h, C.byref(p16), C.byref(n)))
            self.clusters = [p16[i] for i in range(n.value)]
            _check(lib, lib.ac_cluster_qc_assignment(h, C.byref(p16), C.byref(n)))
            self.cluster_of_seq = [p16[i] for i in range(n.value)]
            pr = C.POINTER(ClusterQcRecord)()
            _check(lib, lib.ac_cluster_qc_records(h, C.byref(pr), C.byref(n)))
            self.records = [pr[i].as_dict() for i in range(n.value)]
            m = ClusteringMetrics()
            _check(lib, lib.ac_cluster_qc_metrics(h, C.byref(m)))
            self.metrics = m.as_dict()
            pa, nr, ps, pacc, ns = C.POINTER(C.c_uint32)(), C.c_uint32(), C.POINTER(C.c_double)(), C.POINTER(C.c_uint8)(), C.c_uint64()
            _check(lib, lib.ac_cluster_qc_trace(h, C.byref(pa), C.byref(nr), C.byref(ps), C.byref(pacc), C.byref(ns)))
            self.trace, at = [], 0
            for r in range(nr.value):
                self.trace.append({"scores": [ps[at + i] for i in range(pa[r])], "accepted": [bool(pacc[at + i]) for i in range(pa[r])]})
                at += pa[r]
            assert at == ns.value
            sm = ClusterQcSummary()
            assert lib.ac_cluster_qc_summary_get_sized(h, C.byref(sm), C.sizeof(ClusterQcSummary)) == C.sizeof(ClusterQcSummary)
            self.summary = sm.as_dict()
        finally:
            lib.ac_cluster_qc_free(h)


def cluster_min_assemblies(assembly, lib_path=None):
    """ac_cluster_min_assemblies: set_min_assemblies (cluster.rs:645-661) for the dense assembly indices of the sequences"""
    lib = load_library(lib_path)
    assembly = [int(a) for a in assembly]
    out = C.c_uint32()
    _check(lib, lib.ac_cluster_min_assemblies((C.c_uint32 * max(len(assembly), 1))(*assembly), len(assembly), C.byref(out)))
    return out.value


def _double_matrix(distances):
    n = len(distances)
    try:
        import numpy as np
        if isinstance(distances, np.ndarray):
            a = np.ascontiguousarray(distances, dtype=np.float64)
            if a.shape != (n, n):
                raise AutocyclerError("the distance matrix is not square")
            return a.ctypes.data_as(C.c_void_p), n, a
    except ImportError:
        pass
    if any(len(r) != n for r in distances):
        raise AutocyclerError("the distance matrix is not square")
    arr = (C.c_double * max(n * n, 1))(*[x for r in distances for x in r])
    return arr, n, arr


def cluster_tree(distances, ids, normalise=True, device=0, lib_path=None):
    """ac_cluster_tree_from_distances: make_symmetrical_distances and upgma on the caller's asymmetric S x S matrix (lists of lists or a numpy
    array, row a / column b = distance a vs b) and ascending sequence ids -> ClusterTree."""
    lib = load_library(lib_path)
    ptr, n, _keep = _double_matrix(distances)
    ids = list(ids)
    if len(ids) != n:
        raise AutocyclerError(f"{len(ids)} ids for a matrix of {n} rows")
    if any(not 0 <= i <= 0xFFFF for i in ids):
        raise AutocyclerError("a sequence id is not a u16")
    h = C.c_void_p()
    _check(lib, lib.ac_cluster_tree_from_distances(ptr, (C.c_uint16 * max(n, 1))(*ids), n, 1 if normalise else 0, device, C.byref(h)))
    return ClusterTree(lib, h)


def max_cluster_seqs(lib_path=None):
    """ac_cluster_max_seqs: the most sequences the merge loop takes"""
    return load_library(lib_path).ac_cluster_max_seqs()


def cluster_containment(distances, cluster_of_seq, n_clusters, cutoff, lib_path=None):
    """ac_cluster_containment: ({(x, y): contain_count}, {(x, y): total_count}) over the ordered pairs of different clusters 1 .. n_clusters"""
    lib = load_library(lib_path)
    ptr, n, _keep = _double_matrix(distances)
    if len(cluster_of_seq) != n:
        raise AutocyclerError(f"{len(cluster_of_seq)} cluster numbers for a matrix of {n} rows")
    cs = (C.c_uint16 * max(n, 1))(*cluster_of_seq)
    cc, tc = (C.c_uint64 * max(n_clusters * n_clusters, 1))(), (C.c_uint64 * max(n_clusters * n_clusters, 1))()
    _check(lib, lib.ac_cluster_containment(ptr, n, cs, n_clusters, cutoff, cc, tc))
    pairs = [(x, y) for x in range(1, n_clusters + 1) for y in range(1, n_clusters + 1) if x != y]
    at = lambda x, y: (x - 1) * n_clusters + (y - 1)
    return {p: cc[at(*p)] for p in pairs}, {p: tc[at(*p)] for p in pairs}


class ReadDepth:
    """Read-based unitig depths (set_read_depths, depth.rs:45-76) on the device: ac_depth_*.

    graphs: one entry per consensus graph, either a Graph handle or a pair (unitig sequences as bytes, links as (a, b) pairs of signed
    unitig numbers in L-line order, both directions present).  All graphs share one k-mer table."""

    def __init__(self, k, graphs, device=0, lib_path=None):
        self._lib = lib = load_library(lib_path)
        self._h = C.c_void_p()
        graphs = list(graphs)
        self.n_unitigs = []
        if graphs and all(isinstance(g, Graph) for g in graphs):
            hs = (C.c_void_p * len(graphs))(*[g._h for g in graphs])
            self.n_unitigs = [lib.ac_unitig_count(g._h) for g in graphs]
            _check(lib, lib.ac_depth_begin_handles(C.c_uint32(k), hs, C.c_uint32(len(graphs)), C.c_int(device), C.byref(self._h)))
            return
        arr = (DepthGraph * max(len(graphs), 1))()
        keep = []
        for i, (seqs, links) in enumerate(graphs):
            seqs = [bytes(s) for s in seqs]
            blob = b"".join(seqs)
            begin, at = [], 0
            for s in seqs:
                begin.append(at); at += len(s)
            n = len(seqs)
            c_blob = C.create_string_buffer(blob, max(len(blob), 1))
            c_begin = (C.c_uint64 * max(n, 1))(*begin)
            c_len = (C.c_uint32 * max(n, 1))(*[len(s) for s in seqs])
            c_links = (Link * max(len(links), 1))(*[Link(a, b) for a, b in links])
            keep.append((c_blob, c_begin, c_len, c_links))
            arr[i].seq_bytes, arr[i].seq_begin, arr[i].seq_len = C.addressof(c_blob), C.addressof(c_begin), C.addressof(c_len)
            arr[i].n_unitigs, arr[i].links, arr[i].n_links = n, C.addressof(c_links), len(links)
            self.n_unitigs.append(n)
        _check(lib, lib.ac_depth_begin(C.c_uint32(k), arr, C.c_uint32(len(graphs)), C.c_int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.ac_depth_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_reads(self, reads):
        """reads: a list of bytes objects (one read each)."""
        reads = [bytes(r) for r in reads]
        blob = b"".join(reads)
        off, at = [0], 0
        for r in reads:
            at += len(r); off.append(at)
        self.add_reads_raw(blob, off)

    def add_reads_raw(self, bases, read_off):
        """bases: bytes or a C-contiguous uint8 numpy array; read_off: len(reads) + 1 ascending offsets into it."""
        n = len(read_off) - 1
        if hasattr(read_off, "ctypes"):
            import numpy as np
            read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
            c_off = read_off.ctypes.data_as(C.c_void_p)
        else:
            c_off = (C.c_uint64 * (n + 1))(*read_off)
        c_bases = bases.ctypes.data_as(C.c_void_p) if hasattr(bases, "ctypes") else C.cast(C.c_char_p(bases), C.c_void_p)
        _check(self._lib, self._lib.ac_depth_add_reads(self._h, c_bases, c_off, C.c_uint64(n)))

    def add_fastq(self, path):
        _check(self._lib, self._lib.ac_depth_add_fastq(self._h, os.fsencode(str(path))))

    def totals(self):
        t = DepthTotals(size=C.sizeof(DepthTotals))
        _check(self._lib, self._lib.ac_depth_totals_get(self._h, C.byref(t)))
        return t.as_dict()

    def kmer_counts(self, kmers):
        """canonical k-mer values -> (present, assembly_occurrences, read_count), three lists."""
        kmers = list(kmers)
        n = len(kmers)
        q = (C.c_uint64 * max(n, 1))(*kmers)
        present = (C.c_uint8 * max(n, 1))(); occ = (C.c_uint32 * max(n, 1))(); cnt = (C.c_uint32 * max(n, 1))()
        _check(self._lib, self._lib.ac_depth_kmer_counts(self._h, q, C.c_uint64(n), present, occ, cnt))
        return list(present)[:n], list(occ)[:n], list(cnt)[:n]

    def depths(self, graph_index):
        """-> one entry per unitig of that graph: its read depth (float), or None where the reference leaves it without one."""
        n = self.n_unitigs[graph_index] if 0 <= graph_index < len(self.n_unitigs) else 0
        depth = (C.c_double * max(n, 1))(); has = (C.c_uint8 * max(n, 1))()
        _check(self._lib, self._lib.ac_depth_finish(self._h, C.c_uint32(graph_index), depth, has))
        return [depth[i] if has[i] else None for i in range(n)]


# ---- test hooks: one device primitive on numpy arrays (ac_selftest_*; tests/prim_cases.py holds the references) ----
SCAN_KINDS = {"incl_add_u32": 0, "excl_add_u32": 1, "incl_max_u32": 2, "excl_add_u64": 3}


def _np_in(a, dtype):
    import numpy as np
    return np.ascontiguousarray(a, dtype=dtype)


def selftest_scan(kind, values, in_place=False, misalign_in=0, misalign_out=0, device=0, lib_path=None):
    """ac_selftest_scan: kind is a key of SCAN_KINDS -> the scanned array."""
    import numpy as np
    lib = load_library(lib_path)
    a = _np_in(values, np.uint64 if kind == "excl_add_u64" else np.uint32)
    out = np.empty_like(a)
    _check(lib, lib.ac_selftest_scan(device, SCAN_KINDS[kind], a.ctypes.data, a.size, int(in_place), misalign_in, misalign_out, out.ctypes.data))
    return out


def selftest_radix(keys, vals, begin_bit, end_bit, prep_n=0, prep_bits=0, prep_reuse=False, device=0, lib_path=None):
    """ac_selftest_radix: vals of dtype int32 take the i32 form, anything else the u32 form -> (keys, vals) sorted on [begin_bit, end_bit)."""
    import numpy as np
    lib = load_library(lib_path)
    k = _np_in(keys, np.uint64)
    signed = np.asarray(vals).dtype == np.int32
    v = _np_in(vals, np.int32 if signed else np.uint32)
    ko, vo = np.empty_like(k), np.empty_like(v)
    _check(lib, lib.ac_selftest_radix(device, k.ctypes.data, v.ctypes.data, k.size, begin_bit, end_bit, int(signed), prep_n, prep_bits, int(prep_reuse),
                                      ko.ctypes.data, vo.ctypes.data))
    return ko, vo


def selftest_segments(op, seg, vals, n_segments, deferred_err=False, device=0, lib_path=None):
    """ac_selftest_segments: op "min" (reduce_by_segment) or "argmin" (segment_argmin) -> (out[n_segments], error word)."""
    import numpy as np
    lib = load_library(lib_path)
    s, v = _np_in(seg, np.uint32), _np_in(vals, np.uint64)
    out = np.empty(n_segments, dtype=np.uint64 if op == "min" else np.uint32)
    err = C.c_uint32()
    _check(lib, lib.ac_selftest_segments(device, {"min": 0, "argmin": 1}[op], s.ctypes.data, v.ctypes.data, s.size, n_segments, int(deferred_err), out.ctypes.data,
                                         C.byref(err)))
    return out, err.value


def selftest_sort_pairs_cmp(key_a, key_b, vals, device=0, lib_path=None):
    """ac_selftest_sort_cmp, form 0: sort_by_key_cmp of the keys (key_a[i], key_b[i]) with the payload vals[i] -> (key_a, key_b, vals)."""
    import numpy as np
    lib = load_library(lib_path)
    a, b, v = _np_in(key_a, np.uint64), _np_in(key_b, np.uint32), _np_in(vals, np.uint32)
    ao, bo, vo = np.empty_like(a), np.empty_like(b), np.empty_like(v)
    _check(lib, lib.ac_selftest_sort_cmp(device, 0, a.ctypes.data, b.ctypes.data, v.ctypes.data, a.size, ao.ctypes.data, bo.ctypes.data, vo.ctypes.data))
    return ao, bo, vo


def selftest_sort_indices_cmp(values, indices, device=0, lib_path=None):
    """ac_selftest_sort_cmp, form 1: sort_keys_cmp of `indices` by values[index] -> the sorted indices."""
    import numpy as np
    lib = load_library(lib_path)
    a, v = _np_in(values, np.uint64), _np_in(indices, np.uint32)
    vo = np.empty_like(v)
    _check(lib, lib.ac_selftest_sort_cmp(device, 1, a.ctypes.data, None, v.ctypes.data, v.size, None, None, vo.ctypes.data))
    return vo


def selftest_scan_pool(op="read", value=0, device=0, lib_path=None):
    """ac_selftest_scan_pool: op "read", "advance" (the epoch forward to value) or "invalidate" -> dict(cap, epoch, tickets) afterwards."""
    lib = load_library(lib_path)
    out = (C.c_uint64 * 3)()
    _check(lib, lib.ac_selftest_scan_pool(device, {"read": 0, "advance": 1, "invalidate": 2}[op], value, out))
    return dict(cap=out[0], epoch=out[1], tickets=out[2])


def selftest_wave(program, in_u64, aux_i32, live_mask, out_init, device=0, lib_path=None):
    """ac_selftest_wave: program number (WaveProgram, csrc/selftest_prims.inc); in_u64, aux_i32, out_init: 256 items; live_mask: 4 words."""
    import numpy as np
    lib = load_library(lib_path)
    i, a, m = _np_in(in_u64, np.uint64), _np_in(aux_i32, np.int32), _np_in(live_mask, np.uint64)
    out = np.array(out_init, dtype=np.uint64)
    assert i.size == 256 and a.size == 256 and m.size == 4 and out.size == 256
    _check(lib, lib.ac_selftest_wave(device, program, i.ctypes.data, a.ctypes.data, m.ctypes.data, out.ctypes.data))
    return out


# ---- test hooks: one facility of the device runtime on numpy arrays (csrc/selftest_runtime.inc; tests/runtime_cases.py holds the references) ----
FILL_KINDS = {"all": 0, "from": 1, "first": 2, "side_stream": 3}
FILL_TRIGGERS = {"none": 0, "launch": 1, "launch_full": 2, "launch_wave_kernel": 3, "copy_h2d": 4, "copy_d2h": 5, "copy_d2d": 6, "stream_sync": 7,
                 "arena_rewind": 8, "after_main": 9, "main_event": 10}
READ_PATHS = {"copy_d2h": 0, "batch": 1, "batch_twice": 2, "to_host": 3, "read_scalar": 4, "side_stream": 5}
ARENA_OPS = {"alloc": 0, "mark": 1, "rewind": 2, "reset": 3, "reserve": 4, "release_all": 5, "set_grow": 6}
LAUNCHERS = {"launch": 0, "launch_full": 1, "launch_wave_kernel": 2, "sized": 3}
ATOMIC_OPS = {"add32": 0, "add64": 1, "min32": 2, "max32": 3, "min64": 4, "max64": 5, "or32": 6, "or64": 7, "xor64": 8, "fetch_or32": 9, "fetch_and32": 10,
              "cas32": 11, "cas64": 12, "load32": 13, "wave_alloc32": 14, "wave_add64": 15}
ATOMIC_THREADS = 64 * 256
LAUNCH_SLOTS = 1024


def selftest_fills(regions, trigger, pattern, drop_on_reset=False, device=0, lib_path=None):
    """ac_selftest_fills: regions = [(bytes, kind, arg, byte)], pattern = the whole span's bytes -> (the span afterwards, (launches while queueing,
    launches up to and including the trigger))."""
    import numpy as np
    lib = load_library(lib_path)
    r = _np_in([(b, FILL_KINDS[k], a, v) for b, k, a, v in regions], np.uint64)
    span = np.array(pattern, dtype=np.uint8)
    launches = np.zeros(2, dtype=np.uint32)
    _check(lib, lib.ac_selftest_fills(device, r.ctypes.data, len(regions), FILL_TRIGGERS[trigger], int(drop_on_reset), span.ctypes.data, span.size, launches.ctypes.data))
    return span, (int(launches[0]), int(launches[1]))


def selftest_fill_order(n, byte1, w_lo, w_hi, w_val, from2, byte2, upto3, byte3, device=0, lib_path=None):
    """ac_selftest_fill_order -> the n bytes after fill, functor store, fill_bytes_from and fill_bytes_first."""
    import numpy as np
    lib = load_library(lib_path)
    out = np.empty(n, dtype=np.uint8)
    _check(lib, lib.ac_selftest_fill_order(device, n, byte1, w_lo, w_hi, w_val, from2, byte2, upto3, byte3, out.ctypes.data))
    return out


def selftest_readback(data, path, items, device=0, lib_path=None):
    """ac_selftest_readback: items = [(offset, bytes)] -> ([the bytes each item brought back], launches, read-backs)."""
    import numpy as np
    lib = load_library(lib_path)
    d = _np_in(data, np.uint8)
    it = _np_in(items, np.uint64).reshape(-1, 2)
    out = np.full(int(it[:, 1].sum()) + 1, 0xA5, dtype=np.uint8)
    counters = np.zeros(2, dtype=np.uint32)
    _check(lib, lib.ac_selftest_readback(device, d.ctypes.data, d.size, READ_PATHS[path], it.ctypes.data, it.shape[0], out.ctypes.data, counters.ctypes.data))
    assert out[-1] == 0xA5      # nothing was written behind the last item
    ends = np.cumsum(it[:, 1]).astype(np.int64)
    return [out[e - int(b):e] for e, b in zip(ends, it[:, 1])], int(counters[0]), int(counters[1])


def selftest_scalar_chain(values, device=0, lib_path=None):
    """ac_selftest_scalar_chain -> (what each read_scalar saw, launches, read-backs)."""
    import numpy as np
    lib = load_library(lib_path)
    v = _np_in(values, np.uint64)
    out = np.zeros_like(v)
    counters = np.zeros(2, dtype=np.uint32)
    _check(lib, lib.ac_selftest_scalar_chain(device, v.ctypes.data, v.size, out.ctypes.data, counters.ctypes.data))
    return out, int(counters[0]), int(counters[1])


def selftest_arena(ops, live, device=0, lib_path=None):
    """ac_selftest_arena: ops = [(name of ARENA_OPS, arg)], live[ordinal] = read that allocation back at the end -> (totals[n_ops, 3],
    placements[n_allocs, 3], wrong[n_allocs]: bytes that do not hold the ordinal, -1 where not read)."""
    import numpy as np
    lib = load_library(lib_path)
    o = _np_in([(ARENA_OPS[c], a) for c, a in ops], np.uint64).reshape(-1, 2)
    n_allocs = int((o[:, 0] == 0).sum())
    lv = _np_in(live, np.uint8)
    assert lv.size == n_allocs
    totals = np.zeros((len(ops), 3), dtype=np.uint64)
    allocs = np.zeros((max(n_allocs, 1), 3), dtype=np.uint64)
    wrong = np.full(max(n_allocs, 1), np.iinfo(np.uint64).max, dtype=np.uint64)
    lvp = np.zeros(max(n_allocs, 1), dtype=np.uint8); lvp[:n_allocs] = lv
    _check(lib, lib.ac_selftest_arena(device, o.ctypes.data, len(ops), totals.ctypes.data, allocs.ctypes.data, lvp.ctypes.data, wrong.ctypes.data))
    return totals, allocs[:n_allocs], wrong[:n_allocs].astype(np.int64)


def selftest_launch(which, n, device=0, lib_path=None):
    """ac_selftest_launch -> (slots[1024, 4] = {threads, sum, xor, lanes beyond n}, "grid too large" was thrown, launches)."""
    import numpy as np
    lib = load_library(lib_path)
    slots = np.zeros((LAUNCH_SLOTS, 4), dtype=np.uint64)
    info = np.zeros(2, dtype=np.uint32)
    _check(lib, lib.ac_selftest_launch(device, LAUNCHERS[which], n, slots.ctypes.data, info.ctypes.data))
    return slots, bool(info[0]), int(info[1])


def selftest_atomics(op, init, operand, target, n_words, expected=0, device=0, lib_path=None):
    """ac_selftest_atomics -> (the words afterwards, what each of the 16384 threads' calls returned)."""
    import numpy as np
    lib = load_library(lib_path)
    v, t = _np_in(operand, np.uint64), _np_in(target, np.uint32)
    assert v.size == ATOMIC_THREADS and t.size == ATOMIC_THREADS
    words = np.zeros(n_words, dtype=np.uint64); ret = np.zeros(ATOMIC_THREADS, dtype=np.uint64)
    _check(lib, lib.ac_selftest_atomics(device, ATOMIC_OPS[op], init, expected, v.ctypes.data, t.ctypes.data, n_words, words.ctypes.data, ret.ctypes.data))
    return words, ret


def selftest_side_order(mode, which, seed, n_words, device=0, lib_path=None):
    """ac_selftest_side_order: mode "after_main" or "main_event" -> the words the host saw."""
    import numpy as np
    lib = load_library(lib_path)
    out = np.zeros(n_words, dtype=np.uint32)
    _check(lib, lib.ac_selftest_side_order(device, {"after_main": 0, "main_event": 1}[mode], which, seed, n_words, out.ctypes.data))
    return out


def selftest_event_ring(kinds=None, device=0, lib_path=None):
    """ac_selftest_event_ring.  kinds None: read and clear; else kinds[0] = how the handle is taken ("main_event" / "mark"), kinds[1:] = the
    events taken before it is waited for (those or "after_main") -> dict(events_taken, recycled_waits)."""
    import numpy as np
    lib = load_library(lib_path)
    out = np.zeros(2, dtype=np.uint64)
    if kinds is None:
        _check(lib, lib.ac_selftest_event_ring(device, 0, None, 0, out.ctypes.data))
    else:
        k = _np_in([{"main_event": 0, "mark": 1, "after_main": 2}[x] for x in kinds], np.uint8)
        _check(lib, lib.ac_selftest_event_ring(device, 1, k.ctypes.data, k.size - 1, out.ctypes.data))
    return dict(events_taken=int(out[0]), recycled_waits=int(out[1]))


class VerifyReport(C.Structure):
    _fields_ = [("failed", C.c_uint32)] + [(n, C.c_uint64) for n in ("first_bad_unitig", "first_bad_link", "first_bad_path_entry", "first_bad_sequence",
                                                                      "first_bad_base", "unitigs", "links", "path_entries", "bases_checked",
                                                                      "self_mirror_links")] + [("seconds", C.c_double), ("checks", C.c_uint32),
                                                                                               ("first_bad_junction", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MultiInfo(C.Structure):
    _fields_ = [("n_ranks", C.c_uint32), ("transport", C.c_int)] + \
               [(n, C.c_uint64) for n in ("bytes_fragments", "bytes_bitmap", "bytes_degrees", "bytes_links", "bytes_queries", "bytes_answers",
                                          "bytes_reduce", "queries_total", "queries_sent_away", "table_capacity_max", "table_capacity_sum",
                                          "union_text_bytes", "fragments", "distinct")] + \
               [("seconds_total", C.c_double), ("seconds_exchange_max", C.c_double), ("candidates_total", C.c_uint64), ("candidates_owned_max", C.c_uint64),
                ("bytes_sibling", C.c_uint64), ("bytes_tail", C.c_uint64), ("degrees_open", C.c_uint64), ("bytes_received_max", C.c_uint64), ("path_runs_copied", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def compress_build_multi(k, assembly_count, seqs, devices, lib_path=None):
    """One job over several devices from this one process (ac_compress_build_multi).  seqs as for compress_build; devices: HIP
    ordinals, one per rank (repeats allowed: host-staged exchanges).  Returns (Graph, multi-info dict)."""
    lib = load_library(lib_path)
    seqs = list(seqs)
    arr = (SeqView * len(seqs))()
    keep = []
    for i, (fwd, length, sid) in enumerate(seqs):
        b = bytes(fwd)
        keep.append(b)
        arr[i].fwd, arr[i].length, arr[i].id = b, length, sid
    h = C.c_void_p()
    dv = (C.c_int * len(devices))(*devices)
    _check(lib, lib.ac_compress_build_multi(C.c_uint32(k), C.c_uint32(assembly_count), arr, C.c_uint32(len(seqs)), dv, C.c_int(len(devices)),
                                            C.byref(h)))
    info = MultiInfo()
    _check(lib, lib.ac_multi_info_get(h, C.byref(info)))
    return Graph(lib, h, len(seqs)), info.as_dict()


def compress_build(k, assembly_count, seqs, device=0, lib_path=None):
    """seqs: iterable of (padded_forward_bytes, unpadded_length, seq_id).  Replaces compress.rs:42-44."""
    lib = load_library(lib_path)
    seqs = list(seqs)
    arr = (SeqView * len(seqs))()
    keep = []
    for i, (fwd, length, sid) in enumerate(seqs):
        b = bytes(fwd)
        keep.append(b)
        arr[i].fwd, arr[i].length, arr[i].id = b, length, sid
    h = C.c_void_p()
    _check(lib, lib.ac_compress_build(C.c_uint32(k), C.c_uint32(assembly_count), arr, C.c_uint32(len(seqs)),
                                      C.c_int(device), C.byref(h)))
    return Graph(lib, h, len(seqs))
