"""autocycler_amd — MI355X-native hot path of `autocycler compress` (k-mer de Bruijn graph -> unitig GFA).

The compute lives in libautocycler_hip.so (hand-written HIP for gfx950 behind the C ABI declared in
include/autocycler_hip.h); this package is the thin host-side mirror used by the tests and benchmarks."""
from ._capi import (AutocyclerError, ClusterTree, Components, Graph, HipLibraryMissing, LIB_PATH, ReadDepth, compress_build, graph_from_gfa, load_library,
                    cluster_containment, cluster_min_assemblies, cluster_tree, components_from_links, graph_components, MergePlan, graph_merge_plan, merge_plan_from_links, MergedPaths, Subsets, Finished, merge_finish, Applied, apply_bridges, Cleaned, clean_graph, clean_gfa, Combined, combine_graphs, combine_handles, combine_gfas, combine_dir, gfa2fasta, gfa2fasta_file, TOPOLOGY_NAMES, parse_tig_numbers, gfa_segment_types, graph_subsets, subsets_from_paths, ClusterQC, overlap_alignment, path_distances, resolve_bridge_paths, trim_path_slices, Trimmed, trim_apply, trim_gfa, trim_dir, resolve_dir)  # noqa: F401

__version__ = "0.1.0"
