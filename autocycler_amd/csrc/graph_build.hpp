// Device graph build for the `autocycler compress` hot path: k-mer set -> unitigs -> links -> paths.
// Replaces KmerGraph::add_sequences (kmer_graph.rs:86-134), UnitigGraph::build_unitigs_from_kmer_graph
// + simplify_seqs + create_links' neighbour discovery + trim_overlaps (unitig_graph.rs:176-293) and the
// per-sequence path walk (unitig_graph.rs:407-465).  Output is the compacted graph in *seed order*
// (reference's initial unitig numbering: rank of each unitig's smallest k-mer, unitig_graph.rs:176-226
// with kmer_graph.rs:168-173); the order-dependent tail (link push order, renumber, expand_repeats) is
// host_tail.cpp.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "graph_types.hpp"
#include "trim_host.hpp"
#include "resolve_host.hpp"
#include "components_host.hpp"
#include "merge_host.hpp"
#include "subset_host.hpp"
#include "trim_apply_host.hpp"
#include "finish_host.hpp"
#include "apply_host.hpp"
#include "clean_host.hpp"
#include "combine_host.hpp"
#include "cluster_host.hpp"
#include "cluster_qc_host.hpp"

namespace ac {

struct SeqView {          // one padded, end-repaired forward sequence as at compress.rs:41
    const uint8_t* fwd;   // length + k - 1 bytes over ".ACGT"
    uint32_t length;      // unpadded length (number of forward k-mers)
};

struct BuildTimings {                   // seconds; device stages are bracketed by stream syncs
    double h2d = 0, pack = 0, insert = 0, collect_sort = 0, degree = 0, segment = 0, minkey = 0, rank = 0,
           paths = 0, links = 0, seqs = 0, d2h = 0, total_device = 0;
    double expand = 0;                  // expand_repeats passes on the device (level-scheduled)
    double analysis = 0;                // link push order + expand_repeats candidates + first renumber (device)
    double finalize = 0;                // second renumber + final numbering of links and paths (device)
    double insert_kernel_ms = 0;        // event-timed duration of the dominant kernel (k-mer insert)
    uint64_t insert_positions = 0;      // text positions streamed by that launch
    uint64_t table_capacity = 0;
    uint64_t n_distinct = 0;
    uint64_t n_path_entries = 0;
    uint32_t insert_launches = 0;       // phases of the run-following insert (same kernel, launched per phase)
    uint64_t insert_real = 0;           // positions that actually touched the table
    uint32_t simplify_passes = 0, n_candidates = 0, n_levels = 0;   // expand_repeats: passes, candidate junctions, conflict levels
    uint32_t n_candidates_owned = 0;    // ... and the candidate junctions THIS rank ran (a sharded build with a partitioned tail; else all of them)
    // sharded builds (one job over several devices)
    uint32_t local_hint = 0, graph_hint = 0;   // capacity hints of the local / graph table (assembly counts)
    double fragments = 0;               // novel runs of this rank -> fragment text
    double union_pack = 0, union_insert = 0;   // packing / inserting the union of all ranks' fragments
    uint64_t n_local_distinct = 0, n_fragments = 0, fragment_bytes = 0;
    double upload_device_ms = 0;        // host entry: first copy issued -> last chunk landed and packed (HIP events)
    double insert_rest_known = 0;       // share of a sample of the insert's one-launch rest found in the table after the first two stretches (sizes its chunks)
    uint64_t path_stretches = 0;        // the paths crossed to the host as this many stretches of consecutive text-order numbers (0: as entries)
    uint32_t expand_sparse_sweeps = 0;  // passes of expand_repeats that the one-workgroup tail ran from the list of dirty junctions (kernels_tail.inc expand_mopup_kernel)
    uint32_t expand_sparse_start = 0;   // ... and the dirty junctions on that list when it took over
    double insert_rest_sampled = 0;     // ... and the share of that rest the sample could cover (the text that was on the device when it was taken)
    uint32_t sort_retries = 0;          // builds repeated with checked sorts (a deferred "group too large" flag of the seed sort / a renumbering was set)
    uint32_t position_retries = 0;      // builds repeated with exact smallest positions (AC_POS_CAP; kernels_tail.inc exp_avoid_start_of_path)
    uint32_t launches = 0, readbacks = 0;   // kernel / fill launches and host round trips (mailbox, synchronising copies) of this build on its main stream
    uint64_t n_degrees_open = 0;        // sharded builds: k-mers the light degree step left to the probes (the compact degree exchange's size)
    uint64_t path_runs_copied = 0, path_entries_walked = 0;   // K10c: followed runs whose path entries were copied / entries that were really walked (0 / 0: the plain walk)
};

// sequence_end_repair (compress.rs:202-270) on the device.  d_text: the PADDED, unrepaired sequences in the text layout below;
// it is patched in place and d1 / d2 (surviving dots) are updated.
struct RepairTimings { double total = 0, scan_ms = 0; uint64_t hits = 0, matches = 0; uint32_t patterns = 0; };

class GraphBuilder {
  public:
    explicit GraphBuilder(uint32_t k);
    ~GraphBuilder();
    // Host entry: lays the sequences out as one text ('$' separators) chunk by chunk in a pinned staging ring and streams it to
    // the device; pack_now: K1 packs every chunk right behind its copy (the sequences are final, i.e. end-repaired already).
    void set_sequences_host(const std::vector<SeqView>& seqs, bool pack_now = true);
    // sequence_end_repair (compress.rs:202-270) on the text set_sequences_host(seqs, false) uploaded: patches it in place and
    // updates the surviving-dot counts; the build then packs the repaired text.
    void repair_ends(RepairTimings* tm);
    // Device entry: `d_text` is an ASCII text already resident in HBM with the same layout:
    // text[0] = '$', then for each sequence its padded bytes followed by one '$'.
    // off[s] = index of the first padded byte of sequence s.  d1/d2 = leading/trailing dot counts.
    void set_text_device(const uint8_t* d_text, uint64_t n_text, const std::vector<uint64_t>& off,
                         const std::vector<uint32_t>& len, const std::vector<uint16_t>& d1,
                         const std::vector<uint16_t>& d2);
    // The timed region (compress.rs:42-44): packed text -> final UnitigGraph in host memory.  Everything runs on
    // the device, including expand_repeats and both renumberings; the host only receives the results.
    void build(uint32_t assembly_count_hint, FinalGraph* out);

    // One job sharded by sequence over several devices, the k-mer table partitioned by key hash.  This rank's
    // sequences are set with set_text_device; the collectives between the phases are the caller's (torch.distributed / RCCL).
    //   1. shard_begin: pack + insert this rank's sequences into a LOCAL table, cut its novel runs out as "fragments".
    //      -> all-gather the fragment texts and meta records of all ranks (rank order) = the union text, on every rank.
    //   2. shard_build_union: this rank inserts the union-text k-mers it OWNS (owner = home hash mod n_shards) -> its share of
    //      the novel bitmap.  -> all-reduce SUM of the bitmaps (the owners partition the keys: the shares are disjoint).
    //   3. shard_build_novel: novel list (identical everywhere); degrees + first flags of ALL novel k-mers, probing only owned
    //      groups.  -> all-reduce SUM of the degree words.
    //   4. shard_build_graph: unitigs in seed order (identical everywhere); links, probing only owned groups.
    //      -> all-reduce SUM of the link words.
    //   5. links_import: the keys this rank's walkers start from.  -> all-gather of the keys; answer_queries (owned ones) on
    //      the keys of all ranks; all-reduce SUM of the answers.
    //   6. shard_walk: the paths of this rank's sequences.  -> all-reduce (SUM / MIN) the per-unitig buffers of reduce_export.
    //   7. reduce_import + shard_finish: the order-sensitive tail (identical on every rank); paths of this rank's sequences in
    //      final numbers (kept per rank, or gathered with paths_export to the rank that writes the GFA).
    void shard_begin(uint32_t local_assembly_hint);
    uint64_t local_distinct_count() const;                          // distinct canonical k-mers of this rank's slice
    void set_distinct_upper_bound(uint64_t n);                      // optional: sum of all ranks' local counts sizes the owned tables
    uint64_t fragment_text_bytes() const;
    uint64_t fragment_count() const;
    void fragments_export(void* d_text_out, void* d_meta_out);      // device buffers: text bytes, 8 bytes per fragment
    // The same text as 2-bit codes on the union text's word grid — a quarter of the bytes, and nothing to pack on the receiving side.
    // union_off = where this rank's stretch begins in the union text ('$' + the ranks' fragment texts in rank order).
    uint64_t fragment_packed_words(uint64_t union_off) const;
    void fragments_export_packed(uint64_t union_off, void* d_words_out, void* d_meta_out);
    // d_staged_words: the ranks' word stretches one behind the other (n_words[r] words of rank r, which begin at union word first_word[r])
    void shard_build_union_packed(uint32_t rank, uint32_t n_shards, const void* d_staged_words, const uint64_t* first_word, const uint64_t* n_words,
                                  uint64_t n_union_text, const void* d_meta, uint64_t n_frags_total);
    void shard_build_union(uint32_t rank, uint32_t n_shards, const uint8_t* d_union_text, uint64_t n_union_text,
                           const void* d_meta, uint64_t n_frags_total);
    uint64_t bitmap_words() const;                                  // u64 words of the union text's novel bitmap
    void bitmap_export(void* d_out);
    void shard_build_novel(const void* d_bitmap_sum);               // nullptr: single rank
    // round 5: this rank's sibling bits by novel index (2 bits per distinct k-mer); sib_words() == 0: not in use, the degree stage has run
    uint64_t sib_words() const;
    void sib_export(void* d_out);
    void shard_degrees(const void* d_sib_sum);                      // the degree stage, with the ranks' summed sibling bits
    uint64_t degree_bytes() const;                                  // size of the degree exchange (compact: the k-mers the light step left open)
    uint64_t distinct_count() const;                                // N: distinct canonical k-mers of the whole job
    void degrees_export(void* d_out);                               // degree_bytes() bytes: this rank's contributions
    void shard_build_graph(const void* d_kinfo_sum);                // degree_bytes() bytes (nullptr: single rank)
    uint32_t unitig_count() const;
    void links_export(void* d_links_i32, void* d_wlinks_i64);       // 10 U words each: this rank's contributions
    void links_import(const void* d_links_i32, const void* d_wlinks_i64);   // summed (nullptr, nullptr: single rank)
    uint64_t query_count() const;                                   // walk queries of this rank
    uint32_t query_key_words() const;                               // u64 words per query key
    void queries_export(void* d_out);
    void answer_queries(const void* d_keys, uint64_t n, void* d_out);   // n keys of any ranks -> n u64 (0 where this rank does not own the key)
    void shard_walk(const void* d_answers_mine);                    // query_count() u64
    // The same exchange routed by owner (one all-to-all each way instead of all-gather + SUM): the queries in owner order (stable),
    // counts_host[o] = how many of them rank o's table answers; the owners' answers come back in that order.
    void queries_route(uint32_t n_shards, void* d_routed_keys, uint64_t* counts_host);
    void shard_walk_routed(const void* d_routed_answers);
    void reduce_export(int32_t* d_sum, int32_t* d_min);             // 3U and 2U int32
    void reduce_import(const int32_t* d_sum, const int32_t* d_min);
    // Before shard_finish (optional, the same choice on every rank): an in-place all-reduce of a device buffer over the ranks (dtype 0 =
    // uint8, 1 = int32; op 0 = SUM, 1 = MIN).  With it expand_repeats runs on this rank's share of the junctions only — the conflict
    // components it owns — and the ranks' results are merged by two SUM all-reduces (field lengths, then the sequence bytes).
    void set_tail_exchange(std::function<void(void*, uint64_t, int, int)> all_reduce);
    void shard_finish(FinalGraph* out, bool want_graph, bool want_paths);
    uint64_t path_entry_count() const;
    void paths_export(void* d_out);                                 // int32 per entry, final numbers
    const BuildTimings& timings() const { return tm_; }
    void set_sequence_index_base(uint64_t n);   // a rank of a multi-device build: how many sequences of the job precede its slice (error messages)
    static void set_upload_threads_cap(int n);  // for the calling thread's builds: at most n packing threads (the ranks of a multi-device build share the host)
    uint64_t n_text() const;
    uint64_t n_bases() const;   // sum of unpadded lengths

    struct Impl;   // all device state of one build (graph_build.hip)

  private:
    void build_union_impl(uint32_t rank, uint32_t n_shards, const uint8_t* d_union_text, const void* d_staged_words, const uint64_t* first_word,
                          const uint64_t* n_words, uint64_t n_union_text, const void* d_meta, uint64_t n_frags_total);
    void upload_packed(const std::vector<SeqView>& seqs, const std::vector<uint64_t>& off);
    Impl* impl_;
    BuildTimings tm_;
};

// Builds the text layout used by both entries.  Returns the text; fills off/len/d1/d2.
std::vector<uint8_t> layout_text(const std::vector<SeqView>& seqs, uint32_t k, std::vector<uint64_t>* off,
                                 std::vector<uint32_t>* len, std::vector<uint16_t>* d1, std::vector<uint16_t>* d2);

void end_repair_device(uint32_t k, uint8_t* d_text, uint64_t n_text, const std::vector<uint64_t>& off, const std::vector<uint32_t>& len,
                       std::vector<uint16_t>* d1, std::vector<uint16_t>* d2, RepairTimings* tm, bool reset_arena = true);

// pairwise_contig_distances (cluster.rs:132-157) on the final graph: out[a * n_seqs + b], sequences in path order.
void pairwise_distances_device(const FinalGraph& g, uint32_t n_seqs, double* out);

// ac_verify_graph (kernels_verify.inc): the size-independent properties of a finished graph, checked on the device against the job's text.
struct VerifyReport {
    uint32_t failed = 0;                                   // bit mask of the checks that failed (VerifyFlag); 0 = the graph holds
    uint64_t first_bad_unitig = ~0ULL, first_bad_link = ~0ULL, first_bad_path_entry = ~0ULL, first_bad_sequence = ~0ULL, first_bad_base = ~0ULL;
    uint64_t unitigs = 0, links = 0, path_entries = 0, bases_checked = 0, self_mirror_links = 0;
    double seconds = 0;
    uint32_t checks = 0;                                   // VerifyCheck bits: which of the order-sensitive checks ran
    uint64_t first_bad_junction = ~0ULL;                   // 2 * unitig index + side (0 = its inputs, 1 = its outputs) that would still shift
};
void verify_graph_device(const FinalGraph& g, const uint8_t* d_text, uint64_t n_text, const std::vector<uint64_t>& off,
                         const std::vector<uint32_t>& len, VerifyReport* rep);

// reconstruct_original_sequences (unitig_graph.rs:362-400) for ALL sequences on the device: out_host holds sum(seq_len) bytes, sequence s behind s - 1.
void decompress_device(const FinalGraph& g, const std::vector<uint32_t>& seq_len, uint8_t* out_host);
// overlap_alignment (trim.rs:366-480) for a batch of jobs on the device (kernels_trim.inc); the host side of `trim` is trim_host.cpp.
struct TrimDeviceStats { double seconds_device = 0; uint64_t cells = 0; uint32_t jobs = 0, launches = 0; };
void overlap_alignment_batch(const std::vector<AlignJob>& jobs, const uint32_t* weights, uint32_t max_unitigs, std::vector<AlignOut>* outs,
                             TrimDeviceStats* st);
uint32_t trim_max_unitigs();      // largest min(max_unitigs, path length) the alignment kernels take
// global_alignment_distance (resolve.rs:387-418) for a batch of path pairs on the device (kernels_resolve.inc); the host side of `resolve` is resolve_host.cpp.
struct ResolveDeviceStats { double seconds_device = 0; uint64_t cells = 0, jobs = 0, largest_job_cells = 0; uint32_t launches = 0; };
void path_distance_batch(const PathPool& pool, const std::vector<PathPair>& pairs, const uint32_t* weights, std::vector<uint32_t>* dist,
                         ResolveDeviceStats* st);
uint32_t resolve_max_path();      // longest path the distance kernel takes
// upgma's merge loop (cluster.rs:395-480) on the device (kernels_cluster.inc): the n - 1 merges, rows = sequences in ascending id order; the
// tree and everything after it is cluster_host.cpp.  asym: the n x n matrix of pairwise_contig_distances on the host; the graph form
// computes it on the device in the same arena session (asym_out, when given, receives what pairwise_distances_device writes).
struct ClusterDeviceStats { double seconds = 0; uint64_t rescans = 0, compares = 0; uint32_t launches = 0; };
void cluster_merges_device(const double* asym, uint32_t n, std::vector<ClusterRowMerge>* merges, ClusterDeviceStats* st);
void cluster_merges_graph_device(const FinalGraph& g, uint32_t n_seqs, double* asym_out, std::vector<ClusterRowMerge>* merges, ClusterDeviceStats* st);
uint32_t cluster_max_seqs();      // most sequences the merge loop takes
// qc_clusters' matrix work on the device (kernels_cluster_qc.inc): starts an arena session, uploads the n x n matrix, packs the contain bits
// in the tree's depth-first tip order (dfs_tip: position -> row) and then runs `body`, handing it the function that evaluates one
// ClusterQcPlan (all alternatives of a refinement round): a fixed number of launches and one read-back each.  cluster_qc_host.cpp drives it.
struct ClusterQcDeviceStats {
    double seconds = 0;
    uint32_t launches = 0, readbacks = 0, evaluations = 0, pair_batches = 0;
    uint64_t alternatives = 0, pairs_counted = 0, bytes_read_back = 0;
};
void cluster_qc_device(const double* asym, uint32_t n, const uint32_t* dfs_tip, double cutoff, const std::function<void(const ClusterQcEvaluate&)>& body,
                       ClusterQcDeviceStats* st);
// connected_components / component_is_circular_loop / link_count / topology (unitig_graph.rs:478-545, 905-967) on the device
// (kernels_components.inc): links as ac_links hands them out, unitig_len / alive / marked one entry per unitig or null; totals and
// topology are components_host.cpp's.
void components_device(uint32_t n_unitigs, const Link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* marked,
                       ComponentsResult* out);
// The linear-path merge plan (graph_simplification.rs:315-371, 410-485) on the device (kernels_merge.inc): chains, members, merged sequences
// and the link set after the merge; numbers, depths, types and totals are merge_host.cpp's.  seed_fixed: merge_seed_fixed's bytes;
// path: the signed path entries whose histogram gives the position counts (or null); seq_bytes / seq_begin: both or neither, seq_total =
// the bytes behind seq_bytes.
struct MergePlanInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr;
    const uint8_t* seed_fixed = nullptr; const int32_t* path = nullptr; uint64_t n_path = 0;
    const uint8_t* seq_bytes = nullptr; const uint64_t* seq_begin = nullptr; uint64_t seq_total = 0;
};
void merge_plan_device(const MergePlanInput& in, MergeResult* out);
// Sequence subsets (kernels_subset.inc): per cluster of sequences the unitigs its paths visit with their position counts, and the links whose
// two ends it keeps, in the input's order.  plan: subset_prepare's; the entries of the kept sequences are uploaded cluster after cluster.
// Fills unitig_off, unitigs, positions, length_at, link_off and links of `out`; the rest is subset_host.cpp's.
struct SubsetInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr;
    const int32_t* path = nullptr; const uint64_t* path_off = nullptr; uint32_t n_clusters = 0; const SubsetPlan* plan = nullptr;
};
void subsets_device(const SubsetInput& in, SubsetResult* out);
// The paths of one cluster's kept sequences over the merged unitigs of a plan (kernels_subset.inc): every traversal of a chain becomes the
// chain's signed number.  kept_first / kept_count: the cluster's range of plan.kept_seq.
struct MergedPathsInput {
    uint32_t n_unitigs = 0; const uint32_t* unitig_len = nullptr; const int32_t* path = nullptr; const uint64_t* path_off = nullptr;
    const SubsetPlan* plan = nullptr; size_t kept_first = 0, kept_count = 0; const MergeResult* merge = nullptr;
};
void merged_paths_device(const MergedPathsInput& in, MergedPathsResult* out);
// trim's edit (kernels_trim_apply.inc): the slices of tp (trim_apply_choose's) are uploaded from the caller's paths and checked against their
// new lengths, trim_apply_exclude runs on the host in the middle, and the subset stages run with one cluster on the entries that are on the
// device already.  Fills tp's exclusion, the plan and `out` as subset_prepare + subsets_device would.  At least one entry in the slices.
struct TrimApplyInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr;
    const int32_t* path = nullptr; const uint64_t* path_off = nullptr; double mad = 0;
};
void trim_apply_device(const TrimApplyInput& in, TrimApplyPlan* tp, SubsetPlan* plan, SubsetResult* out);
// A finished graph (kernels_finish.inc): a merge plan applied to the arrays it was made from — the S-line order (renumbered or not), the
// gathered sequences, the L lines in get_links_for_gfa order and the relabelled path entries.  unitigs_after: finish_check_inputs'.
struct FinishInput {
    uint32_t n_unitigs = 0; const Link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const uint8_t* alive = nullptr;
    const double* depth = nullptr; const uint8_t* type = nullptr; const uint8_t* seq_bytes = nullptr; const uint64_t* seq_begin = nullptr; uint64_t seq_total = 0;
    const MergeResult* plan = nullptr; const int32_t* path = nullptr; uint64_t n_path = 0; bool renumber = false; uint64_t unitigs_after = 0;
};
void merge_finish_device(const FinishInput& in, FinishResult* out);
// apply_bridges, reduce_depths and the two removals (resolve.rs:223-282) on the device (kernels_apply.inc): plan: apply_prepare's.  Fills the
// per-unitig arrays over n_unitigs + the bridge unitigs, the links in get_links_for_gfa order and the bridge sequences; calls
// components_device in the middle.  n_unitigs > 0.
void apply_bridges_device(const ApplyInput& in, const ApplyPlan& plan, ApplyResult* out);
// `autocycler clean`'s edit (clean.rs:33-41) on the device (kernels_clean.inc): removal, duplication (clean_duplicate_edit on the host over the
// entries the device gathers) and remove_low_depth_unitigs in rounds.  in: checked by clean_prepare.  Fills the per-unitig arrays over
// n_unitigs + 2 per duplication, the links in get_links_for_gfa order, the rounds and the stats.  n_unitigs > 0.
void clean_device(const CleanInput& in, CleanResult* out);
// `autocycler combine`'s graph order, offsets, flags, topology and L-line order (combine.rs:144-224) on the device (kernels_combine.inc), for the
// concatenation of in.n_graphs graphs.  in: checked by combine_prepare; at least one unitig.  Fills the cluster and unitig records and the links
// in output order and the stats; combine_finish does the rest.
void combine_device(const CombineInput& in, CombineResult* out);
// device_prims.hpp against std:: on n pseudo-random items (tests); throws on a mismatch.
void primitives_selftest(uint64_t n, uint64_t seed, int end_bit, int key_kind);
// One primitive of device_prims.hpp / wave_rt.hpp on the caller's arrays (tests: the reference is the test's own): selftest_prims.inc.
void selftest_scan(int kind, const void* in, uint64_t n, bool in_place, int misalign_in, int misalign_out, void* out);
void selftest_radix(const uint64_t* keys, const void* vals, uint64_t n, int begin_bit, int end_bit, int val_kind, uint64_t prep_n, int prep_bits, bool prep_reuse,
                    uint64_t* keys_out, void* vals_out);
void selftest_segments(int op, const uint32_t* seg, const uint64_t* vals, uint64_t n, uint64_t n_segments, bool deferred_err, void* out, uint32_t* err_out);
void selftest_sort_cmp(int form, const uint64_t* a, const uint32_t* b, const uint32_t* vals, uint64_t n, uint64_t* a_out, uint32_t* b_out, uint32_t* vals_out);
void selftest_scan_pool(int op, uint64_t value, uint64_t* out);
void selftest_wave(int program, const uint64_t* in_u64, const int32_t* aux_i32, const uint64_t* live_mask, uint64_t* out_u64);
// One facility of the device runtime (device_rt.hpp) on the caller's data (tests: the reference is the test's own): selftest_runtime.inc.
void selftest_fills(const uint64_t* regions, uint64_t n_regions, int trigger, int mode, uint8_t* span, uint64_t span_bytes, uint32_t* launches_out);
void selftest_fill_order(uint64_t n, int byte1, uint64_t w_lo, uint64_t w_hi, int w_val, uint64_t from2, int byte2, uint64_t upto3, int byte3, uint8_t* out);
void selftest_readback(const uint8_t* data, uint64_t n_data, int path, const uint64_t* items, uint64_t n_items, uint8_t* out, uint32_t* counters_out);
void selftest_scalar_chain(const uint64_t* values, uint64_t n, uint64_t* out, uint32_t* counters_out);
void selftest_arena(const uint64_t* ops, uint64_t n_ops, uint64_t* totals_out, uint64_t* allocs_out, const uint8_t* live, uint64_t* wrong_out);
void selftest_launch(int which, uint64_t n, uint64_t* slots_out, uint32_t* info_out);
void selftest_atomics(int op, uint64_t init, uint64_t expected, const uint64_t* operand, const uint32_t* target, uint32_t n_words, uint64_t* words_out, uint64_t* returns_out);
void selftest_side_order(int mode, int which, uint32_t seed, uint64_t n_words, uint32_t* out_words);
void selftest_event_ring(int op, const uint8_t* kinds, uint32_t n_more, uint64_t* out);

// Measured ceilings of the device for random atomicCAS / random 8-byte reads on a 134 MB table, in 10^9 operations per second.
void random_access_ceilings(double* cas_gops, double* read_gops, uint64_t table_slots = (uint64_t)1 << 24);

// Brings the HIP context and this library's code objects up on `device` (first use costs ~0.2 s): callable from a helper
// thread while the caller is still busy on the host.
void device_warmup(int device, uint32_t k = 0, uint64_t text_bytes_estimate = 0);

// K1 on the host (what the packed upload of set_sequences_host runs per piece): n_text bytes -> (n_text + 31) / 32 words of 2-bit
// codes (first base most significant) and as many 32-bit mask words (bit i = byte i is not a base).
void pack_text_host(const uint8_t* text, uint64_t n_text, uint64_t* bits, uint32_t* mask32, bool force_scalar);

// Frees the pinned staging ring of the host entry (192 MB; it otherwise stays for the next build of the process).
void release_host_stager();

int max_supported_k();
// The environment knobs are read once per process (graph_impl.hpp: Knobs); these are the ones code outside the graph build asks for.
void tuning_refresh();                       // re-reads them if AC_TUNING_FOLLOW_ENV was set (tests, tools/ab_knobs.py); called under the build lock
int tuning_multi_transport();                // AC_MULTI_TRANSPORT: 0 unset, 1 host, 2 rccl
bool tuning_multi_fragments_as_bytes();      // AC_MULTI_FRAGMENTS=bytes
bool tuning_multi_tail_replicated();         // AC_MULTI_TAIL=replicated
void set_stage_timing(bool on);   // per-stage timers (a stream sync per stage); off by default
bool stage_timing();

}  // namespace ac
