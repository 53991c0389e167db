/* autocycler_hip.h — C ABI of libautocycler_hip.so, the MI355X (gfx950) drop-in for the hot path of
 * `autocycler compress` (rrwick/Autocycler v0.7.0).
 *
 * The reference has no FFI or plugin interface; the seam is cut in src/compress.rs:42-44:
 *
 *     let kmer_graph = build_kmer_graph(k_size, assembly_count, &sequences);   // KmerGraph::add_sequences, kmer_graph.rs:86-134
 *     let mut unitig_graph = build_unitig_graph(kmer_graph);                   // UnitigGraph::from_kmer_graph, unitig_graph.rs:36-48
 *     simplify_unitig_graph(&mut unitig_graph, &sequences);                    // simplify_structure, graph_simplification.rs:26-40
 *
 * ac_compress_build() replaces those three calls; the accessors hand back exactly what the consumers
 * (save_gfa unitig_graph.rs:317-331, save_metrics compress.rs:181-189, print_basic_graph_info
 * unitig_graph.rs:509-516) read.  INTEGRATION.md shows the Rust `extern "C"` block and the patch.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returning int returns 0 on
 * success and non-zero on failure; ac_last_error() then holds the text the Rust shim should pass to
 * quit_with_error (misc.rs:131-137).  The library never exits, aborts or unwinds across the ABI.
 * Inputs are only read during the call (the reference's raw pointers into Sequence buffers,
 * kmer_graph.rs:30,115, need not outlive it).  Results are owned by the handle until ac_free().
 * There is no CPU fallback: without a usable gfx950 device every build call fails with an error.
 */
#ifndef AUTOCYCLER_HIP_H
#define AUTOCYCLER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_graph ac_graph; /* opaque: the final unitig graph (UnitigGraph after simplify_structure) */

/* One loaded sequence as `load_sequences` returns it (compress.rs:98-133, sequence.rs:19-59). */
typedef struct {
    const uint8_t* fwd; /* Sequence::forward_seq: padded + end-repaired, length + k - 1 bytes over ".ACGT" */
    uint32_t length;    /* Sequence::length (unpadded) */
    uint16_t id;        /* Sequence::id (1-based; gaps allowed, compress.rs:111,120) */
} ac_seq_view;

typedef struct { uint32_t pos; uint16_t seq_id_and_strand; } ac_position; /* position.rs:18-22; strand = bit 15 */
/* A link a -> b (UnitigStrand pairs, unitig_graph.rs:234-287) as two SIGNED unitig numbers: +n = the forward strand of unitig n, -n = its
 * reverse strand — the form of the reference's own path entries (get_unitig_path_for_sequence_i32).  ABI 7: 8 bytes; ABI <= 6 carried
 * { uint32_t a; uint8_t a_fwd; uint32_t b; uint8_t b_fwd; } = 16 bytes with padding (the link array is the largest late result of a
 * mixed-species build and crosses PCIe behind everything else). */
typedef struct { int32_t a; int32_t b; } ac_link;
typedef struct { uint32_t unitigs; uint64_t links_one_way; uint64_t total_length; } ac_stats;

/* Seconds spent in each stage of the last build.  The per-stage fields are only filled while stage timing is on
 * (ac_set_stage_timing(1): one stream synchronisation per stage, ~0.3 ms per build); total_device, insert_kernel_ms and
 * the counts are always filled. */
typedef struct {
    double h2d, pack, insert, collect_sort, degree, segment, minkey, rank, paths, links, seqs, d2h;
    double total_device; /* pack .. d2h: the whole replaced region */
    double expand;       /* expand_repeats passes (device, level-scheduled) */
    double insert_kernel_ms;    /* HIP-event duration of the k-mer insert kernel, summed over its phase launches */
    uint64_t insert_positions;  /* text positions those launches streamed */
    uint64_t table_capacity, n_distinct, n_path_entries;
    uint32_t simplify_passes;
    uint32_t insert_launches;   /* phases of the run-following insert (launches of that kernel per build) */
    uint64_t insert_real;       /* positions that really accessed the k-mer table (the rest were run-followed) */
    double analysis;            /* link push order, expand_repeats candidates, first renumber */
    double finalize;            /* second renumber, final numbering of links and paths */
    uint32_t n_candidates;      /* junctions that pass the static tests of expand_repeats */
    uint32_t n_levels;          /* conflict levels they are scheduled in */
    /* sharded builds only */
    double fragments;           /* cutting this rank's novel runs out of its text */
    double union_pack, union_insert;   /* packing / inserting the union of all ranks' fragments */
    uint64_t n_local_distinct, n_fragments, fragment_bytes;
    double upload_device_ms;    /* ac_compress_build only: the upload from its first byte to its last chunk on the device (host clock when the packers
                                 * store into device memory themselves, HIP events around the copies of the pinned-ring path) */
    uint64_t path_runs_copied, path_entries_walked;   /* the copying path walk: runs whose entries were copied, entries really walked (0, 0: plain walk) */
    uint64_t position_retries;   /* builds repeated with exact smallest positions because expand_repeats met a common sequence longer than the bound kept (AC_POS_CAP) */
    uint32_t n_candidates_owned; /* the candidate junctions THIS rank ran (a job over several devices with a partitioned tail; else = n_candidates) */
    uint32_t launches;           /* kernel launches of this build on its main stream (fused fills count once per batch) */
    uint32_t readbacks;          /* host round trips of this build: small device -> host reads the host waited for */
    uint64_t n_degrees_open;     /* sharded builds: k-mers whose degrees the sibling bits did not settle (= bytes of the compact degree exchange) */
    uint64_t sort_retries;       /* builds repeated because a sort's "group too large" flag, read with the last read-back, was set */
    double insert_rest_known;    /* share of a sample of the insert's one-launch rest that the first two stretches already held (sizes the rest's chunks); 0 = no such rest */
    double insert_rest_sampled;  /* share of that rest the sample could cover: only text that was on the device when it was taken (an upload still in flight: its first chunks) */
    uint64_t path_stretches;     /* > 0: the path entries crossed to the host as this many stretches of consecutive text-order numbers (8 bytes each) and were written out there */
    uint32_t expand_sparse_sweeps; /* passes of expand_repeats run by the one-workgroup tail from the list of dirty junctions (0: level launches to the end) */
    uint32_t expand_sparse_start;  /* ... and the length of that list when it took over */
} ac_timings;

/* Replaces compress.rs:42-44.  k: --kmer (odd).  assembly_count: the reference's capacity hint
 * (kmer_graph.rs:40), used the same way (initial table sizing).  device: HIP device ordinal. */
int ac_compress_build(uint32_t k, uint32_t assembly_count, const ac_seq_view* seqs, uint32_t n_seqs, int device,
                      ac_graph** out);

/* The same over SEVERAL devices of one node, still one call from one process: devices[r] = HIP ordinal of rank r.  The
 * library runs one host thread per device; the sequences are sharded by rank (contiguous slices balanced by bases), the k-mer table is
 * partitioned over the ranks by key hash, and the exchanges between the phases of the build happen inside the library: RCCL over xGMI
 * (ncclAllReduce, and grouped ncclSend / ncclRecv that route every walk-start key to the one rank that owns it), loaded on first use.  A
 * device may be named more than once (those ranks then share it and the exchanges are staged through host memory: tests and dry runs);
 * AC_MULTI_TRANSPORT=host|rccl overrides the choice.  The graph is the one ac_compress_build builds (byte-identical GFA); n_devices = 1
 * is allowed.  Rust: the shim of INTEGRATION.md passes the ordinals it wants instead of one `device`. */
int ac_compress_build_multi(uint32_t k, uint32_t assembly_count, const ac_seq_view* seqs, uint32_t n_seqs, const int* devices,
                            int n_devices, ac_graph** out);
/* What the multi-device build behind a graph moved between its ranks (n_ranks = 0: a single-device build). */
typedef struct {
    uint32_t n_ranks; int transport;   /* transport: 1 = staged through host memory, 2 = RCCL, 3 = one rank: built as a single-device job */
    uint64_t bytes_fragments, bytes_bitmap, bytes_degrees, bytes_links, bytes_queries, bytes_answers, bytes_reduce;   /* received, all ranks */
    uint64_t queries_total, queries_sent_away;        /* walk-start queries of all ranks / those another rank answered */
    uint64_t table_capacity_max, table_capacity_sum;  /* slots of the ranks' shares of the job's k-mer table */
    uint64_t union_text_bytes, fragments, distinct;
    double seconds_total, seconds_exchange_max;
    /* expand_repeats partitioned by conflict component: candidate junctions of the job / the most any one rank ran */
    uint64_t candidates_total, candidates_owned_max;
    /* round 5 */
    uint64_t bytes_sibling;      /* the sibling bits (2 per distinct k-mer), received, all ranks */
    uint64_t bytes_tail;         /* the partitioned tail's merges (field lengths, sequence bytes) */
    uint64_t degrees_open;       /* k-mers the light degree step left to the probes (bytes_degrees is their exchange) */
    uint64_t bytes_received_max; /* the most any ONE rank received from the others over the whole build */
    uint64_t path_runs_copied;   /* pieces of followed runs the ranks' copying walks copied instead of walking (their local inserts note the runs; 0: all text walked) */
} ac_multi_info;
int ac_multi_info_get(const ac_graph*, ac_multi_info* out);
/* The same for a caller compiled against an older header: at most out_size bytes are written (the struct only grows at its end); returns
 * the library's own sizeof(ac_multi_info). */
size_t ac_multi_info_get_sized(const ac_graph*, ac_multi_info* out, size_t out_size);

/* ---- the round-trip verifier: what the reference's own tests hold a compress result to (tests.rs:108-127), as device
 * kernels over the result arrays of `graph` and the job's sequences — for inputs no CPU oracle can hold:
 *   every path spells its input sequence base for base (reconstruct_original_sequences, unitig_graph.rs:362-400; decompress.rs:83-105);
 *   every step of every path is a link, links are unique and come in reverse-complement pairs (check_links, unitig_graph.rs:752-793);
 *   depth == number of path occurrences (unitig.rs:149-156); unitigs are in renumber_unitigs order (unitig_graph.rs:295-315);
 *   the statistics are consistent (total_length, link_count().1, kmers.len() == 2 x pre-simplification length).
 * Returns 0 when the checks RAN (report->failed says what they found: 0 = the graph holds), non-zero on a usage error (ac_last_error).
 * `failed` bits: 1 unitig length / range, 2 renumber order, 4 link endpoint out of range, 8 duplicate link, 16 link without mirror,
 * 32 path entry out of range, 64 path step that is no link, 128 path length != sequence length, 256 a path does not spell its sequence,
 * 512 depth != occurrences, 1024 statistics.  first_bad_*: the smallest offending index of each kind (all ones: none).
 * Path offsets that do not ascend from 0 to the number of path entries end the run at once: failed = 128, first_bad_sequence = the first
 * sequence whose offsets are no range (the last sequence when the offsets end beside the entries), checks = 0 and nothing else filled in —
 * every other check reaches the entries through them.
 *
 * ABI 6 adds the three ORDER-SENSITIVE guarantees of the reference, so that a graph no CPU oracle can hold is checked as "the reference's
 * graph" and not only as "lossless and consistent" (the struct grew at its end: `checks`, `first_bad_junction`):
 *   2048  L-line order: the links are not in get_links_for_gfa order (unitig_graph.rs:333-350: unitigs ascending, forward_next before
 *         reverse_next, inside a list create_links' push order :248-286).  The order inside a class of one list is by SEED number, which a
 *         built graph carries and a graph reloaded from a GFA does not (`checks` bit 2 says whether that part ran);
 *   4096  maximality: a link a -> b that is a's only successor and b's only predecessor, and none of the walk's break cases
 *         (unitig_graph.rs:192-223: the end of a / start of b on a sequence-strand end, b == -a, b == a): a unitig cut in two
 *         (first_bad_link names it);
 *   8192  expand_repeats has not reached its fixed point (graph_simplification.rs:26-40): junction `first_bad_junction` = 2 x unitig index
 *         + side (0 = its exclusive inputs, 1 = its exclusive outputs) passes the reference's candidate test (:190-280) and its clamps
 *         (:145-181) still leave a shift > 0.
 * `checks`: 1 link order, 2 ... with seed numbers, 4 maximality, 8 fixed point — 4 and 8 need a link set that holds (no 4 / 8 / 16), 8 also
 * paths that add up. */
typedef struct {
    uint32_t failed;
    uint64_t first_bad_unitig, first_bad_link, first_bad_path_entry, first_bad_sequence, first_bad_base;
    uint64_t unitigs, links, path_entries, bases_checked, self_mirror_links;
    double seconds;
    uint32_t checks;
    uint64_t first_bad_junction;
} ac_verify_report;
/* seqs: the sequences the graph was built from, as for ac_compress_build (host memory; they are laid out and uploaded as text) */
int ac_verify_graph(const ac_graph* graph, const ac_seq_view* seqs, uint32_t n_seqs, int device, ac_verify_report* report);
/* the same against a text that is resident on the device (the layout ac_compress_build_device takes) */
int ac_verify_graph_device(const ac_graph* graph, const void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                           uint32_t n_seqs, int device, ac_verify_report* report);

/* reconstruct_original_sequences (unitig_graph.rs:362-400; decompress.rs:83-105) for ALL sequences of the graph on the device: sequence i lands
 * at out[sum of the lengths before it ...]; out_bytes >= the sum of the lengths (ac_graph_seq_info).  ac_decompress_seq is the per-sequence
 * host form. */
int ac_decompress_device(const ac_graph*, int device, uint8_t* out, uint64_t out_bytes);

/* Test hook: the library's own scan / radix sort / comparator sort kernels (csrc/device_prims.hpp) against the host's std:: algorithms on
 * n pseudo-random items; key_kind 0 uniform, 1 few distinct values, 2 sorted, 3 reverse sorted, 4 one hot digit.  0 = equal. */
int ac_selftest_primitives(int device, uint64_t n, uint64_t seed, int end_bit, int key_kind);

/* Test hooks, data in / data out: ONE primitive of csrc/device_prims.hpp or csrc/wave_rt.hpp on the caller's host arrays, its output handed
 * back — the reference is the caller's (tests/prim_cases.py: numpy and Python integers).  Additive to ABI 7.  All arrays are host memory.
 *   ac_selftest_scan       kind 0 u32 inclusive add, 1 u32 exclusive add, 2 u32 inclusive max, 3 u64 exclusive add; in / out hold n items of
 *                          that width.  in_place: the scan writes over its input.  misalign_in / misalign_out: the device pointers start that
 *                          many ELEMENTS behind a 16-byte boundary (below 4 for u32, below 2 for u64).  The grand total of an add scan must
 *                          stay below 2^46 for u64 items (the documented limit; a u32 scan is exact modulo 2^32 whatever its total); totals at
 *                          or above it and more than 2^32 items are outside what the hooks test.
 *   ac_selftest_radix      the stable sort of (u64 key, 32-bit value) pairs on key bits [begin_bit, end_bit).  val_kind 0: u32 values, 1: i32
 *                          values (no prepared scratch there).  prep_n != 0: a RadixScratch prepared for (prep_n items, prep_bits key bits) is
 *                          handed to the sort, which falls back to its own if that one is too small; prep_reuse != 0: the prepared scratch has
 *                          already been used up by another sort when the sort under test gets it.
 *   ac_selftest_segments   op 0: reduce_by_segment with the u64 minimum, out = uint64_t[n_segments]; op 1: segment_argmin with "the index of
 *                          the smaller vals[], the lower index on ties", out = uint32_t[n_segments].  seg: non-decreasing ids that step by one.
 *                          Entries of out that no segment wrote come back with all bits set.  deferred_err != 0: the error-word form, the word
 *                          in *err_out (bit 128: n_segments is not the number of segments); otherwise such a mismatch is an error return.
 *   ac_selftest_sort_cmp   form 0: sort_by_key_cmp of the keys (key_a[i], key_b[i]), compared field by field, with the payload vals[i]; form 1:
 *                          sort_keys_cmp of the indices vals[i] (each below n) by key_a[index] (key_b and the key outputs unused).  Both stable.
 *   ac_selftest_scan_pool  the calling thread's scan state pool.  op 0: read; 1: its epoch forward to `value` (never back, below 2^16); 2:
 *                          invalidate().  out[3] = {capacity in words, epoch, tickets handed out} afterwards.
 *   ac_selftest_wave       one workgroup of 256 threads; thread t returns before any cross-lane operation if bit t of live_mask[4] is clear,
 *                          the others run `program` — one primitive of wave_rt.hpp each, numbered as WaveProgram in csrc/selftest_prims.inc —
 *                          on in_u64[t] / aux_i32[t] (aux_i32[0] where the primitive takes one distance) and write out_u64[t]; a returned
 *                          thread's out_u64[t] stays as the caller left it. */
int ac_selftest_scan(int device, int kind, const void* in, uint64_t n, int in_place, int misalign_in, int misalign_out, void* out);
int ac_selftest_radix(int device, const uint64_t* keys, const void* vals, uint64_t n, int begin_bit, int end_bit, int val_kind, uint64_t prep_n, int prep_bits,
                      int prep_reuse, uint64_t* keys_out, void* vals_out);
int ac_selftest_segments(int device, int op, const uint32_t* seg, const uint64_t* vals, uint64_t n, uint64_t n_segments, int deferred_err, void* out, uint32_t* err_out);
int ac_selftest_sort_cmp(int device, int form, const uint64_t* key_a, const uint32_t* key_b, const uint32_t* vals, uint64_t n, uint64_t* key_a_out, uint32_t* key_b_out,
                         uint32_t* vals_out);
int ac_selftest_scan_pool(int device, int op, uint64_t value, uint64_t* out);
int ac_selftest_wave(int device, int program, const uint64_t* in_u64, const int32_t* aux_i32, const uint64_t* live_mask, uint64_t* out_u64);

/* Test hooks of the device runtime itself (csrc/device_rt.hpp), data in / data out as above: ONE facility on the caller's host arrays, the
 * reference is the caller's (tests/runtime_cases.py).  Additive (ABI 11).  Every bad argument is an error return before anything is launched.
 *   ac_selftest_fills        regions: n_regions x {bytes, kind, arg, byte}; kind 0 fill_bytes, 1 fill_bytes_from(arg), 2 fill_bytes_first(arg), 3
 *                            fill_bytes on a stream other than 0.  One arena run holds {256-byte sentinel, region rounded up to 256 (an empty one:
 *                            256)} per region and a last sentinel: span_bytes.  span: in = the pattern uploaded over all of it, out = all of it
 *                            afterwards.  trigger, what makes the queued fills go out: 0 nothing but the queue filling up (and the final read),
 *                            1 launch, 2 launch_full, 3 launch_wave_kernel, 4 copy_h2d, 5 copy_d2h, 6 copy_d2d, 7 stream_sync, 8 Arena::rewind, 9
 *                            SideStream::after_main, 10 SideStream::main_event.  mode 1: the fills are queued, then the arena is reset, the same
 *                            buffers allocated again and the pattern uploaded: it must come back intact.  launches_out[2] = kernel launches
 *                            counted {while queueing, up to and including the trigger}.
 *   ac_selftest_fill_order   fill(byte1) of n bytes, a functor that writes w_val over [w_lo, w_hi), fill_bytes_from(from2, byte2),
 *                            fill_bytes_first(upto3, byte3) -> out[n].
 *   ac_selftest_readback     uploads data[n_data], fetches items (n_items x {offset, bytes}) and writes them to out one behind the other.  path 0
 *                            copy_d2h per item, 1 one ReadBatch, 2 one ReadBatch object run twice (half the items each), 3 to_host, 4
 *                            read_scalar (4 or 8 aligned bytes), 5 copy_d2h on the side stream behind after_main.  counters_out[2] = {kernel
 *                            launches, read-backs} of the fetches.
 *   ac_selftest_scalar_chain n times: a functor stores values[i] into one device word, read_scalar fetches it -> out[i]; counters_out as above.
 *   ac_selftest_arena        ops: n_ops x {code, arg} on an arena that starts empty; 0 alloc(arg), 1 mark, 2 rewind(mark number arg), 3 reset, 4
 *                            reserve(arg), 5 release_all, 6 set_grow(arg).  totals_out: n_ops x {capacity, total_used, peak}; allocs_out: per alloc
 *                            {block ordinal, offset, address}.  Each allocation is filled with its ordinal's low byte on the device; at the end
 *                            those with live[ordinal] != 0 are read: wrong_out[ordinal] = bytes that hold something else.  The arena is left empty
 *                            with its own growth step.
 *   ac_selftest_launch       which 0 launch, 1 launch_full, 2 launch_wave_kernel over n logical threads: slots_out[1024 x 4] = per (workgroup
 *                            mod 1024) {threads, sum of their indices mod 2^64, xor of their indices, lanes beyond n}.  which 3:
 *                            launch_wave_kernel_sized with n blocks (0 or more than 2^24 - 1).  info_out[2] = {"grid too large" was thrown, launches}.
 *   ac_selftest_atomics      64 workgroups x 256 threads; thread t applies op to word target[t] (< n_words; all words start as init) with
 *                            operand[t].  op 0 add32, 1 add64, 2 min32, 3 max32, 4 min64, 5 max64, 6 or32, 7 or64, 8 xor64, 9 fetch_or32, 10
 *                            fetch_and32, 11 cas32, 12 cas64 (both compare with `expected`), 13 atomic_load32 of words an earlier launch set to
 *                            w * 2654435761 + init, 14 wave_alloc32, 15 wave_add64 (one counter per wavefront).  words_out[n_words], returns_out[16384].
 *   ac_selftest_side_order   a functor on stream 0 writes n_words words (i * 2654435761 + seed); mode 0: after_main(which), a copy on side
 *                            stream `which`, mark(which), wait_event; mode 1: main_event, wait_event, then the same copy -> out_words.
 *   ac_selftest_event_ring   op 0: reads and clears {events taken from the side stream's ring, waits on a handle whose slot had gone out again}
 *                            -> out[2].  op 1: clears, takes a handle (kinds[0]: 0 main_event, 1 mark), n_more further events (kinds[1 ..]: 0, 1,
 *                            2 after_main), waits for the handle, then as op 0. */
int ac_selftest_fills(int device, const uint64_t* regions, uint64_t n_regions, int trigger, int mode, uint8_t* span, uint64_t span_bytes, uint32_t* launches_out);
int ac_selftest_fill_order(int device, uint64_t n, int byte1, uint64_t w_lo, uint64_t w_hi, int w_val, uint64_t from2, int byte2, uint64_t upto3, int byte3, uint8_t* out);
int ac_selftest_readback(int device, const uint8_t* data, uint64_t n_data, int path, const uint64_t* items, uint64_t n_items, uint8_t* out, uint32_t* counters_out);
int ac_selftest_scalar_chain(int device, const uint64_t* values, uint64_t n, uint64_t* out, uint32_t* counters_out);
int ac_selftest_arena(int device, const uint64_t* ops, uint64_t n_ops, uint64_t* totals_out, uint64_t* allocs_out, const uint8_t* live, uint64_t* wrong_out);
int ac_selftest_launch(int device, int which, uint64_t n, uint64_t* slots_out, uint32_t* info_out);
int ac_selftest_atomics(int device, int op, uint64_t init, uint64_t expected, const uint64_t* operand, const uint32_t* target, uint32_t n_words, uint64_t* words_out,
                        uint64_t* returns_out);
int ac_selftest_side_order(int device, int mode, int which, uint32_t seed, uint64_t n_words, uint32_t* out_words);
int ac_selftest_event_ring(int device, int op, const uint8_t* kinds, uint32_t n_more, uint64_t* out);

/* The 2-bit packing the host entry applies before the upload (sequence.rs:39-48 validates the same alphabet): n_text bytes ->
 * (n_text + 31) / 32 words of 2-bit codes (A, C, G, T = 0..3, first base most significant) and as many 32-bit mask words
 * (bit i = byte i is not a base).  force_scalar != 0 selects the portable loop instead of the AVX2 / BMI2 one (both are
 * tested against each other and against the device kernel). */
int ac_pack_text(const uint8_t* text, uint64_t n_text, uint64_t* bits, uint32_t* mask32, int force_scalar);

/* Same, for a text that is already resident in device memory (benchmarks, multi-GPU shards):
 * d_text[0] = '$', then for every sequence its padded bytes followed by one '$'; n_text bytes in total.
 * seq_off[s] = index of the first padded byte of sequence s (host array). */
int ac_compress_build_device(uint32_t k, uint32_t assembly_count, const void* d_text, uint64_t n_text,
                             const uint64_t* seq_off, const uint32_t* seq_len, const uint16_t* seq_ids,
                             const uint16_t* seq_d1, const uint16_t* seq_d2, uint32_t n_seqs, int device,
                             ac_graph** out);

/* ---- one compress job over several devices: sequences sharded by rank, the k-mer table partitioned by key hash --
 * One process per device; every rank holds a slice of the job's sequences (rank order = sequence order) as a device text laid out
 * as above.  The library never communicates: the collectives between the phases belong to the caller (torch.distributed over
 * RCCL in autocycler_amd/sharded.py; anything that moves device buffers works).  Every exported buffer holds this rank's
 * CONTRIBUTIONS — the owners partition the keys, so the ranks' contributions are disjoint and a SUM all-reduce completes them.
 *
 *   ac_shard_begin            pack + insert this rank's sequences into a LOCAL table (KmerGraph::add_sequences on the slice), cut the
 *                             runs of rank-novel positions out as "fragments" (+ the first and last k-mer of every sequence, which
 *                             carry first_position, kmer_graph.rs:57-60)
 *   [all-gather]              fragment texts and 8-byte meta records of all ranks, concatenated in rank order;
 *                             union text = '$' + the concatenated fragment texts (every rank holds it)
 *   ac_shard_build_union      this rank inserts the union-text k-mers it OWNS: owner = hash of the k-mer's canonical middle mod
 *                             n_shards — the four successors of a k-mer share the middle, hence the owner — into a table of about
 *                             1/n_shards of the job's k-mers                          -> ac_shard_bitmap_export (novel positions)
 *   [all-reduce SUM int64]    the novel bitmaps (disjoint bits: the sum is the OR)
 *   ac_shard_build_novel      sorted novel list (identical on every rank).  If ac_shard_sib_words() > 0 afterwards (round 5; k >= 3):
 *   [all-reduce SUM uint64]     ac_shard_sib_export: the sibling bits this rank's insert collected, 2 per distinct k-mer by novel index
 *                               (two k-mers of one canonical middle that share their first or last base: the only way a k-mer's
 *                               text neighbour can have a second successor / predecessor; all k-mers of a middle have one owner)
 *   ac_shard_degrees            next_kmers / prev_kmers counts (kmer_graph.rs:136-166): with the summed sibling bits 97-99 % are settled
 *                               without a table access, the same on every rank; the rest, and the first flags, by probing the groups
 *                               this rank owns                                                       -> ac_shard_degrees_export
 *                             (ac_shard_sib_words() == 0: ac_shard_build_novel has run the degree stage itself, every degree by probing)
 *   [all-reduce SUM uint8]    ac_shard_degree_bytes() bytes: one per k-mer left open + four per flagged fragment end (compact), or
 *                             one per distinct k-mer
 *   ac_shard_build_graph      unitigs in seed order (identical on every rank); links (create_links, unitig_graph.rs:234-287),
 *                             probing only owned groups                                                   -> ac_shard_links_export
 *   [all-reduce SUM int32]    10 U link words, U = ac_shard_unitig_count() (the 10 U walk words are derived from them on import)
 *   ac_shard_links_import     the complete links; the keys this rank's path walkers start from      -> ac_shard_queries_export
 *   [all-gather]              the query keys of all ranks (ac_shard_query_count() x ac_shard_query_key_words() u64 per rank)
 *   ac_shard_answer           looks the owned ones among ALL ranks' keys up in this rank's table
 *   [all-reduce SUM int64]    the answers; every rank keeps the slice that answers its own queries
 *   ac_shard_walk             the paths of this rank's sequences (get_unitig_path_for_sequence, unitig_graph.rs:407-465)
 *   [all-reduce SUM, MIN]     ac_shard_reduce_export -> sum buffer (3U int32: depth, path starts, path ends) and min buffer
 *                             (2U int32: smallest forward / reverse position, biased so signed MIN orders them)
 *   ac_shard_reduce_import    the reduced buffers
 *   ac_shard_finish           link order, renumber, expand_repeats, final numbering (identical on every rank).  want: bit 0 =
 *                             unitigs + links to host memory, bit 1 = this rank's paths to host memory.  Either every rank
 *                             keeps the P lines of its own sequences (ac_gfa_string_parts), or:
 *   [gather]                  ac_shard_paths_export (final numbers) -> the writing rank calls ac_graph_set_paths with the
 *                             paths of all sequences in rank order
 * With n_shards == 1 the import pointers may be NULL (nothing to sum).  All `d_` pointers are device pointers into caller-owned
 * buffers of the stated sizes. */
typedef struct ac_shard ac_shard;
int ac_shard_begin(uint32_t k, uint32_t local_assembly_count, const void* d_text, uint64_t n_text, const uint64_t* seq_off,
                   const uint32_t* seq_len, const uint16_t* seq_ids, const uint16_t* seq_d1, const uint16_t* seq_d2,
                   uint32_t n_seqs, int device, ac_shard** out);
int ac_shard_fragment_sizes(const ac_shard*, uint64_t* text_bytes, uint64_t* n_fragments);
int ac_shard_fragments_export(ac_shard*, void* d_text_out /* text_bytes */, void* d_meta_out /* 8 * n_fragments */);
/* The same fragment text as 2-bit codes laid out on the UNION text's word grid (a quarter of the bytes over the links, and the receivers do
 * not pack again): union_off = where this rank's stretch begins in the union text (1 + the text bytes of the ranks before it).  Every rank's
 * words are all-gathered one behind the other; ac_shard_build_union_packed ORs them into place (rank r's n_words[r] words begin at union
 * word first_word[r] = union_off_r / 32) and derives the mask plane from the fragment records. */
uint64_t ac_shard_fragment_packed_words(const ac_shard*, uint64_t union_off);
int ac_shard_fragments_export_packed(ac_shard*, uint64_t union_off, void* d_words_u64, void* d_meta_out /* 8 * n_fragments */);
int ac_shard_build_union_packed(ac_shard*, uint32_t rank, uint32_t n_shards, const void* d_staged_words_u64, const uint64_t* first_word,
                                const uint64_t* n_words, uint64_t n_union_text, const void* d_meta, uint64_t n_fragments_total);
uint64_t ac_shard_local_distinct(const ac_shard*);                 /* distinct canonical k-mers of this rank's slice */
void ac_shard_set_distinct_upper_bound(ac_shard*, uint64_t n);     /* optional, before ac_shard_build_union: the sum of all ranks'
                                                                      local counts sizes the owned tables without a retry */
int ac_shard_build_union(ac_shard*, uint32_t rank, uint32_t n_shards, const void* d_union_text, uint64_t n_union_text,
                         const void* d_meta, uint64_t n_fragments_total);
uint64_t ac_shard_table_capacity(const ac_shard*);     /* slots of this rank's share of the job's k-mer table */
uint64_t ac_shard_bitmap_words(const ac_shard*);       /* u64 words of the union text's novel bitmap */
int ac_shard_bitmap_export(ac_shard*, void* d_out_u64);
int ac_shard_build_novel(ac_shard*, const void* d_bitmap_sum_u64 /* or NULL */);
uint64_t ac_shard_distinct_count(const ac_shard*);     /* N: distinct canonical k-mers of the whole job */
uint64_t ac_shard_sib_words(const ac_shard*);          /* after ac_shard_build_novel: u64 words of the sibling bits to sum (0: none, the degree stage has run) */
int ac_shard_sib_export(ac_shard*, void* d_out_u64 /* ac_shard_sib_words() */);
int ac_shard_degrees(ac_shard*, const void* d_sib_sum_u64);
uint64_t ac_shard_degree_bytes(const ac_shard*);       /* size of the degree exchange (after the degree stage) */
int ac_shard_degrees_export(ac_shard*, void* d_out_u8 /* ac_shard_degree_bytes() */);
int ac_shard_build_graph(ac_shard*, const void* d_degrees_sum_u8 /* ac_shard_degree_bytes(), or NULL */);
uint32_t ac_shard_unitig_count(const ac_shard*);       /* U: sizes the link and reduce buffers */
int ac_shard_links_export(ac_shard*, void* d_links_i32 /* 10 U */, void* d_wlinks_i64 /* 10 U, or NULL: not wanted */);
int ac_shard_links_import(ac_shard*, const void* d_links_sum_i32 /* or NULL: one rank */, const void* d_wlinks_sum_i64 /* or NULL: derived from the link words */);
uint64_t ac_shard_query_count(const ac_shard*);        /* walk queries of this rank */
uint32_t ac_shard_query_key_words(const ac_shard*);    /* u64 words per query key (depends on k only) */
int ac_shard_queries_export(ac_shard*, void* d_out_u64 /* query_count * query_key_words */);
int ac_shard_answer(ac_shard*, const void* d_keys_u64, uint64_t n_queries, void* d_out_u64 /* n_queries */);
int ac_shard_walk(ac_shard*, const void* d_answers_u64 /* query_count: this rank's slice of the summed answers */);
/* The same exchange routed by owner (north_star's bucket exchange; what ac_compress_build_multi does inside the library): the keys
 * ordered by owner rank, counts[r] of them for rank r -> all-to-all -> ac_shard_answer on what arrived -> reverse all-to-all ->
 * ac_shard_walk_routed with the answers in the order ac_shard_queries_route gave the keys.  A rank receives ~1/n_shards of the keys. */
int ac_shard_queries_route(ac_shard*, uint32_t n_shards, void* d_routed_keys_u64 /* query_count * query_key_words */,
                           uint64_t* counts /* n_shards */);
int ac_shard_walk_routed(ac_shard*, const void* d_routed_answers_u64 /* query_count */);
int ac_shard_reduce_export(ac_shard*, void* d_sum_i32 /* 3U */, void* d_min_i32 /* 2U */);
int ac_shard_reduce_import(ac_shard*, const void* d_sum_i32, const void* d_min_i32);
/* Optional, before ac_shard_finish, the same choice on every rank: an in-place all-reduce of a DEVICE buffer over the ranks (dtype 0 =
 * uint8, 1 = int32; op 0 = SUM, 1 = MIN; returns 0 on success), called from inside ac_shard_finish on the calling thread.  With it the
 * order-sensitive tail is no longer replicated in full: expand_repeats (graph_simplification.rs:43-86) runs on this rank's share of the
 * junctions — the conflict components it owns — and the ranks' results are merged by two SUM all-reduces (field lengths, sequence bytes). */
typedef int (*ac_allreduce_fn)(void* user, void* d_buf, uint64_t count, int dtype, int op);
int ac_shard_set_allreduce(ac_shard*, ac_allreduce_fn fn, void* user);
/* Plain copy between two buffers of `device` (or host memory), finished on return: for callers whose collectives want buffers of their
 * own (autocycler_amd/sharded.py stages ac_allreduce_fn's buffer through a torch tensor with it).  Takes no library lock. */
int ac_device_copy(void* dst, const void* src, uint64_t bytes, int device);
int ac_shard_finish(ac_shard*, int want, ac_graph** out);
uint64_t ac_shard_path_entries(const ac_shard*);
/* Only for ranks that did NOT keep their own paths: after ac_shard_finish(want & 2) the rank's entries got their final numbers in host
 * memory (the handle's paths; the device copy stays in seed numbers) and this call fails with an error (ABI 5). */
int ac_shard_paths_export(ac_shard*, void* d_out_i32 /* ac_shard_path_entries() */);
void ac_shard_free(ac_shard*);
/* path_counts[s] = number of path entries of sequence s; d_path_i32 = all entries, concatenated (device). */
int ac_graph_set_paths(ac_graph*, uint32_t n_seqs_total, const uint16_t* seq_ids, const uint32_t* seq_lens,
                       const uint64_t* path_counts, const void* d_path_i32, int device);
uint32_t ac_graph_seq_count(const ac_graph*);
int ac_path_counts(const ac_graph*, uint64_t* counts /* ac_graph_seq_count() */);   /* path entries per sequence */

/* sequence_end_repair (compress.rs:202-270) on the device, for a text that is already resident there: d_text holds the
 * PADDED, UNREPAIRED sequences (Sequence::new_with_seq, sequence.rs:31-59) in the layout above; the chosen matches are
 * patched into it in place and seq_d1 / seq_d2 (dots surviving at each end) are updated, so the same buffer can go straight
 * into ac_compress_build_device / ac_shard_begin.  One pass over the packed text replaces the reference's 2S regex scans. */
int ac_end_repair_device(uint32_t k, void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                         uint16_t* seq_d1, uint16_t* seq_d2, uint32_t n_seqs, int device, double* seconds, uint64_t* n_matches);

/* pairwise_contig_distances (cluster.rs:132-157), the first step of `autocycler cluster`, computed on the device from the
 * graph this library has just built: out[a * S + b] = 1 - len(unitigs shared by the paths of a and b) / len(unitigs of a),
 * S = ac_graph_seq_count(), sequences in input order. */
int ac_pairwise_distances(const ac_graph*, int device, double* out);

/* The compute of `autocycler trim` (trim.rs:45-47: trim_start_end_overlap :104-136, trim_harpin_overlap :139-186, the counts of
 * choose_trim_type :189-211) on the paths of a graph handle (a build, or ac_graph_from_gfa): overlap_alignment (trim.rs:366-480), a
 * (k + 1)^2 dynamic programme per sequence and kind with k = min(max_unitigs, path length), runs on the device for all sequences at once
 * (exact: int64 of the doubled f64 scores; one traceback bit per cell instead of the score matrix).  max_unitigs = 0 disables trimming as
 * in the reference; min(max_unitigs, path length) above ac_trim_max_unitigs() is an error, never a silent cap.
 * A result is the slice [begin, end) of the sequence's own path (ac_path) that survives and its length in bases:
 *   start_end: trim_path_start_end (trim.rs:288-296, find_midpoint :482-507);
 *   hairpin:   trim_path_hairpin_start (:320-326), then trim_path_hairpin_end (:299-317) on the start-trimmed path (:152-164);
 *              hairpin_start_trimmed / hairpin_end_trimmed say which of the two fired (the reference's message, :171-177).
 * status: 0 = not trimmed (the slice is the whole path), 1 = trimmed, 2 = the reference itself would have stopped on this input (the
 * assertion of trim.rs:310, or a path[start..end] that cannot be taken): reported, not guessed at; such a sequence counts as not trimmed.
 * Not done here: remove_sequence_from_graph, create_sequence_and_positions, exclude_outliers_in_length, clean_up_graph — ac_graph_trim_apply /
 * ac_trim_apply take this table and do them; ac_graph_trim and ac_trim_gfa run both halves in one call. */
typedef struct { uint32_t status, begin, end, trimmed_length; } ac_trim_slice;
typedef struct { ac_trim_slice start_end, hairpin; uint32_t hairpin_start_trimmed, hairpin_end_trimmed; } ac_trim_result;
typedef struct {
    uint64_t size;            /* in: sizeof the caller's ac_trim_summary (at most that many bytes are written); out: the library's */
    uint32_t c_se, c_hp;      /* sequences trimmed by start-end / by hairpin trimming */
    uint32_t chosen;          /* choose_trim_type: 0 = none, 1 = the start-end results, 2 = the hairpin results */
    uint32_t launches;        /* launches of the fill kernel (more than 2 when a phase ran in batches) */
    uint64_t cells;           /* matrix cells filled */
    double seconds_device;    /* the alignment kernels, by device events */
} ac_trim_summary;
int ac_trim_paths(const ac_graph*, double min_identity, uint32_t max_unitigs, int device, ac_trim_result* out /* ac_graph_seq_count() */,
                  ac_trim_summary* summary /* may be NULL */);
/* The same on caller-supplied paths: path_entries[path_off[s] .. path_off[s + 1]) signed unitig numbers, weights[u - 1] = length of unitig u. */
int ac_trim_path_slices(const int32_t* path_entries, const uint64_t* path_off, uint32_t n_seqs, const uint32_t* weights, uint32_t n_weights,
                        double min_identity, uint32_t max_unitigs, int device, ac_trim_result* out, ac_trim_summary* summary);
/* overlap_alignment (trim.rs:366-480) itself, one job through the same kernels: a, b of n entries each, weights[u - 1] = w(u).  pieces
 * holds 2 * min(n, max_unitigs) entries; *n_pieces = 0: no alignment.  A gap is unitig AC_ALIGN_GAP with index AC_ALIGN_NONE.
 * Errors (return 1, ac_last_error), never aborts: min_identity outside [0, 1], an entry that is 0 or beyond the weights, the weights of
 * one path adding up to 2^32 or more, min(n, max_unitigs) above ac_trim_max_unitigs(). */
#define AC_ALIGN_GAP 0
#define AC_ALIGN_NONE 0xFFFFFFFFu
typedef struct { int32_t a_unitig; uint32_t a_index; int32_t b_unitig; uint32_t b_index; } ac_alignment_piece;
int ac_overlap_alignment(const int32_t* a, const int32_t* b, uint32_t n, const uint32_t* weights, uint32_t n_weights, double min_identity,
                         uint32_t max_unitigs, int skip_diagonal, int device, ac_alignment_piece* pieces, uint32_t* n_pieces);
uint32_t ac_trim_max_unitigs(void);   /* 65536: the bit matrix of one alignment is then 537 MB */

/* The compute of `autocycler resolve` (resolve.rs:44-57) up to the point where the graph is edited: the anchor unitigs
 * (find_anchor_unitigs :134-163: the unitigs that occur exactly once, on either strand, in every sequence's path), the bridges between
 * consecutive anchors with their best paths (create_bridges :166-190, Bridge::new :430-462), their ambiguity (determine_ambiguity
 * :193-220) and the culling order (cull_ambiguity :285-313).  Bridge::new aligns every path of a bridge with every other one
 * (global_alignment_distance :387-418, an n x m dynamic programme in u32); here equal paths of a bridge are merged into distinct paths with
 * multiplicities, every unordered pair of distinct paths is one job, and the jobs of all bridges run on the device together (one wavefront
 * per job, exact: the same u32 arithmetic).  A sequence's paths count Sequence::consensus_weight times (sequence.rs:104-109; 0 leaves the
 * sequence out of the bridges, not out of the anchor test).
 * The bridges come in Bridge::cmp order (resolve.rs:506-514).  best path = best_paths[best_off .. best_off + best_len), start and end anchor
 * stripped as in the reference: the distinct path with the smallest (sum of distances to all other paths, path), paths compared as Rust
 * compares Vec<i32>.  The bridge's distinct paths are paths [first_distinct, first_distinct + n_distinct) of ac_resolve_distinct_paths, in
 * ascending path order, with their multiplicities (what reduce_depths, resolve.rs:261-270, subtracts).
 * status: 0 = fine; 2 = the reference's own u32 arithmetic would overflow on this bridge (two of its paths whose weights add up to 2^32 or
 * more, or a total at or above 2^32 - 1): reported, not guessed at, and no best path.  conflicting: the flag determine_ambiguity gives with
 * all bridges present; culled / cull_rank: cull_ambiguity removed it as the cull_rank-th (1-based; 0 = kept).
 * The edit itself is further down: ac_graph_resolve_apply / ac_apply_bridges (apply_bridges, reduce_depths and the removals), then
 * ac_applied_merge_plan and ac_applied_finish (merge_linear_paths, renumber_unitigs); ac_resolve_graphs runs all of it.
 * Errors (return 1, ac_last_error), never aborts: an entry that is 0 or beyond the weights, offsets that do not ascend, a path that enters a
 * distance job with more than ac_resolve_max_path() entries, a pair that names no path. */
typedef struct ac_resolve ac_resolve;
typedef struct {
    int32_t start, end;          /* signed unitig numbers of the two anchors */
    uint32_t depth;              /* Bridge::depth: the bridge's paths, copies counted */
    uint32_t n_distinct;
    uint64_t best_off;
    uint64_t best_total;         /* sum over the other paths of their distance to the best path */
    uint64_t first_distinct;
    uint32_t best_len, status;
    uint32_t conflicting, culled;
    uint32_t cull_rank, reserved;
} ac_bridge;
typedef struct {
    uint64_t size;               /* the library's sizeof(ac_resolve_summary) */
    uint64_t jobs;               /* distance jobs run on the device */
    uint64_t jobs_not_launched;  /* pairs that would overflow (status 2) */
    uint64_t cells;              /* matrix cells those jobs stand for */
    uint64_t largest_job_cells;
    uint32_t launches, reserved;
    double seconds_device;       /* the distance kernel, by device events */
} ac_resolve_summary;
/* On the paths of a graph handle (a build, or ac_graph_from_gfa: weights = unitig lengths, consensus weights from the HD:Z headers; a built
 * graph carries no headers and every sequence counts once). */
int ac_resolve_bridges(const ac_graph*, int device, ac_resolve** out);
/* The same on caller-supplied paths: path_entries[path_off[s] .. path_off[s + 1]) signed unitig numbers, weights[u - 1] = length of unitig u
 * (as for ac_trim_path_slices), consensus_weight[s] per sequence or NULL (all 1). */
int ac_resolve_bridge_paths(const int32_t* path_entries, const uint64_t* path_off, uint32_t n_seqs, const uint32_t* consensus_weight,
                            const uint32_t* weights, uint32_t n_weights, int device, ac_resolve** out);
int ac_resolve_anchors(const ac_resolve*, const uint32_t** anchors /* ascending unitig numbers */, uint32_t* n);
int ac_resolve_bridge_records(const ac_resolve*, const ac_bridge** bridges, uint32_t* n);
int ac_resolve_best_paths(const ac_resolve*, const int32_t** entries, uint64_t* n_entries /* may be NULL */);
/* any out pointer may be NULL; path_off holds n_paths + 1 offsets */
int ac_resolve_distinct_paths(const ac_resolve*, const int32_t** entries, const uint64_t** path_off, const uint32_t** multiplicity, uint64_t* n_paths);
/* at most out_size bytes are written (the struct only grows at its end); returns the library's sizeof(ac_resolve_summary) */
size_t ac_resolve_summary_get_sized(const ac_resolve*, ac_resolve_summary* out, size_t out_size);
void ac_resolve_free(ac_resolve*);
/* global_alignment_distance (resolve.rs:387-418) itself for a batch of pairs of the caller's paths, through the same kernel: dist[q] for
 * paths pair_a[q], pair_b[q].  status[q]: 0 = dist[q] holds; 2 = the two paths' weights add up to 2^32 or more (the reference's matrix
 * could overflow): not launched, dist[q] = 0. */
int ac_path_distances(const int32_t* entries, const uint64_t* path_off, uint32_t n_paths, const uint32_t* pair_a, const uint32_t* pair_b,
                      uint64_t n_pairs, const uint32_t* weights, uint32_t n_weights, int device, uint32_t* dist, uint8_t* status);
uint32_t ac_resolve_max_path(void);   /* 65536 entries: the longest path a distance job takes */

/* Connected components and graph topology: UnitigGraph::connected_components, component_is_circular_loop, link_count and topology
 * (unitig_graph.rs:478-545, 905-967) with the per-unitig end tests of unitig.rs:197-215, 276-293 — what resolve deletes components by
 * (resolve.rs:273-282), what merge_linear_paths starts from (fix_circular_loops, graph_simplification.rs:374-384) and what combine and
 * gfa2fasta print per unitig.  Read-only: no graph is edited here.
 * The graph is what build_links_from_gfa (unitig_graph.rs:91-115) makes of the link entries in their order: an entry (a, b) puts b into a's
 * next list (forward_next for a > 0, reverse_next otherwise) and a into b's prev list (forward_prev for b > 0, reverse_prev otherwise).
 * Entries may repeat (list lengths count repeats, link_count does not: it is two sets) and their reverse complements may be missing.  Two
 * unitigs are connected when any of the four lists of one names the other.  Components come in connected_components() order — ascending
 * lowest member — and their members ascend.  circular_loop is the literal walk of unitig_graph.rs:949-967 from (first, +): among its
 * consequences a single unitig with a hairpin link at both ends is a "loop".
 * Everything runs on the device in a number of launches that grows with log2(n_unitigs) only, never with the graph's diameter or its
 * number of components; the host reads a 48-byte header once the last kernel is done and then the results, sized by it.
 * Errors (return 1, ac_last_error), never faults: a link that names unitig 0 or one above n_unitigs (the first such entry is quoted), NULL
 * out, n_links > 0 without links, a handle without host arrays.  n_unitigs == 0 is a valid, empty result (topology "empty"). */
typedef struct ac_components ac_components;
typedef struct {
    uint32_t first;          /* lowest member = the reference's component[0] */
    uint32_t unitigs;
    uint64_t length;         /* sum of member lengths; 0 when no lengths were given */
    uint64_t links_all;      /* link_count() restricted to this component: .0 */
    uint64_t links_one_way;  /*                                            .1 */
    uint32_t open_ends;      /* unitig ends whose next list is empty (open_start + open_end over members) */
    uint32_t marked;         /* members with marked[u-1] != 0 */
    uint8_t  circular_loop;  /* component_is_circular_loop(members ascending) */
} ac_component;
typedef struct {
    uint32_t size;           /* the library's sizeof(ac_components_summary) */
    uint32_t unitigs, components, topology;   /* unitigs: the alive ones; topology: AC_TOPOLOGY_* over them */
    uint64_t links_all, links_one_way, total_length;
    uint32_t launches, read_backs;   /* kernel launches (fused fills and the read-back's own kernel included) and host round trips of the call */
    double seconds_device;   /* first kernel to last, by device events */
} ac_components_summary;
enum { AC_TOPOLOGY_EMPTY, AC_TOPOLOGY_FRAGMENTED, AC_TOPOLOGY_LINEAR_OPEN_OPEN, AC_TOPOLOGY_CIRCULAR,
       AC_TOPOLOGY_LINEAR_HAIRPIN_HAIRPIN, AC_TOPOLOGY_LINEAR_OPEN_HAIRPIN, AC_TOPOLOGY_OTHER };
/* On the links (ac_links: one entry per L line) and unitig lengths of a graph handle (a build, or ac_graph_from_gfa).  marked: one byte
 * per unitig or NULL; ac_component.marked counts them per component (e.g. the anchors of ac_resolve_anchors: a component with marked == 0
 * is what delete_unitigs_not_connected_to_anchor removes). */
int ac_graph_components(const ac_graph*, const uint8_t* marked /* n_unitigs, or NULL */, int device, ac_components** out);
/* The same on the caller's arrays, for a graph that has been edited.  alive: the reference's removed unitigs without renumbering — a unitig
 * that is not alive is in no component and every link touching it is ignored (remove_unitigs_by_number + delete_dangling_links). */
int ac_components_from_links(uint32_t n_unitigs, const ac_link* links, uint64_t n_links,
                             const uint32_t* unitig_len /* or NULL */, const uint8_t* alive /* or NULL = all */,
                             const uint8_t* marked /* or NULL */, int device, ac_components** out);
/* The arrays belong to the handle. */
int ac_components_records(const ac_components*, const ac_component** records, uint32_t* n);      /* in connected_components() order */
int ac_components_of_unitig(const ac_components*, const uint32_t** component /* n_unitigs; UINT32_MAX = not alive */);
int ac_components_members(const ac_components*, const uint64_t** off /* n + 1 */, const uint32_t** members /* ascending in each */);
/* 1 open_start, 2 open_end, 4 hairpin_start, 8 hairpin_end, 16 is_isolated_and_circular, 32 is_isolated_and_linear; 0 when not alive */
int ac_components_unitig_flags(const ac_components*, const uint8_t** flags);
/* at most out_size bytes are written (the struct only grows at its end); returns the library's sizeof(ac_components_summary) */
size_t ac_components_summary_get_sized(const ac_components*, ac_components_summary* out, size_t out_size);
const char* ac_topology_name(uint32_t topology);    /* the reference's strings: "circular", "linear-open-hairpin", ...; NULL beyond AC_TOPOLOGY_OTHER */
void ac_components_free(ac_components*);

/* The linear-path merge plan: what merge_linear_paths (graph_simplification.rs:315-371) would do to a graph, and the products of doing it —
 * which unitigs merge into which chains, in which order and on which strand, the new numbers, the merged sequences, depths and types
 * (merge_path :410-485, get_merge_path_depth :501-526) and the link set after the merge and delete_dangling_links.  Read-only: no handle
 * is edited; the plan is applied by ac_merge_finish / ac_subsets_finish (renumber_unitigs, the L and P lines, the GFA) and made for a graph
 * after resolve's apply_bridges by ac_applied_merge_plan, all further down.
 * The link entries among alive unitigs must be a SET that is closed under reverse complement: a duplicated entry, or an entry (a, b)
 * without (-b, -a), is an error (the first one by index is quoted), because the reference's sequential loop has an order-free form only
 * then.  The fixed starts and ends are the reference's own (get_fixed_unitig_starts_and_ends :190-230 on the first and last entry of every
 * path, then fix_circular_loops :374-384).
 * Chains come in the order the reference finds them — ascending number of the unitig they are found from — and chain i gets the number
 * n_unitigs + 1 + i (n_unitigs = the highest number, alive or not).  A chain's members are signed numbers in path order.
 * Everything but the depth and type rules runs on the device; the number of launches grows with log2(n_unitigs) only, never with the
 * length of a chain.  The host reads one 64-byte header and then the results, sized by it.
 * Errors (return 1, ac_last_error), never faults: a link that names unitig 0 or one above n_unitigs, a duplicated link, a link whose reverse
 * complement is missing, a path end that names a dead or nonexistent unitig, unitig_len NULL, only one of seq_bytes and seq_begin, NULL
 * out, a handle without host arrays.  n_unitigs == 0 is a valid, empty result. */
typedef struct ac_merge ac_merge;
typedef struct {
    uint32_t number;         /* the merged unitig's number: n_unitigs + 1 + index */
    uint32_t members;        /* >= 2 */
    uint64_t length;         /* sum of member lengths = bytes of the merged sequence */
    uint64_t member_off;     /* first member in ac_merge_members */
    uint64_t seq_off;        /* first byte in ac_merge_sequences (filled whether or not sequences were copied) */
    double   depth;          /* get_merge_path_depth: the first member's position count on its strand if non-zero, else the first Anchor member's
                                depth, else sum(depth * len) / sum(len) as one sequential sum in path order */
    uint8_t  type;           /* AC_UNITIG_CONSENTIG if any member is Anchor or Consentig, else AC_UNITIG_OTHER */
    uint8_t  loop;           /* the last member links to the first: the merged unitig gets the link + -> + (and - -> -) */
} ac_merge_chain;
typedef struct {
    uint32_t size;           /* the library's sizeof(ac_merge_summary) */
    uint32_t chains, merged_unitigs, unitigs_after;   /* unitigs_after: alive - merged_unitigs + chains */
    uint64_t links_after, bases_copied;
    uint32_t launches, read_backs;
    double seconds_device;   /* the kernels of the call, by device events (the components pass included) */
    double seconds_copy;     /* of those, the kernel that copies the merged sequences */
} ac_merge_summary;
enum { AC_UNITIG_OTHER, AC_UNITIG_ANCHOR, AC_UNITIG_CONSENTIG, AC_UNITIG_BRIDGE };
/* On a graph handle (a build, or ac_graph_from_gfa): its links, lengths, depths and sequences; every unitig alive and of type Other.
 * use_paths = 1: the path ends and the per-strand position counts (a histogram of the signed path entries, taken on the device: what
 * create_sequence_and_positions yields, unitig_graph.rs:151-174) come from the handle's paths.  use_paths = 0: a call with `seqs` empty on
 * a graph without positions — everything mergeable merges.  with_sequences = 0: no bytes are copied (seq_off is still filled). */
int ac_graph_merge_plan(const ac_graph*, int use_paths, int with_sequences, int device, ac_merge** out);
/* The same on the caller's arrays, for a graph that has been edited.  alive as for ac_components_from_links.  path_ends: the first and
 * last signed entry of each of n_seqs non-empty paths.  fwd_positions / rev_positions: how many positions each unitig holds per strand. */
int ac_merge_plan_from_links(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len,
        const uint8_t* alive /* or NULL */, const int32_t* path_ends /* first,last per sequence; or NULL */, uint32_t n_seqs,
        const double* depth /* or NULL = 0 */, const uint32_t* fwd_positions, const uint32_t* rev_positions /* or NULL = none */,
        const uint8_t* type /* AC_UNITIG_OTHER/ANCHOR/CONSENTIG/BRIDGE, or NULL */,
        const uint8_t* seq_bytes, const uint64_t* seq_begin /* both or neither */, int device, ac_merge** out);
/* The arrays belong to the handle. */
int ac_merge_chains(const ac_merge*, const ac_merge_chain** chains, uint32_t* n);
int ac_merge_members(const ac_merge*, const int32_t** members /* signed numbers in path order, chain after chain */, uint64_t* n);
int ac_merge_chain_of_unitig(const ac_merge*, const uint32_t** chain /* n_unitigs; UINT32_MAX = not merged */);
int ac_merge_fixed_flags(const ac_merge*, const uint8_t** flags /* n_unitigs; 1 = fixed start, 2 = fixed end, after fix_circular_loops */);
int ac_merge_sequences(const ac_merge*, const uint8_t** bytes, uint64_t* n /* 0 when no sequences were given or asked for */);
/* The links after the merge as a SET, ascending by (a, b) as signed numbers — not get_links_for_gfa order. */
int ac_merge_links(const ac_merge*, const ac_link** links, uint64_t* n);
size_t ac_merge_summary_get_sized(const ac_merge*, ac_merge_summary* out, size_t out_size);
void ac_merge_free(ac_merge*);

/* Sequence subsets: what every cluster of sequences keeps of a graph — the edit that save_cluster_gfa (cluster.rs:794-806), clean_up_graph
 * (trim.rs:260-269) and resolve.rs:248 make before merge_linear_paths: drop the other sequences, recount the positions, remove the unitigs
 * nobody visits any more (remove_zero_depth_unitigs, unitig_graph.rs:582-586) and their links (delete_dangling_links :547-564) — for all
 * clusters in one call.  Read-only and on plain arrays: no handle is edited and none is made; the results feed ac_components_from_links and
 * ac_merge_plan_from_links directly (ac_subsets_dense, or the two composed entries below).  renumber_unitigs and the GFA text stay with the
 * caller.
 * cluster_of_seq: one label per sequence in path order, 0 = dropped, 1..n_clusters — the form ac_cluster_assign and
 * ac_cluster_qc_assignment return.  Everything comes in compressed-row form, clusters 1..n_clusters in order:
 *   unitigs     the alive unitigs of the cluster, ascending, with their position counts.  create_sequence_and_positions (:151-174) walks a path
 *               forwards and its reverse backwards, so an entry on either strand adds one position to the unitig's forward list and one to its
 *               reverse list: fwd_positions and rev_positions are both the number of entries of the kept paths that name the unitig (the two
 *               pointers name the same array).  A unitig is alive in the cluster iff that number is above 0 (depth = forward_positions.len())
 *   links       the input's links whose two unitigs are both alive in the cluster, in the input's order
 *   seqs        the kept sequences, ascending
 *   path_ends   first and last signed entry of every kept sequence with a non-empty path, in that order: ac_merge_plan_from_links' path_ends
 * Everything that grows with the path entries or the links runs on the device: a radix sort of one key per kept entry and a run-length pass
 * (no atomic per entry), one row of cluster bits per unitig for the links.  The host does what grows with n_seqs alone (labels, sequence
 * lists, path ends).  The number of launches follows the bit widths of the sort keys only — not n_clusters, n_seqs or how the labels are
 * spread; the host reads one fixed-size header and then the results, sized by it: two read-backs for 1 cluster as for 300.
 * Working memory on the device: about 72 bytes per kept path entry (keys, sort buffers, run-length arrays), 24 per link, 32 per kept link
 * over all clusters, 5 per unitig, and ceil(n_clusters / 64) * 8 bytes per unitig (one bit per cluster and unitig); never a counter per
 * cluster and unitig.  Fewer than 2^32 - 16 kept entries, links, and kept links over all clusters; sums of unitig lengths below 2^46.
 * Lifetime: the object BORROWS the arrays it was made from (links, unitig_len, path_entries, path_off; for ac_graph_subsets the handle) — they
 * must stay valid and unchanged until ac_subsets_free; a handle-made object must be freed before ac_free of its graph.
 * Errors (return 1, ac_last_error), never faults: a label above n_clusters; n_clusters 0 or above 65535; an entry of a kept path that names
 * unitig 0 or one above n_unitigs, or enters a unitig that is not alive in the input (the first such entry is quoted); a link that names no
 * unitig; path_off that decreases; NULL cluster_of_seq, path_off, out or unitig_len; a handle without host arrays or paths.  Valid results,
 * not errors: a cluster without sequences, a sequence with an empty path, every label 0, n_unitigs == 0. */
typedef struct ac_subsets ac_subsets;
typedef struct ac_merged_paths ac_merged_paths;
typedef struct {
    uint32_t seqs;           /* kept sequences */
    uint32_t unitigs;        /* alive unitigs */
    uint64_t entries;        /* path entries of the kept sequences */
    uint64_t links;          /* kept links */
    uint64_t length;         /* total length of the alive unitigs */
} ac_subset_cluster;
typedef struct {
    uint32_t size;           /* the library's sizeof(ac_subsets_summary) */
    uint32_t clusters, sequences_kept, n_unitigs;
    uint64_t entries_kept, unitigs, links;   /* sums over the clusters */
    uint32_t launches, read_backs;
    double seconds_device;   /* the kernels of the call, by device events */
} ac_subsets_summary;
/* On a graph handle (a build, or ac_graph_from_gfa): its links (get_links_for_gfa order), lengths and paths. */
int ac_graph_subsets(const ac_graph*, const uint16_t* cluster_of_seq /* ac_graph_seq_count() labels */, uint32_t n_clusters, int device, ac_subsets** out);
/* The same on the caller's arrays, for an edited graph or edited paths (the slices of ac_trim_path_slices).  alive as for
 * ac_components_from_links. */
int ac_subsets_from_paths(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive /* or NULL */,
                          const int32_t* path_entries, const uint64_t* path_off /* n_seqs + 1 */, uint32_t n_seqs, const uint16_t* cluster_of_seq,
                          uint32_t n_clusters, int device, ac_subsets** out);
/* The arrays belong to the object; every `off` has n_clusters + 1 entries, cluster c (1-based) = [off[c - 1], off[c]). */
int ac_subsets_records(const ac_subsets*, const ac_subset_cluster** records, uint32_t* n_clusters);
int ac_subsets_unitigs(const ac_subsets*, const uint64_t** off, const uint32_t** unitigs, const uint32_t** fwd_positions, const uint32_t** rev_positions);
int ac_subsets_links(const ac_subsets*, const uint64_t** off, const ac_link** links);
int ac_subsets_seqs(const ac_subsets*, const uint64_t** off, const uint32_t** seq_index);
int ac_subsets_path_ends(const ac_subsets*, const uint64_t** off /* in (first, last) pairs */, const int32_t** path_ends);
/* One cluster as the argument arrays of ac_components_from_links / ac_merge_plan_from_links: n_unitigs entries each, allocated by the
 * caller, any may be NULL.  depth = fwd_positions as a double (recalculate_depth, unitig.rs:260-262). */
int ac_subsets_dense(const ac_subsets*, uint32_t cluster, uint8_t* alive, uint32_t* fwd_positions, uint32_t* rev_positions, double* depth);
size_t ac_subsets_summary_get_sized(const ac_subsets*, ac_subsets_summary* out, size_t out_size);
void ac_subsets_free(ac_subsets*);
/* ac_components_from_links / ac_merge_plan_from_links on cluster c: its kept links, alive mask, path ends and position counts, depth =
 * fwd_positions, every type Other — save_cluster_gfa's graph at the point it calls merge_linear_paths.  seq_bytes / seq_begin: both or
 * neither, as for ac_merge_plan_from_links; NULL, NULL on a handle-made object takes the handle's sequences.  with_sequences = 0: none. */
int ac_subsets_components(const ac_subsets*, uint32_t cluster, const uint8_t* marked /* or NULL */, int device, ac_components** out);
int ac_subsets_merge_plan(const ac_subsets*, uint32_t cluster, const uint8_t* seq_bytes, const uint64_t* seq_begin, int with_sequences, int device,
                          ac_merge** out);
/* The P lines after the merge: the path of every kept sequence of the cluster with every traversal of a chain replaced by the chain's number,
 * + where the path runs through the members in chain order on their chain strands, - where it runs through them backwards on the opposite
 * strands (a merged loop walked several times: once per lap).  This is what get_unitig_path_for_sequence (unitig_graph.rs:407-465) walks after
 * merge_path (graph_simplification.rs:414-415): members inside a chain have one way in and one way out and path ends are fixed, so a path
 * that touches a chain runs through all of it.  plan: from ac_subsets_merge_plan of the same cluster.  Three kernels and three scans
 * whatever the paths; for every sequence the unitig lengths along the new path must add up to those along the old one (checked on the device).
 * Errors: a plan of another cluster or another n_unitigs, or one that ac_subsets_merge_plan did not make; a kept path that begins or ends strictly inside a chain, or whose length
 * changes (the sequence is named) — only a plan that was not made from these paths can do either. */
typedef struct {
    uint32_t size;           /* the library's sizeof(ac_merged_paths_summary) */
    uint32_t sequences;
    uint64_t entries_before, entries_after;
    uint32_t launches, read_backs;
    double seconds_device;
} ac_merged_paths_summary;
int ac_subsets_merged_paths(const ac_subsets*, uint32_t cluster, const ac_merge* plan, int device, ac_merged_paths** out);
int ac_merged_paths_get(const ac_merged_paths*, const uint32_t** seq_index, uint32_t* n_seqs, const uint64_t** path_off /* n_seqs + 1 */,
                        const int32_t** entries);
size_t ac_merged_paths_summary_get_sized(const ac_merged_paths*, ac_merged_paths_summary* out, size_t out_size);
void ac_merged_paths_free(ac_merged_paths*);

/* A finished graph: a merge plan applied — what the reference holds after merge_linear_paths and, optionally, renumber_unitigs
 * (unitig_graph.rs:295-315), up to the text of save_gfa (:317-360).  Read-only: made from a plan plus the arrays the plan was made from.
 * Additions of ABI generation 13, found by name; AC_ABI_VERSION stays 13.
 *   S lines   renumber = 0: graph.unitigs after merge_path's push and retain — the unmerged alive unitigs in ascending old number, then the
 *             merged unitigs in chain order; numbers stay as they are (old numbers; n_unitigs + 1 + i for chain i).
 *             renumber = 1: a stable sort of that order by length descending, forward sequence bytewise ascending, depth descending
 *             (partial_cmp; -0.0 == 0.0); ties keep the order above; the printed number is the place + 1.
 *   L lines   get_links_for_gfa order (:333-350) after merge_path's list pushes (graph_simplification.rs:410-485) and delete_dangling_links:
 *             per unitig in S order its forward_next, then its reverse_next.  The input's link order matters: every source's entries must be
 *             in list order, as ac_links, ac_subsets_links and the L lines of a GFA are.
 *   P lines   the entries of an ac_merged_paths under the printed numbers (paths = NULL: none).
 * On the device: the order (three radix sorts — depth, the first 8 bytes, length — then an exact merge sort of what they leave open, a
 * wavefront per comparison), the gather of the sequences in final order, the link order (one key per input link, a radix sort) and both
 * relabellings.  The number of launches follows the key widths and log2 of the unitigs alone.
 * Errors (return 1, ac_last_error), never faults: a plan over another n_unitigs; n_links that differs from the plan's; an alive mask that
 * leaves another number of unitigs than the plan; renumber = 1 with a NaN depth (the unitig is named: the reference's comparator is no total
 * order there); missing sequences (seq_bytes / seq_begin NULL while unmerged unitigs have bases, or a plan made without sequences); links
 * that touch the inside of a chain; a path entry that names no unitig after the merge; NULL plan, out or unitig_len. */
typedef struct ac_finished ac_finished;
typedef struct {
    uint32_t number;         /* as printed */
    uint32_t source;         /* where it comes from: an old number, or n_unitigs + 1 + chain index */
    uint64_t length;
    uint64_t seq_off;        /* first byte in ac_finished_sequences */
    double   depth;
    uint8_t  type;           /* AC_UNITIG_* */
} ac_finished_unitig;
typedef struct {
    uint32_t size;           /* the library's sizeof(ac_finished_summary) */
    uint32_t unitigs, renumbered;
    uint32_t launches, read_backs;
    uint64_t links, path_entries, bases;
    uint64_t tie_items;      /* unitigs whose place the radix keys left open: longer than 8 bases, same length and first 8 bytes as another */
    double seconds_device;   /* the kernels of the call, by device events */
    double seconds_gather;   /* of those, the kernel that gathers the sequences */
} ac_finished_summary;
int ac_merge_finish(const ac_merge* plan, uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len,
        const uint8_t* alive /* or NULL */, const double* depth /* or NULL = 0 */, const uint8_t* type /* or NULL = Other */,
        const uint8_t* seq_bytes, const uint64_t* seq_begin, const ac_merged_paths* paths /* or NULL */, int renumber, int device,
        ac_finished** out);
/* The same for cluster c of an ac_subsets: its kept links, alive mask and depths (the position counts), every type Other; plan and
 * merged_paths (or NULL) from ac_subsets_merge_plan / ac_subsets_merged_paths of that cluster.  seq_bytes / seq_begin: NULL, NULL on a
 * handle-made object takes the handle's sequences. */
int ac_subsets_finish(const ac_subsets*, uint32_t cluster, const ac_merge* plan, const ac_merged_paths* merged_paths, const uint8_t* seq_bytes,
        const uint64_t* seq_begin, int renumber, int device, ac_finished** out);
/* The arrays belong to the object. */
int ac_finished_unitigs(const ac_finished*, const ac_finished_unitig** unitigs, uint32_t* n);
int ac_finished_sequences(const ac_finished*, const uint8_t** bytes, uint64_t* n);
int ac_finished_new_of_old(const ac_finished*, const uint32_t** printed /* n_unitigs + chains; 0 = gone */, uint64_t* n);
int ac_finished_links(const ac_finished*, const ac_link** links, uint64_t* n);
int ac_finished_paths(const ac_finished*, const uint32_t** seq_index, uint32_t* n_seqs, const uint64_t** path_off /* n_seqs + 1 */, const int32_t** entries);
size_t ac_finished_summary_get_sized(const ac_finished*, ac_finished_summary* out, size_t out_size);
void ac_finished_free(ac_finished*);
/* save_gfa's text: the printed numbers, DP:f:{:.2}, colour_tag's CL:Z: (unitig.rs:174-182), CL:i:<cluster> on a P line whose tag is above 0
 * (unitig_graph.rs:357).  One seq_id / seq_length / filename / header (and cluster tag, or cluster_tags = NULL) per P line.  *out is
 * malloc'ed and 0-terminated (ac_string_free); *len, when given, its length. */
int ac_finished_gfa_string(const ac_finished*, uint32_t k, const uint16_t* seq_ids, const uint32_t* seq_lengths, const char* const* filenames,
        const char* const* headers, const uint32_t* cluster_tags, int use_other_colour, char** out, uint64_t* len);
/* An ordinary graph handle, as ac_graph_from_gfa makes, of a finished graph made with renumber = 1 whose unitigs are all of type Other. */
int ac_finished_to_graph(const ac_finished*, uint32_t k, const uint16_t* seq_ids, const uint32_t* seq_lengths, const char* const* filenames,
        const char* const* headers, ac_graph** out);

/* apply_bridges of `autocycler resolve` with what it runs at its end (resolve.rs:223-282): the link edits, the new Bridge unitigs with their
 * sequences, reduce_depths, delete_unitigs_not_connected_to_anchor and remove_zero_depth_unitigs — the step between ac_resolve_bridges and
 * the merge plan.  Additions of ABI generation 13, found by name; AC_ABI_VERSION stays 13.  Read-only: the result is a new object.
 * The reference applies the bridges one after the other; the library runs the order-free form of DESIGN.md §9k, which holds where no two
 * applied bridges share a start or an end on either strand — what determine_ambiguity says of the bridges it leaves unflagged — and where the
 * links among alive unitigs are a duplicate-free set closed under reverse complement.  Both are checked on the device.
 *   bridges   in Bridge::cmp order, as ac_resolve_bridge_records gives them; apply[b] != 0 applies bridge b.  Of a record the edit reads start,
 *             end, best_off, best_len, first_distinct, n_distinct and status.  best_paths: the pool of ac_resolve_best_paths; distinct_entries,
 *             distinct_off (n_distinct_paths + 1), multiplicity: ac_resolve_distinct_paths.
 *   unitigs   the result counts n_total = n_unitigs + the applied bridges with a non-empty best path: the i-th of those, in order, is unitig
 *             n_unitigs + 1 + i, of type AC_UNITIG_BRIDGE, depth bridge_depth, its sequence the best path's members on their strands.  A bridge
 *             with an empty best path becomes the link start -> end.  type: AC_UNITIG_ANCHOR for the anchors, AC_UNITIG_OTHER else.
 *   depth     every visit of a unitig by a path of an applied bridge with a non-empty best path (copies counted) is one reduce_depth_by_one;
 *             the result is the reference's f64, bit for bit (NaN stays NaN).  depth = NULL: 0.
 *   alive     0 for what was dead at entry, for the components of the edited graph without an anchor, and then for every depth that is not
 *             above 0.  The components are taken before the zero-depth removal, as the reference takes them.
 *   links     the survivors and the created links whose two ends are alive, in get_links_for_gfa order over the alive originals ascending, then
 *             the bridge unitigs: what 3_bridged.gfa prints and what ac_merge_finish wants.  The input's order matters as it does there.
 * The number of launches (those of the components analysis apart, reported separately) follows the key widths alone, not the bridges.
 * Errors (return 1, ac_last_error), never faults: an applied bridge with status 2; applied bridges that conflict (both are named); a start,
 * an end or a path entry that is 0, beyond n_unitigs or dead; a start or end that is not among anchors; anchors that do not ascend; links
 * that are no closed duplicate-free set or name no unitig; only one of seq_bytes / seq_begin; n_unitigs + bridge unitigs above 2^31 - 2; pool
 * ranges outside their pools; a NULL out.  n_unitigs == 0 gives an empty result; without anchors everything is removed. */
typedef struct ac_applied ac_applied;
enum { AC_APPLY_UNIQUE = 0, AC_APPLY_KEPT = 1 };
typedef struct {
    uint32_t size;                  /* the library's sizeof(ac_applied_summary) */
    uint32_t bridges_applied;
    uint32_t direct_links;          /* of those: empty best path, a link instead of a unitig */
    uint32_t launches;              /* the step's own: the components analysis apart */
    uint32_t launches_components;
    uint32_t read_backs;            /* all host round trips of the call */
    uint64_t removed_no_anchor;     /* unitigs (bridge unitigs included) in components without an anchor */
    uint64_t removed_zero_depth;    /* then: unitigs whose depth is not above 0 */
    uint64_t links_in, links_out;
    uint64_t bases_copied;          /* bytes of the bridge sequences */
    double seconds_device;          /* the kernels of the call, by device events (the components analysis included) */
    double seconds_copy;            /* of those, the kernel that writes the bridge sequences */
    double seconds_components;      /* of those, the components analysis */
} ac_applied_summary;
int ac_apply_bridges(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive /* or NULL */,
        const double* depth /* or NULL = 0 */, const uint32_t* anchors /* ascending unitig numbers */, uint32_t n_anchors,
        const uint8_t* seq_bytes, const uint64_t* seq_begin /* both or neither */, const ac_bridge* bridges, uint32_t n_bridges,
        const int32_t* best_paths, uint64_t n_best, const int32_t* distinct_entries, const uint64_t* distinct_off, const uint32_t* multiplicity,
        uint64_t n_distinct_paths, const uint8_t* apply /* one byte per bridge */, double bridge_depth, int device, ac_applied** out);
/* The same on a handle's links, lengths, depths and sequences with the bridges of an ac_resolve made from it.  which = AC_APPLY_UNIQUE: the
 * bridges that do not conflict (the first pass, resolve.rs:52); AC_APPLY_KEPT: the bridges cull_ambiguity kept (the final pass, :61).
 * bridge_depth = the handle's sequence count (:47). */
int ac_graph_resolve_apply(const ac_graph*, const ac_resolve*, int which, int device, ac_applied** out);
/* The arrays belong to the object.  Per unitig 1 .. n_total (any of the four may be NULL): */
int ac_applied_unitigs(const ac_applied*, uint32_t* n_total, const uint32_t** len, const uint8_t** alive, const double** depth, const uint8_t** type);
int ac_applied_bridge_of(const ac_applied*, const uint32_t** bridge /* unitig n_unitigs + 1 + i was made from bridge[i] */, uint32_t* n);
int ac_applied_links(const ac_applied*, const ac_link** links, uint64_t* n);
/* bridge unitig i = bytes[off[i] .. off[i + 1]) (off: n + 1 entries); without seq_bytes the offsets are there and *n_bytes is 0 */
int ac_applied_bridge_sequences(const ac_applied*, const uint8_t** bytes, const uint64_t** off, uint64_t* n_bytes /* may be NULL */);
size_t ac_applied_summary_get_sized(const ac_applied*, ac_applied_summary* out, size_t out_size);
void ac_applied_free(ac_applied*);
/* merge_after_bridging (resolve.rs:254-258) on the edited graph: the plan of merge_linear_paths(graph, &vec![]) after clear_positions — no
 * path ends, no positions — and the finished graph of that plan (renumber = 1: renumber_unitigs), over the object's own arrays: the
 * original and the bridge sequences are one array there.  Free with ac_merge_free / ac_finished_free. */
int ac_applied_merge_plan(const ac_applied*, int with_sequences, int device, ac_merge** out);
int ac_applied_finish(const ac_applied*, const ac_merge* plan, int renumber, int device, ac_finished** out);
/* 3_bridged.gfa: save_gfa's text of the edited graph under its own numbers, no P lines.  *out is malloc'ed (ac_string_free). */
int ac_applied_gfa_string(const ac_applied*, uint32_t k, int use_other_colour, char** out, uint64_t* len /* may be NULL */);
/* resolve.rs:44-67 from a handle (a build, or ac_graph_from_gfa of 2_trimmed.gfa) to the texts of 3_bridged.gfa, 4_merged.gfa and
 * 5_final.gfa: ac_resolve_bridges; the first pass (AC_APPLY_UNIQUE), its text, the merge and renumbering, its text; if anything was culled a
 * second pass (AC_APPLY_KEPT) from the unedited handle, else the merged graph again; the final text with use_other_colour.  The three
 * strings are malloc'ed (ac_string_free each). */
int ac_resolve_graphs(const ac_graph*, int device, char** bridged, char** merged, char** final_text, uint32_t* cull_count);

/* `autocycler clean` (clean.rs:23-45): the command that edits a consensus graph which is not fully resolved — the user's tigs out
 * (remove_unitigs_by_number), a tig that two replicons share doubled (duplicate_unitig_by_number), low-depth tigs out where that leaves no
 * dead end (remove_low_depth_unitigs; unitig_graph.rs:588-721), then merge_linear_paths, renumber_unitigs and save_gfa.  Additions of ABI
 * generation 13, found by name; AC_ABI_VERSION stays 13.  Read-only: the result is a new object.
 *   links      one entry per L line in L-line order (unitigs ascending, a unitig's forward links before its reverse links: ac_links, or a loaded
 *              GFA); among alive unitigs a duplicate-free set closed under reverse complement.  Anything else is an error that quotes the
 *              first offending entry.  The order inside a list decides which link of a duplicated tig goes to which copy.
 *   remove, duplicate   ascending unitig numbers (ac_parse_tig_numbers); every number must name a unitig alive at entry, or the error is
 *              "<graph> does not contain tig N".  A number listed twice in remove is harmless.
 *   duplicate  one number at a time, ascending, against the graph as it is then: the tig must have exactly two non-self links, counted over its
 *              forward then its reverse list ("unitig N does not contain exactly two non-self links"); copies a and b of duplicate[i] are
 *              unitigs n_unitigs + 1 + 2 i and n_unitigs + 2 + 2 i, same bytes and type, half the depth; the first non-self link goes to a, the
 *              second to b, self links to both.  A number that was removed, or duplicated earlier in the call, is an error (the reference
 *              panics there).  A loop u+ -> u+ is re-created once from each strand's list, so each copy carries it TWICE, as in the reference;
 *              a hairpin once.  ac_cleaned_links reports that multiset literally; the composed entries below refuse it with the merge plan's
 *              duplicate-entry error, whose order-free form holds for sets only.
 *   min_depth  with has_min_depth != 0: the unitigs are walked from the last (the copies, b before a) to the first; one whose depth is not
 *              above min_depth (a NaN on either side counts as low) goes iff every neighbour it leads to or comes from keeps another entry on
 *              that side; each decision sees the deletions before it.  The device runs the round form of DESIGN.md 9l: the same result, the
 *              number of rounds in the summary; a chain of n low unitigs takes n rounds.
 *   result     over n_out = n_unitigs + 2 * n_duplicate unitigs: alive, depth, type, length, seq_begin (a copy points at its original's bytes;
 *              NULL without sequences), copy_of (0 for the originals) and a reason code; the links among alive unitigs in get_links_for_gfa
 *              order over the originals ascending, then the copies: what ac_merge_finish wants.
 * The number of launches is a constant plus a constant per batch of rounds_per_batch rounds; the host reads one counter per batch.
 * Errors (return 1, ac_last_error), never faults; n_unitigs == 0 gives an empty result. */
typedef struct ac_cleaned ac_cleaned;
enum { AC_CLEAN_KEPT = 0, AC_CLEAN_REMOVED = 1, AC_CLEAN_DUPLICATED = 2, AC_CLEAN_LOW_DEPTH = 3,
       AC_CLEAN_KEPT_DEAD_END = 4 /* low, but kept to avoid a dead end */, AC_CLEAN_ABSENT = 5 /* not alive at entry */ };
typedef struct {
    uint32_t size;                  /* the library's sizeof(ac_cleaned_summary) */
    uint32_t unitigs_in, unitigs_out;   /* n_unitigs; n_unitigs + 2 per duplication */
    uint32_t rounds;                /* of the low-depth step */
    uint32_t rounds_per_batch;      /* rounds between two read-backs */
    uint32_t launches, read_backs;
    uint32_t reserved;
    uint64_t kept, removed, duplicated, low_depth, kept_dead_end, absent;   /* unitigs per reason code */
    uint64_t links_in, links_out;
    double seconds_device;          /* the kernels of the call, by device events */
} ac_cleaned_summary;
int ac_clean_graph(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const double* depth /* or NULL = 0 */,
        const uint8_t* type /* AC_UNITIG_*, or NULL = Other */, const uint8_t* alive /* or NULL */, const uint8_t* seq_bytes,
        const uint64_t* seq_begin /* both or neither */, const uint32_t* remove, uint32_t n_remove, const uint32_t* duplicate, uint32_t n_duplicate,
        int has_min_depth, double min_depth, int device, ac_cleaned** out);
/* The same on a handle's links, lengths, depths and sequences.  A handle holds no types: type = one AC_UNITIG_* byte per unitig
 * (ac_gfa_segment_types of the text the handle was loaded from), or NULL = every unitig Other. */
int ac_graph_clean(const ac_graph*, const uint8_t* type, const uint32_t* remove, uint32_t n_remove, const uint32_t* duplicate, uint32_t n_duplicate,
        int has_min_depth, double min_depth, int device, ac_cleaned** out);
/* The arrays belong to the object.  Per unitig 1 .. n_out (any of the seven may be NULL): */
int ac_cleaned_unitigs(const ac_cleaned*, uint32_t* n_out, const uint32_t** len, const uint8_t** alive, const double** depth, const uint8_t** type,
        const uint64_t** seq_begin, const uint32_t** copy_of, const uint8_t** reason);
int ac_cleaned_links(const ac_cleaned*, const ac_link** links, uint64_t* n);
size_t ac_cleaned_summary_get_sized(const ac_cleaned*, ac_cleaned_summary* out, size_t out_size);
void ac_cleaned_free(ac_cleaned*);
/* merge_graph (clean.rs:111-117) on the edited graph: the plan of merge_linear_paths(graph, &vec![]) — no path ends, no positions — and the
 * finished graph of that plan (renumber = 1: renumber_unitigs), over the object's own arrays.  Free with ac_merge_free / ac_finished_free.
 * After a duplicated loop the links are a multiset and both entries fail with the merge plan's duplicate-entry error. */
int ac_cleaned_merge_plan(const ac_cleaned*, int with_sequences, int device, ac_merge** out);
int ac_cleaned_finish(const ac_cleaned*, const ac_merge* plan, int renumber, int device, ac_finished** out);
/* save_gfa's text of the edited graph under its own numbers, before the merge; no P lines.  *out is malloc'ed (ac_string_free). */
int ac_cleaned_gfa_string(const ac_cleaned*, uint32_t k, int use_other_colour, char** out, uint64_t* len /* may be NULL */);
/* parse_tig_numbers (clean.rs:142-149): spaces removed, split at ',', every piece a u32, sorted.  text == NULL: the option is absent, an empty
 * list.  A piece that does not parse (the empty string is one) fails with "failed to parse '<piece>' as a node number".  *numbers is
 * malloc'ed (free it with ac_string_free). */
int ac_parse_tig_numbers(const char* text, uint32_t** numbers, uint32_t* n);
/* The type of every S line of a GFA text, in file order, from its CL:Z colour as Unitig::from_segment_line reads it (unitig.rs:79-87):
 * AC_UNITIG_* bytes.  ac_graph_from_gfa drops the colours; this entry is how a caller keeps them.  *types is malloc'ed (ac_string_free). */
int ac_gfa_segment_types(const char* gfa_text, uint64_t len, uint8_t** types, uint32_t* n);
/* clean.rs:27-43 from text to text: parse both lists, load the graph (segments numbered 1, 2, 3, ... as ac_graph_from_gfa wants them), check
 * the numbers, remove, duplicate, low depth, merge, renumber, and save_gfa(out, &vec![], true): no P lines, use_other_colour, KM:i of the
 * input (0 without one).  remove / duplicate: the option's string, or NULL.  *out_text is malloc'ed (ac_string_free). */
int ac_clean_gfa(const char* gfa_text, uint64_t len, const char* remove, const char* duplicate, int has_min_depth, double min_depth, int device,
        char** out_text, uint64_t* out_len /* may be NULL */);
/* The whole command: in_gfa must exist; the cleaned graph is written to out_gfa.  "<in_gfa> does not contain tig N" names the file. */
int ac_clean(const char* in_gfa, const char* out_gfa, const char* remove, const char* duplicate, int has_min_depth, double min_depth, int device);

/* `autocycler trim` after the alignments, through to 2_trimmed.gfa and 2_trimmed.yaml (trim.rs:47-51): choose_trim_type (:189-226),
 * create_sequence_and_positions' length check (unitig_graph.rs:173), exclude_outliers_in_length (:229-257) and clean_up_graph (:260-269).
 * The slices' entries go to the device once: every entry is checked and its slice summed there (64-bit sums), the host computes median, MAD
 * and the allowed range (f64::round half away from zero, `as usize` saturating), the kept sequences' entries are compacted on the device when
 * somebody was excluded, and the sequence-subset stages run with one cluster on the entries that are there already.  Additions of ABI
 * generation 13, found by name; AC_ABI_VERSION stays 13.  Read-only: the result is a new object.
 *   chosen: AC_TRIM_CHOOSE_AUTO = choose_trim_type's rule over `results` (status 1 counts, status 2 counts as not trimmed; start-end wins a
 *           tie; nothing is trimmed when both counts are 0), or one kind forced, or none.
 *   A sequence whose result of the chosen kind has status 1 gets path[begin:end] and trimmed_length; every other keeps path and length.
 *   mad: 0 excludes nobody; mad < 0 is an error.  A sequence is kept iff min <= length <= max; the kept ones keep their order.
 * Errors (return 1, ac_last_error), never aborts: a slice whose unitig lengths do not add up to its new length (names the sequence),
 * begin > end, end beyond the path, an entry that names no unitig or a dead one (the subsets' texts), a KEPT sequence with an empty slice
 * (the reference asserts in find_starting_unitig, unitig_graph.rs:423), more than 32767 sequences, null pointers.  Everyone excluded is no
 * error: the object's one cluster is empty, its text is the H line alone and no further kernel is launched. */
typedef struct ac_trimmed ac_trimmed;
#define AC_TRIM_CHOOSE_AUTO 0
#define AC_TRIM_CHOOSE_NONE 1
#define AC_TRIM_CHOOSE_START_END 2
#define AC_TRIM_CHOOSE_HAIRPIN 3
typedef struct {
    uint32_t begin, end;        /* the slice of the sequence's path that stays */
    uint64_t length;            /* its new length in bases */
    uint32_t trimmed, excluded; /* 0 / 1 */
} ac_trimmed_record;
typedef struct {
    uint32_t size;              /* the library's sizeof(ac_trimmed_summary) */
    uint32_t chosen;            /* 0 = none, 1 = start-end, 2 = hairpin (ac_trim_summary.chosen's values) */
    uint32_t c_se, c_hp;        /* results with status 1 per kind */
    uint32_t sequences, trimmed, excluded, rejected;   /* in; given a slice; outside the range; with a status-2 result of either kind */
    uint32_t unitigs_in, unitigs_alive;                /* of the input; visited by a kept slice */
    uint32_t launches, read_backs;                     /* of the edit: the slice stage and the subset stages */
    uint64_t median, mad;       /* median_isize / mad_isize of the new lengths of all sequences */
    uint64_t min_length, max_length;                   /* the allowed range; 0 and 2^64 - 1 when mad == 0 */
    uint64_t entries_kept, links;                      /* path entries of the kept slices; links between alive unitigs */
    double seconds_device;      /* the edit's kernels, by device events */
    uint32_t align_launches, reserved;                 /* ac_graph_trim / ac_trim_gfa: the alignment, as ac_trim_summary reports it (else 0) */
    uint64_t align_cells;
    double align_seconds_device;
} ac_trimmed_summary;
/* On the caller's arrays: links / unitig_len / alive as for ac_subsets_from_paths, path_entries / path_off / seq_length per sequence, results =
 * ac_trim_path_slices' table (may be NULL with AC_TRIM_CHOOSE_NONE).  The arrays except `results` are borrowed until ac_trimmed_free. */
int ac_trim_apply(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive /* or NULL */,
        const uint8_t* type /* AC_UNITIG_*, or NULL = Other */, const int32_t* path_entries, const uint64_t* path_off, const uint32_t* seq_length,
        uint32_t n_seqs, const ac_trim_result* results, uint32_t chosen, double mad, int device, ac_trimmed** out);
/* The same on a handle (which must outlive the object); results = ac_trim_paths' table. */
int ac_graph_trim_apply(const ac_graph*, const ac_trim_result* results, uint32_t chosen, double mad, int device, ac_trimmed** out);
/* ac_trim_paths' computation followed by the edit (chosen = auto).  min_identity outside [0, 1]: "--min_identity must be between 0.0 and 1
 * (inclusive)"; mad < 0: "--mad cannot be less than 0" (trim.rs:60-65).  max_unitigs = 0 disables trimming, not the exclusion. */
int ac_graph_trim(const ac_graph*, double min_identity, uint32_t max_unitigs, double mad, int device, ac_trimmed** out);
int ac_trimmed_records(const ac_trimmed*, const ac_trimmed_record** records, uint32_t* n_seqs);
size_t ac_trimmed_summary_get_sized(const ac_trimmed*, ac_trimmed_summary* out, size_t out_size);
void ac_trimmed_free(ac_trimmed*);
/* The trimmed graph before the merge, as a borrowed one-cluster ac_subsets (do not free it; it dies with the object): every ac_subsets_*
 * accessor and composed entry serves it as it stands, cluster = 1.  Its sequences are the input's, the excluded ones with label 0; its
 * paths are the slices. */
const ac_subsets* ac_trimmed_subsets(const ac_trimmed*);
/* merge_linear_paths with the kept paths' ends fixed, the paths over the merged unitigs and renumber_unitigs in one call: the finished graph
 * (ac_finished_free).  seq_bytes / seq_begin: the unitigs' bases for the S lines, NULL, NULL on a handle-made object (the handle's are
 * used) or for a finish without sequences.  ac_finished_gfa_string with the kept sequences' ids, NEW lengths, file names and headers prints
 * 2_trimmed.gfa; ac_finished_to_graph gives the handle `resolve` starts from. */
int ac_trimmed_finish(const ac_trimmed*, const uint8_t* seq_bytes, const uint64_t* seq_begin, int device, ac_finished** out);
/* 2_trimmed.yaml: TrimmedClusterMetrics (metrics.rs:213-230) in serde_yaml 0.9 block style.  *out is malloc'ed (ac_string_free). */
int ac_trimmed_yaml_string(const ac_trimmed*, char** out, uint64_t* len /* may be NULL */);
/* trim.rs:43-51 from text to texts.  Reads GFAs as `cluster` writes them (save_cluster_gfa, cluster.rs:794-806): segment numbers in any
 * order and with holes, mapped to 1..n in file order (the output does not depend on them: trim compares entries for equality and renumbers
 * at its end); the P lines' CL:i tags and the S lines' colours are kept.  *gfa and *yaml are malloc'ed (ac_string_free); summary may be NULL. */
int ac_trim_gfa(const char* gfa_text, uint64_t len, double min_identity, uint32_t max_unitigs, double mad, int device, char** gfa, uint64_t* gfa_len,
        char** yaml, ac_trimmed_summary* summary /* its size field set by the caller */);
/* The whole command: <cluster_dir>/1_untrimmed.gfa -> 2_trimmed.gfa and 2_trimmed.yaml, each written to a temporary file and renamed. */
int ac_trim_dir(const char* cluster_dir, double min_identity, uint32_t max_unitigs, double mad, int device);
/* `autocycler resolve` as a command (resolve.rs:41-67 without --verbose): <cluster_dir>/2_trimmed.gfa -> 3_bridged.gfa, 4_merged.gfa and
 * 5_final.gfa through ac_resolve_graphs. */
int ac_resolve_dir(const char* cluster_dir, int device);

/* `autocycler combine` (combine.rs:28-54) and `autocycler gfa2fasta` (gfa2fasta.rs:56-83): the clusters' final graphs gathered into
 * consensus_assembly.gfa, .fasta and .yaml.  Additions of ABI generation 13, found by name; AC_ABI_VERSION stays 13.  Read-only.
 * The input is the concatenation of n_graphs graphs (an empty graph is legal):
 *   unitig_off, link_off   n_graphs + 1 words each, from 0, ascending: a graph's unitigs and links in the arrays below
 *   number     per unitig its own number (any order, holes allowed; two unitigs of one graph with one number are an error: the reference's
 *              index would silently keep the last)
 *   links      one entry per L line in L-line order: signed 1-based FILE-ORDER INDICES within their graph (not numbers).  An entry that is
 *              0 or beyond its graph is an error.
 *   depth, type   DP:f and AC_UNITIG_* per unitig, or NULL (0 / Other)
 *   read_depth, has_read_depth   both or neither: with them the result is that of `combine --reads` (has_read_depth 0 = the reference's
 *              None); what ac_depth_finish writes goes straight in
 *   seq_bytes, seq_begin   both or neither: the unitigs' bytes, kept for the texts only.  They are never sent to the device: no decision
 *              reads them.
 * The graphs come out in order of total length, descending, ties in input order (load_clusters' stable sort); a unitig prints as its number
 * plus its graph's offset, the sum of max_unitig_number() over the graphs before it (the maximum, not the count); a graph's links in
 * get_links_for_gfa order: per unitig in file order its forward list, then its reverse list, each in L-line order.
 * The number of launches depends on the bits of twice the number of unitigs (the link sort's key) and on nothing else.
 * Errors (return 1, ac_last_error; never an abort): no graph; null pointers; offsets that do not ascend; "combine: graph G: unitig number
 * N occurs more than once" (the lowest such (G, N)); "combine: graph G: offset O + its highest unitig number M does not fit 32 bits" (the
 * first such graph in output order); "combine: graph G: link I (a -> b) names no unitig of its graph" (the lowest such link); "combine:
 * graph G: the total of bases reaches 2^46 with this graph".  G is the graph's place in the caller's list, from 0. */
typedef struct ac_combined ac_combined;
typedef struct {
    uint32_t input_index;           /* the graph's place in the caller's list */
    uint32_t unitigs;
    uint64_t length, links;         /* total_length(); entries of its link list */
    uint64_t offset;                /* added to its numbers */
    uint32_t max_number;            /* max_unitig_number(); 0 for an empty graph */
    uint32_t topology;              /* AC_TOPOLOGY_* (ac_topology_name) */
    uint32_t has_read_depth;        /* cluster_depth (combine.rs:107-119) is Some */
    uint32_t reserved;
    double read_depth;              /* cluster_depth: sum of depth * length over sum of length, over the unitigs that have a depth, in unitig order */
} ac_combined_cluster;
typedef struct {
    uint32_t graph, index;          /* the input index of its graph; its place in that graph's file order, from 0 */
    uint32_t number, length;        /* printed number: its own + the graph's offset */
    double depth;                   /* printed in DP:f: the caller's depth; with read depths the read depth, 0.0 where there is none */
    double read_depth;              /* 0 where has_read_depth is 0 */
    uint8_t has_read_depth;
    uint8_t flags;                  /* as ac_components_unitig_flags: 1 open start, 2 open end, 4 hairpin start, 8 hairpin end, 16 isolated and circular, 32 isolated and linear */
    uint8_t type;                   /* AC_UNITIG_* */
    uint8_t reserved[5];
} ac_combined_unitig;
typedef struct {
    uint32_t size;                  /* the library's sizeof(ac_combined_summary) */
    uint32_t graphs;
    uint64_t bases, unitigs, links; /* consensus_assembly_bases, consensus_assembly_unitigs */
    uint32_t fully_resolved;        /* every graph has exactly one unitig */
    uint32_t with_reads;
    uint32_t launches, read_backs;
    double seconds_device;          /* the kernels of the call, by device events */
} ac_combined_summary;
int ac_combine_graphs(uint32_t n_graphs, const uint64_t* unitig_off, const uint64_t* link_off, const uint32_t* number, const uint32_t* unitig_len,
        const double* depth /* or NULL */, const uint8_t* type /* or NULL */, const ac_link* links, const double* read_depth, const uint8_t* has_read_depth /* both or NULL */,
        const uint8_t* seq_bytes, const uint64_t* seq_begin /* both or NULL */, int device, ac_combined** out);
/* The same on graph handles (ac_graph_from_gfa of each 5_final.gfa: numbers 1, 2, 3, ...).  type, read_depth, has_read_depth: one array per
 * graph (an entry may be NULL for a graph without unitigs; type[g] NULL = Other), or NULL.  The bytes are copied into the object. */
int ac_combine_handles(const ac_graph* const* graphs, uint32_t n_graphs, const uint8_t* const* type, const double* const* read_depth,
        const uint8_t* const* has_read_depth, int device, ac_combined** out);
/* The arrays belong to the object.  Clusters and unitigs in output order; the links carry printed numbers, graph after graph. */
int ac_combined_clusters(const ac_combined*, const ac_combined_cluster** clusters, uint32_t* n);
int ac_combined_unitigs(const ac_combined*, const ac_combined_unitig** unitigs, uint64_t* n);
int ac_combined_links(const ac_combined*, const ac_link** links, uint64_t* n);
size_t ac_combined_summary_get_sized(const ac_combined*, ac_combined_summary* out, size_t out_size);
void ac_combined_free(ac_combined*);
/* consensus_assembly.gfa ("H\tVN:Z:1.0", S lines with DP:f to two decimals and colour_tag(true), each graph's L lines behind its S lines),
 * consensus_assembly.fasta (">N length=L[ depth=D| depth=unavailable][ circular=true topology=circular| circular=false topology=linear]")
 * and consensus_assembly.yaml (CombineMetrics, metrics.rs:234-248, serde_yaml 0.9 block style).  The first two need the bytes.  The depth
 * lines are what combine.rs:94-104 prints on stderr (empty without reads).  *out is malloc'ed (ac_string_free). */
int ac_combined_gfa_string(const ac_combined*, char** out, uint64_t* len /* may be NULL */);
int ac_combined_fasta_string(const ac_combined*, char** out, uint64_t* len /* may be NULL */);
int ac_combined_yaml_string(const ac_combined*, char** out, uint64_t* len /* may be NULL */);
int ac_combined_depth_lines(const ac_combined*, char** out, uint64_t* len /* may be NULL */);
/* From the texts of the cluster GFAs to the three texts.  The loader is combine's own (UnitigGraph::from_gfa_file as combine uses it): segment
 * numbers in any order and with holes, L lines attached in file order, an L line naming a segment the file lacks dropped, the S lines' CL:Z
 * colours kept, H and P lines ignored.  read_depth, has_read_depth: one array per graph in file order, or both NULL.  summary may be NULL
 * (its size field set by the caller, 0 = the library's).  The three texts are malloc'ed (ac_string_free each). */
int ac_combine_gfas(const char* const* texts, const uint64_t* lens, uint32_t n, const double* const* read_depth, const uint8_t* const* has_read_depth, int device,
        char** gfa, uint64_t* gfa_len, char** fasta, uint64_t* fasta_len, char** yaml, uint64_t* yaml_len /* lengths may be NULL */, ac_combined_summary* summary);
/* The whole command: every file must exist; with reads (n_reads > 0) depth_kmer must be odd and 11 .. 31 and the reads are counted against
 * all graphs together (ac_depth_begin / ac_depth_add_fastq / ac_depth_finish: one table, as the reference).  Creates autocycler_dir when it is
 * missing and writes consensus_assembly.gfa, .fasta and .yaml, each through a temporary file and a rename.  report, when given, receives
 * the depth lines followed by one line saying whether the assembly is fully resolved (malloc'ed, ac_string_free). */
int ac_combine(const char* autocycler_dir, const char* const* in_gfas, uint32_t n_gfas, const char* const* reads, uint32_t n_reads, uint32_t depth_kmer, int device,
        char** report /* may be NULL */);
/* `autocycler gfa2fasta`: one graph, no offset, unitigs with an empty sequence skipped, ">N length=L depth=D[ circular=...]" with the file's
 * DP:f to one decimal.  counts, when given, receives the circular, linear and other sequences.  *fasta is malloc'ed (ac_string_free). */
int ac_gfa2fasta_string(const char* gfa_text, uint64_t len, int device, char** fasta, uint64_t* fasta_len /* may be NULL */, uint64_t* counts /* 3, may be NULL */);
int ac_gfa2fasta(const char* in_gfa, const char* out_fasta, int device, uint64_t* counts /* 3, may be NULL */);

/* The UPGMA tree of `autocycler cluster` and what the reference derives from it, up to the point where clusters are scored and written.
 * The merge loop of upgma (cluster.rs:395-458 with get_closest_pair :461-480) runs on the device: S - 1 merges, each three launches over a
 * nearest-neighbour cache per row, nothing read by the host in between.  Sequences are rows in ascending id order.
 * Arithmetic.  The reference sums the original distances of all member pairs in HashSet order, which differs from process to process, so
 * its means are only defined up to the rounding of an f64 sum in some order.  The library fixes one order: per cluster pair it keeps
 * sum(A, X); at the start sum(i, j) = max(d(i,j), d(j,i)) (make_symmetrical_distances :177-192) and that is the compared value; merging
 * a < b sets sum(a, X) = sum(a, X) + sum(b, X) and compares sum(a, X) / (double)(size(a u b) * size(X)).  Mathematically the reference's
 * mean; bit for bit the reference's result wherever the sums are exact (e.g. distances that are multiples of 2^-16, S <= 300).
 * Among equal minima the lexicographically smallest (a, b) wins, as in get_closest_pair; the merged cluster keeps id a; its node gets the
 * next number after the largest sequence id; left = the node of a, right = the node of b, distance = compared value / 2.
 * normalise != 0: normalise_tree (:483-494) afterwards, on the host.
 * Errors (return 1, ac_last_error), all found before anything is launched except the last: n == 0; ids that do not ascend strictly;
 * largest id + n - 1 > 65535 (the reference's u16 node counter would overflow); n > ac_cluster_max_seqs(); a distance that is NaN,
 * infinite or negative (a device flag, read once after the loop).
 * After the tree: ac_cluster_generate / ac_cluster_qc_nodes below (refine_auto_clusters, score_clustering, clustering_metrics, the QC
 * verdicts) and ac_cluster_min_assemblies (set_min_assemblies).
 * Not done here (the caller's): the per-cluster GFAs, the TSV / YAML / PHYLIP files. */
typedef struct ac_cluster_tree ac_cluster_tree;
typedef struct {
    uint16_t id;                 /* a tip: the sequence id; an internal node: largest id + 1, + 2, ... in merge order */
    int32_t left, right;         /* indices into the node array; -1 at a tip */
    double distance;             /* from the node to the tips (TreeNode::distance) */
} ac_cluster_node;
typedef struct {
    uint16_t a, b;               /* cluster ids, a < b */
    double distance;             /* the value get_closest_pair compared (twice the node's distance before normalisation) */
} ac_cluster_merge;
typedef struct {
    uint32_t n_seqs, launches;
    uint64_t rescans;            /* cache rows scanned again after a merge */
    uint64_t compares;           /* cache rows that only compared the new column */
    double seconds;              /* the merge loop alone, by device events */
} ac_cluster_summary;
/* pairwise_contig_distances, make_symmetrical_distances and upgma on the paths of a graph handle; the matrix is computed and consumed on
 * the device in one session.  asym_out (S x S doubles, or NULL) receives exactly what ac_pairwise_distances writes. */
int ac_cluster_tree_build(const ac_graph*, int normalise, int device, double* asym_out, ac_cluster_tree** out);
/* The same from the caller's asymmetric matrix (row-major, asym[a * n + b] = distance a vs b) and ascending sequence ids. */
int ac_cluster_tree_from_distances(const double* asym, const uint16_t* ids, uint32_t n, int normalise, int device, ac_cluster_tree** out);
/* A tree the caller already holds (any node order; checked to be one binary tree with distinct ids).  No device.  "Tip order" below is
 * the order of the tips in the node array. */
int ac_cluster_tree_from_nodes(const ac_cluster_node* nodes, uint32_t n_nodes, int32_t root, ac_cluster_tree** out);
/* A built tree: the tips first, in sequence order, then the internal nodes in merge order (the root last). */
int ac_cluster_nodes(const ac_cluster_tree*, const ac_cluster_node** nodes, uint32_t* n_nodes, int32_t* root);
int ac_cluster_merges(const ac_cluster_tree*, const ac_cluster_merge** merges, uint32_t* n_merges);   /* none for a from_nodes tree */
/* at most out_size bytes are written; returns the library's sizeof(ac_cluster_summary) */
size_t ac_cluster_summary_get_sized(const ac_cluster_tree*, ac_cluster_summary* out, size_t out_size);
void ac_cluster_free(ac_cluster_tree*);
uint32_t ac_cluster_max_seqs(void);   /* 16384: the loop keeps three S x S f64 arrays on the device, 6.4 GB at this size */
/* automatic_clustering (n_manual == 0, cluster.rs:219-226) or manual_clustering (:228-237, with check_consistency :260-271: nested manual
 * clusters are an error here, not an exit): the node ids of the clusters, ascending, into nodes_out (room for as many as the tree has
 * tips).  A node is a cluster when distance <= cutoff / 2 (inclusive) and nothing below it is manual (collect_clusters :239-247). */
int ac_cluster_cut(const ac_cluster_tree*, double cutoff, const uint16_t* manual, uint32_t n_manual, uint16_t* nodes_out, uint32_t* n_out);
/* The first half of qc_clusters (cluster.rs:522-546): cluster k + 1 = the tips under node cluster_nodes[k] (assign_cluster_to_node
 * :633-642), then reorder_clusters (:882-903: median sequence length descending — median_usize, misc.rs:423-430 — old number ascending on
 * ties).  seq_len and cluster_of_seq have one entry per tip, in tip order; a tip under none of the nodes gets 0.  cluster_dist (n entries)
 * [c - 1] = max_pairwise_distance (:208-217) = 2 * distance of the node behind the reordered cluster c; -1 for a number no sequence
 * carries.  n_clusters (may be NULL): the largest cluster number in use.  An id that is not in the tree is an error. */
int ac_cluster_assign(const ac_cluster_tree*, const uint16_t* cluster_nodes, uint32_t n, const uint64_t* seq_len, uint16_t* cluster_of_seq,
                      double* cluster_dist, uint32_t* n_clusters);
/* The two counts of cluster_is_contained_in_another (cluster.rs:705-717) for every ordered pair of different clusters x, y at
 * [(x - 1) * n_clusters + (y - 1)]: total = pairs (sequence of x, sequence of y), contain = those with d(a,b) < d(b,a) and d(a,b) < cutoff.
 * A host loop, O(S^2) once.  Sequences of cluster 0 take no part. */
int ac_cluster_containment(const double* asym, uint32_t n, const uint16_t* cluster_of_seq, uint32_t n_clusters, double cutoff,
                           uint64_t* contain_count, uint64_t* total_count);
/* tree_to_newick (cluster.rs:381-392; file_form = 0) or the line save_tree_to_newick writes (:363-378; file_form = 1: with the
 * "(...:root_length);" wrapper when the root's distance is below 0.5, and the newline).  Numbers as Rust's `{}` prints an f64.  tip_names:
 * one per tip in tip order (Sequence::string_for_newick), or NULL (the ids).  Free *out with ac_string_free. */
int ac_cluster_newick(const ac_cluster_tree*, const char* const* tip_names, int file_form, char** out);

/* `autocycler cluster` after the tree: generate_clusters (cluster.rs:497-508) = the cut, refine_auto_clusters (:607-630) when there are no
 * manual clusters, check_complete_coverage, the final qc_clusters (:511-570) with its pass / fail verdicts, and clustering_metrics (:852-879).
 * Inputs: the tree; the S x S asymmetric matrix of ac_pairwise_distances / ac_cluster_tree_build (row-major, rows in tip order); and one
 * entry per tip, in tip order: seq_len, assembly (the index 0 .. F - 1 of the sequence's file name, every index in use), cluster_weight
 * (Sequence::cluster_weight) and trusted (Sequence::is_trusted).  ac_cluster_seq_inputs fills the four from a graph loaded from a GFA.
 * Where the work happens.  Whether cluster x is "contained" in cluster y (cluster_is_contained_in_another :692-723: d(a,b) < d(b,a) and
 * d(a,b) < cutoff for more than half of the sequence pairs) and the order-dependent chain over it (:560-567) run on the device for ALL
 * alternatives of a refinement round at once: the matrix goes up once per call and becomes one bit per ordered sequence pair; a round then
 * costs a fixed number of launches and one read-back of one word per cluster and alternative, whatever the number of alternatives.  The
 * comparison contain / total > 0.5 is made as 2 * contain > total in integers (the same for every total <= 2^28).  Per-node facts, the f64
 * scores and the accept walk (alt_score > best_score + 1e-12, every alternative of a round computed from the round's start, the LAST one
 * that beat the running best wins) are the host's.  With manual clusters nothing is launched and the matrix is not read.
 * Arithmetic of the scores.  The reference sums the balance terms in HashMap order; the library fixes c ascending:
 *   balance = (sum over c = 1 .. max of ((double)ones_c / (double)F) * (double)size_c) / (double)S,
 *   tightness = (sum over the passing c ascending of (1.0 - sqrt(dist_c)) * (double)size_c) / (double)(their total size), 0 when none pass,
 *   overall = (balance + tightness) / 2.0.  Bit for bit the reference's wherever every balance term is exact (e.g. F a power of two).
 * Where several passing clusters contain c the reference names whichever its HashMap yields first; the library names the smallest number.
 * Errors (return 1, ac_last_error), found before anything is launched: a tip count that is not n; a node id that is not in the tree; node
 * lists that do not cover every tip exactly once (the reference panics); nested manual clusters; assembly indices that are not dense.  A
 * NaN, infinite or negative distance is a device flag that comes back with the first read-back.  min_assemblies == 0 fails nothing. */
typedef struct ac_cluster_qc ac_cluster_qc;
typedef struct {
    uint16_t node;               /* the cluster's node id */
    uint16_t container;          /* fail & 4: the smallest passing cluster number that contains this one; else 0 */
    uint32_t size;               /* sequences */
    uint32_t assembly_count;     /* cluster_assembly_count (:573-585): per file name the largest cluster_weight, summed */
    uint32_t fail;               /* 0 = passes; 1 = not included in manual clusters, 2 = present in too few assemblies, 4 = contained */
    uint32_t trusted;
    uint32_t reserved;
    uint64_t median_length;      /* median_usize of the sequence lengths: what reorder_clusters sorted by */
    double cluster_dist;         /* max_pairwise_distance */
} ac_cluster_qc_record;
typedef struct {                 /* ClusteringMetrics (metrics.rs:111-121) */
    uint32_t pass_cluster_count, fail_cluster_count, pass_contig_count, fail_contig_count;
    double pass_contig_fraction, fail_contig_fraction, cluster_balance_score, cluster_tightness_score, overall_clustering_score;
} ac_clustering_metrics;
typedef struct {
    uint32_t n_seqs, n_clusters;
    uint32_t rounds;             /* passes of refine_auto_clusters' loop (the last one accepted nothing); 0 for manual clusters and qc_nodes */
    uint32_t evaluations;        /* clusterings or rounds scored on the device: 1 + the rounds that had an alternative; 0 with manual clusters */
    uint32_t pair_batches;       /* launches of the pair kernel: one per evaluation unless AC_CLUSTER_QC_PAIR_BATCH cuts them */
    uint32_t launches;           /* evaluations ? 1 + pair_batches + evaluations : 0 */
    uint32_t readbacks;          /* == evaluations */
    uint32_t reserved;
    uint64_t alternatives;       /* clusterings scored, the start included */
    uint64_t node_pairs;         /* ordered cluster pairs counted on the device */
    uint64_t bytes_read_back;
    double seconds;              /* the evaluations, by device events */
    double start_score;          /* overall score of the clustering refinement started from */
} ac_cluster_qc_summary;
int ac_cluster_generate(const ac_cluster_tree*, const double* asym, uint32_t n, const uint64_t* seq_len, const uint32_t* assembly,
                        const uint32_t* cluster_weight, const uint8_t* trusted, double cutoff, uint32_t min_assemblies,
                        const uint16_t* manual, uint32_t n_manual, int device, ac_cluster_qc** out);
/* qc_clusters alone on the caller's node list (cluster k + 1 = cluster_nodes[k]: the old number reorder_clusters breaks ties by): the final
 * verdicts without refinement, and the score of one clustering. */
int ac_cluster_qc_nodes(const ac_cluster_tree*, const double* asym, uint32_t n, const uint64_t* seq_len, const uint32_t* assembly,
                        const uint32_t* cluster_weight, const uint8_t* trusted, double cutoff, uint32_t min_assemblies,
                        const uint16_t* cluster_nodes, uint32_t n_nodes, const uint16_t* manual, uint32_t n_manual, int device, ac_cluster_qc** out);
/* The arrays belong to the handle.  clusters: the node ids of the final clustering (ascending from ac_cluster_generate; as given from
 * ac_cluster_qc_nodes).  assignment: the reordered cluster number of every tip, in tip order.  records: one per reordered cluster. */
int ac_cluster_qc_clusters(const ac_cluster_qc*, const uint16_t** nodes, uint32_t* n_nodes);
int ac_cluster_qc_assignment(const ac_cluster_qc*, const uint16_t** cluster_of_seq, uint32_t* n);
int ac_cluster_qc_records(const ac_cluster_qc*, const ac_cluster_qc_record** records, uint32_t* n);
int ac_cluster_qc_metrics(const ac_cluster_qc*, ac_clustering_metrics* out);
/* The refinement: per round the number of alternatives (split_clusters :311-335, in its order); scores / accepted hold every alternative's
 * overall score and whether it replaced the running best, round after round (n_scores = the sum of round_alternatives). */
int ac_cluster_qc_trace(const ac_cluster_qc*, const uint32_t** round_alternatives, uint32_t* n_rounds, const double** scores,
                        const uint8_t** accepted, uint64_t* n_scores);
/* at most out_size bytes are written; returns the library's sizeof(ac_cluster_qc_summary) */
size_t ac_cluster_qc_summary_get_sized(const ac_cluster_qc*, ac_cluster_qc_summary* out, size_t out_size);
void ac_cluster_qc_free(ac_cluster_qc*);
/* set_min_assemblies (cluster.rs:645-661) without a user's value: F == 1 -> 1, else max(2, (F + 2) / 4); F = the distinct (dense) indices */
int ac_cluster_min_assemblies(const uint32_t* assembly, uint32_t n, uint32_t* out);
/* The four per-sequence arrays (ac_graph_seq_count entries each; any may be NULL) from a handle that carries file names and headers
 * (ac_graph_from_gfa): assembly numbered by first appearance of the file name; trusted = the lowercased header contains
 * "autocycler_trusted"; cluster_weight = the first whitespace-separated token of the lowercased header that is
 * "autocycler_cluster_weight=" followed by an unsigned integer, else 1 (sequence.rs:89-102; values beyond 2^32 - 1 saturate). */
int ac_cluster_seq_inputs(const ac_graph*, uint64_t* seq_len, uint32_t* assembly, uint32_t* cluster_weight, uint8_t* trusted, uint32_t* n_assemblies);

/* Read-based unitig depths, the --reads step of `autocycler combine` (set_read_depths, depth.rs:45-76; combine.rs:43-46 calls it): a table
 * of the consensus assembly's canonical k-mers (every k-mer of every unitig's forward sequence plus the k-mers that run across a link,
 * each occurrence counted; k odd, 11 .. 31) is built on the device, every read is streamed through it in two passes (count_one_read,
 * depth.rs:394-419: a read with fewer than 0.5 % of its k-mers in the table is left out), and a unitig's depth is the clipped mean of its
 * non-repeat k-mers' read counts times span_bases / hits (tig_kmer_counts, clipped_mean: sequential f64 on the host, in the reference's
 * order).  All graphs of a handle share one table: a k-mer is a repeat when it occurs more than once across all of them together.
 * A graph comes as plain arrays — segments as ac_unitigs_bulk gives them, links in L-line (file) order with both directions present,
 * signed unitig numbers as ac_link — or, ac_depth_begin_handles, as graph handles (ac_unitigs_bulk + ac_links).  Anything in a sequence or
 * a read that is not ACGTacgt breaks the run of k-mers.  Reads may be added in any number of calls; device memory per batch of reads is
 * capped (AC_DEPTH_BATCH_BYTES lowers the cap: tests), a read longer than the cap is a batch of its own.
 * Errors (return 1, ac_last_error), never aborts: k even or outside 11 .. 31, a link end that is 0 or beyond its graph, a read_off that
 * does not ascend, a FASTQ that ends inside a record, ac_depth_finish when no read was accepted ("no reads were found ... which match the
 * consensus assembly", depth.rs:385-391). */
typedef struct ac_depth ac_depth;
typedef struct { const uint8_t* seq_bytes; const uint64_t* seq_begin; const uint32_t* seq_len; uint32_t n_unitigs;
                 const ac_link* links; uint64_t n_links; } ac_depth_graph;
int ac_depth_begin(uint32_t k, const ac_depth_graph* graphs, uint32_t n_graphs, int device, ac_depth** out);
int ac_depth_begin_handles(uint32_t k, const ac_graph* const* graphs, uint32_t n_graphs, int device, ac_depth** out);
int ac_depth_add_reads(ac_depth*, const uint8_t* bases, const uint64_t* read_off /* n_reads + 1 */, uint64_t n_reads);
int ac_depth_add_fastq(ac_depth*, const char* path);   /* plain or gzip, strict 4-line records; host parsing, then ac_depth_add_reads */
typedef struct {
    uint64_t size;            /* in: sizeof the caller's ac_depth_totals (at most that many bytes are written); out: the library's */
    uint64_t reads, rejected_reads, read_bases, span_bases, span_kmers, hits;   /* ReadTotals, depth.rs:446-453 */
    uint64_t distinct_kmers, repeat_kmers, table_slots;
    uint32_t batches, launches;
    double seconds_device;    /* pass 1 + accept + pass 2 of every batch, by device events */
} ac_depth_totals;
int ac_depth_totals_get(const ac_depth*, ac_depth_totals* out);
/* lookup of canonical k-mer values: present[i], assembly_occurrences[i] (before the reset), read_count[i]; any out pointer may be NULL */
int ac_depth_kmer_counts(ac_depth*, const uint64_t* kmers, uint64_t n, uint8_t* present, uint32_t* assembly_occurrences, uint32_t* read_count);
int ac_depth_finish(ac_depth*, uint32_t graph_index, double* depth /* n_unitigs */, uint8_t* has_depth /* 0 = the reference's None */);
void ac_depth_free(ac_depth*);

/* The loader side of save_gfa for the GFAs `compress` writes (UnitigGraph::from_gfa_lines, unitig_graph.rs:55-174): what
 * `autocycler cluster` (cluster.rs:42-43) and `autocycler decompress` (decompress.rs:27-39) start from.  The handle then serves
 * every accessor above (ac_gfa_string on it reproduces the file: tests.rs:108-112), ac_pairwise_distances and: */
int ac_graph_from_gfa(const char* gfa_text, uint64_t len, ac_graph** out);
uint32_t ac_graph_kmer_size(const ac_graph*);
int ac_graph_seq_info(const ac_graph*, uint32_t seq_index, uint16_t* id, uint32_t* length, const char** filename, const char** header);
/* reconstruct_original_sequences (unitig_graph.rs:362-388) for one sequence: out receives its `length` bytes. */
int ac_decompress_seq(const ac_graph*, uint32_t seq_index, uint8_t* out);

/* The whole `autocycler decompress` command (decompress.rs:27-39): in_gfa -> one FASTA per original file name in out_dir
 * (gzip when the name ends in .gz) and / or every contig in out_file (">{filename}__{header}").  Host code. */
int ac_decompress(const char* in_gfa, const char* out_dir, const char* out_file, int threads);

/* Host helper: lay sequences out as the text described above.  text must hold ac_text_size() bytes. */
uint64_t ac_text_size(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs);
int ac_layout_text(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs, uint8_t* text, uint64_t* seq_off,
                   uint16_t* seq_d1, uint16_t* seq_d2);

uint64_t ac_kmer_count(const ac_graph*);                 /* KmerGraph.kmers.len(), both strands (compress.rs:152) */
ac_stats ac_stats_pre(const ac_graph*);                  /* print_basic_graph_info after from_kmer_graph (compress.rs:165) */
ac_stats ac_stats_post(const ac_graph*);                 /* ... and after simplify_structure (compress.rs:177) */
uint32_t ac_unitig_count(const ac_graph*);
/* Unitig idx (0-based, final order; Unitig::number == idx + 1): forward_seq, length, depth. */
int ac_unitig(const ac_graph*, uint32_t idx, const uint8_t** seq, uint32_t* len, double* depth);
/* Unitig::forward_positions / reverse_positions as from_gfa_lines rebuilds them (unitig_graph.rs:151-174). */
int ac_unitig_positions(ac_graph*, uint32_t idx, int forward, const ac_position** positions, uint32_t* n);
int ac_links(const ac_graph*, const ac_link** links, uint64_t* n);   /* get_links_for_gfa order (unitig_graph.rs:333-350) */
/* get_unitig_path_for_sequence_i32 (unitig_graph.rs:467-472) of the seq_index-th input sequence. */
int ac_path(const ac_graph*, uint32_t seq_index, const int32_t** signed_unitigs, uint32_t* n);
/* Bulk views of the finished graph, zero-copy and valid until ac_free(): everything save_gfa (unitig_graph.rs:317-331) reads, in
 * five arrays instead of one call per unitig / sequence — what a caller that rebuilds its own UnitigGraph, or checks a graph of
 * 10^8 unitigs, wants.  seq_bytes + seq_begin[i] .. + seq_len[i] = Unitig::forward_seq of unitig i (number i + 1); depth[i] =
 * Unitig::depth; path_entries[path_off[s] .. path_off[s + 1]) = get_unitig_path_for_sequence_i32 of the s-th input sequence.
 * Any out pointer may be NULL. */
int ac_unitigs_bulk(const ac_graph*, const uint8_t** seq_bytes, const uint64_t** seq_begin, const uint32_t** seq_len,
                    const double** depth);
int ac_paths_bulk(const ac_graph*, const int32_t** path_entries, const uint64_t** path_off /* ac_graph_seq_count() + 1 */,
                  uint64_t* n_entries);
int ac_timings_get(const ac_graph*, ac_timings* out);
/* ac_timings only ever grows at its end.  A client that may meet a newer or older library passes sizeof its own ac_timings: at most
 * that many bytes are written, the library's sizeof(ac_timings) is returned. */
size_t ac_timings_get_sized(const ac_graph*, ac_timings* out, size_t out_size);
void ac_free(ac_graph*);

/* The GFA text save_gfa would write (unitig_graph.rs:317-331): H, S*, L*, P* lines.  filenames/headers:
 * Sequence::filename / contig_header per input sequence (FN:Z / HD:Z tags).  Free with ac_string_free. */
int ac_gfa_string(const ac_graph*, const char* const* filenames, const char* const* headers, char** out,
                  uint64_t* out_len);
/* parts: bit 0 = H, S and L lines, bit 1 = P lines (of the sequences this handle holds paths for). */
int ac_gfa_string_parts(const ac_graph*, int parts, const char* const* filenames, const char* const* headers, char** out,
                        uint64_t* out_len);
void ac_string_free(char*);

/* ---- host side around the hot path ("boundary" and "next" rows of SURVEY.md §8) -------------------------------
 * ac_seqs mirrors what load_sequences returns (compress.rs:98-133): padded, end-repaired Sequences + the
 * per-assembly details for the YAML metrics.  The Rust CLI keeps its own loader; these serve the standalone
 * CLI (autocycler-compress), the tests and the benchmarks. */
typedef struct ac_seqs ac_seqs;
int ac_seqs_load(const char* assemblies_dir, uint32_t k, uint32_t max_contigs, int threads, ac_seqs** out);
/* The device the host-side helpers below run sequence_end_repair on (ac_seqs_load, ac_seqs_from_raw with repair: the padded sequences
 * go up as text, the device kernels of ac_end_repair_device patch it, the sequence ends come back — the library holds no host
 * implementation of the repair).  Default 0; one process per GPU sets its own ordinal. */
int ac_set_host_side_device(int device);
/* Sequence::new_with_seq (sequence.rs:31-59) for ids 1..n + optional sequence_end_repair (compress.rs:202-236, on the device). */
int ac_seqs_from_raw(uint32_t k, uint32_t n, const uint8_t* const* seqs, const uint32_t* lens,
                     const char* const* filenames, const char* const* headers, uint32_t assembly_count, int repair,
                     int threads, ac_seqs** out);
uint32_t ac_seqs_count(const ac_seqs*);
uint32_t ac_seqs_assembly_count(const ac_seqs*);
const ac_seq_view* ac_seqs_views(const ac_seqs*);
int ac_seqs_get(const ac_seqs*, uint32_t i, ac_seq_view* view, const char** filename, const char** header);
double ac_seqs_repair_seconds(const ac_seqs*);
int ac_seqs_metrics_yaml(const ac_seqs*, uint32_t unitig_count, uint64_t unitig_total_length, char** out); /* metrics.rs:65-107 */
void ac_seqs_free(ac_seqs*);
int ac_compress_seqs(uint32_t k, const ac_seqs*, int device, ac_graph** out);
/* The whole command (compress.rs:32-50): writes input_assemblies.gfa / .yaml into autocycler_dir.
 * times[4] = load, end repair, graph build (hot path), write (seconds).  graph_out may be NULL. */
int ac_compress_dir(const char* assemblies_dir, const char* autocycler_dir, uint32_t k, uint32_t max_contigs,
                    int threads, int device, ac_graph** graph_out, double* times);

/* The same over several devices (ac_compress_build_multi behind the host loader; end repair on devices[0]). */
int ac_compress_dir_multi(const char* assemblies_dir, const char* autocycler_dir, uint32_t k, uint32_t max_contigs, int threads,
                          const int* devices, int n_devices, ac_graph** graph_out, double* times);

/* Measured ceilings of the device for the two access patterns the graph build is bound by: random atomicCAS and random 8-byte
 * reads on a 134 MB table, in 10^9 operations per second (a ~20 ms microbenchmark; bench.py prices its kernels against them).
 * _at: on a table of table_slots 8-byte slots (rounded up to a power of two between 2^24 and 2^30) — the size of the k-mer table
 * the workload in question builds (ac_timings.table_capacity): a table beyond the 256 MB Infinity Cache takes fewer claims per second. */
int ac_random_access_ceilings(int device, double* cas_gops, double* read_gops);
int ac_random_access_ceilings_at(int device, uint64_t table_slots, double* cas_gops, double* read_gops);
void ac_set_stage_timing(int on);   /* off by default */
int ac_release_memory(void);        /* frees the device arena and the pinned result pool kept between builds */
const char* ac_last_error(void);
int ac_device_count(void);       /* number of visible HIP devices (0 if none / no driver) */
uint32_t ac_max_kmer(void);      /* largest --kmer this build supports */
const char* ac_version(void);
/* The ABI generation of this header (the round it was last changed incompatibly in); ac_abi_version() is the library's.  A caller
 * compiled against another generation must not pass caller-allocated structs that grew (ac_verify_report) or drive the ac_shard_* phases.
 *   5: ac_shard_*: sib_export / all-reduce / ac_shard_degrees between ac_shard_build_novel and the degree exchange whenever
 *      ac_shard_sib_words() > 0; degree buffers are ac_shard_degree_bytes() bytes; ac_shard_paths_export fails after
 *      ac_shard_finish(want & 2) (the rank's own paths were renumbered on the host: read them from the handle).
 *   6: ac_verify_report grew (checks, first_bad_junction; failed bits 2048 / 4096 / 8192).
 *   7: ac_link is two signed unitig numbers (8 bytes; it was { u32 a; u8 a_fwd; u32 b; u8 b_fwd } = 16).
 *   8: additions only (a caller of generation 7 runs unchanged): ac_resolve_bridges, ac_resolve_bridge_paths, ac_path_distances, the
 *      ac_resolve_* accessors with ac_bridge and ac_resolve_summary, ac_resolve_max_path, ac_resolve_free.
 *   9: additions only: ac_cluster_tree_build, ac_cluster_tree_from_distances, ac_cluster_tree_from_nodes, ac_cluster_nodes,
 *      ac_cluster_merges, ac_cluster_summary_get_sized, ac_cluster_cut, ac_cluster_assign, ac_cluster_containment, ac_cluster_newick,
 *      ac_cluster_max_seqs, ac_cluster_free with ac_cluster_node, ac_cluster_merge and ac_cluster_summary.
 *  10: additions only: ac_cluster_generate, ac_cluster_qc_nodes, ac_cluster_qc_clusters, ac_cluster_qc_assignment, ac_cluster_qc_records,
 *      ac_cluster_qc_metrics, ac_cluster_qc_trace, ac_cluster_qc_summary_get_sized, ac_cluster_qc_free, ac_cluster_min_assemblies,
 *      ac_cluster_seq_inputs with ac_cluster_qc_record, ac_clustering_metrics and ac_cluster_qc_summary.
 *  11: additions only: the runtime's test hooks ac_selftest_fills, ac_selftest_fill_order, ac_selftest_readback, ac_selftest_scalar_chain,
 *      ac_selftest_arena, ac_selftest_launch, ac_selftest_atomics, ac_selftest_side_order, ac_selftest_event_ring.
 *  12: additions only: ac_graph_components, ac_components_from_links, ac_components_records, ac_components_of_unitig,
 *      ac_components_members, ac_components_unitig_flags, ac_components_summary_get_sized, ac_topology_name, ac_components_free with
 *      ac_component, ac_components_summary and the AC_TOPOLOGY_* values.
 *  13: additions only: ac_graph_merge_plan, ac_merge_plan_from_links, ac_merge_chains, ac_merge_members, ac_merge_chain_of_unitig,
 *      ac_merge_fixed_flags, ac_merge_sequences, ac_merge_links, ac_merge_summary_get_sized, ac_merge_free with ac_merge_chain,
 *      ac_merge_summary and the AC_UNITIG_* values.  Later additions of the same generation (a caller that does not use them runs
 *      unchanged): ac_graph_subsets, ac_subsets_from_paths, ac_subsets_records, ac_subsets_unitigs, ac_subsets_links, ac_subsets_seqs,
 *      ac_subsets_path_ends, ac_subsets_dense, ac_subsets_summary_get_sized, ac_subsets_free, ac_subsets_components, ac_subsets_merge_plan,
 *      ac_subsets_merged_paths, ac_merged_paths_get, ac_merged_paths_summary_get_sized, ac_merged_paths_free with ac_subset_cluster,
 *      ac_subsets_summary and ac_merged_paths_summary; then, still generation 13 and found by name: ac_merge_finish, ac_subsets_finish,
 *      ac_finished_unitigs, ac_finished_sequences, ac_finished_new_of_old, ac_finished_links, ac_finished_paths,
 *      ac_finished_summary_get_sized, ac_finished_free, ac_finished_gfa_string, ac_finished_to_graph with ac_finished_unitig and
 *      ac_finished_summary; then, likewise: ac_apply_bridges, ac_graph_resolve_apply, ac_applied_unitigs, ac_applied_bridge_of,
 *      ac_applied_links, ac_applied_bridge_sequences, ac_applied_summary_get_sized, ac_applied_free, ac_applied_merge_plan,
 *      ac_applied_finish, ac_applied_gfa_string, ac_resolve_graphs with ac_applied_summary and the AC_APPLY_* values; then, likewise:
 *      ac_clean_graph, ac_graph_clean, ac_cleaned_unitigs, ac_cleaned_links, ac_cleaned_summary_get_sized, ac_cleaned_free,
 *      ac_cleaned_merge_plan, ac_cleaned_finish, ac_cleaned_gfa_string, ac_parse_tig_numbers, ac_gfa_segment_types, ac_clean_gfa, ac_clean
 *      with ac_cleaned_summary and the AC_CLEAN_* values; then, likewise: ac_trim_apply, ac_graph_trim_apply, ac_graph_trim,
 *      ac_trimmed_records, ac_trimmed_summary_get_sized, ac_trimmed_free, ac_trimmed_subsets, ac_trimmed_finish, ac_trimmed_yaml_string,
 *      ac_trim_gfa, ac_trim_dir, ac_resolve_dir with ac_trimmed_record, ac_trimmed_summary and the AC_TRIM_CHOOSE_* values; then, likewise: ac_combine_graphs,
 *      ac_combine_handles, ac_combined_clusters, ac_combined_unitigs, ac_combined_links, ac_combined_summary_get_sized, ac_combined_free,
 *      ac_combined_gfa_string, ac_combined_fasta_string, ac_combined_yaml_string, ac_combined_depth_lines, ac_combine_gfas, ac_combine,
 *      ac_gfa2fasta_string, ac_gfa2fasta with ac_combined_cluster, ac_combined_unitig and ac_combined_summary. */
#define AC_ABI_VERSION 13
int ac_abi_version(void);
const char* ac_source_hash(void);   /* 16 hex digits: digest of the sources this library was built from (csrc/Makefile; tools/source_hash.py) */

#ifdef __cplusplus
}
#endif
#endif
