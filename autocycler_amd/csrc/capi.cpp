// C ABI of libautocycler_hip.so (include/autocycler_hip.h).  No CPU fallback: every build call runs the
// HIP pipeline on a gfx950 device or fails.  (Under -DAC_EMU the very same entry points drive the serial
// emulation; that library is built only by the CPU test-suite and is named libautocycler_emu.so.)
// This unit: what the others share (capi_common.hpp), the build entries and the accessors of a graph handle.  capi_shard.cpp: the
// sharded build; capi_steps.cpp: the neighbouring steps on a handle; capi_command.cpp: everything that touches files.
#include <algorithm>
#include <cstring>
#include <memory>

#include "capi_common.hpp"
#include "gfa_writer.hpp"

using namespace ac;
using namespace ac::abi;

static void select_device(int device, bool refresh_tuning = true) {
    // (tests / the A/B tool change AC_* variables between builds: AC_TUNING_FOLLOW_ENV; else the knobs were read once.  The rank threads of a
    // multi-device build do not refresh: their entry point did, before it started them)
    if (refresh_tuning) tuning_refresh();
#ifndef AC_EMU
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        throw DeviceError("no HIP device available: the MI355X backend has no CPU fallback");
    if (device < 0 || device >= n) throw DeviceError("invalid HIP device ordinal " + std::to_string(device));
    AC_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    AC_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        throw DeviceError(std::string("device is ") + prop.gcnArchName + "; this library is built for gfx950 only");
#endif
    // The device arena is one process-wide bump allocator: its blocks live on the device they were allocated on.  A call that
    // names another ordinal gives them back first (a build never runs on HBM of another device), together with everything else
    // that is tied to the previous device's memory.  One build at a time per process (g_build_mutex), so nothing is in flight.
    int& arena_device = device_ctx().arena_device;      // (per context: the threads of a multi-device build each have their own)
    if (arena_device != device) {
        if (arena_device >= 0) {
            if (g_live_shards) throw DeviceError("a sharded build is in flight on device " + std::to_string(arena_device) + ": this process cannot use device " + std::to_string(device) + " until it is freed");
            Arena::device().release_all();
#ifndef AC_EMU
            Mailbox::get().release();      // the read-back page is mapped into the previous device's address space
#endif
        }
        arena_device = device;
    }
}

namespace ac {
void select_device_checked(int device) { select_device(device, /*refresh_tuning=*/false); }

namespace abi __attribute__((visibility("hidden"))) {

std::string& last_error() { static thread_local std::string err; return err; }
std::mutex g_build_mutex;
int g_live_shards = 0;
std::atomic<int> g_host_side_device{0};

DeviceCall::DeviceCall(int device, Kind kind) : lock(g_build_mutex) {
    if (g_live_shards && kind != SHARD_PHASE)
        throw DeviceError(kind == SHARD_BEGIN ? "another sharded build is in flight in this process" : "a sharded build is in flight in this process");
    if (kind == ALL_DEVICES) tuning_refresh();
    else select_device(device);
}

void validate(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs) {
    if (!seqs || n_seqs == 0) throw DeviceError("no sequences found in input assemblies");
    if (k % 2 == 0) throw DeviceError("--kmer must be odd");
    if (n_seqs > 32767) throw DeviceError("no more than 32767 input sequences are allowed");
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (!seqs[i].fwd) throw DeviceError("null sequence pointer");
        if (seqs[i].length < k) throw DeviceError("sequence shorter than k");
    }
}

void validate_layout(uint32_t k, uint64_t n_text, const uint64_t* off, const uint32_t* len, const uint16_t* d1, const uint16_t* d2,
                     uint32_t n_seqs) {
    if (k < 1 || k % 2 == 0) throw DeviceError("--kmer must be odd");
    if (!off || !len || !d1 || !d2) throw DeviceError("null sequence table");
    uint64_t prev_end = 0;      // index of the separator before the next sequence
    for (uint32_t i = 0; i < n_seqs; i++) {
        if (len[i] < k) throw DeviceError("sequence " + std::to_string(i + 1) + " is shorter than k");
        const uint64_t plen = (uint64_t)len[i] + k - 1;
        if (off[i] != prev_end + 1) throw DeviceError("sequence table: sequence " + std::to_string(i + 1) + " does not start right behind the separator of the previous one");
        if (off[i] + plen + 1 > n_text) throw DeviceError("sequence table: sequence " + std::to_string(i + 1) + " runs past the end of the text");
        if (d1[i] > k - 1 || d2[i] > k - 1 || (uint32_t)d1[i] + d2[i] > k - 1) throw DeviceError("sequence table: more padding dots than k - 1 on sequence " + std::to_string(i + 1));
        prev_end = off[i] + plen;
    }
    if (n_seqs && prev_end + 1 != n_text) throw DeviceError("sequence table: the text does not end with the separator of the last sequence");
}

std::vector<SeqView> seq_views(const ac_seq_view* seqs, uint32_t n_seqs, std::vector<uint16_t>* seq_ids, std::vector<uint32_t>* seq_lens) {
    std::vector<SeqView> v(n_seqs);
    for (uint32_t i = 0; i < n_seqs; i++) {
        v[i] = SeqView{seqs[i].fwd, seqs[i].length};
        seq_ids->push_back(seqs[i].id);
        seq_lens->push_back(seqs[i].length);
    }
    return v;
}

void set_device_text(GraphBuilder& b, const void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                     const uint16_t* ids, const uint16_t* seq_d1, const uint16_t* seq_d2, uint32_t n_seqs,
                     std::vector<uint16_t>* seq_ids, std::vector<uint32_t>* seq_lens) {
    std::vector<uint64_t> off(seq_off, seq_off + n_seqs);
    std::vector<uint32_t> len(seq_len, seq_len + n_seqs);
    std::vector<uint16_t> d1(seq_d1, seq_d1 + n_seqs), d2(seq_d2, seq_d2 + n_seqs);
    seq_ids->assign(ids, ids + n_seqs);
    *seq_lens = len;
    b.set_text_device((const uint8_t*)d_text, n_text, off, len, d1, d2);
}

}  // namespace abi
}  // namespace ac

// compress.rs:42-44 behind the ABI: one device pipeline from the packed text to the final UnitigGraph.
static void build_graph(GraphBuilder& b, uint32_t assembly_count, ac_graph* h) {
    b.build(assembly_count, &h->g);
    h->tm = b.timings();
}

// The _sized getters, for a caller that was compiled against another version of the header: at most out_size bytes are written (the
// structs only ever grow at their end), the library's own size is returned.
template <class T> static size_t copy_sized(const T& full, T* out, size_t out_size) {
    memcpy(out, &full, std::min(out_size, sizeof full));
    return sizeof full;
}

extern "C" {

const char* ac_last_error(void) { return last_error().c_str(); }
const char* ac_version(void) {
#ifdef AC_EMU
    return "autocycler_amd 0.1 (CPU emulation, tests only)";
#else
    return "autocycler_amd 0.1 (gfx950)";
#endif
}
int ac_abi_version(void) { return AC_ABI_VERSION; }
int ac_set_host_side_device(int device) { if (device < 0) return fail("invalid HIP device ordinal"); g_host_side_device.store(device); return 0; }
void ac_set_stage_timing(int on) { set_stage_timing(on != 0); }
// The device arena and the pool of pinned result blocks stay allocated between builds; this gives them back (e.g. before a
// long-lived host process turns to other work).  Graph handles that are still alive keep their blocks.
int ac_release_memory(void) {
    return guarded([&] {
        std::lock_guard<std::mutex> lock(g_build_mutex);
        if (g_live_shards) throw DeviceError("a sharded build is in flight in this process");
        Arena::device().release_all();
        release_multi_contexts();
        PinnedPool::get().trim();
        release_host_stager();
        scan_pool().release();
#ifndef AC_EMU
        Mailbox::get().release();
#endif
    });
}
uint32_t ac_max_kmer(void) { int m = max_supported_k(); return (uint32_t)(m % 2 ? m : m - 1); }
int ac_device_count(void) {
#ifndef AC_EMU
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
#else
    return 0;
#endif
}

uint64_t ac_text_size(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs) {
    uint64_t n = 1;
    for (uint32_t i = 0; i < n_seqs; i++) n += (uint64_t)seqs[i].length + k - 1 + 1;
    return n;
}
int ac_layout_text(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs, uint8_t* text, uint64_t* seq_off,
                   uint16_t* seq_d1, uint16_t* seq_d2) {
    return guarded([&] {
        std::vector<SeqView> v(n_seqs);
        for (uint32_t i = 0; i < n_seqs; i++) v[i] = SeqView{seqs[i].fwd, seqs[i].length};
        std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<uint16_t> d1, d2;
        std::vector<uint8_t> t = layout_text(v, k, &off, &len, &d1, &d2);
        memcpy(text, t.data(), t.size());
        for (uint32_t i = 0; i < n_seqs; i++) { seq_off[i] = off[i]; seq_d1[i] = d1[i]; seq_d2[i] = d2[i]; }
    });
}

int ac_pack_text(const uint8_t* text, uint64_t n_text, uint64_t* bits, uint32_t* mask32, int force_scalar) {
    return guarded([&] {
        if (!text || !bits || !mask32) throw DeviceError("null pointer");
        pack_text_host(text, n_text, bits, mask32, force_scalar != 0);
    });
}

int ac_compress_build(uint32_t k, uint32_t assembly_count, const ac_seq_view* seqs, uint32_t n_seqs, int device,
                      ac_graph** out) {
    return guarded([&] {
        validate(k, seqs, n_seqs);
        DeviceCall call(device);
        auto h = std::make_unique<ac_graph>();
        const std::vector<SeqView> v = seq_views(seqs, n_seqs, &h->seq_ids, &h->seq_lens);      // (the upload reads them until the build has its last chunk)
        GraphBuilder b(k);
        b.set_sequences_host(v);
        build_graph(b, assembly_count, h.get());
        *out = h.release();
    });
}

// compress.rs:42-44 over several devices of one node: one call, one process, the same graph.
int ac_compress_build_multi(uint32_t k, uint32_t assembly_count, const ac_seq_view* seqs, uint32_t n_seqs, const int* devices, int n_devices,
                            ac_graph** out) {
    return guarded([&] {
        validate(k, seqs, n_seqs);
        if (!devices || n_devices < 1) throw DeviceError("ac_compress_build_multi: no devices");
        if (n_devices > 64) throw DeviceError("ac_compress_build_multi: more than 64 devices");
        DeviceCall call(-1, DeviceCall::ALL_DEVICES);
        auto h = std::make_unique<ac_graph>();
        const std::vector<SeqView> v = seq_views(seqs, n_seqs, &h->seq_ids, &h->seq_lens);
        int transport = MULTI_AUTO;
        if (const int e = tuning_multi_transport()) transport = e == 1 ? MULTI_HOST_STAGED : MULTI_RCCL;
        build_multi(k, assembly_count, v, std::vector<int>(devices, devices + n_devices), transport, &h->g, &h->tm, &h->multi);
        *out = h.release();
    });
}
int ac_multi_info_get(const ac_graph* g, ac_multi_info* o) {
    if (!g || !o) return fail("null pointer");
    const MultiStats& m = g->multi;
    memset(o, 0, sizeof *o);
    o->n_ranks = m.n_ranks; o->transport = m.transport;
    o->bytes_fragments = m.bytes_fragments; o->bytes_bitmap = m.bytes_bitmap; o->bytes_degrees = m.bytes_degrees; o->bytes_links = m.bytes_links;
    o->bytes_queries = m.bytes_queries; o->bytes_answers = m.bytes_answers; o->bytes_reduce = m.bytes_reduce;
    o->queries_total = m.queries_total; o->queries_sent_away = m.queries_sent_away;
    o->table_capacity_max = m.table_capacity_max; o->table_capacity_sum = m.table_capacity_sum;
    o->union_text_bytes = m.union_text_bytes; o->fragments = m.fragments; o->distinct = m.distinct;
    o->seconds_total = m.seconds_total; o->seconds_exchange_max = m.seconds_exchange_max;
    o->candidates_total = m.candidates_total; o->candidates_owned_max = m.candidates_owned_max;
    o->bytes_sibling = m.bytes_sibling; o->bytes_tail = m.bytes_tail; o->degrees_open = m.degrees_open; o->bytes_received_max = m.bytes_received_max;
    o->path_runs_copied = m.path_runs_copied;
    return 0;
}
size_t ac_multi_info_get_sized(const ac_graph* g, ac_multi_info* out, size_t out_size) {
    ac_multi_info t;
    if (!g || !out) { fail("null pointer"); return sizeof t; }
    ac_multi_info_get(g, &t);
    return copy_sized(t, out, out_size);
}

int ac_compress_build_device(uint32_t k, uint32_t assembly_count, const void* d_text, uint64_t n_text,
                             const uint64_t* seq_off, const uint32_t* seq_len, const uint16_t* seq_ids,
                             const uint16_t* seq_d1, const uint16_t* seq_d2, uint32_t n_seqs, int device,
                             ac_graph** out) {
    return guarded([&] {
        if (!d_text || n_seqs == 0) throw DeviceError("no sequences found in input assemblies");
        if (n_seqs > 32767) throw DeviceError("no more than 32767 input sequences are allowed");
        validate_layout(k, n_text, seq_off, seq_len, seq_d1, seq_d2, n_seqs);
        DeviceCall call(device);
        auto h = std::make_unique<ac_graph>();
        GraphBuilder b(k);
        set_device_text(b, d_text, n_text, seq_off, seq_len, seq_ids, seq_d1, seq_d2, n_seqs, &h->seq_ids, &h->seq_lens);
        build_graph(b, assembly_count, h.get());
        *out = h.release();
    });
}

uint32_t ac_graph_seq_count(const ac_graph* g) { return (uint32_t)g->seq_ids.size(); }
int ac_path_counts(const ac_graph* g, uint64_t* counts) {   // entries per sequence; also valid without host arrays
    for (size_t s = 0; s + 1 < g->g.path_off.size(); s++) counts[s] = g->g.path_off[s + 1] - g->g.path_off[s];
    return 0;
}

uint32_t ac_graph_kmer_size(const ac_graph* g) { return g->g.k; }
int ac_graph_seq_info(const ac_graph* g, uint32_t i, uint16_t* id, uint32_t* length, const char** filename, const char** header) {
    if (i >= g->seq_ids.size()) return fail("sequence index out of range");
    if (id) *id = g->seq_ids[i];
    if (length) *length = g->seq_lens[i];
    if (filename) *filename = i < g->filenames.size() ? g->filenames[i].c_str() : nullptr;
    if (header) *header = i < g->headers.size() ? g->headers[i].c_str() : nullptr;
    return 0;
}

uint64_t ac_kmer_count(const ac_graph* g) { return g->g.n_kmers; }
ac_stats ac_stats_pre(const ac_graph* g) { return ac_stats{g->g.pre.unitigs, g->g.pre.links_one_way, g->g.pre.total_length}; }
ac_stats ac_stats_post(const ac_graph* g) { return ac_stats{g->g.post.unitigs, g->g.post.links_one_way, g->g.post.total_length}; }
uint32_t ac_unitig_count(const ac_graph* g) { return g->g.n_unitigs; }

int ac_unitig(const ac_graph* g, uint32_t idx, const uint8_t** seq, uint32_t* len, double* depth) {
    if (idx >= g->g.n_unitigs) return fail("unitig index out of range");
    if (!g->host_arrays) return fail("this rank kept no host arrays (sharded build, not the writing rank)");
    if (seq) *seq = (const uint8_t*)g->g.seq(idx);
    if (len) *len = g->g.seq_len[idx];
    if (depth) *depth = g->g.depth[idx];
    return 0;
}
int ac_unitig_positions(ac_graph* g, uint32_t idx, int forward, const ac_position** positions, uint32_t* n) {
    if (idx >= g->g.n_unitigs) return fail("unitig index out of range");
    return guarded([&] {
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        if (!g->positions_built) { build_positions(&g->g, g->seq_ids, g->seq_lens); g->positions_built = true; }
        auto& v = forward ? g->g.fwd_positions[idx] : g->g.rev_positions[idx];
        static_assert(sizeof(ac_position) == sizeof(Position), "layout");
        *positions = (const ac_position*)v.data();
        *n = (uint32_t)v.size();
    });
}
int ac_links(const ac_graph* g, const ac_link** links, uint64_t* n) {
    static_assert(sizeof(ac_link) == sizeof(Link), "layout");
    if (!g->host_arrays) return fail("this rank kept no host arrays (sharded build, not the writing rank)");
    *links = (const ac_link*)g->g.links;
    *n = g->g.n_links;
    return 0;
}
int ac_path(const ac_graph* g, uint32_t seq_index, const int32_t** signed_unitigs, uint32_t* n) {
    if ((size_t)seq_index + 1 >= g->g.path_off.size()) return fail("sequence index out of range");
    if (!g->host_paths) return fail("this rank kept no paths on the host (sharded build)");
    uint64_t b = g->g.path_off[seq_index], e = g->g.path_off[seq_index + 1];
    *signed_unitigs = g->g.path + b;
    *n = (uint32_t)(e - b);
    return 0;
}
int ac_unitigs_bulk(const ac_graph* g, const uint8_t** seq_bytes, const uint64_t** seq_begin, const uint32_t** seq_len, const double** depth) {
    if (!g->host_arrays) return fail("this rank kept no host arrays (sharded build, not the writing rank)");
    if (seq_bytes) *seq_bytes = (const uint8_t*)g->g.seq_block.p;
    if (seq_begin) *seq_begin = g->g.seq_begin;
    if (seq_len) *seq_len = g->g.seq_len;
    if (depth) *depth = g->g.depth;
    return 0;
}
int ac_paths_bulk(const ac_graph* g, const int32_t** path_entries, const uint64_t** path_off, uint64_t* n_entries) {
    if (!g->host_paths) return fail("this rank kept no paths on the host (sharded build)");
    if (path_entries) *path_entries = g->g.path;
    if (path_off) *path_off = g->g.path_off.data();
    if (n_entries) *n_entries = g->g.n_path;
    return 0;
}
int ac_timings_get(const ac_graph* g, ac_timings* o) {
    const BuildTimings& t = g->tm;
    o->h2d = t.h2d; o->pack = t.pack; o->insert = t.insert; o->collect_sort = t.collect_sort; o->degree = t.degree;
    o->segment = t.segment; o->minkey = t.minkey; o->rank = t.rank; o->paths = t.paths; o->links = t.links; o->seqs = t.seqs;
    o->d2h = t.d2h; o->total_device = t.total_device; o->expand = t.expand;
    o->insert_kernel_ms = t.insert_kernel_ms; o->insert_positions = t.insert_positions;
    o->table_capacity = t.table_capacity; o->n_distinct = t.n_distinct; o->n_path_entries = t.n_path_entries;
    o->simplify_passes = t.simplify_passes; o->n_candidates = t.n_candidates; o->n_levels = t.n_levels;
    o->insert_launches = t.insert_launches; o->insert_real = t.insert_real;
    o->analysis = t.analysis; o->finalize = t.finalize;
    o->fragments = t.fragments; o->union_pack = t.union_pack; o->union_insert = t.union_insert;
    o->n_local_distinct = t.n_local_distinct; o->n_fragments = t.n_fragments; o->fragment_bytes = t.fragment_bytes;
    o->upload_device_ms = t.upload_device_ms;
    o->path_runs_copied = t.path_runs_copied; o->path_entries_walked = t.path_entries_walked; o->position_retries = t.position_retries;
    o->n_candidates_owned = t.n_candidates_owned;
    o->launches = t.launches; o->readbacks = t.readbacks; o->n_degrees_open = t.n_degrees_open; o->sort_retries = t.sort_retries;
    o->insert_rest_known = t.insert_rest_known; o->insert_rest_sampled = t.insert_rest_sampled; o->path_stretches = t.path_stretches;
    o->expand_sparse_sweeps = t.expand_sparse_sweeps; o->expand_sparse_start = t.expand_sparse_start;
    return 0;
}
size_t ac_timings_get_sized(const ac_graph* g, ac_timings* out, size_t out_size) {
    ac_timings t;
    memset(&t, 0, sizeof t);
    ac_timings_get(g, &t);
    return out ? copy_sized(t, out, out_size) : sizeof t;
}
void ac_free(ac_graph* g) { delete g; }

static int gfa_parts_impl(const ac_graph* g, int parts, const char* const* filenames, const char* const* headers, char** out,
                          uint64_t* out_len) {
    return guarded([&] {
        if ((parts & 1) && !g->host_arrays) throw DeviceError("this rank kept no unitigs / links on the host (sharded build)");
        if ((parts & 2) && !g->host_paths) throw DeviceError("this rank kept no paths on the host (sharded build)");
        std::vector<SeqMeta> meta(g->seq_ids.size());
        for (size_t i = 0; i < meta.size(); i++) meta[i] = SeqMeta{g->seq_ids[i], g->seq_lens[i], filenames[i], headers[i]};
        std::string s = gfa_string(g->g, meta, parts);
        char* p = (char*)malloc(s.size() + 1);
        if (!p) throw DeviceError("out of memory");
        memcpy(p, s.data(), s.size()); p[s.size()] = 0;
        *out = p;
        if (out_len) *out_len = s.size();
    });
}
int ac_gfa_string(const ac_graph* g, const char* const* filenames, const char* const* headers, char** out, uint64_t* out_len) {
    return gfa_parts_impl(g, 3, filenames, headers, out, out_len);
}
int ac_gfa_string_parts(const ac_graph* g, int parts, const char* const* filenames, const char* const* headers, char** out,
                        uint64_t* out_len) {
    return gfa_parts_impl(g, parts, filenames, headers, out, out_len);
}
void ac_string_free(char* p) { free(p); }

}  // extern "C"
