// C ABI, the sharded build: one job sharded by sequence over several devices, one ac_shard per rank (the collectives between the
// phases are the caller's: autocycler_amd/sharded.py), and what the rank that writes the GFA needs on top of it.
#include <cstring>
#include <memory>

#include "capi_common.hpp"

using namespace ac;
using namespace ac::abi;

struct ac_shard {
    std::unique_ptr<GraphBuilder> b;
    std::vector<uint16_t> seq_ids;
    std::vector<uint32_t> seq_lens;
    int device = 0;
    uint32_t n_shards = 1;
    int phase = 0;   // 1 fragments ready, 2 owned k-mers inserted, 3 novel list + degree words, 4 unitigs + link words, 5 links complete + walk
                     // queries ready, 6 walked, 7 reduced quantities imported, 8 finished
};

// One phase call: the phase check first (then the call's own argument check, if it has one: `refuse` is its text when the check
// fails), the lock and the shard's device second, the builder call, then the phase the call leaves the shard in.
template <class F> static int shard_step(ac_shard* s, const char* name, int need, int next, const char* refuse, F&& call) {
    return guarded([&] {
        if (s->phase != need) throw DeviceError(std::string(name) + ": wrong phase");
        if (refuse) throw DeviceError(refuse);
        DeviceCall on(s->device, DeviceCall::SHARD_PHASE);
        call();
        s->phase = next;
    });
}
template <class F> static int shard_step(ac_shard* s, const char* name, int need, int next, F&& call) {
    return shard_step(s, name, need, next, nullptr, call);
}
// the summed buffer of an exchange may only be left out by a single rank
static const char* sum_required(const ac_shard* s, const void* d_sum, const char* refuse) { return !d_sum && s->n_shards > 1 ? refuse : nullptr; }

extern "C" {

int ac_shard_begin(uint32_t k, uint32_t local_assembly_count, const void* d_text, uint64_t n_text, const uint64_t* seq_off,
                   const uint32_t* seq_len, const uint16_t* seq_ids, const uint16_t* seq_d1, const uint16_t* seq_d2,
                   uint32_t n_seqs, int device, ac_shard** out) {
    return guarded([&] {
        if (!d_text || n_seqs == 0) throw DeviceError("no sequences found in input assemblies");
        if (n_seqs > 32767) throw DeviceError("no more than 32767 input sequences are allowed");
        validate_layout(k, n_text, seq_off, seq_len, seq_d1, seq_d2, n_seqs);
        DeviceCall call(device, DeviceCall::SHARD_BEGIN);
        auto h = std::make_unique<ac_shard>();
        h->device = device;
        h->b = std::make_unique<GraphBuilder>(k);
        set_device_text(*h->b, d_text, n_text, seq_off, seq_len, seq_ids, seq_d1, seq_d2, n_seqs, &h->seq_ids, &h->seq_lens);
        h->b->shard_begin(local_assembly_count);
        h->phase = 1;
        g_live_shards++;
        *out = h.release();
    });
}
int ac_shard_fragment_sizes(const ac_shard* s, uint64_t* text_bytes, uint64_t* n_fragments) {
    *text_bytes = s->b->fragment_text_bytes();
    *n_fragments = s->b->fragment_count();
    return 0;
}
uint64_t ac_shard_local_distinct(const ac_shard* s) { return s->b->local_distinct_count(); }
void ac_shard_set_distinct_upper_bound(ac_shard* s, uint64_t n) { s->b->set_distinct_upper_bound(n); }
int ac_shard_fragments_export(ac_shard* s, void* d_text_out, void* d_meta_out) {
    return guarded([&] {
        if (s->phase < 1) throw DeviceError("ac_shard_fragments_export: no fragments yet");
        DeviceCall on(s->device, DeviceCall::SHARD_PHASE);
        s->b->fragments_export(d_text_out, d_meta_out);
    });
}
// The fragment text as 2-bit codes on the union text's word grid (a quarter of the bytes; nothing to pack on the receiving side).
uint64_t ac_shard_fragment_packed_words(const ac_shard* s, uint64_t union_off) { return s->phase >= 1 ? s->b->fragment_packed_words(union_off) : 0; }
int ac_shard_fragments_export_packed(ac_shard* s, uint64_t union_off, void* d_words_out, void* d_meta_out) {
    return guarded([&] {
        if (s->phase < 1) throw DeviceError("ac_shard_fragments_export_packed: no fragments yet");
        DeviceCall on(s->device, DeviceCall::SHARD_PHASE);
        s->b->fragments_export_packed(union_off, d_words_out, d_meta_out);
    });
}
int ac_shard_build_union_packed(ac_shard* s, uint32_t rank, uint32_t n_shards, const void* d_staged_words, const uint64_t* first_word,
                                const uint64_t* n_words, uint64_t n_union_text, const void* d_meta, uint64_t n_fragments_total) {
    return shard_step(s, "ac_shard_build_union_packed", 1, 2, !first_word || !n_words ? "ac_shard_build_union_packed: no word table" : nullptr, [&] {
        s->b->shard_build_union_packed(rank, n_shards, d_staged_words, first_word, n_words, n_union_text, d_meta, n_fragments_total);
        s->n_shards = n_shards;
    });
}
int ac_shard_build_union(ac_shard* s, uint32_t rank, uint32_t n_shards, const void* d_union_text, uint64_t n_union_text,
                         const void* d_meta, uint64_t n_fragments_total) {
    return shard_step(s, "ac_shard_build_union", 1, 2, [&] {
        s->b->shard_build_union(rank, n_shards, (const uint8_t*)d_union_text, n_union_text, d_meta, n_fragments_total);
        s->n_shards = n_shards;
    });
}
uint64_t ac_shard_bitmap_words(const ac_shard* s) { return s->phase >= 2 ? s->b->bitmap_words() : 0; }
int ac_shard_bitmap_export(ac_shard* s, void* d_out_u64) {
    return shard_step(s, "ac_shard_bitmap_export", 2, 2, [&] { s->b->bitmap_export(d_out_u64); });
}
int ac_shard_build_novel(ac_shard* s, const void* d_bitmap_sum_u64) {
    return shard_step(s, "ac_shard_build_novel", 2, 3, sum_required(s, d_bitmap_sum_u64, "ac_shard_build_novel: the summed bitmap is required when there are several shards"),
                      [&] { s->b->shard_build_novel(d_bitmap_sum_u64); });
}
// round 5: the sibling bits (2 per distinct k-mer, by novel index).  ac_shard_sib_words() > 0 after ac_shard_build_novel: the degree stage
// waits for their sum — ac_shard_sib_export -> all-reduce SUM (uint64) -> ac_shard_degrees; 0: it has run already.
uint64_t ac_shard_sib_words(const ac_shard* s) { return s->phase == 3 ? s->b->sib_words() : 0; }
int ac_shard_sib_export(ac_shard* s, void* d_out_u64) {
    return shard_step(s, "ac_shard_sib_export", 3, 3, [&] { s->b->sib_export(d_out_u64); });
}
int ac_shard_degrees(ac_shard* s, const void* d_sib_sum_u64) {
    return shard_step(s, "ac_shard_degrees", 3, 3, [&] { s->b->shard_degrees(d_sib_sum_u64); });
}
uint64_t ac_shard_degree_bytes(const ac_shard* s) {
    if (s->phase != 3) return 0;
    try { return s->b->degree_bytes(); } catch (const std::exception& e) { last_error() = e.what(); return 0; }
}
uint64_t ac_shard_distinct_count(const ac_shard* s) { return s->b->distinct_count(); }
uint64_t ac_shard_table_capacity(const ac_shard* s) { return s->b->timings().table_capacity; }
int ac_shard_degrees_export(ac_shard* s, void* d_out_u32) {
    return shard_step(s, "ac_shard_degrees_export", 3, 3, [&] { s->b->degrees_export(d_out_u32); });
}
int ac_shard_build_graph(ac_shard* s, const void* d_degrees_sum_u32) {
    return shard_step(s, "ac_shard_build_graph", 3, 4, sum_required(s, d_degrees_sum_u32, "ac_shard_build_graph: the summed degree bytes are required when there are several shards"),
                      [&] { s->b->shard_build_graph(d_degrees_sum_u32); });
}
uint32_t ac_shard_unitig_count(const ac_shard* s) { return s->b->unitig_count(); }
int ac_shard_links_export(ac_shard* s, void* d_links_i32, void* d_wlinks_i64) {
    return shard_step(s, "ac_shard_links_export", 4, 4, [&] { s->b->links_export(d_links_i32, d_wlinks_i64); });
}
int ac_shard_links_import(ac_shard* s, const void* d_links_i32, const void* d_wlinks_i64) {
    return shard_step(s, "ac_shard_links_import", 4, 5, sum_required(s, d_links_i32, "ac_shard_links_import: the summed link words are required when there are several shards"),
                      [&] { s->b->links_import(d_links_i32, d_wlinks_i64); });
}
uint64_t ac_shard_query_count(const ac_shard* s) { return s->phase >= 5 ? s->b->query_count() : 0; }
uint32_t ac_shard_query_key_words(const ac_shard* s) { return s->b->query_key_words(); }
int ac_shard_queries_export(ac_shard* s, void* d_out_u64) {
    return shard_step(s, "ac_shard_queries_export", 5, 5, [&] { s->b->queries_export(d_out_u64); });
}
int ac_shard_answer(ac_shard* s, const void* d_keys_u64, uint64_t n_queries, void* d_out_u64) {
    return shard_step(s, "ac_shard_answer", 5, 5, [&] { s->b->answer_queries(d_keys_u64, n_queries, d_out_u64); });
}
// The owner-routed form of the walk-start exchange (what ac_compress_build_multi does inside the library, multi_build.cpp): the
// rank's keys ordered by owner, counts[r] of them for rank r — one all-to-all sends each key to the ONE rank whose table can answer it,
// ac_shard_answer looks the received keys up, the reverse all-to-all brings the answers back in the same order.
int ac_shard_queries_route(ac_shard* s, uint32_t n_shards, void* d_routed_keys_u64, uint64_t* counts) {
    return shard_step(s, "ac_shard_queries_route", 5, 5, n_shards == 0 || !counts ? "ac_shard_queries_route: no ranks" : nullptr,
                      [&] { s->b->queries_route(n_shards, d_routed_keys_u64, counts); });
}
int ac_shard_walk_routed(ac_shard* s, const void* d_routed_answers_u64) {
    return shard_step(s, "ac_shard_walk_routed", 5, 6, [&] { s->b->shard_walk_routed(d_routed_answers_u64); });
}
int ac_shard_walk(ac_shard* s, const void* d_answers_u64) {
    return shard_step(s, "ac_shard_walk", 5, 6, [&] { s->b->shard_walk(d_answers_u64); });
}
int ac_shard_reduce_export(ac_shard* s, void* d_sum_i32, void* d_min_i32) {
    return shard_step(s, "ac_shard_reduce_export", 6, 6, [&] { s->b->reduce_export((int32_t*)d_sum_i32, (int32_t*)d_min_i32); });
}
int ac_shard_reduce_import(ac_shard* s, const void* d_sum_i32, const void* d_min_i32) {
    return shard_step(s, "ac_shard_reduce_import", 6, 7, [&] { s->b->reduce_import((const int32_t*)d_sum_i32, (const int32_t*)d_min_i32); });
}
int ac_shard_set_allreduce(ac_shard* s, ac_allreduce_fn fn, void* user) {
    return guarded([&] {
        if (s->phase > 7) throw DeviceError("ac_shard_set_allreduce: wrong phase");
        if (!fn) { s->b->set_tail_exchange(nullptr); return; }
        s->b->set_tail_exchange([fn, user](void* d_buf, uint64_t count, int dtype, int op) {
            if (fn(user, d_buf, count, dtype, op) != 0) throw DeviceError("the caller's all-reduce failed (ac_shard_set_allreduce)");
        });
    });
}
int ac_device_copy(void* dst, const void* src, uint64_t bytes, int device) {
    return guarded([&] {
        if (!bytes) return;
#ifdef AC_EMU
        (void)device;
        memmove(dst, src, (size_t)bytes);
#else
        AC_HIP_CHECK(hipSetDevice(device));
        AC_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDefault));
#endif
    });
}
int ac_shard_finish(ac_shard* s, int want, ac_graph** out) {
    return shard_step(s, "ac_shard_finish", 7, 8, [&] {
        auto h = std::make_unique<ac_graph>();
        h->seq_ids = s->seq_ids;
        h->seq_lens = s->seq_lens;
        s->b->shard_finish(&h->g, (want & 1) != 0, (want & 2) != 0);
        h->tm = s->b->timings();
        h->host_arrays = (want & 1) != 0;
        h->host_paths = (want & 2) != 0;
        *out = h.release();
    });
}
uint64_t ac_shard_path_entries(const ac_shard* s) { return s->b->path_entry_count(); }
int ac_shard_paths_export(ac_shard* s, void* d_out_i32) {
    return shard_step(s, "ac_shard_paths_export", 8, 8, [&] { s->b->paths_export(d_out_i32); });
}
void ac_shard_free(ac_shard* s) {
    if (!s) return;
    std::lock_guard<std::mutex> lock(g_build_mutex);
    if (s->phase >= 1) g_live_shards--;
    delete s;
}
// The rank that writes the GFA replaces its own paths by those of ALL sequences of the job (rank order).
int ac_graph_set_paths(ac_graph* g, uint32_t n_seqs_total, const uint16_t* seq_ids, const uint32_t* seq_lens,
                       const uint64_t* path_counts, const void* d_path_i32, int device) {
    return guarded([&] {
        if (!g->host_arrays) throw DeviceError("ac_graph_set_paths: this graph was finished without host arrays");
        if (n_seqs_total == 0 || n_seqs_total > 32767) throw DeviceError("no more than 32767 input sequences are allowed");
        DeviceCall call(device, DeviceCall::SHARD_PHASE);
        std::vector<uint64_t> off((size_t)n_seqs_total + 1, 0);
        for (uint32_t i = 0; i < n_seqs_total; i++) off[i + 1] = off[i] + path_counts[i];
        uint64_t n = off[n_seqs_total];
        HostBlock blk = PinnedPool::get().alloc(n * 4);
        copy_d2h(blk.p, d_path_i32, n * 4);
        const int32_t* p = (const int32_t*)blk.p;
        for (uint32_t s = 0; s < n_seqs_total; s++) {   // every path must spell its sequence (unitig_graph.rs:160-174)
            uint64_t sum = 0;
            for (uint64_t i = off[s]; i < off[s + 1]; i++) {
                uint32_t u = (uint32_t)(p[i] < 0 ? -p[i] : p[i]);
                if (u == 0 || u > g->g.n_unitigs) throw DeviceError("internal error: gathered path names an unknown unitig");
                sum += g->g.seq_len[u - 1];
            }
            if (sum != seq_lens[s]) throw DeviceError("internal error: gathered path length mismatch for sequence " + std::to_string(s + 1));
        }
        g->g.path_block = std::move(blk);
        g->g.path = p;
        g->g.n_path = n;
        g->g.path_off = off;
        g->host_paths = true;
        g->seq_ids.assign(seq_ids, seq_ids + n_seqs_total);
        g->seq_lens.assign(seq_lens, seq_lens + n_seqs_total);
        g->positions_built = false;
    });
}

}  // extern "C"
