// Bounds check of the shipped kernel and stage sources: the CPU emulation (-DAC_EMU) linked into this stand-alone program under the address
// and undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2: only the bytes a DBuf asked for are
// addressable, a red zone follows every allocation, reset — and at level 2 rewound — memory is poisoned).  `make kernel_bounds_check` in
// autocycler_amd/csrc builds it; tests/test_kernel_bounds_emu.py builds it the same way and feeds it.  CPU only.
//
//   kernel_bounds_check selfcheck             the guard's own check: what the arena poisons, asked of the sanitizer, nothing dereferenced
//   kernel_bounds_check CALLS RESULTS         replays a call file (tests/bounds_cases.py writes it) through the C ABI of autocycler_hip.h,
//                                             call by call, and writes every call's outputs to RESULTS; stops at the first call that fails
//
// Call file: "ACBC1\n", then per call  str name | u32 n_env {str key, str value} | u32 n_scalars {i64} | u32 n_arrays {u64 bytes, data}
// (str = u32 length + bytes; little endian; the environment entries hold for that call only).  Result file: per call  u32 return code |
// u32 n_arrays {u64 bytes, data}.  Which scalars and arrays an entry takes and gives is written above its function below.
#include "../../include/autocycler_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
struct Call { std::string name; std::vector<std::pair<std::string, std::string>> env; std::vector<int64_t> s; std::vector<Bytes> a; };
struct Out {
    std::vector<Bytes> a;
    void put(const void* p, size_t bytes) { a.emplace_back((const uint8_t*)p, (const uint8_t*)p + (p ? bytes : 0)); }
    template <class T> void put_vec(const std::vector<T>& v) { put(v.data(), v.size() * sizeof(T)); }
    void put_u64(std::initializer_list<uint64_t> v) { std::vector<uint64_t> t(v); put_vec(t); }
};
template <class T> static const T* arr(const Call& c, size_t i) { return c.a.at(i).empty() ? nullptr : (const T*)c.a[i].data(); }
static double as_double(int64_t bits) { double d; memcpy(&d, &bits, 8); return d; }
static std::vector<std::string> lines_of(const Bytes& b) {
    std::vector<std::string> v; std::string cur;
    for (uint8_t ch : b) { if (ch == '\n') { v.push_back(cur); cur.clear(); } else cur.push_back((char)ch); }
    return v;
}
#define TRY(expr) do { if ((expr) != 0) { fprintf(stderr, "%s: %s failed: %s\n", c.name.c_str(), #expr, ac_last_error()); return 1; } } while (0)

// ---- the graph build, three ways in, and what runs on a built handle --------------------------------------------------------------------
// s: k, assembly_count, n_seqs, mode (0 ac_compress_build, 1 ac_compress_build_multi, 2 ac_compress_build_device on a laid-out text), ranks
//    (mode 1), repair (mode 2: ac_end_repair_device on the text first), extras (1 distances, 2 decompress_device, 4 decompress_seq, 8 verify)
// a: padded sequences one behind the other (length + k - 1 bytes each), u32 lengths, u16 ids, file names and headers (each ends in \n)
// out: GFA | u64 {kmers, pre: unitigs links length, post: unitigs links length} | mode 2: the text after the repair | u16 d1[n] d2[n] |
//      u64 {repair matches} | f64 distances | decompress_device bytes | decompress_seq bytes | the verify report as u64[15]
static void put_report(Out& o, const ac_verify_report& r) {
    o.put_u64({r.failed, r.first_bad_unitig, r.first_bad_link, r.first_bad_path_entry, r.first_bad_sequence, r.first_bad_base, r.unitigs, r.links,
               r.path_entries, r.bases_checked, r.self_mirror_links, r.checks, r.first_bad_junction});
}
static int graph_extras(const Call& c, Out& o, ac_graph* g, int64_t extras, const std::vector<ac_seq_view>& views) {
    const uint32_t S = ac_graph_seq_count(g);
    std::vector<uint32_t> len(S);
    uint64_t total = 0;
    for (uint32_t i = 0; i < S; i++) { uint16_t id; TRY(ac_graph_seq_info(g, i, &id, &len[i], nullptr, nullptr)); total += len[i]; }
    std::vector<double> dist(extras & 1 ? (size_t)S * S : 0);
    if (extras & 1) TRY(ac_pairwise_distances(g, 0, dist.data()));
    o.put_vec(dist);
    Bytes all(extras & 2 ? total : 0);      // (exact sizes: the sanitizer watches the host side of the copies too)
    if (extras & 2) TRY(ac_decompress_device(g, 0, all.data(), total));
    o.put_vec(all);
    Bytes each;
    if (extras & 4)
        for (uint32_t i = 0; i < S; i++) { Bytes one(len[i]); TRY(ac_decompress_seq(g, i, one.data())); each.insert(each.end(), one.begin(), one.end()); }
    o.put_vec(each);
    if (extras & 8) {
        ac_verify_report r; memset(&r, 0, sizeof r);
        TRY(ac_verify_graph(g, views.data(), (uint32_t)views.size(), 0, &r));
        put_report(o, r);
    } else o.put(nullptr, 0);
    return 0;
}
static std::vector<ac_seq_view> views_of(uint32_t k, uint32_t n, const uint8_t* fwd, const uint32_t* len, const uint16_t* ids, std::vector<Bytes>& store) {
    std::vector<ac_seq_view> v(n);
    store.resize(n);
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) {      // one exact heap block per sequence: a read past a sequence's padding is the sanitizer's to see
        const size_t plen = (size_t)len[i] + k - 1;
        store[i].assign(fwd + at, fwd + at + plen);
        at += plen;
        v[i].fwd = store[i].data(); v[i].length = len[i]; v[i].id = ids[i];
    }
    return v;
}
static int do_build(const Call& c, Out& o) {
    const uint32_t k = (uint32_t)c.s.at(0), ac = (uint32_t)c.s.at(1), n = (uint32_t)c.s.at(2);
    const int mode = (int)c.s.at(3), ranks = (int)c.s.at(4), repair = (int)c.s.at(5);
    const int64_t extras = c.s.at(6);
    std::vector<Bytes> store;
    std::vector<ac_seq_view> views = views_of(k, n, arr<uint8_t>(c, 0), arr<uint32_t>(c, 1), arr<uint16_t>(c, 2), store);
    const std::vector<std::string> fn = lines_of(c.a.at(3)), hd = lines_of(c.a.at(4));
    if (fn.size() != n || hd.size() != n) { fprintf(stderr, "build: %zu file names, %zu headers for %u sequences\n", fn.size(), hd.size(), n); return 1; }
    ac_graph* g = nullptr;
    Bytes text; std::vector<uint16_t> d12; uint64_t matches = 0;
    if (mode == 0) TRY(ac_compress_build(k, ac, views.data(), n, 0, &g));
    else if (mode == 1) { std::vector<int> dev((size_t)ranks, 0); TRY(ac_compress_build_multi(k, ac, views.data(), n, dev.data(), ranks, &g)); }
    else {
        text.resize(ac_text_size(k, views.data(), n));
        std::vector<uint64_t> off(n); std::vector<uint16_t> d1(n), d2(n);
        TRY(ac_layout_text(k, views.data(), n, text.data(), off.data(), d1.data(), d2.data()));
        if (repair) { double secs = 0; TRY(ac_end_repair_device(k, text.data(), text.size(), off.data(), arr<uint32_t>(c, 1), d1.data(), d2.data(), n, 0, &secs, &matches)); }
        d12 = d1; d12.insert(d12.end(), d2.begin(), d2.end());
        TRY(ac_compress_build_device(k, ac, text.data(), text.size(), off.data(), arr<uint32_t>(c, 1), arr<uint16_t>(c, 2), d1.data(), d2.data(), n, 0, &g));
        if (repair)      // what the verifier and the caller compare with: the repaired sequences
            for (uint32_t i = 0; i < n; i++) memcpy(store[i].data(), text.data() + off[i], store[i].size());
    }
    std::vector<const char*> fnp(n), hdp(n);
    for (uint32_t i = 0; i < n; i++) { fnp[i] = fn[i].c_str(); hdp[i] = hd[i].c_str(); }
    char* gfa = nullptr; uint64_t gfa_len = 0;
    TRY(ac_gfa_string(g, fnp.data(), hdp.data(), &gfa, &gfa_len));
    o.put(gfa, gfa_len);
    ac_string_free(gfa);
    const ac_stats pre = ac_stats_pre(g), post = ac_stats_post(g);
    o.put_u64({ac_kmer_count(g), pre.unitigs, pre.links_one_way, pre.total_length, post.unitigs, post.links_one_way, post.total_length});
    o.put_vec(text); o.put_vec(d12); o.put_u64({matches});
    const int rc = graph_extras(c, o, g, extras, views);
    ac_free(g);
    return rc;
}
// s: k (of the sequences' padding), n_seqs, extras as above.  a: GFA text, then the sequences as above (verify only).  out: as the extras above
static int do_gfa_ops(const Call& c, Out& o) {
    ac_graph* g = nullptr;
    TRY(ac_graph_from_gfa((const char*)c.a.at(0).data(), c.a[0].size(), &g));
    std::vector<Bytes> store;
    std::vector<ac_seq_view> views;
    if (c.s.at(2) & 8) views = views_of((uint32_t)c.s.at(0), (uint32_t)c.s.at(1), arr<uint8_t>(c, 1), arr<uint32_t>(c, 2), arr<uint16_t>(c, 3), store);
    const int rc = graph_extras(c, o, g, c.s.at(2), views);
    ac_free(g);
    return rc;
}

// ---- trim ------------------------------------------------------------------------------------------------------------------------------
// s: n, max_unitigs, skip_diagonal, min_identity (the double's bits).  a: a i32[n], b i32[n], weights u32.  out: pieces (16 bytes each)
static int do_overlap_alignment(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), mu = (uint32_t)c.s.at(1);
    std::vector<ac_alignment_piece> pieces(2 * (size_t)std::min(n, mu));
    uint32_t np = 0;
    TRY(ac_overlap_alignment(arr<int32_t>(c, 0), arr<int32_t>(c, 1), n, arr<uint32_t>(c, 2), (uint32_t)(c.a.at(2).size() / 4), as_double(c.s.at(3)), mu, (int)c.s.at(2), 0,
                             pieces.data(), &np));
    pieces.resize(np);
    o.put_vec(pieces);
    return 0;
}
// s: n_seqs, max_unitigs, min_identity bits.  a: entries i32, path_off u64[n_seqs + 1], weights u32.  out: ac_trim_result[n_seqs] | u32 {c_se, c_hp, chosen, launches}
static int do_trim_path_slices(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0);
    std::vector<ac_trim_result> res(n);
    ac_trim_summary sm; memset(&sm, 0, sizeof sm); sm.size = sizeof sm;
    TRY(ac_trim_path_slices(arr<int32_t>(c, 0), arr<uint64_t>(c, 1), n, arr<uint32_t>(c, 2), (uint32_t)(c.a.at(2).size() / 4), as_double(c.s.at(2)), (uint32_t)c.s.at(1), 0,
                            res.data(), &sm));
    o.put_vec(res);
    const std::vector<uint32_t> t{sm.c_se, sm.c_hp, sm.chosen, sm.launches};
    o.put_vec(t);
    return 0;
}

// ---- resolve ---------------------------------------------------------------------------------------------------------------------------
// s: n_paths, n_pairs.  a: entries i32, path_off u64, pair_a u32, pair_b u32, weights u32.  out: dist u32[n_pairs] | status u8[n_pairs]
static int do_path_distances(const Call& c, Out& o) {
    const uint64_t np = (uint64_t)c.s.at(1);
    std::vector<uint32_t> dist(np); Bytes status(np);
    TRY(ac_path_distances(arr<int32_t>(c, 0), arr<uint64_t>(c, 1), (uint32_t)c.s.at(0), arr<uint32_t>(c, 2), arr<uint32_t>(c, 3), np, arr<uint32_t>(c, 4),
                          (uint32_t)(c.a.at(4).size() / 4), 0, dist.data(), status.data()));
    o.put_vec(dist); o.put_vec(status);
    return 0;
}
// s: n_seqs.  a: entries i32, path_off u64, consensus weights u32 (empty: all 1), weights u32.
// out: anchors u32 | ac_bridge[] | best paths i32 | distinct entries i32 | distinct path_off u64 | multiplicity u32 | u64 {jobs, jobs_not_launched, launches}
static int do_resolve_bridge_paths(const Call& c, Out& o) {
    ac_resolve* r = nullptr;
    TRY(ac_resolve_bridge_paths(arr<int32_t>(c, 0), arr<uint64_t>(c, 1), (uint32_t)c.s.at(0), arr<uint32_t>(c, 2), arr<uint32_t>(c, 3), (uint32_t)(c.a.at(3).size() / 4), 0, &r));
    const uint32_t* anchors; uint32_t na; TRY(ac_resolve_anchors(r, &anchors, &na)); o.put(anchors, (size_t)na * 4);
    const ac_bridge* br; uint32_t nb; TRY(ac_resolve_bridge_records(r, &br, &nb)); o.put(br, (size_t)nb * sizeof(ac_bridge));
    const int32_t* best; uint64_t nbest; TRY(ac_resolve_best_paths(r, &best, &nbest)); o.put(best, nbest * 4);
    const int32_t* de; const uint64_t* doff; const uint32_t* mult; uint64_t ndp;
    TRY(ac_resolve_distinct_paths(r, &de, &doff, &mult, &ndp));
    o.put(de, (ndp ? doff[ndp] : 0) * 4); o.put(doff, ndp ? (ndp + 1) * 8 : 0); o.put(mult, ndp * 4);
    ac_resolve_summary sm; memset(&sm, 0, sizeof sm);
    ac_resolve_summary_get_sized(r, &sm, sizeof sm);
    o.put_u64({sm.jobs, sm.jobs_not_launched, sm.launches});
    ac_resolve_free(r);
    return 0;
}

// ---- components and the merge plan -----------------------------------------------------------------------------------------------------
// s: n_unitigs, n_links.  a: links (8 bytes each), unitig_len u32, alive u8, marked u8 (each may be empty = NULL).
// out: ac_component[] | component of unitig u32 | member offsets u64 | members u32 | flags u8 | u64 {unitigs, components, topology, links_all, links_one_way, total_length}
static int do_components(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0);
    ac_components* h = nullptr;
    TRY(ac_components_from_links(n, arr<ac_link>(c, 0), (uint64_t)c.s.at(1), arr<uint32_t>(c, 1), arr<uint8_t>(c, 2), arr<uint8_t>(c, 3), 0, &h));
    const ac_component* rec; uint32_t nc; TRY(ac_components_records(h, &rec, &nc)); o.put(rec, (size_t)nc * sizeof(ac_component));
    const uint32_t* of; TRY(ac_components_of_unitig(h, &of)); o.put(of, (size_t)n * 4);
    const uint64_t* off; const uint32_t* mem; TRY(ac_components_members(h, &off, &mem));
    o.put(off, ((size_t)nc + 1) * 8); o.put(mem, (size_t)off[nc] * 4);
    const uint8_t* fl; TRY(ac_components_unitig_flags(h, &fl)); o.put(fl, n);
    ac_components_summary sm; memset(&sm, 0, sizeof sm);
    ac_components_summary_get_sized(h, &sm, sizeof sm);
    o.put_u64({sm.unitigs, sm.components, sm.topology, sm.links_all, sm.links_one_way, sm.total_length});
    ac_components_free(h);
    return 0;
}
// s: n_unitigs, n_links, n_seqs.  a: links, unitig_len u32, alive u8, path_ends i32[2 n_seqs], depth f64, fwd_positions u32, rev_positions u32, type u8,
//    seq_bytes, seq_begin u64 (each but the first two may be empty = NULL).
// out: ac_merge_chain[] | members i32 | chain of unitig u32 | fixed flags u8 | sequences | links | u64 {chains, merged_unitigs, unitigs_after, links_after, bases_copied}
static int do_merge_plan(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0);
    ac_merge* h = nullptr;
    TRY(ac_merge_plan_from_links(n, arr<ac_link>(c, 0), (uint64_t)c.s.at(1), arr<uint32_t>(c, 1), arr<uint8_t>(c, 2), arr<int32_t>(c, 3), (uint32_t)c.s.at(2), arr<double>(c, 4),
                                 arr<uint32_t>(c, 5), arr<uint32_t>(c, 6), arr<uint8_t>(c, 7), arr<uint8_t>(c, 8), arr<uint64_t>(c, 9), 0, &h));
    const ac_merge_chain* ch; uint32_t nc; TRY(ac_merge_chains(h, &ch, &nc)); o.put(ch, (size_t)nc * sizeof(ac_merge_chain));
    const int32_t* mem; uint64_t nm; TRY(ac_merge_members(h, &mem, &nm)); o.put(mem, nm * 4);
    const uint32_t* of; TRY(ac_merge_chain_of_unitig(h, &of)); o.put(of, (size_t)n * 4);
    const uint8_t* fx; TRY(ac_merge_fixed_flags(h, &fx)); o.put(fx, n);
    const uint8_t* sq; uint64_t nsq; TRY(ac_merge_sequences(h, &sq, &nsq)); o.put(sq, nsq);
    const ac_link* lk; uint64_t nl; TRY(ac_merge_links(h, &lk, &nl)); o.put(lk, nl * sizeof(ac_link));
    ac_merge_summary sm; memset(&sm, 0, sizeof sm);
    ac_merge_summary_get_sized(h, &sm, sizeof sm);
    o.put_u64({sm.chains, sm.merged_unitigs, sm.unitigs_after, sm.links_after, sm.bases_copied});
    ac_merge_free(h);
    return 0;
}

// ---- cluster ---------------------------------------------------------------------------------------------------------------------------
// s: n, normalise.  a: asym f64[n * n], ids u16[n].  out: ac_cluster_node[] | i32 {root} | ac_cluster_merge[]
static int do_cluster_tree(const Call& c, Out& o) {
    ac_cluster_tree* t = nullptr;
    TRY(ac_cluster_tree_from_distances(arr<double>(c, 0), arr<uint16_t>(c, 1), (uint32_t)c.s.at(0), (int)c.s.at(1), 0, &t));
    const ac_cluster_node* nodes; uint32_t nn; int32_t root; TRY(ac_cluster_nodes(t, &nodes, &nn, &root));
    o.put(nodes, (size_t)nn * sizeof(ac_cluster_node)); o.put(&root, 4);
    const ac_cluster_merge* mg; uint32_t nm; TRY(ac_cluster_merges(t, &mg, &nm)); o.put(mg, (size_t)nm * sizeof(ac_cluster_merge));
    ac_cluster_free(t);
    return 0;
}

// ---- read depths -----------------------------------------------------------------------------------------------------------------------
// s: k, n_unitigs, n_links, n_batches.  a: seq_bytes, seq_begin u64, seq_len u32, links, then per batch: bases, read_off u64 (n_reads + 1).
// out: u64 {reads, rejected_reads, read_bases, span_bases, span_kmers, hits, distinct_kmers, repeat_kmers, batches} | depth f64[n_unitigs] | has_depth u8[n_unitigs]
static int do_depth(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(1);
    ac_depth_graph dg; dg.seq_bytes = arr<uint8_t>(c, 0); dg.seq_begin = arr<uint64_t>(c, 1); dg.seq_len = arr<uint32_t>(c, 2); dg.n_unitigs = n;
    dg.links = arr<ac_link>(c, 3); dg.n_links = (uint64_t)c.s.at(2);
    ac_depth* d = nullptr;
    TRY(ac_depth_begin((uint32_t)c.s.at(0), &dg, 1, 0, &d));
    for (int64_t b = 0; b < c.s.at(3); b++) {
        const Bytes& off = c.a.at(5 + 2 * (size_t)b);
        TRY(ac_depth_add_reads(d, arr<uint8_t>(c, 4 + 2 * (size_t)b), (const uint64_t*)off.data(), off.size() / 8 - 1));
    }
    std::vector<double> depth(n); Bytes has(n);
    TRY(ac_depth_finish(d, 0, depth.data(), has.data()));
    ac_depth_totals t; memset(&t, 0, sizeof t); t.size = sizeof t;
    TRY(ac_depth_totals_get(d, &t));
    o.put_u64({t.reads, t.rejected_reads, t.read_bases, t.span_bases, t.span_kmers, t.hits, t.distinct_kmers, t.repeat_kmers, t.batches});
    o.put_vec(depth); o.put_vec(has);
    ac_depth_free(d);
    return 0;
}

// ---- the replay ------------------------------------------------------------------------------------------------------------------------
struct Reader {
    FILE* f; bool ok = true;
    void raw(void* p, size_t n) { if (n && fread(p, 1, n, f) != n) ok = false; }
    uint32_t u32() { uint32_t v = 0; raw(&v, 4); return v; }
    uint64_t u64() { uint64_t v = 0; raw(&v, 8); return v; }
    std::string str() { std::string s(u32(), '\0'); raw(&s[0], s.size()); return s; }
};
static const struct { const char* name; int (*fn)(const Call&, Out&); } ENTRIES[] = {
    {"build", do_build}, {"gfa_ops", do_gfa_ops}, {"overlap_alignment", do_overlap_alignment}, {"trim_path_slices", do_trim_path_slices},
    {"path_distances", do_path_distances}, {"resolve_bridge_paths", do_resolve_bridge_paths}, {"components", do_components}, {"merge_plan", do_merge_plan},
    {"cluster_tree", do_cluster_tree}, {"depth", do_depth}};

int guard_selfcheck();      // kernel_bounds_guard.cpp: the one part that looks inside the runtime (device_rt.hpp)

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "selfcheck")) return guard_selfcheck();
    if (argc != 3) { fprintf(stderr, "usage: %s selfcheck | CALLS RESULTS\n", argv[0]); return 2; }
    setenv("AC_TUNING_FOLLOW_ENV", "1", 1);      // (the knobs are read again at every build: the calls set them one by one)
    Reader in{fopen(argv[1], "rb")};
    FILE* out = fopen(argv[2], "wb");
    if (!in.f || !out) { fprintf(stderr, "cannot open the call or the result file\n"); return 2; }
    char magic[6]; in.raw(magic, 6);
    if (!in.ok || memcmp(magic, "ACBC1\n", 6)) { fprintf(stderr, "not a call file\n"); return 2; }
    size_t done = 0;
    for (;;) {
        Call c;
        const uint32_t name_len = in.u32();
        if (!in.ok) break;      // the end of the file
        c.name.assign(name_len, '\0'); in.raw(&c.name[0], name_len);
        for (uint32_t i = in.u32(); i-- > 0;) { std::string a = in.str(), b = in.str(); c.env.emplace_back(a, b); }
        for (uint32_t i = in.u32(); i-- > 0;) c.s.push_back((int64_t)in.u64());
        for (uint32_t i = in.u32(); i-- > 0;) { Bytes b(in.u64()); in.raw(b.data(), b.size()); c.a.push_back(std::move(b)); }
        if (!in.ok) { fprintf(stderr, "call %zu is cut short\n", done); return 2; }
        int (*fn)(const Call&, Out&) = nullptr;
        for (auto& e : ENTRIES) if (c.name == e.name) fn = e.fn;
        if (!fn) { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        for (auto& e : c.env) setenv(e.first.c_str(), e.second.c_str(), 1);
        Out o;
        int rc = 1;
        try { rc = fn(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
        for (auto& e : c.env) unsetenv(e.first.c_str());
        const uint32_t rc32 = (uint32_t)rc, na = (uint32_t)o.a.size();
        fwrite(&rc32, 4, 1, out); fwrite(&na, 4, 1, out);
        for (auto& b : o.a) { const uint64_t n = b.size(); fwrite(&n, 8, 1, out); if (n) fwrite(b.data(), 1, n, out); }
        fflush(out);
        if (rc != 0) { fprintf(stderr, "call %zu (%s) failed: nothing after it is run\n", done, c.name.c_str()); fclose(out); return 1; }
        done++;
    }
    fclose(out);
    ac_release_memory();
    printf("kernel_bounds_check: %zu calls OK\n", done);
    return 0;
}
