// C ABI, the neighbouring steps on a graph handle or on the caller's arrays: end repair, pairwise distances, trim, resolve, cluster, read depths, the
// verifier, decompress, the GFA reload, `clean` (with its file command, a thin wrapper around the text entry), and the self-tests of the device primitives.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>

#include "capi_common.hpp"
#include "gfa_writer.hpp"
#include "graph_depth.hpp"

using namespace ac;
using namespace ac::abi;

extern "C" {

// sequence_end_repair (compress.rs:202-270) on a device-resident text of padded, unrepaired sequences.
int ac_end_repair_device(uint32_t k, void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                         uint16_t* seq_d1, uint16_t* seq_d2, uint32_t n_seqs, int device, double* seconds, uint64_t* n_matches) {
    return guarded([&] {
        if (!d_text || n_seqs == 0) throw DeviceError("no sequences found in input assemblies");
        if (!seq_d1 || !seq_d2) throw DeviceError("null sequence table");
        {   // seq_d1 / seq_d2 are outputs here (the repair counts the surviving dots itself): only the layout is checked
            std::vector<uint16_t> zero(n_seqs, 0);
            validate_layout(k, n_text, seq_off, seq_len, zero.data(), zero.data(), n_seqs);
        }
        DeviceCall call(device);
        std::vector<uint64_t> off(seq_off, seq_off + n_seqs);
        std::vector<uint32_t> len(seq_len, seq_len + n_seqs);
        std::vector<uint16_t> d1(n_seqs, 0), d2(n_seqs, 0);
        RepairTimings tm;
        end_repair_device(k, (uint8_t*)d_text, n_text, off, len, &d1, &d2, &tm);
        for (uint32_t i = 0; i < n_seqs; i++) { seq_d1[i] = d1[i]; seq_d2[i] = d2[i]; }
        if (seconds) *seconds = tm.total;
        if (n_matches) *n_matches = tm.matches;
    });
}

// pairwise_contig_distances (cluster.rs:132-157), the first step of `autocycler cluster`, on the graph just built.
int ac_pairwise_distances(const ac_graph* g, int device, double* out) {
    return guarded([&] {
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        DeviceCall call(device);
        pairwise_distances_device(g->g, (uint32_t)g->seq_ids.size(), out);
    });
}

// ---- `autocycler trim`: the path-overlap alignments on the device (kernels_trim.inc), their post-processing on the host (trim_host.cpp) ----
static void check_min_identity(double min_identity) {
    if (!(min_identity >= 0.0 && min_identity <= 1.0)) throw DeviceError("min_identity must be between 0 and 1");
}
static void trim_slices(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint32_t* weights, uint32_t n_weights, double min_identity,
                        uint32_t max_unitigs, int device, ac_trim_result* out, ac_trim_summary* summary) {
    if (!out || (n_seqs && (!path || !off)) || !weights) throw DeviceError("null pointer");
    check_min_identity(min_identity);
    if (summary && summary->size < sizeof(uint64_t)) throw DeviceError("ac_trim_summary.size must hold the caller's sizeof(ac_trim_summary)");
    for (uint32_t s = 0; s < n_seqs; s++) {
        if (off[s + 1] < off[s] || off[s + 1] - off[s] > 0xFFFFFFFFull) throw DeviceError("path offsets must ascend");
        validate_trim_path(path + off[s], off[s + 1] - off[s], weights, n_weights, ("path of sequence " + std::to_string(s + 1)).c_str());
    }
    DeviceCall call(device);
    TrimDeviceStats st;
    std::vector<TrimResult> res(n_seqs);
    TrimSummary sm;
    trim_paths_host(path, off, n_seqs, weights, min_identity, max_unitigs,
                    [&](const std::vector<AlignJob>& jobs, std::vector<AlignOut>& outs) { overlap_alignment_batch(jobs, weights, max_unitigs, &outs, &st); },
                    res.data(), &sm);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const TrimResult& r = res[s];
        out[s].start_end = ac_trim_slice{r.se.status, r.se.begin, r.se.end, r.se.length};
        out[s].hairpin = ac_trim_slice{r.hp.status, r.hp.begin, r.hp.end, r.hp.length};
        out[s].hairpin_start_trimmed = r.hp_start; out[s].hairpin_end_trimmed = r.hp_end;
    }
    if (summary) {
        ac_trim_summary full;
        memset(&full, 0, sizeof full);
        full.size = sizeof full; full.c_se = sm.c_se; full.c_hp = sm.c_hp; full.chosen = sm.chosen; full.launches = st.launches;
        full.cells = st.cells; full.seconds_device = st.seconds_device;
        const size_t take = std::min<size_t>((size_t)summary->size, sizeof full);
        memcpy(summary, &full, take);
    }
}
int ac_trim_path_slices(const int32_t* path_entries, const uint64_t* path_off, uint32_t n_seqs, const uint32_t* weights, uint32_t n_weights,
                        double min_identity, uint32_t max_unitigs, int device, ac_trim_result* out, ac_trim_summary* summary) {
    return guarded([&] { trim_slices(path_entries, path_off, n_seqs, weights, n_weights, min_identity, max_unitigs, device, out, summary); });
}
int ac_trim_paths(const ac_graph* g, double min_identity, uint32_t max_unitigs, int device, ac_trim_result* out, ac_trim_summary* summary) {
    return guarded([&] {
        if (!g) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        const uint32_t n_seqs = (uint32_t)g->seq_ids.size();
        if (n_seqs == 0 || g->g.path_off.size() != (size_t)n_seqs + 1 || !g->g.seq_len) throw DeviceError("trim: the graph holds no paths");
        trim_slices(g->g.path, g->g.path_off.data(), n_seqs, g->g.seq_len, g->g.n_unitigs, min_identity, max_unitigs, device, out, summary);
    });
}
int ac_overlap_alignment(const int32_t* a, const int32_t* b, uint32_t n, const uint32_t* weights, uint32_t n_weights, double min_identity,
                         uint32_t max_unitigs, int skip_diagonal, int device, ac_alignment_piece* pieces, uint32_t* n_pieces) {
    return guarded([&] {
        if ((n && (!a || !b)) || !weights || !n_pieces || (n && max_unitigs && !pieces)) throw DeviceError("null pointer");
        check_min_identity(min_identity);
        validate_trim_path(a, n, weights, n_weights, "path a");
        validate_trim_path(b, n, weights, n_weights, "path b");
        *n_pieces = 0;
        DeviceCall call(device);
        std::vector<AlignJob> jobs(1);
        jobs[0].a.assign(a, a + n); jobs[0].b.assign(b, b + n); jobs[0].skip_diagonal = skip_diagonal != 0;
        std::vector<AlignOut> outs;
        overlap_alignment_batch(jobs, weights, max_unitigs, &outs, nullptr);
        if (!alignment_passes(&outs[0], min_identity)) return;
        static_assert(sizeof(ac_alignment_piece) == sizeof(AlignPiece), "the piece layouts must agree");
        memcpy(pieces, outs[0].pieces.data(), outs[0].pieces.size() * sizeof(AlignPiece));
        *n_pieces = (uint32_t)outs[0].pieces.size();
    });
}
uint32_t ac_trim_max_unitigs(void) { return trim_max_unitigs(); }

// ---- `autocycler resolve`: anchors, bridges and their best paths.  The path distances on the device (kernels_resolve.inc), everything around
// them on the host (resolve_host.cpp).  Applying the bridges to the graph: ac_graph_resolve_apply, further down ----
struct ac_resolve {
    ResolveResult r;
    std::vector<ac_bridge> records;
    ac_resolve_summary summary;
};
static void check_path_table(const int32_t* entries, const uint64_t* off, uint32_t n_paths, uint32_t n_weights, const char* what) {
    if (n_paths && (!off || (off[n_paths] > off[0] && !entries))) throw DeviceError("null pointer");
    for (uint32_t p = 0; p < n_paths; p++) {
        if (off[p + 1] < off[p]) throw DeviceError("path offsets must ascend");
        validate_resolve_path(entries + off[p], off[p + 1] - off[p], n_weights, (std::string(what) + " " + std::to_string(p + 1)).c_str());
    }
}
int ac_path_distances(const int32_t* entries, const uint64_t* path_off, uint32_t n_paths, const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs,
                      const uint32_t* weights, uint32_t n_weights, int device, uint32_t* dist, uint8_t* status) {
    return guarded([&] {
        if ((n_pairs && (!pair_a || !pair_b || !dist || !status)) || (n_weights && !weights)) throw DeviceError("null pointer");
        check_path_table(entries, path_off, n_paths, n_weights, "path");
        PathPool pool;
        std::vector<uint64_t> weight(n_paths);
        for (uint32_t p = 0; p < n_paths; p++) {
            pool.add(entries + path_off[p], path_off[p + 1] - path_off[p]);
            weight[p] = path_weight(pool.at(p), pool.len(p), weights);
        }
        std::vector<PathPair> jobs;
        std::vector<uint64_t> where;
        for (uint64_t q = 0; q < n_pairs; q++) {
            if (pair_a[q] >= n_paths || pair_b[q] >= n_paths) throw DeviceError("pair " + std::to_string(q) + " names a path that does not exist");
            if (std::max(pool.len(pair_a[q]), pool.len(pair_b[q])) > resolve_max_path())
                throw DeviceError("a path of " + std::to_string(std::max(pool.len(pair_a[q]), pool.len(pair_b[q]))) + " entries is above the " +
                                  std::to_string(resolve_max_path()) + " this library supports (ac_resolve_max_path)");
            dist[q] = 0;
            status[q] = pair_overflows(weight[pair_a[q]], weight[pair_b[q]]) ? 2 : 0;      // 2: the reference's u32 matrix could overflow — not launched
            if (status[q] == 0) { jobs.push_back(PathPair{pair_a[q], pair_b[q]}); where.push_back(q); }
        }
        if (jobs.empty()) return;
        DeviceCall call(device);
        std::vector<uint32_t> d;
        path_distance_batch(pool, jobs, weights, &d, nullptr);
        for (size_t i = 0; i < jobs.size(); i++) dist[where[i]] = d[i];
    });
}
static void resolve_run(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint16_t* seq_ids, const uint32_t* consensus_weight,
                        const uint32_t* weights, uint32_t n_weights, int device, ac_resolve** out) {
    if (!out) throw DeviceError("null pointer");
    *out = nullptr;
    if (n_weights && !weights) throw DeviceError("null pointer");
    check_path_table(path, off, n_seqs, n_weights, "path of sequence");
    auto h = std::make_unique<ac_resolve>();
    ResolveDeviceStats st;
    resolve_bridges_host(path, off, n_seqs, seq_ids, consensus_weight, weights, n_weights,
                         [&](const PathPool& pool, const std::vector<PathPair>& pairs, std::vector<uint32_t>& dist) {
                             DeviceCall call(device);      // (only when there is something to launch)
                             path_distance_batch(pool, pairs, weights, &dist, &st);
                         },
                         &h->r);
    h->records.resize(h->r.bridges.size());
    for (size_t b = 0; b < h->records.size(); b++) {
        const ResolveBridge& s = h->r.bridges[b];
        ac_bridge& d = h->records[b];
        memset(&d, 0, sizeof d);
        d.start = s.start; d.end = s.end; d.depth = s.depth; d.n_distinct = s.n_distinct; d.best_off = s.best_off; d.best_total = s.best_total;
        d.first_distinct = s.first_distinct; d.best_len = s.best_len; d.status = s.status; d.conflicting = s.conflicting; d.culled = s.culled;
        d.cull_rank = s.cull_rank;
    }
    ac_resolve_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = sizeof sm; sm.jobs = st.jobs; sm.jobs_not_launched = h->r.pairs_overflowing; sm.cells = st.cells; sm.largest_job_cells = st.largest_job_cells;
    sm.launches = st.launches; sm.seconds_device = st.seconds_device;
    *out = h.release();
}
int ac_resolve_bridge_paths(const int32_t* path_entries, const uint64_t* path_off, uint32_t n_seqs, const uint32_t* consensus_weight, const uint32_t* weights,
                            uint32_t n_weights, int device, ac_resolve** out) {
    return guarded([&] { resolve_run(path_entries, path_off, n_seqs, nullptr, consensus_weight, weights, n_weights, device, out); });
}
int ac_resolve_bridges(const ac_graph* g, int device, ac_resolve** out) {
    return guarded([&] {
        if (!g) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        const uint32_t n_seqs = (uint32_t)g->seq_ids.size();
        if (n_seqs == 0 || g->g.path_off.size() != (size_t)n_seqs + 1 || !g->g.seq_len) throw DeviceError("resolve: the graph holds no paths");
        std::vector<uint32_t> cw(n_seqs, 1);      // (a built graph carries no headers: every weight is 1, as for headers without the tag)
        for (uint32_t s = 0; s < n_seqs && s < g->headers.size(); s++) cw[s] = consensus_weight_of(g->headers[s].c_str());
        resolve_run(g->g.path, g->g.path_off.data(), n_seqs, g->seq_ids.data(), cw.data(), g->g.seq_len, g->g.n_unitigs, device, out);
    });
}
int ac_resolve_anchors(const ac_resolve* r, const uint32_t** anchors, uint32_t* n) {
    return guarded([&] {
        if (!r || !anchors || !n) throw DeviceError("null pointer");
        *anchors = r->r.anchors.data(); *n = (uint32_t)r->r.anchors.size();
    });
}
int ac_resolve_bridge_records(const ac_resolve* r, const ac_bridge** bridges, uint32_t* n) {
    return guarded([&] {
        if (!r || !bridges || !n) throw DeviceError("null pointer");
        *bridges = r->records.data(); *n = (uint32_t)r->records.size();
    });
}
int ac_resolve_best_paths(const ac_resolve* r, const int32_t** entries, uint64_t* n_entries) {
    return guarded([&] {
        if (!r || !entries) throw DeviceError("null pointer");
        *entries = r->r.best_pool.data();
        if (n_entries) *n_entries = r->r.best_pool.size();
    });
}
int ac_resolve_distinct_paths(const ac_resolve* r, const int32_t** entries, const uint64_t** path_off, const uint32_t** multiplicity, uint64_t* n_paths) {
    return guarded([&] {
        if (!r) throw DeviceError("null pointer");
        if (entries) *entries = r->r.distinct.entries.data();
        if (path_off) *path_off = r->r.distinct.off.data();
        if (multiplicity) *multiplicity = r->r.multiplicity.data();
        if (n_paths) *n_paths = r->r.distinct.size();
    });
}
size_t ac_resolve_summary_get_sized(const ac_resolve* r, ac_resolve_summary* out, size_t out_size) {
    if (r && out) memcpy(out, &r->summary, std::min(out_size, sizeof(ac_resolve_summary)));
    return sizeof(ac_resolve_summary);
}
uint32_t ac_resolve_max_path(void) { return resolve_max_path(); }
void ac_resolve_free(ac_resolve* r) { delete r; }

// ---- connected components and topology: the analysis on the device (kernels_components.inc), totals and the topology chain on the host
// (components_host.cpp).  Read-only: of the graph edits that rest on it, resolve's removal of the anchorless components is ac_graph_resolve_apply ----
struct ac_components {
    ComponentsResult r;
    ac_components_summary summary;
};
static_assert(sizeof(ac_component) == sizeof(ComponentRecord) && offsetof(ac_component, length) == offsetof(ComponentRecord, length) &&
              offsetof(ac_component, marked) == offsetof(ComponentRecord, marked) && offsetof(ac_component, circular_loop) == offsetof(ComponentRecord, circular_loop),
              "ac_component and ComponentRecord are one layout");
static_assert(sizeof(ac_link) == sizeof(Link), "ac_link and Link are one layout");
static void components_run(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* marked,
                           int device, ac_components** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (n_links && !links) throw DeviceError("null pointer: n_links > 0 without links");
    auto h = std::make_unique<ac_components>();
    if (n_unitigs == 0 && n_links == 0) {      // (nothing to launch: no device is asked for)
        h->r.member_off.assign(1, 0);
        components_finish(&h->r);
    } else {
        DeviceCall call(device);
        components_device(n_unitigs, (const Link*)links, n_links, unitig_len, alive, marked, &h->r);
    }
    ac_components_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.unitigs = h->r.alive; sm.components = (uint32_t)h->r.records.size(); sm.topology = h->r.topology;
    sm.links_all = h->r.links_all; sm.links_one_way = h->r.links_one_way; sm.total_length = h->r.total_length;
    sm.launches = h->r.stats.launches; sm.read_backs = h->r.stats.read_backs; sm.seconds_device = h->r.stats.seconds_device;
    *out = h.release();
}
int ac_components_from_links(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* marked,
                             int device, ac_components** out) {
    return guarded([&] { components_run(n_unitigs, links, n_links, unitig_len, alive, marked, device, out); });
}
int ac_graph_components(const ac_graph* g, const uint8_t* marked, int device, ac_components** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!g) throw DeviceError("null pointer");
        if (!g->host_arrays) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        components_run(g->g.n_unitigs, (const ac_link*)g->g.links, g->g.n_links, g->g.seq_len, nullptr, marked, device, out);
    });
}
int ac_components_records(const ac_components* c, const ac_component** records, uint32_t* n) {
    return guarded([&] {
        if (!c || !records || !n) throw DeviceError("null pointer");
        *records = (const ac_component*)c->r.records.data(); *n = (uint32_t)c->r.records.size();
    });
}
int ac_components_of_unitig(const ac_components* c, const uint32_t** component) {
    return guarded([&] {
        if (!c || !component) throw DeviceError("null pointer");
        *component = c->r.component_of.data();
    });
}
int ac_components_members(const ac_components* c, const uint64_t** off, const uint32_t** members) {
    return guarded([&] {
        if (!c || !off || !members) throw DeviceError("null pointer");
        *off = c->r.member_off.data(); *members = c->r.members.data();
    });
}
int ac_components_unitig_flags(const ac_components* c, const uint8_t** flags) {
    return guarded([&] {
        if (!c || !flags) throw DeviceError("null pointer");
        *flags = c->r.flags.data();
    });
}
size_t ac_components_summary_get_sized(const ac_components* c, ac_components_summary* out, size_t out_size) {
    if (c && out) memcpy(out, &c->summary, std::min(out_size, sizeof(ac_components_summary)));
    return sizeof(ac_components_summary);
}
const char* ac_topology_name(uint32_t topology) { return components_topology_name(topology); }
void ac_components_free(ac_components* c) { delete c; }

// ---- the linear-path merge plan: chains, members, sequences and the link set after the merge on the device (kernels_merge.inc); the fixed
// seeds, depths, types and totals on the host (merge_host.cpp).  Read-only: the plan is applied by ac_merge_finish, further down ----
struct ac_merge {
    MergeResult r;
    ac_merge_summary summary;
    uint32_t cluster = 0;      // made by ac_subsets_merge_plan: for which cluster (ac_subsets_merged_paths checks it); 0: by another entry
};
static_assert(sizeof(ac_merge_chain) == sizeof(MergeChainRecord) && offsetof(ac_merge_chain, length) == offsetof(MergeChainRecord, length) &&
              offsetof(ac_merge_chain, seq_off) == offsetof(MergeChainRecord, seq_off) && offsetof(ac_merge_chain, depth) == offsetof(MergeChainRecord, depth) &&
              offsetof(ac_merge_chain, type) == offsetof(MergeChainRecord, type) && offsetof(ac_merge_chain, loop) == offsetof(MergeChainRecord, loop),
              "ac_merge_chain and MergeChainRecord are one layout");
static_assert((int)AC_UNITIG_OTHER == (int)MERGE_TYPE_OTHER && (int)AC_UNITIG_ANCHOR == (int)MERGE_TYPE_ANCHOR &&
              (int)AC_UNITIG_CONSENTIG == (int)MERGE_TYPE_CONSENTIG && (int)AC_UNITIG_BRIDGE == (int)MERGE_TYPE_BRIDGE, "the AC_UNITIG_* values are merge_host.hpp's");
// path: the signed entries whose histogram gives the position counts (a handle with use_paths), or null: fwd / rev are the caller's
static void merge_run(uint32_t n, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const int32_t* path_ends, uint32_t n_seqs,
                      const double* depth, const uint32_t* fwd, const uint32_t* rev, const uint8_t* type, const uint8_t* seq_bytes, const uint64_t* seq_begin,
                      uint64_t seq_total, const int32_t* path, uint64_t n_path, int device, ac_merge** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (n_links && !links) throw DeviceError("null pointer: n_links > 0 without links");
    if (n && !unitig_len) throw DeviceError("null pointer: unitig_len");
    if ((seq_bytes == nullptr) != (seq_begin == nullptr)) throw DeviceError("seq_bytes and seq_begin: both or neither");
    if (n_seqs && !path_ends) throw DeviceError("null pointer: n_seqs > 0 without path_ends");
    if ((fwd == nullptr) != (rev == nullptr)) throw DeviceError("fwd_positions and rev_positions: both or neither");
    auto h = std::make_unique<ac_merge>();
    std::vector<uint8_t> seed;
    merge_seed_fixed(n, alive, path_ends, n_seqs, &seed);
    if (n == 0 && n_links == 0) {      // (nothing to launch: no device is asked for)
        merge_finish(&h->r, unitig_len, alive, depth, fwd, rev, type);
    } else {
        MergePlanInput in;
        in.n_unitigs = n; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.alive = alive; in.seed_fixed = seed.data();
        in.path = path; in.n_path = n_path; in.seq_bytes = seq_bytes; in.seq_begin = seq_begin; in.seq_total = seq_total;
        DeviceCall call(device);
        merge_plan_device(in, &h->r);
        if (path && n_path) { fwd = h->r.fwd_positions.data(); rev = h->r.rev_positions.data(); }
        merge_finish(&h->r, unitig_len, alive, depth, fwd, rev, type);
    }
    ac_merge_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.chains = (uint32_t)h->r.chains.size(); sm.merged_unitigs = h->r.merged_unitigs; sm.unitigs_after = h->r.unitigs_after;
    sm.links_after = h->r.links.size(); sm.bases_copied = h->r.bases_copied; sm.launches = h->r.stats.launches; sm.read_backs = h->r.stats.read_backs;
    sm.seconds_device = h->r.stats.seconds_device; sm.seconds_copy = h->r.seconds_copy;
    *out = h.release();
}
int ac_merge_plan_from_links(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const int32_t* path_ends,
                             uint32_t n_seqs, const double* depth, const uint32_t* fwd_positions, const uint32_t* rev_positions, const uint8_t* type,
                             const uint8_t* seq_bytes, const uint64_t* seq_begin, int device, ac_merge** out) {
    return guarded([&] {
        uint64_t seq_total = 0;      // the bytes behind seq_bytes: up to the end of the last unitig
        if (seq_bytes && seq_begin && unitig_len)
            for (uint32_t u = 0; u < n_unitigs; u++) seq_total = std::max<uint64_t>(seq_total, seq_begin[u] + unitig_len[u]);
        merge_run(n_unitigs, links, n_links, unitig_len, alive, path_ends, n_seqs, depth, fwd_positions, rev_positions, type, seq_bytes, seq_begin, seq_total, nullptr, 0,
                  device, out);
    });
}
int ac_graph_merge_plan(const ac_graph* g, int use_paths, int with_sequences, int device, ac_merge** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!g) throw DeviceError("null pointer");
        if (!g->host_arrays || (use_paths && !g->host_paths)) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        const FinalGraph& f = g->g;
        std::vector<int32_t> ends;      // first and last entry of every non-empty path
        if (use_paths)
            for (size_t s = 0; s + 1 < f.path_off.size(); s++)
                if (f.path_off[s + 1] > f.path_off[s]) { ends.push_back(f.path[f.path_off[s]]); ends.push_back(f.path[f.path_off[s + 1] - 1]); }
        const bool seqs = with_sequences && f.seq_block.p && f.seq_begin;
        merge_run(f.n_unitigs, (const ac_link*)f.links, f.n_links, f.seq_len, nullptr, ends.data(), (uint32_t)(ends.size() / 2), f.depth, nullptr, nullptr, nullptr,
                  seqs ? (const uint8_t*)f.seq_block.p : nullptr, seqs ? f.seq_begin : nullptr, seqs ? f.seq_block.bytes : 0, use_paths ? f.path : nullptr,
                  use_paths ? f.n_path : 0, device, out);
    });
}
int ac_merge_chains(const ac_merge* m, const ac_merge_chain** chains, uint32_t* n) {
    return guarded([&] {
        if (!m || !chains || !n) throw DeviceError("null pointer");
        *chains = (const ac_merge_chain*)m->r.chains.data(); *n = (uint32_t)m->r.chains.size();
    });
}
int ac_merge_members(const ac_merge* m, const int32_t** members, uint64_t* n) {
    return guarded([&] {
        if (!m || !members || !n) throw DeviceError("null pointer");
        *members = m->r.members.data(); *n = m->r.members.size();
    });
}
int ac_merge_chain_of_unitig(const ac_merge* m, const uint32_t** chain) {
    return guarded([&] {
        if (!m || !chain) throw DeviceError("null pointer");
        *chain = m->r.chain_of.data();
    });
}
int ac_merge_fixed_flags(const ac_merge* m, const uint8_t** flags) {
    return guarded([&] {
        if (!m || !flags) throw DeviceError("null pointer");
        *flags = m->r.fixed.data();
    });
}
int ac_merge_sequences(const ac_merge* m, const uint8_t** bytes, uint64_t* n) {
    return guarded([&] {
        if (!m || !bytes || !n) throw DeviceError("null pointer");
        *bytes = m->r.seq.data(); *n = m->r.seq.size();
    });
}
int ac_merge_links(const ac_merge* m, const ac_link** links, uint64_t* n) {
    return guarded([&] {
        if (!m || !links || !n) throw DeviceError("null pointer");
        *links = (const ac_link*)m->r.links.data(); *n = m->r.links.size();
    });
}
size_t ac_merge_summary_get_sized(const ac_merge* m, ac_merge_summary* out, size_t out_size) {
    if (m && out) memcpy(out, &m->summary, std::min(out_size, sizeof(ac_merge_summary)));
    return sizeof(ac_merge_summary);
}
void ac_merge_free(ac_merge* m) { delete m; }

// ---- sequence subsets: what every cluster of sequences keeps of a graph, and one cluster's paths over the merged unitigs of its plan, on the
// device (kernels_subset.inc); labels, sequence lists, path ends and the densified arrays on the host (subset_host.cpp).  Read-only ----
struct ac_subsets {
    SubsetResult r;
    SubsetPlan plan;
    ac_subsets_summary summary;
    // borrowed from the caller until ac_subsets_free
    const ac_link* links = nullptr; uint64_t n_links = 0; const uint32_t* unitig_len = nullptr; const int32_t* path = nullptr; const uint64_t* path_off = nullptr;
    const ac_graph* graph = nullptr;
    const uint8_t* type = nullptr;      // AC_UNITIG_* per unitig, or null = Other: only an ac_trimmed's view carries any
};
struct ac_merged_paths {
    MergedPathsResult r;
    ac_merged_paths_summary summary;
};
static_assert(sizeof(ac_subset_cluster) == sizeof(SubsetClusterRecord) && offsetof(ac_subset_cluster, entries) == offsetof(SubsetClusterRecord, entries) &&
              offsetof(ac_subset_cluster, length) == offsetof(SubsetClusterRecord, length), "ac_subset_cluster and SubsetClusterRecord are one layout");
static void subsets_run(uint32_t n, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const int32_t* path, const uint64_t* path_off,
                        uint32_t n_seqs, const uint16_t* cluster_of_seq, uint32_t n_clusters, const ac_graph* graph, int device, ac_subsets** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!cluster_of_seq) throw DeviceError("null pointer: cluster_of_seq");
    if (!path_off) throw DeviceError("null pointer: path_off");
    if (!unitig_len) throw DeviceError("null pointer: unitig_len");
    if (n_links && !links) throw DeviceError("null pointer: n_links > 0 without links");
    auto h = std::make_unique<ac_subsets>();
    h->links = links; h->n_links = n_links; h->unitig_len = unitig_len; h->path = path; h->path_off = path_off; h->graph = graph;
    h->r.n_unitigs = n;
    subset_prepare(n_seqs, path, path_off, cluster_of_seq, n_clusters, &h->plan, &h->r);
    if (n == 0 || h->plan.kept_entries() == 0) {      // (nothing is alive anywhere; no device is asked for)
        if (h->plan.kept_entries()) {
            uint32_t seq = 0; uint64_t index = 0;
            subset_locate(h->plan, 0, &seq, &index);
            throw DeviceError(subset_bad_entry_message(seq, index, path[path_off[seq] + index], n));
        }
        if (n == 0 && n_links) throw DeviceError(components_bad_link_message(0, links[0].a, links[0].b, 0));
        subset_empty_products(&h->r);
    } else {
        SubsetInput in;
        in.n_unitigs = n; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.alive = alive; in.path = path; in.path_off = path_off;
        in.n_clusters = n_clusters; in.plan = &h->plan;
        DeviceCall call(device);
        subsets_device(in, &h->r);
    }
    subset_finish(&h->r, h->plan);
    ac_subsets_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.clusters = n_clusters; sm.sequences_kept = (uint32_t)h->plan.kept_seq.size(); sm.n_unitigs = n;
    sm.entries_kept = h->r.kept_entries; sm.unitigs = h->r.unitigs.size(); sm.links = h->r.links.size();
    sm.launches = h->r.stats.launches; sm.read_backs = h->r.stats.read_backs; sm.seconds_device = h->r.stats.seconds_device;
    *out = h.release();
}
int ac_subsets_from_paths(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const int32_t* path_entries,
                          const uint64_t* path_off, uint32_t n_seqs, const uint16_t* cluster_of_seq, uint32_t n_clusters, int device, ac_subsets** out) {
    return guarded([&] { subsets_run(n_unitigs, links, n_links, unitig_len, alive, path_entries, path_off, n_seqs, cluster_of_seq, n_clusters, nullptr, device, out); });
}
int ac_graph_subsets(const ac_graph* g, const uint16_t* cluster_of_seq, uint32_t n_clusters, int device, ac_subsets** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!g) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        const FinalGraph& f = g->g;
        const uint32_t n_seqs = (uint32_t)g->seq_ids.size();
        if (f.path_off.size() != (size_t)n_seqs + 1) throw DeviceError("subsets: the graph holds no paths");
        subsets_run(f.n_unitigs, (const ac_link*)f.links, f.n_links, f.seq_len, nullptr, f.path, f.path_off.data(), n_seqs, cluster_of_seq, n_clusters, g, device, out);
    });
}
int ac_subsets_records(const ac_subsets* s, const ac_subset_cluster** records, uint32_t* n_clusters) {
    return guarded([&] {
        if (!s || !records || !n_clusters) throw DeviceError("null pointer");
        *records = (const ac_subset_cluster*)s->r.records.data(); *n_clusters = s->r.n_clusters;
    });
}
int ac_subsets_unitigs(const ac_subsets* s, const uint64_t** off, const uint32_t** unitigs, const uint32_t** fwd_positions, const uint32_t** rev_positions) {
    return guarded([&] {
        if (!s || !off || !unitigs) throw DeviceError("null pointer");
        *off = s->r.unitig_off.data(); *unitigs = s->r.unitigs.data();
        if (fwd_positions) *fwd_positions = s->r.positions.data();
        if (rev_positions) *rev_positions = s->r.positions.data();
    });
}
int ac_subsets_links(const ac_subsets* s, const uint64_t** off, const ac_link** links) {
    return guarded([&] {
        if (!s || !off || !links) throw DeviceError("null pointer");
        *off = s->r.link_off.data(); *links = (const ac_link*)s->r.links.data();
    });
}
int ac_subsets_seqs(const ac_subsets* s, const uint64_t** off, const uint32_t** seq_index) {
    return guarded([&] {
        if (!s || !off || !seq_index) throw DeviceError("null pointer");
        *off = s->r.seq_off.data(); *seq_index = s->r.seq_index.data();
    });
}
int ac_subsets_path_ends(const ac_subsets* s, const uint64_t** off, const int32_t** path_ends) {
    return guarded([&] {
        if (!s || !off || !path_ends) throw DeviceError("null pointer");
        *off = s->r.ends_off.data(); *path_ends = s->r.path_ends.data();
    });
}
int ac_subsets_dense(const ac_subsets* s, uint32_t cluster, uint8_t* alive, uint32_t* fwd_positions, uint32_t* rev_positions, double* depth) {
    return guarded([&] {
        if (!s) throw DeviceError("null pointer");
        subset_dense(s->r, cluster, alive, fwd_positions, rev_positions, depth);
    });
}
size_t ac_subsets_summary_get_sized(const ac_subsets* s, ac_subsets_summary* out, size_t out_size) {
    if (s && out) memcpy(out, &s->summary, std::min(out_size, sizeof(ac_subsets_summary)));
    return sizeof(ac_subsets_summary);
}
void ac_subsets_free(ac_subsets* s) { delete s; }

int ac_subsets_components(const ac_subsets* s, uint32_t cluster, const uint8_t* marked, int device, ac_components** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!s) throw DeviceError("null pointer");
        const uint32_t n = s->r.n_unitigs;
        std::vector<uint8_t> alive(n);
        subset_dense(s->r, cluster, alive.data(), nullptr, nullptr, nullptr);
        const uint64_t l0 = s->r.link_off[cluster - 1], l1 = s->r.link_off[cluster];
        components_run(n, (const ac_link*)s->r.links.data() + l0, l1 - l0, s->unitig_len, alive.data(), marked, device, out);
    });
}
int ac_subsets_merge_plan(const ac_subsets* s, uint32_t cluster, const uint8_t* seq_bytes, const uint64_t* seq_begin, int with_sequences, int device, ac_merge** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!s) throw DeviceError("null pointer");
        if ((seq_bytes == nullptr) != (seq_begin == nullptr)) throw DeviceError("seq_bytes and seq_begin: both or neither");
        const uint32_t n = s->r.n_unitigs;
        std::vector<uint8_t> alive(n);
        std::vector<uint32_t> positions(n);
        std::vector<double> depth(n);
        subset_dense(s->r, cluster, alive.data(), positions.data(), nullptr, depth.data());
        uint64_t seq_total = 0;
        if (!with_sequences) { seq_bytes = nullptr; seq_begin = nullptr; }
        else if (!seq_bytes && s->graph && s->graph->g.seq_block.p && s->graph->g.seq_begin) {
            seq_bytes = (const uint8_t*)s->graph->g.seq_block.p; seq_begin = s->graph->g.seq_begin; seq_total = s->graph->g.seq_block.bytes;
        } else if (seq_bytes)
            for (uint32_t u = 0; u < n; u++) seq_total = std::max<uint64_t>(seq_total, seq_begin[u] + s->unitig_len[u]);
        const uint64_t l0 = s->r.link_off[cluster - 1], l1 = s->r.link_off[cluster], e0 = s->r.ends_off[cluster - 1], e1 = s->r.ends_off[cluster];
        merge_run(n, (const ac_link*)s->r.links.data() + l0, l1 - l0, s->unitig_len, alive.data(), s->r.path_ends.data() + 2 * e0, (uint32_t)(e1 - e0), depth.data(),
                  positions.data(), positions.data(), s->type, seq_bytes, seq_begin, seq_total, nullptr, 0, device, out);
        (*out)->cluster = cluster;
    });
}
int ac_subsets_merged_paths(const ac_subsets* s, uint32_t cluster, const ac_merge* plan, int device, ac_merged_paths** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!s || !plan) throw DeviceError("null pointer");
        subset_check_cluster(s->r, cluster);
        if (plan->r.n_unitigs != s->r.n_unitigs)
            throw DeviceError("merged paths: the plan is over " + std::to_string(plan->r.n_unitigs) + " unitigs, the subsets over " + std::to_string(s->r.n_unitigs));
        if (plan->cluster == 0) throw DeviceError("merged paths: the plan was not made by ac_subsets_merge_plan");
        if (plan->cluster != cluster)
            throw DeviceError("merged paths: the plan was made for cluster " + std::to_string(plan->cluster) + ", not for cluster " + std::to_string(cluster));
        auto h = std::make_unique<ac_merged_paths>();
        const size_t first = (size_t)s->r.seq_off[cluster - 1], count = (size_t)(s->r.seq_off[cluster] - s->r.seq_off[cluster - 1]);
        h->r.seq_index.assign(s->r.seq_index.begin() + first, s->r.seq_index.begin() + first + count);
        if (s->plan.kept_off[first + count] == s->plan.kept_off[first]) {      // (no entry: nothing to launch)
            h->r.path_off.assign(count + 1, 0);
        } else {
            MergedPathsInput in;
            in.n_unitigs = s->r.n_unitigs; in.unitig_len = s->unitig_len; in.path = s->path; in.path_off = s->path_off; in.plan = &s->plan; in.kept_first = first;
            in.kept_count = count; in.merge = &plan->r;
            DeviceCall call(device);
            merged_paths_device(in, &h->r);
        }
        ac_merged_paths_summary& sm = h->summary;
        memset(&sm, 0, sizeof sm);
        sm.size = (uint32_t)sizeof sm; sm.sequences = (uint32_t)count; sm.entries_before = h->r.entries_before; sm.entries_after = h->r.entries.size();
        sm.launches = h->r.stats.launches; sm.read_backs = h->r.stats.read_backs; sm.seconds_device = h->r.stats.seconds_device;
        *out = h.release();
    });
}
int ac_merged_paths_get(const ac_merged_paths* p, const uint32_t** seq_index, uint32_t* n_seqs, const uint64_t** path_off, const int32_t** entries) {
    return guarded([&] {
        if (!p || !seq_index || !n_seqs || !path_off || !entries) throw DeviceError("null pointer");
        *seq_index = p->r.seq_index.data(); *n_seqs = (uint32_t)p->r.seq_index.size(); *path_off = p->r.path_off.data(); *entries = p->r.entries.data();
    });
}
size_t ac_merged_paths_summary_get_sized(const ac_merged_paths* p, ac_merged_paths_summary* out, size_t out_size) {
    if (p && out) memcpy(out, &p->summary, std::min(out_size, sizeof(ac_merged_paths_summary)));
    return sizeof(ac_merged_paths_summary);
}
void ac_merged_paths_free(ac_merged_paths* p) { delete p; }

// ---- a finished graph: a merge plan applied.  The S-line order with renumber_unitigs, the gather, the L lines and the relabelling on the device
// (kernels_finish.inc); the checks and save_gfa's text on the host (finish_host.cpp, gfa_writer.cpp).  Read-only ----
struct ac_finished {
    FinishResult r;
    ac_finished_summary summary;
};
static_assert(sizeof(ac_finished_unitig) == sizeof(FinishedUnitigRecord) && offsetof(ac_finished_unitig, length) == offsetof(FinishedUnitigRecord, length) &&
              offsetof(ac_finished_unitig, seq_off) == offsetof(FinishedUnitigRecord, seq_off) && offsetof(ac_finished_unitig, depth) == offsetof(FinishedUnitigRecord, depth) &&
              offsetof(ac_finished_unitig, type) == offsetof(FinishedUnitigRecord, type), "ac_finished_unitig and FinishedUnitigRecord are one layout");
static void finish_run(const ac_merge* plan, uint32_t n, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const double* depth,
                       const uint8_t* type, const uint8_t* seq_bytes, const uint64_t* seq_begin, uint64_t seq_total, const ac_merged_paths* paths, int renumber, int device,
                       ac_finished** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!plan) throw DeviceError("null pointer: plan");
    if (n_links && !links) throw DeviceError("null pointer: n_links > 0 without links");
    FinishArrays a;
    a.n_unitigs = n; a.unitig_len = unitig_len; a.alive = alive; a.depth = depth; a.type = type; a.seq_bytes = seq_bytes; a.seq_begin = seq_begin; a.n_links = n_links;
    const uint64_t after = finish_check_inputs(plan->r, a, renumber != 0);
    auto h = std::make_unique<ac_finished>();
    if (after == 0) {      // (nothing to launch: no device is asked for)
        finish_empty(&h->r, renumber != 0);
        h->r.new_of_old.assign((size_t)n + plan->r.chains.size(), 0);
        if (paths && !paths->r.entries.empty()) throw DeviceError(finish_bad_path_entry_message(0, paths->r.entries[0]));
    } else {
        FinishInput in;
        in.n_unitigs = n; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.alive = alive; in.depth = depth; in.type = type;
        in.seq_bytes = seq_bytes; in.seq_begin = seq_begin; in.seq_total = seq_total; in.plan = &plan->r; in.renumber = renumber != 0; in.unitigs_after = after;
        if (paths) { in.path = paths->r.entries.data(); in.n_path = paths->r.entries.size(); }
        DeviceCall call(device);
        merge_finish_device(in, &h->r);
        finish_check_result(h->r, plan->r, after);
    }
    h->r.n_unitigs = n; h->r.n_chains = (uint32_t)plan->r.chains.size(); h->r.renumbered = renumber != 0;
    if (paths) { h->r.path_seq = paths->r.seq_index; h->r.path_off = paths->r.path_off; }
    else h->r.path_off.assign(1, 0);
    ac_finished_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.unitigs = (uint32_t)h->r.unitigs.size(); sm.renumbered = renumber != 0; sm.launches = h->r.stats.launches;
    sm.read_backs = h->r.stats.read_backs; sm.links = h->r.links.size(); sm.path_entries = h->r.path_entries.size(); sm.bases = h->r.seq.size();
    sm.tie_items = h->r.tie_items; sm.seconds_device = h->r.stats.seconds_device; sm.seconds_gather = h->r.seconds_gather;
    *out = h.release();
}
int ac_merge_finish(const ac_merge* plan, uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const double* depth,
                    const uint8_t* type, const uint8_t* seq_bytes, const uint64_t* seq_begin, const ac_merged_paths* paths, int renumber, int device, ac_finished** out) {
    return guarded([&] {
        uint64_t seq_total = 0;
        if (seq_bytes && seq_begin && unitig_len)
            for (uint32_t u = 0; u < n_unitigs; u++) seq_total = std::max<uint64_t>(seq_total, seq_begin[u] + unitig_len[u]);
        finish_run(plan, n_unitigs, links, n_links, unitig_len, alive, depth, type, seq_bytes, seq_begin, seq_total, paths, renumber, device, out);
    });
}
int ac_subsets_finish(const ac_subsets* s, uint32_t cluster, const ac_merge* plan, const ac_merged_paths* merged_paths, const uint8_t* seq_bytes, const uint64_t* seq_begin,
                      int renumber, int device, ac_finished** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!s || !plan) throw DeviceError("null pointer");
        if ((seq_bytes == nullptr) != (seq_begin == nullptr)) throw DeviceError("seq_bytes and seq_begin: both or neither");
        subset_check_cluster(s->r, cluster);
        if (plan->cluster != cluster)
            throw DeviceError("finish: the plan was made for cluster " + std::to_string(plan->cluster) + ", not for cluster " + std::to_string(cluster));
        const uint32_t n = s->r.n_unitigs;
        std::vector<uint8_t> alive(n);
        std::vector<double> depth(n);
        subset_dense(s->r, cluster, alive.data(), nullptr, nullptr, depth.data());
        uint64_t seq_total = 0;
        if (!seq_bytes && s->graph && s->graph->g.seq_block.p && s->graph->g.seq_begin) {
            seq_bytes = (const uint8_t*)s->graph->g.seq_block.p; seq_begin = s->graph->g.seq_begin; seq_total = s->graph->g.seq_block.bytes;
        } else if (seq_bytes)
            for (uint32_t u = 0; u < n; u++) seq_total = std::max<uint64_t>(seq_total, seq_begin[u] + s->unitig_len[u]);
        const uint64_t l0 = s->r.link_off[cluster - 1], l1 = s->r.link_off[cluster];
        finish_run(plan, n, (const ac_link*)s->r.links.data() + l0, l1 - l0, s->unitig_len, alive.data(), depth.data(), s->type, seq_bytes, seq_begin, seq_total, merged_paths,
                   renumber, device, out);
    });
}
int ac_finished_unitigs(const ac_finished* f, const ac_finished_unitig** unitigs, uint32_t* n) {
    return guarded([&] {
        if (!f || !unitigs || !n) throw DeviceError("null pointer");
        *unitigs = (const ac_finished_unitig*)f->r.unitigs.data(); *n = (uint32_t)f->r.unitigs.size();
    });
}
int ac_finished_sequences(const ac_finished* f, const uint8_t** bytes, uint64_t* n) {
    return guarded([&] {
        if (!f || !bytes || !n) throw DeviceError("null pointer");
        *bytes = f->r.seq.data(); *n = f->r.seq.size();
    });
}
int ac_finished_new_of_old(const ac_finished* f, const uint32_t** printed, uint64_t* n) {
    return guarded([&] {
        if (!f || !printed || !n) throw DeviceError("null pointer");
        *printed = f->r.new_of_old.data(); *n = f->r.new_of_old.size();
    });
}
int ac_finished_links(const ac_finished* f, const ac_link** links, uint64_t* n) {
    return guarded([&] {
        if (!f || !links || !n) throw DeviceError("null pointer");
        *links = (const ac_link*)f->r.links.data(); *n = f->r.links.size();
    });
}
int ac_finished_paths(const ac_finished* f, const uint32_t** seq_index, uint32_t* n_seqs, const uint64_t** path_off, const int32_t** entries) {
    return guarded([&] {
        if (!f || !seq_index || !n_seqs || !path_off || !entries) throw DeviceError("null pointer");
        *seq_index = f->r.path_seq.data(); *n_seqs = (uint32_t)f->r.path_seq.size(); *path_off = f->r.path_off.data(); *entries = f->r.path_entries.data();
    });
}
size_t ac_finished_summary_get_sized(const ac_finished* f, ac_finished_summary* out, size_t out_size) {
    if (f && out) memcpy(out, &f->summary, std::min(out_size, sizeof(ac_finished_summary)));
    return sizeof(ac_finished_summary);
}
void ac_finished_free(ac_finished* f) { delete f; }
static std::vector<FinishSeqMeta> finish_meta(const ac_finished* f, const uint16_t* seq_ids, const uint32_t* seq_lengths, const char* const* filenames,
                                              const char* const* headers, const uint32_t* cluster_tags) {
    const size_t np = f->r.path_seq.size();
    if (np && (!seq_ids || !seq_lengths || !filenames || !headers)) throw DeviceError("null pointer: the P lines want ids, lengths, filenames and headers");
    std::vector<FinishSeqMeta> meta(np);
    for (size_t i = 0; i < np; i++) {
        if (!filenames[i] || !headers[i]) throw DeviceError("null pointer: filename or header of P line " + std::to_string(i));
        meta[i] = FinishSeqMeta{seq_ids[i], seq_lengths[i], filenames[i], headers[i], cluster_tags ? cluster_tags[i] : 0u};
    }
    return meta;
}
int ac_finished_gfa_string(const ac_finished* f, uint32_t k, const uint16_t* seq_ids, const uint32_t* seq_lengths, const char* const* filenames, const char* const* headers,
                           const uint32_t* cluster_tags, int use_other_colour, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!f) throw DeviceError("null pointer");
        const std::string s = finish_gfa_string(f->r, k, finish_meta(f, seq_ids, seq_lengths, filenames, headers, cluster_tags), use_other_colour != 0);
        char* p = (char*)malloc(s.size() + 1);
        if (!p) throw DeviceError("out of memory");
        memcpy(p, s.c_str(), s.size() + 1);
        *out = p;
        if (len) *len = s.size();
    });
}
int ac_finished_to_graph(const ac_finished* f, uint32_t k, const uint16_t* seq_ids, const uint32_t* seq_lengths, const char* const* filenames, const char* const* headers,
                         ac_graph** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!f) throw DeviceError("null pointer");
        if (!f->r.renumbered) throw DeviceError("finish: a graph handle numbers its unitigs 1, 2, 3, ...: make the finished graph with renumber = 1");
        for (const FinishedUnitigRecord& u : f->r.unitigs)
            if (u.type != MERGE_TYPE_OTHER) throw DeviceError("finish: unitig " + std::to_string(u.number) + " is not of type Other: a graph handle holds no types");
        const std::string s = finish_gfa_string(f->r, k, finish_meta(f, seq_ids, seq_lengths, filenames, headers, nullptr), false);
        auto h = std::make_unique<ac_graph>();
        std::vector<SeqMeta> meta;
        load_gfa(s.data(), s.size(), &h->g, &meta);
        for (auto& m : meta) { h->seq_ids.push_back(m.id); h->seq_lens.push_back(m.length); h->filenames.push_back(m.filename); h->headers.push_back(m.contig_header); }
        *out = h.release();
    });
}

// ---- `autocycler resolve`, the edit: apply_bridges with reduce_depths and the two removals on the device (kernels_apply.inc); the checks on the
// bridge records, the numbering and the text on the host (apply_host.cpp).  The composed entries hand the edited arrays to the merge plan and the
// finished graph above; ac_resolve_graphs is resolve.rs:44-67 from a handle to the three texts ----
struct ac_applied {
    ApplyResult r;
    ac_applied_summary summary;
};
static void apply_run(const ApplyInput& in, int device, ac_applied** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    ApplyPlan plan;
    apply_prepare(in, &plan);
    auto h = std::make_unique<ac_applied>();
    if (in.n_unitigs == 0) {      // (nothing to launch: no device is asked for)
        if (in.n_links) throw DeviceError(components_bad_link_message(0, in.links[0].a, in.links[0].b, 0));
        apply_empty(&h->r);
    } else {
        DeviceCall call(device);
        apply_bridges_device(in, plan, &h->r);
    }
    apply_finish(in, plan, &h->r);
    ac_applied_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.bridges_applied = h->r.applied; sm.direct_links = h->r.direct; sm.launches_components = h->r.stats_components.launches;
    sm.launches = h->r.stats.launches - h->r.stats_components.launches; sm.read_backs = h->r.stats.read_backs; sm.removed_no_anchor = h->r.removed_no_anchor;
    sm.removed_zero_depth = h->r.removed_zero_depth; sm.links_in = h->r.links_in; sm.links_out = h->r.links.size(); sm.bases_copied = h->r.bases_copied;
    sm.seconds_device = h->r.stats.seconds_device; sm.seconds_copy = h->r.seconds_copy; sm.seconds_components = h->r.stats_components.seconds_device;
    *out = h.release();
}
static std::vector<ApplyBridgeIn> apply_bridge_records(const ac_bridge* bridges, uint32_t n) {
    std::vector<ApplyBridgeIn> v(n);
    for (uint32_t b = 0; b < n; b++)
        v[b] = ApplyBridgeIn{bridges[b].start, bridges[b].end, bridges[b].best_off, bridges[b].first_distinct, bridges[b].best_len, bridges[b].n_distinct, bridges[b].status};
    return v;
}
int ac_apply_bridges(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const double* depth,
                     const uint32_t* anchors, uint32_t n_anchors, const uint8_t* seq_bytes, const uint64_t* seq_begin, const ac_bridge* bridges, uint32_t n_bridges,
                     const int32_t* best_paths, uint64_t n_best, const int32_t* distinct_entries, const uint64_t* distinct_off, const uint32_t* multiplicity,
                     uint64_t n_distinct_paths, const uint8_t* apply, double bridge_depth, int device, ac_applied** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (n_bridges && !bridges) throw DeviceError("null pointer: n_bridges > 0 without bridges");
        const std::vector<ApplyBridgeIn> recs = apply_bridge_records(bridges, n_bridges);
        ApplyInput in;
        in.n_unitigs = n_unitigs; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.alive = alive; in.depth = depth;
        in.anchors = anchors; in.n_anchors = n_anchors; in.seq_bytes = seq_bytes; in.seq_begin = seq_begin;
        if (seq_bytes && seq_begin && unitig_len)
            for (uint32_t u = 0; u < n_unitigs; u++) in.seq_total = std::max<uint64_t>(in.seq_total, seq_begin[u] + unitig_len[u]);
        in.bridges = recs.data(); in.n_bridges = n_bridges; in.apply = apply; in.best = best_paths; in.n_best = n_best;
        in.dist_entries = distinct_entries; in.dist_off = distinct_off; in.dist_mult = multiplicity; in.n_dist_paths = n_distinct_paths;
        in.n_dist_entries = n_distinct_paths && distinct_off ? distinct_off[n_distinct_paths] : 0;
        in.bridge_depth = bridge_depth;
        apply_run(in, device, out);
    });
}
static void apply_on_graph(const ac_graph* g, const ac_resolve* r, int which, int device, ac_applied** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!g || !r) throw DeviceError("null pointer");
    if (which != AC_APPLY_UNIQUE && which != AC_APPLY_KEPT) throw DeviceError("apply bridges: which must be AC_APPLY_UNIQUE or AC_APPLY_KEPT");
    if (!g->host_arrays) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
    const FinalGraph& f = g->g;
    const std::vector<ApplyBridgeIn> recs = apply_bridge_records(r->records.data(), (uint32_t)r->records.size());
    std::vector<uint8_t> apply(recs.size());
    for (size_t b = 0; b < recs.size(); b++) apply[b] = which == AC_APPLY_UNIQUE ? !r->records[b].conflicting : !r->records[b].culled;
    const bool seqs = f.seq_block.p && f.seq_begin;
    ApplyInput in;
    in.n_unitigs = f.n_unitigs; in.links = f.links; in.n_links = f.n_links; in.unitig_len = f.seq_len; in.depth = f.depth;
    in.anchors = r->r.anchors.data(); in.n_anchors = (uint32_t)r->r.anchors.size();
    in.seq_bytes = seqs ? (const uint8_t*)f.seq_block.p : nullptr; in.seq_begin = seqs ? f.seq_begin : nullptr; in.seq_total = seqs ? f.seq_block.bytes : 0;
    in.bridges = recs.data(); in.n_bridges = (uint32_t)recs.size(); in.apply = apply.data(); in.best = r->r.best_pool.data(); in.n_best = r->r.best_pool.size();
    in.dist_entries = r->r.distinct.entries.data(); in.dist_off = r->r.distinct.off.data(); in.dist_mult = r->r.multiplicity.data();
    in.n_dist_paths = r->r.distinct.size(); in.n_dist_entries = r->r.distinct.entries.size();
    in.bridge_depth = (double)g->seq_ids.size();      // sequences.len() as f64 (resolve.rs:47)
    apply_run(in, device, out);
}
int ac_graph_resolve_apply(const ac_graph* g, const ac_resolve* r, int which, int device, ac_applied** out) {
    return guarded([&] { apply_on_graph(g, r, which, device, out); });
}
int ac_applied_unitigs(const ac_applied* a, uint32_t* n_total, const uint32_t** len, const uint8_t** alive, const double** depth, const uint8_t** type) {
    return guarded([&] {
        if (!a || !n_total) throw DeviceError("null pointer");
        *n_total = a->r.n_total;
        if (len) *len = a->r.len.data();
        if (alive) *alive = a->r.alive.data();
        if (depth) *depth = a->r.depth.data();
        if (type) *type = a->r.type.data();
    });
}
int ac_applied_bridge_of(const ac_applied* a, const uint32_t** bridge, uint32_t* n) {
    return guarded([&] {
        if (!a || !bridge || !n) throw DeviceError("null pointer");
        *bridge = a->r.bridge_of.data(); *n = (uint32_t)a->r.bridge_of.size();
    });
}
int ac_applied_links(const ac_applied* a, const ac_link** links, uint64_t* n) {
    return guarded([&] {
        if (!a || !links || !n) throw DeviceError("null pointer");
        *links = (const ac_link*)a->r.links.data(); *n = a->r.links.size();
    });
}
int ac_applied_bridge_sequences(const ac_applied* a, const uint8_t** bytes, const uint64_t** off, uint64_t* n_bytes) {
    return guarded([&] {
        if (!a || !bytes || !off) throw DeviceError("null pointer");
        *bytes = a->r.bridge_seq.data(); *off = a->r.bridge_seq_off.data();
        if (n_bytes) *n_bytes = a->r.bridge_seq.size();
    });
}
size_t ac_applied_summary_get_sized(const ac_applied* a, ac_applied_summary* out, size_t out_size) {
    if (a && out) memcpy(out, &a->summary, std::min(out_size, sizeof(ac_applied_summary)));
    return sizeof(ac_applied_summary);
}
void ac_applied_free(ac_applied* a) { delete a; }
// merge_linear_paths(graph, &vec![]) after clear_positions: no path ends, no positions
static void applied_merge_plan(const ac_applied* a, int with_sequences, int device, ac_merge** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!a) throw DeviceError("null pointer");
    const ApplyResult& r = a->r;
    const bool seqs = with_sequences && !r.seq_all.empty();
    merge_run(r.n_total, (const ac_link*)r.links.data(), r.links.size(), r.len.data(), r.alive.data(), nullptr, 0, r.depth.data(), nullptr, nullptr, r.type.data(),
              seqs ? r.seq_all.data() : nullptr, seqs ? r.seq_begin_all.data() : nullptr, seqs ? r.seq_all.size() : 0, nullptr, 0, device, out);
}
static void applied_finish(const ac_applied* a, const ac_merge* plan, int renumber, int device, ac_finished** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!a || !plan) throw DeviceError("null pointer");
    const ApplyResult& r = a->r;
    const bool seqs = !r.seq_all.empty();
    finish_run(plan, r.n_total, (const ac_link*)r.links.data(), r.links.size(), r.len.data(), r.alive.data(), r.depth.data(), r.type.data(),
               seqs ? r.seq_all.data() : nullptr, seqs ? r.seq_begin_all.data() : nullptr, seqs ? r.seq_all.size() : 0, nullptr, renumber, device, out);
}
int ac_applied_merge_plan(const ac_applied* a, int with_sequences, int device, ac_merge** out) {
    return guarded([&] { applied_merge_plan(a, with_sequences, device, out); });
}
int ac_applied_finish(const ac_applied* a, const ac_merge* plan, int renumber, int device, ac_finished** out) {
    return guarded([&] { applied_finish(a, plan, renumber, device, out); });
}
static char* malloc_string(const std::string& s, uint64_t* len) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) throw DeviceError("out of memory");
    memcpy(p, s.c_str(), s.size() + 1);
    if (len) *len = s.size();
    return p;
}
int ac_applied_gfa_string(const ac_applied* a, uint32_t k, int use_other_colour, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!a) throw DeviceError("null pointer");
        *out = malloc_string(apply_gfa_string(a->r, k, use_other_colour != 0), len);
    });
}
int ac_resolve_graphs(const ac_graph* g, int device, char** bridged, char** merged, char** final_text, uint32_t* cull_count) {
    return guarded([&] {
        if (!bridged || !merged || !final_text || !cull_count) throw DeviceError("null pointer: out");
        *bridged = *merged = *final_text = nullptr; *cull_count = 0;
        if (!g) throw DeviceError("null pointer");
        struct Free {
            void operator()(ac_resolve* p) const { ac_resolve_free(p); }
            void operator()(ac_applied* p) const { ac_applied_free(p); }
            void operator()(ac_merge* p) const { ac_merge_free(p); }
            void operator()(ac_finished* p) const { ac_finished_free(p); }
        };
        ac_resolve* rp = nullptr;
        if (ac_resolve_bridges(g, device, &rp)) throw DeviceError(last_error());
        std::unique_ptr<ac_resolve, Free> r(rp);
        const uint32_t k = g->g.k;
        // one pass: apply, 3_bridged's text (the first pass), merge_after_bridging = merge_linear_paths + renumber_unitigs
        auto pass = [&](int which, std::string* bridged_text, std::unique_ptr<ac_finished, Free>* fin) {
            ac_applied* ap = nullptr;
            apply_on_graph(g, r.get(), which, device, &ap);
            std::unique_ptr<ac_applied, Free> a(ap);
            if (bridged_text) *bridged_text = apply_gfa_string(a->r, k, false);
            ac_merge* mp = nullptr;
            applied_merge_plan(a.get(), 1, device, &mp);
            std::unique_ptr<ac_merge, Free> m(mp);
            ac_finished* fp = nullptr;
            applied_finish(a.get(), m.get(), 1, device, &fp);
            fin->reset(fp);
        };
        std::string text_bridged;
        std::unique_ptr<ac_finished, Free> fin;
        pass(AC_APPLY_UNIQUE, &text_bridged, &fin);
        const std::string text_merged = finish_gfa_string(fin->r, k, std::vector<FinishSeqMeta>(), false);
        uint32_t culled = 0;
        for (const ac_bridge& b : r->records) culled += b.culled ? 1 : 0;
        if (culled) pass(AC_APPLY_KEPT, nullptr, &fin);      // from the unedited handle (resolve.rs:58-62)
        const std::string text_final = finish_gfa_string(fin->r, k, std::vector<FinishSeqMeta>(), true);
        char* b = malloc_string(text_bridged, nullptr);
        char* m = nullptr; char* f = nullptr;
        try { m = malloc_string(text_merged, nullptr); f = malloc_string(text_final, nullptr); }
        catch (...) { free(b); free(m); throw; }
        *bridged = b; *merged = m; *final_text = f; *cull_count = culled;
    });
}

// ---- `autocycler clean`, the edit: remove_unitigs_by_number, duplicate_unitig_by_number and remove_low_depth_unitigs on the device
// (kernels_clean.inc); the number lists, the sequential duplication over the gathered entries and the text on the host (clean_host.cpp).  The
// composed entries hand the edited arrays to the merge plan and the finished graph above; ac_clean_gfa is clean.rs:27-43 from text to text ----
struct ac_cleaned {
    CleanResult r;
    ac_cleaned_summary summary;
};
static_assert((int)AC_CLEAN_KEPT == (int)CLEAN_KEPT && (int)AC_CLEAN_REMOVED == (int)CLEAN_REMOVED && (int)AC_CLEAN_DUPLICATED == (int)CLEAN_DUPLICATED &&
              (int)AC_CLEAN_LOW_DEPTH == (int)CLEAN_LOW_DEPTH && (int)AC_CLEAN_KEPT_DEAD_END == (int)CLEAN_KEPT_DEAD_END && (int)AC_CLEAN_ABSENT == (int)CLEAN_ABSENT,
              "the AC_CLEAN_* values are clean_host.hpp's");
static void clean_run(const CleanInput& in, int device, ac_cleaned** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    clean_prepare(in);
    auto h = std::make_unique<ac_cleaned>();
    if (in.n_unitigs == 0) {      // (nothing to launch: no device is asked for)
        if (in.n_links) throw DeviceError(components_bad_link_message(0, in.links[0].a, in.links[0].b, 0));
        clean_empty(&h->r);
    } else {
        DeviceCall call(device);
        clean_device(in, &h->r);
    }
    clean_finish(in, &h->r);
    const CleanResult& r = h->r;
    ac_cleaned_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.unitigs_in = r.n_unitigs; sm.unitigs_out = r.n_out; sm.rounds = r.rounds; sm.rounds_per_batch = CLEAN_ROUNDS_PER_BATCH;
    sm.launches = r.stats.launches; sm.read_backs = r.stats.read_backs; sm.kept = r.count[CLEAN_KEPT]; sm.removed = r.count[CLEAN_REMOVED];
    sm.duplicated = r.count[CLEAN_DUPLICATED]; sm.low_depth = r.count[CLEAN_LOW_DEPTH]; sm.kept_dead_end = r.count[CLEAN_KEPT_DEAD_END]; sm.absent = r.count[CLEAN_ABSENT];
    sm.links_in = r.links_in; sm.links_out = r.links.size(); sm.seconds_device = r.stats.seconds_device;
    *out = h.release();
}
int ac_clean_graph(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const double* depth, const uint8_t* type, const uint8_t* alive,
                   const uint8_t* seq_bytes, const uint64_t* seq_begin, const uint32_t* remove, uint32_t n_remove, const uint32_t* duplicate, uint32_t n_duplicate,
                   int has_min_depth, double min_depth, int device, ac_cleaned** out) {
    return guarded([&] {
        CleanInput in;
        in.n_unitigs = n_unitigs; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.depth = depth; in.type = type; in.alive = alive;
        in.seq_bytes = seq_bytes; in.seq_begin = seq_begin;
        if (seq_bytes && seq_begin && unitig_len)
            for (uint32_t u = 0; u < n_unitigs; u++) in.seq_total = std::max<uint64_t>(in.seq_total, seq_begin[u] + unitig_len[u]);
        in.remove = remove; in.n_remove = n_remove; in.duplicate = duplicate; in.n_duplicate = n_duplicate; in.has_min_depth = has_min_depth != 0; in.min_depth = min_depth;
        clean_run(in, device, out);
    });
}
static void clean_on_graph(const ac_graph* g, const uint8_t* type, const uint32_t* remove, uint32_t n_remove, const uint32_t* duplicate, uint32_t n_duplicate, int has_min_depth,
                           double min_depth, const std::string& name, int device, ac_cleaned** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!g) throw DeviceError("null pointer");
    if (!g->host_arrays) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
    const FinalGraph& f = g->g;
    const bool seqs = f.seq_block.p && f.seq_begin;
    CleanInput in;
    in.n_unitigs = f.n_unitigs; in.links = f.links; in.n_links = f.n_links; in.unitig_len = f.seq_len; in.depth = f.depth; in.type = type;
    in.seq_bytes = seqs ? (const uint8_t*)f.seq_block.p : nullptr; in.seq_begin = seqs ? f.seq_begin : nullptr; in.seq_total = seqs ? f.seq_block.bytes : 0;
    in.remove = remove; in.n_remove = n_remove; in.duplicate = duplicate; in.n_duplicate = n_duplicate; in.has_min_depth = has_min_depth != 0; in.min_depth = min_depth;
    in.name = name;
    clean_run(in, device, out);
}
int ac_graph_clean(const ac_graph* g, const uint8_t* type, const uint32_t* remove, uint32_t n_remove, const uint32_t* duplicate, uint32_t n_duplicate, int has_min_depth,
                   double min_depth, int device, ac_cleaned** out) {
    return guarded([&] { clean_on_graph(g, type, remove, n_remove, duplicate, n_duplicate, has_min_depth, min_depth, "the graph", device, out); });
}
int ac_cleaned_unitigs(const ac_cleaned* c, uint32_t* n_out, const uint32_t** len, const uint8_t** alive, const double** depth, const uint8_t** type,
                       const uint64_t** seq_begin, const uint32_t** copy_of, const uint8_t** reason) {
    return guarded([&] {
        if (!c || !n_out) throw DeviceError("null pointer");
        *n_out = c->r.n_out;
        if (len) *len = c->r.len.data();
        if (alive) *alive = c->r.alive.data();
        if (depth) *depth = c->r.depth.data();
        if (type) *type = c->r.type.data();
        if (seq_begin) *seq_begin = c->r.seq_begin.empty() ? nullptr : c->r.seq_begin.data();
        if (copy_of) *copy_of = c->r.copy_of.data();
        if (reason) *reason = c->r.reason.data();
    });
}
int ac_cleaned_links(const ac_cleaned* c, const ac_link** links, uint64_t* n) {
    return guarded([&] {
        if (!c || !links || !n) throw DeviceError("null pointer");
        *links = (const ac_link*)c->r.links.data(); *n = c->r.links.size();
    });
}
size_t ac_cleaned_summary_get_sized(const ac_cleaned* c, ac_cleaned_summary* out, size_t out_size) {
    if (c && out) memcpy(out, &c->summary, std::min(out_size, sizeof(ac_cleaned_summary)));
    return sizeof(ac_cleaned_summary);
}
void ac_cleaned_free(ac_cleaned* c) { delete c; }
// merge_linear_paths(graph, &vec![]) (clean.rs:114): no path ends, no positions.  A duplicated loop left a link multiset: the plan's own
// check refuses it.
static void cleaned_merge_plan(const ac_cleaned* c, int with_sequences, int device, ac_merge** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!c) throw DeviceError("null pointer");
    const CleanResult& r = c->r;
    const bool seqs = with_sequences && !r.seq_all.empty();
    merge_run(r.n_out, (const ac_link*)r.links.data(), r.links.size(), r.len.data(), r.alive.data(), nullptr, 0, r.depth.data(), nullptr, nullptr, r.type.data(),
              seqs ? r.seq_all.data() : nullptr, seqs ? r.seq_begin.data() : nullptr, seqs ? r.seq_all.size() : 0, nullptr, 0, device, out);
}
static void cleaned_finish(const ac_cleaned* c, const ac_merge* plan, int renumber, int device, ac_finished** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!c || !plan) throw DeviceError("null pointer");
    const CleanResult& r = c->r;
    const bool seqs = !r.seq_all.empty();
    finish_run(plan, r.n_out, (const ac_link*)r.links.data(), r.links.size(), r.len.data(), r.alive.data(), r.depth.data(), r.type.data(),
               seqs ? r.seq_all.data() : nullptr, seqs ? r.seq_begin.data() : nullptr, seqs ? r.seq_all.size() : 0, nullptr, renumber, device, out);
}
int ac_cleaned_merge_plan(const ac_cleaned* c, int with_sequences, int device, ac_merge** out) {
    return guarded([&] { cleaned_merge_plan(c, with_sequences, device, out); });
}
int ac_cleaned_finish(const ac_cleaned* c, const ac_merge* plan, int renumber, int device, ac_finished** out) {
    return guarded([&] { cleaned_finish(c, plan, renumber, device, out); });
}
int ac_cleaned_gfa_string(const ac_cleaned* c, uint32_t k, int use_other_colour, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!c) throw DeviceError("null pointer");
        *out = malloc_string(clean_gfa_string(c->r, k, use_other_colour != 0), len);
    });
}
int ac_parse_tig_numbers(const char* text, uint32_t** numbers, uint32_t* n) {
    return guarded([&] {
        if (!numbers || !n) throw DeviceError("null pointer: out");
        *numbers = nullptr; *n = 0;
        const std::vector<uint32_t> v = clean_parse_tig_numbers(text);
        uint32_t* p = (uint32_t*)malloc((v.size() + 1) * sizeof(uint32_t));
        if (!p) throw DeviceError("out of memory");
        if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(uint32_t));
        *numbers = p; *n = (uint32_t)v.size();
    });
}
int ac_gfa_segment_types(const char* gfa_text, uint64_t len, uint8_t** types, uint32_t* n) {
    return guarded([&] {
        if (!types || !n) throw DeviceError("null pointer: out");
        *types = nullptr; *n = 0;
        if (!gfa_text && len) throw DeviceError("null pointer: gfa_text");
        const std::vector<uint8_t> v = clean_gfa_types(gfa_text, len);
        uint8_t* p = (uint8_t*)malloc(v.size() + 1);
        if (!p) throw DeviceError("out of memory");
        if (!v.empty()) memcpy(p, v.data(), v.size());
        *types = p; *n = (uint32_t)v.size();
    });
}
static std::string clean_gfa_text(const char* gfa_text, uint64_t len, const std::string& name, const char* remove, const char* duplicate, int has_min_depth,
                                  double min_depth, int device) {
    {
        if (!gfa_text && len) throw DeviceError("null pointer: gfa_text");
        struct Free {
            void operator()(ac_cleaned* p) const { ac_cleaned_free(p); }
            void operator()(ac_merge* p) const { ac_merge_free(p); }
            void operator()(ac_finished* p) const { ac_finished_free(p); }
        };
        // clean.rs:27-32: both lists are parsed before the graph is loaded, and checked against it before anything is edited
        const std::vector<uint32_t> rm = clean_parse_tig_numbers(remove), dup = clean_parse_tig_numbers(duplicate);
        ac_graph g;
        std::vector<SeqMeta> meta;
        load_gfa(gfa_text, len, &g.g, &meta);
        const std::vector<uint8_t> types = clean_gfa_types(gfa_text, len);
        if (types.size() != g.g.n_unitigs) throw DeviceError("clean: the S lines of the text and the loaded graph disagree (internal error)");
        ac_cleaned* cp = nullptr;
        clean_on_graph(&g, types.data(), rm.data(), (uint32_t)rm.size(), dup.data(), (uint32_t)dup.size(), has_min_depth, min_depth, name, device, &cp);
        std::unique_ptr<ac_cleaned, Free> c(cp);
        ac_merge* mp = nullptr;
        cleaned_merge_plan(c.get(), 1, device, &mp);
        std::unique_ptr<ac_merge, Free> m(mp);
        ac_finished* fp = nullptr;
        cleaned_finish(c.get(), m.get(), 1, device, &fp);
        std::unique_ptr<ac_finished, Free> f(fp);
        return finish_gfa_string(f->r, g.g.k, std::vector<FinishSeqMeta>(), true);      // save_gfa(out, &vec![], true)
    }
}
int ac_clean_gfa(const char* gfa_text, uint64_t len, const char* remove, const char* duplicate, int has_min_depth, double min_depth, int device, char** out_text,
                 uint64_t* out_len) {
    return guarded([&] {
        if (!out_text) throw DeviceError("null pointer: out");
        *out_text = nullptr;
        *out_text = malloc_string(clean_gfa_text(gfa_text, len, "the graph", remove, duplicate, has_min_depth, min_depth, device), out_len);
    });
}
// The whole command (clean.rs:23-45): check_if_file_exists, then the above from in_gfa to out_gfa.
int ac_clean(const char* in_gfa, const char* out_gfa, const char* remove, const char* duplicate, int has_min_depth, double min_depth, int device) {
    return guarded([&] {
        if (!in_gfa || !out_gfa) throw DeviceError("null pointer: in_gfa and out_gfa are required");
        std::string text;
        {
            std::ifstream f(in_gfa, std::ios::binary);
            if (!f) throw DeviceError(std::string("file does not exist: ") + in_gfa);
            text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        }
        const std::string out = clean_gfa_text(text.data(), text.size(), in_gfa, remove, duplicate, has_min_depth, min_depth, device);
        std::ofstream o(out_gfa, std::ios::binary);
        o.write(out.data(), (std::streamsize)out.size());
        o.close();
        if (!o) throw DeviceError(std::string("failed to write ") + out_gfa);
    });
}

// ---- `autocycler trim`, the edit: choose_trim_type's slices, their length check, exclude_outliers_in_length and clean_up_graph's subset on the
// device (kernels_trim_apply.inc, then the stages of kernels_subset.inc on the same entries); the choice, the statistics and the yaml on the host
// (trim_apply_host.cpp).  The object owns a one-cluster ac_subsets: merge plan, merged paths and finish are the subsets' own ----
struct ac_trimmed {
    ac_subsets sub;      // path / path_off: the slices below
    TrimApplyPlan tp;
    ac_trimmed_summary summary;
};
static_assert(sizeof(ac_trimmed_record) == sizeof(TrimApplyRecord) && offsetof(ac_trimmed_record, length) == offsetof(TrimApplyRecord, length) &&
              offsetof(ac_trimmed_record, excluded) == offsetof(TrimApplyRecord, excluded), "ac_trimmed_record and TrimApplyRecord are one layout");
static_assert(AC_TRIM_CHOOSE_AUTO == TRIM_CHOOSE_AUTO && AC_TRIM_CHOOSE_NONE == TRIM_CHOOSE_NONE && AC_TRIM_CHOOSE_START_END == TRIM_CHOOSE_START_END &&
              AC_TRIM_CHOOSE_HAIRPIN == TRIM_CHOOSE_HAIRPIN, "the AC_TRIM_CHOOSE_* values are trim_apply_host.hpp's");
static void trimmed_run(uint32_t n, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* type, const int32_t* path,
                        const uint64_t* path_off, const uint32_t* seq_length, uint32_t n_seqs, const ac_trim_result* results, uint32_t chosen, double mad,
                        const ac_graph* graph, const ac_trim_summary* align, int device, std::unique_ptr<ac_trimmed>* out) {
    if (!path_off) throw DeviceError("null pointer: path_off");
    if (!seq_length) throw DeviceError("null pointer: seq_length");
    if (n && !unitig_len) throw DeviceError("null pointer: unitig_len");
    if (n_links && !links) throw DeviceError("null pointer: n_links > 0 without links");
    if (mad < 0.0) throw DeviceError("--mad cannot be less than 0");
    auto h = std::make_unique<ac_trimmed>();
    TrimApplyPlan& tp = h->tp;
    std::vector<TrimResult> res(results ? n_seqs : 0);
    for (size_t s = 0; s < res.size(); s++) {
        const ac_trim_result& r = results[s];
        res[s].se = TrimSlice{r.start_end.status, r.start_end.begin, r.start_end.end, r.start_end.trimmed_length};
        res[s].hp = TrimSlice{r.hairpin.status, r.hairpin.begin, r.hairpin.end, r.hairpin.trimmed_length};
    }
    trim_apply_choose(results ? res.data() : nullptr, n_seqs, path, path_off, seq_length, chosen, &tp);
    ac_subsets& sub = h->sub;
    sub.links = links; sub.n_links = n_links; sub.unitig_len = unitig_len; sub.path = tp.sliced.data(); sub.path_off = tp.sliced_off.data(); sub.graph = graph;
    sub.type = type;
    sub.r.n_unitigs = n;
    const uint64_t ne = tp.sliced_off[n_seqs];
    if (n == 0 || ne == 0) {      // (no entry anywhere: every sum is 0; no device is asked for)
        if (ne) throw DeviceError(subset_bad_entry_message(0, tp.seqs[0].begin, tp.sliced[0], n));
        if (n == 0 && n_links) throw DeviceError(components_bad_link_message(0, links[0].a, links[0].b, 0));
        for (uint32_t s = 0; s < n_seqs; s++)
            if (tp.seqs[s].length != 0) throw DeviceError(trim_apply_mismatch_message(s, 0, tp.seqs[s].length));
        trim_apply_exclude(&tp, mad);
        subset_prepare(n_seqs, tp.sliced.data(), tp.sliced_off.data(), tp.label.data(), 1, &sub.plan, &sub.r);
        subset_empty_products(&sub.r);
    } else {
        TrimApplyInput in;
        in.n_unitigs = n; in.links = (const Link*)links; in.n_links = n_links; in.unitig_len = unitig_len; in.alive = alive; in.path = path; in.path_off = path_off;
        in.mad = mad;
        DeviceCall call(device);
        trim_apply_device(in, &tp, &sub.plan, &sub.r);
    }
    subset_finish(&sub.r, sub.plan);
    ac_subsets_summary& ss = sub.summary;
    memset(&ss, 0, sizeof ss);
    ss.size = (uint32_t)sizeof ss; ss.clusters = 1; ss.sequences_kept = (uint32_t)sub.plan.kept_seq.size(); ss.n_unitigs = n;
    ss.entries_kept = sub.r.kept_entries; ss.unitigs = sub.r.unitigs.size(); ss.links = sub.r.links.size();
    ss.launches = sub.r.stats.launches; ss.read_backs = sub.r.stats.read_backs; ss.seconds_device = sub.r.stats.seconds_device;
    ac_trimmed_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.chosen = tp.chosen; sm.c_se = tp.c_se; sm.c_hp = tp.c_hp; sm.sequences = n_seqs; sm.trimmed = tp.n_trimmed;
    sm.excluded = tp.n_excluded; sm.rejected = tp.rejected; sm.unitigs_in = n; sm.unitigs_alive = (uint32_t)sub.r.unitigs.size();
    sm.launches = sub.r.stats.launches; sm.read_backs = sub.r.stats.read_backs; sm.median = tp.median; sm.mad = tp.mad; sm.min_length = tp.min_length;
    sm.max_length = tp.max_length; sm.entries_kept = sub.r.kept_entries; sm.links = sub.r.links.size(); sm.seconds_device = sub.r.stats.seconds_device;
    if (align) { sm.align_launches = align->launches; sm.align_cells = align->cells; sm.align_seconds_device = align->seconds_device; }
    *out = std::move(h);
}
static const ac_graph* trimmed_check_graph(const ac_graph* g) {
    if (!g) throw DeviceError("null pointer");
    if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
    const uint32_t n_seqs = (uint32_t)g->seq_ids.size();
    if (n_seqs == 0 || g->g.path_off.size() != (size_t)n_seqs + 1 || !g->g.seq_len) throw DeviceError("trim: the graph holds no paths");
    return g;
}
static void trimmed_on_graph(const ac_graph* g, const uint8_t* type, const ac_trim_result* results, uint32_t chosen, double mad, const ac_trim_summary* align, int device,
                             std::unique_ptr<ac_trimmed>* out) {
    const FinalGraph& f = g->g;
    trimmed_run(f.n_unitigs, (const ac_link*)f.links, f.n_links, f.seq_len, nullptr, type, f.path, f.path_off.data(), g->seq_lens.data(), (uint32_t)g->seq_ids.size(),
                results, chosen, mad, g, align, device, out);
}
// trim_start_end_overlap, trim_harpin_overlap, then the edit with choose_trim_type's own choice
static void trimmed_whole(const ac_graph* g, const uint8_t* type, double min_identity, uint32_t max_unitigs, double mad, int device, std::unique_ptr<ac_trimmed>* out) {
    trim_apply_check_settings(min_identity, mad);
    const uint32_t n_seqs = (uint32_t)g->seq_ids.size();
    std::vector<ac_trim_result> results(n_seqs);
    ac_trim_summary align;
    memset(&align, 0, sizeof align);
    align.size = sizeof align;
    trim_slices(g->g.path, g->g.path_off.data(), n_seqs, g->g.seq_len, g->g.n_unitigs, min_identity, max_unitigs, device, results.data(), &align);
    trimmed_on_graph(g, type, results.data(), AC_TRIM_CHOOSE_AUTO, mad, &align, device, out);
}
int ac_trim_apply(uint32_t n_unitigs, const ac_link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* type,
                  const int32_t* path_entries, const uint64_t* path_off, const uint32_t* seq_length, uint32_t n_seqs, const ac_trim_result* results, uint32_t chosen,
                  double mad, int device, ac_trimmed** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        std::unique_ptr<ac_trimmed> h;
        trimmed_run(n_unitigs, links, n_links, unitig_len, alive, type, path_entries, path_off, seq_length, n_seqs, results, chosen, mad, nullptr, nullptr, device, &h);
        *out = h.release();
    });
}
int ac_graph_trim_apply(const ac_graph* g, const ac_trim_result* results, uint32_t chosen, double mad, int device, ac_trimmed** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        std::unique_ptr<ac_trimmed> h;
        trimmed_on_graph(trimmed_check_graph(g), nullptr, results, chosen, mad, nullptr, device, &h);
        *out = h.release();
    });
}
int ac_graph_trim(const ac_graph* g, double min_identity, uint32_t max_unitigs, double mad, int device, ac_trimmed** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        std::unique_ptr<ac_trimmed> h;
        trimmed_whole(trimmed_check_graph(g), nullptr, min_identity, max_unitigs, mad, device, &h);
        *out = h.release();
    });
}
int ac_trimmed_records(const ac_trimmed* t, const ac_trimmed_record** records, uint32_t* n_seqs) {
    return guarded([&] {
        if (!t || !records || !n_seqs) throw DeviceError("null pointer");
        *records = (const ac_trimmed_record*)t->tp.seqs.data(); *n_seqs = (uint32_t)t->tp.seqs.size();
    });
}
size_t ac_trimmed_summary_get_sized(const ac_trimmed* t, ac_trimmed_summary* out, size_t out_size) {
    if (t && out) memcpy(out, &t->summary, std::min(out_size, sizeof(ac_trimmed_summary)));
    return sizeof(ac_trimmed_summary);
}
void ac_trimmed_free(ac_trimmed* t) { delete t; }
const ac_subsets* ac_trimmed_subsets(const ac_trimmed* t) { return t ? &t->sub : nullptr; }
static void trimmed_finish(const ac_trimmed* t, const uint8_t* seq_bytes, const uint64_t* seq_begin, int device, ac_finished** out) {
    struct Free {
        void operator()(ac_merge* p) const { ac_merge_free(p); }
        void operator()(ac_merged_paths* p) const { ac_merged_paths_free(p); }
    };
    ac_merge* mp = nullptr;
    if (ac_subsets_merge_plan(&t->sub, 1, seq_bytes, seq_begin, 1, device, &mp)) throw DeviceError(last_error());
    std::unique_ptr<ac_merge, Free> m(mp);
    ac_merged_paths* pp = nullptr;
    if (ac_subsets_merged_paths(&t->sub, 1, m.get(), device, &pp)) throw DeviceError(last_error());
    std::unique_ptr<ac_merged_paths, Free> p(pp);
    if (ac_subsets_finish(&t->sub, 1, m.get(), p.get(), seq_bytes, seq_begin, 1, device, out)) throw DeviceError(last_error());
}
int ac_trimmed_finish(const ac_trimmed* t, const uint8_t* seq_bytes, const uint64_t* seq_begin, int device, ac_finished** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!t) throw DeviceError("null pointer");
        trimmed_finish(t, seq_bytes, seq_begin, device, out);
    });
}
int ac_trimmed_yaml_string(const ac_trimmed* t, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!t) throw DeviceError("null pointer");
        *out = malloc_string(trim_apply_yaml(t->tp), len);
    });
}
// trim.rs:43-51 from text to texts (capi_command.cpp's ac_trim_dir is the file form)
int ac_trim_gfa(const char* gfa_text, uint64_t len, double min_identity, uint32_t max_unitigs, double mad, int device, char** gfa, uint64_t* gfa_len, char** yaml,
                ac_trimmed_summary* summary) {
    return guarded([&] {
        if (!gfa || !yaml) throw DeviceError("null pointer: out");
        *gfa = nullptr; *yaml = nullptr;
        if (!gfa_text && len) throw DeviceError("null pointer: gfa_text");
        trim_apply_check_settings(min_identity, mad);
        auto g = std::make_unique<ac_graph>();
        std::vector<SeqMeta> meta;
        std::vector<uint32_t> tags;
        load_gfa_any_numbers(gfa_text, len, &g->g, &meta, nullptr, &tags);
        for (auto& m : meta) { g->seq_ids.push_back(m.id); g->seq_lens.push_back(m.length); g->filenames.push_back(m.filename); g->headers.push_back(m.contig_header); }
        const std::vector<uint8_t> types = clean_gfa_types(gfa_text, len);
        if (types.size() != g->g.n_unitigs) throw DeviceError("trim: the S lines of the text and the loaded graph disagree (internal error)");
        std::unique_ptr<ac_trimmed> t;
        trimmed_whole(trimmed_check_graph(g.get()), types.data(), min_identity, max_unitigs, mad, device, &t);
        ac_finished* fp = nullptr;
        trimmed_finish(t.get(), nullptr, nullptr, device, &fp);
        std::unique_ptr<ac_finished, void (*)(ac_finished*)> f(fp, ac_finished_free);
        std::vector<FinishSeqMeta> kept;      // save_gfa's P lines: the kept sequences in input order, with their new lengths
        for (uint32_t s : f->r.path_seq) kept.push_back(FinishSeqMeta{meta[s].id, (uint32_t)t->tp.seqs[s].length, meta[s].filename, meta[s].contig_header, tags[s]});
        char* text = malloc_string(finish_gfa_string(f->r, g->g.k, kept, false), gfa_len);
        try { *yaml = malloc_string(trim_apply_yaml(t->tp), nullptr); }
        catch (...) { free(text); throw; }
        *gfa = text;
        if (summary) memcpy(summary, &t->summary, std::min<size_t>(summary->size, sizeof(ac_trimmed_summary)));
    });
}

// ---- `autocycler cluster`: the UPGMA tree.  The merge loop on the device (kernels_cluster.inc), the tree and what the reference derives
// from it on the host (cluster_host.cpp); the QC verdicts, scores and refinement further down.  Writing the clusters stays with the caller ----
struct ac_cluster_tree {
    ClusterTree t;
    std::vector<ac_cluster_node> nodes;
    std::vector<ac_cluster_merge> merges;
    ac_cluster_summary summary;
    void publish(uint32_t n_seqs, const ClusterDeviceStats& st) {
        nodes.resize(t.nodes.size());
        for (size_t i = 0; i < nodes.size(); i++) {
            memset(&nodes[i], 0, sizeof nodes[i]);
            nodes[i].id = t.nodes[i].id; nodes[i].left = t.nodes[i].left; nodes[i].right = t.nodes[i].right; nodes[i].distance = t.nodes[i].distance;
        }
        merges.resize(t.merges.size());
        for (size_t i = 0; i < merges.size(); i++) {
            memset(&merges[i], 0, sizeof merges[i]);
            merges[i].a = t.merges[i].a; merges[i].b = t.merges[i].b; merges[i].distance = t.merges[i].distance;
        }
        memset(&summary, 0, sizeof summary);
        summary.n_seqs = n_seqs; summary.launches = st.launches; summary.rescans = st.rescans; summary.compares = st.compares; summary.seconds = st.seconds;
    }
};
static void cluster_check_count(uint32_t n) {
    if (n > cluster_max_seqs())
        throw DeviceError("cluster: " + std::to_string(n) + " sequences are above the " + std::to_string(cluster_max_seqs()) + " this library supports (ac_cluster_max_seqs)");
}
int ac_cluster_tree_from_distances(const double* asym, const uint16_t* ids, uint32_t n, int normalise, int device, ac_cluster_tree** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer");
        *out = nullptr;
        cluster_check_ids(ids, n);
        cluster_check_count(n);
        if (!asym) throw DeviceError("null pointer");
        auto h = std::make_unique<ac_cluster_tree>();
        std::vector<ClusterRowMerge> merges;
        ClusterDeviceStats st;
        {
            DeviceCall call(device);
            cluster_merges_device(asym, n, &merges, &st);
        }
        cluster_tree_from_merges(ids, n, merges, normalise != 0, &h->t);
        h->publish(n, st);
        *out = h.release();
    });
}
int ac_cluster_tree_build(const ac_graph* g, int normalise, int device, double* asym_out, ac_cluster_tree** out) {
    return guarded([&] {
        if (!g || !out) throw DeviceError("null pointer");
        *out = nullptr;
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        const uint32_t n = (uint32_t)g->seq_ids.size();
        if (n == 0 || g->g.path_off.size() != (size_t)n + 1 || !g->g.seq_len) throw DeviceError("cluster: the graph holds no paths");
        cluster_check_ids(g->seq_ids.data(), n);
        cluster_check_count(n);
        auto h = std::make_unique<ac_cluster_tree>();
        std::vector<ClusterRowMerge> merges;
        ClusterDeviceStats st;
        {
            DeviceCall call(device);
            cluster_merges_graph_device(g->g, n, asym_out, &merges, &st);
        }
        cluster_tree_from_merges(g->seq_ids.data(), n, merges, normalise != 0, &h->t);
        h->publish(n, st);
        *out = h.release();
    });
}
int ac_cluster_tree_from_nodes(const ac_cluster_node* nodes, uint32_t n_nodes, int32_t root, ac_cluster_tree** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer");
        *out = nullptr;
        if (!nodes && n_nodes) throw DeviceError("null pointer");
        std::vector<ClusterNode> in(n_nodes);
        for (uint32_t i = 0; i < n_nodes; i++) in[i] = ClusterNode{nodes[i].id, nodes[i].left, nodes[i].right, nodes[i].distance};
        auto h = std::make_unique<ac_cluster_tree>();
        cluster_tree_from_nodes(in.data(), n_nodes, root, &h->t);
        h->publish((uint32_t)h->t.tips.size(), ClusterDeviceStats());
        *out = h.release();
    });
}
int ac_cluster_nodes(const ac_cluster_tree* t, const ac_cluster_node** nodes, uint32_t* n_nodes, int32_t* root) {
    return guarded([&] {
        if (!t || !nodes || !n_nodes) throw DeviceError("null pointer");
        *nodes = t->nodes.data(); *n_nodes = (uint32_t)t->nodes.size();
        if (root) *root = t->t.root;
    });
}
int ac_cluster_merges(const ac_cluster_tree* t, const ac_cluster_merge** merges, uint32_t* n_merges) {
    return guarded([&] {
        if (!t || !merges || !n_merges) throw DeviceError("null pointer");
        *merges = t->merges.data(); *n_merges = (uint32_t)t->merges.size();
    });
}
size_t ac_cluster_summary_get_sized(const ac_cluster_tree* t, ac_cluster_summary* out, size_t out_size) {
    if (t && out) memcpy(out, &t->summary, std::min(out_size, sizeof(ac_cluster_summary)));
    return sizeof(ac_cluster_summary);
}
void ac_cluster_free(ac_cluster_tree* t) { delete t; }
uint32_t ac_cluster_max_seqs(void) { return cluster_max_seqs(); }
int ac_cluster_cut(const ac_cluster_tree* t, double cutoff, const uint16_t* manual, uint32_t n_manual, uint16_t* nodes_out, uint32_t* n_out) {
    return guarded([&] {
        if (!t || !nodes_out || !n_out) throw DeviceError("null pointer");
        const std::vector<uint16_t> c = cluster_cut(t->t, cutoff, manual, n_manual);
        std::copy(c.begin(), c.end(), nodes_out);      // (disjoint subtrees: never more than there are tips)
        *n_out = (uint32_t)c.size();
    });
}
int ac_cluster_assign(const ac_cluster_tree* t, const uint16_t* cluster_nodes, uint32_t n, const uint64_t* seq_len, uint16_t* cluster_of_seq,
                      double* cluster_dist, uint32_t* n_clusters) {
    return guarded([&] {
        if (!t) throw DeviceError("null pointer");
        const uint32_t c = cluster_assign(t->t, cluster_nodes, n, seq_len, cluster_of_seq, cluster_dist);
        if (n_clusters) *n_clusters = c;
    });
}
int ac_cluster_containment(const double* asym, uint32_t n, const uint16_t* cluster_of_seq, uint32_t n_clusters, double cutoff,
                           uint64_t* contain_count, uint64_t* total_count) {
    return guarded([&] { cluster_containment(asym, n, cluster_of_seq, n_clusters, cutoff, contain_count, total_count); });
}
int ac_cluster_newick(const ac_cluster_tree* t, const char* const* tip_names, int file_form, char** out) {
    return guarded([&] {
        if (!t || !out) throw DeviceError("null pointer");
        *out = nullptr;
        const std::string s = cluster_newick(t->t, tip_names, file_form != 0);
        char* p = (char*)malloc(s.size() + 1);
        if (!p) throw DeviceError("out of memory");
        memcpy(p, s.c_str(), s.size() + 1);
        *out = p;
    });
}

// ---- `autocycler cluster` after the tree: generate_clusters / qc_clusters / clustering_metrics / refine_auto_clusters.  The containment
// test and the verdict chain of every alternative of a round on the device (kernels_cluster_qc.inc), everything else on the host
// (cluster_qc_host.cpp) ----
struct ac_cluster_qc {
    ClusterQcResult r;
    std::vector<ac_cluster_qc_record> records;
    ac_clustering_metrics metrics;
    ac_cluster_qc_summary summary;
    void publish(uint32_t n_seqs, bool refined, const ClusterQcDeviceStats& st) {
        records.resize(r.records.size());
        for (size_t i = 0; i < records.size(); i++) {
            const ClusterQcRecord& x = r.records[i];
            memset(&records[i], 0, sizeof records[i]);
            records[i].node = x.node; records[i].container = x.container; records[i].size = x.size; records[i].assembly_count = x.assembly_count;
            records[i].fail = x.fail; records[i].trusted = x.trusted; records[i].median_length = x.median; records[i].cluster_dist = x.cluster_dist;
        }
        memset(&metrics, 0, sizeof metrics);
        metrics.pass_cluster_count = r.metrics.pass_cluster_count; metrics.fail_cluster_count = r.metrics.fail_cluster_count;
        metrics.pass_contig_count = r.metrics.pass_contig_count; metrics.fail_contig_count = r.metrics.fail_contig_count;
        metrics.pass_contig_fraction = r.metrics.pass_contig_fraction; metrics.fail_contig_fraction = r.metrics.fail_contig_fraction;
        metrics.cluster_balance_score = r.metrics.cluster_balance_score; metrics.cluster_tightness_score = r.metrics.cluster_tightness_score;
        metrics.overall_clustering_score = r.metrics.overall_clustering_score;
        memset(&summary, 0, sizeof summary);
        summary.n_seqs = n_seqs; summary.n_clusters = (uint32_t)records.size(); summary.rounds = refined ? (uint32_t)r.round_alternatives.size() : 0;
        summary.evaluations = st.evaluations; summary.pair_batches = st.pair_batches; summary.launches = st.launches; summary.readbacks = st.readbacks;
        summary.alternatives = st.alternatives; summary.node_pairs = st.pairs_counted; summary.bytes_read_back = st.bytes_read_back;
        summary.seconds = st.seconds; summary.start_score = r.start_score;
    }
};
// the checks both entries share, all before a device is touched; returns the indexed tree
static void cluster_qc_prologue(const ac_cluster_tree* t, const double* asym, uint32_t n, const uint64_t* seq_len, const uint32_t* assembly,
                                const uint32_t* cluster_weight, const uint8_t* trusted, double cutoff, const uint16_t* manual, uint32_t n_manual,
                                ac_cluster_qc** out, ClusterQcIndex* ix) {
    if (!out) throw DeviceError("null pointer");
    *out = nullptr;
    if (!t || (n_manual && !manual) || (!n_manual && !asym)) throw DeviceError("null pointer");
    cluster_check_count(n);
    ClusterSeqInputs in{seq_len, assembly, cluster_weight, trusted, n, 0};
    if (n && (!seq_len || !assembly || !cluster_weight || !trusted)) throw DeviceError("null pointer");
    in.n_assemblies = cluster_assembly_count_checked(assembly, n);
    cluster_qc_index(t->t, in, ix);
    if (n_manual) (void)cluster_cut(t->t, cutoff, manual, n_manual);      // check_consistency: nested manual clusters
}
int ac_cluster_generate(const ac_cluster_tree* t, const double* asym, uint32_t n, const uint64_t* seq_len, const uint32_t* assembly,
                        const uint32_t* cluster_weight, const uint8_t* trusted, double cutoff, uint32_t min_assemblies,
                        const uint16_t* manual, uint32_t n_manual, int device, ac_cluster_qc** out) {
    return guarded([&] {
        ClusterQcIndex ix;
        cluster_qc_prologue(t, asym, n, seq_len, assembly, cluster_weight, trusted, cutoff, manual, n_manual, out, &ix);
        auto h = std::make_unique<ac_cluster_qc>();
        ClusterQcDeviceStats st;
        if (n_manual) cluster_generate_host(ix, cutoff, manual, n_manual, min_assemblies, ClusterQcEvaluate(), &h->r);
        else {
            DeviceCall call(device);
            cluster_qc_device(asym, n, ix.dfs_tip.data(), cutoff, [&](const ClusterQcEvaluate& ev) { cluster_generate_host(ix, cutoff, nullptr, 0, min_assemblies, ev, &h->r); }, &st);
        }
        h->publish(n, n_manual == 0, st);
        *out = h.release();
    });
}
int ac_cluster_qc_nodes(const ac_cluster_tree* t, const double* asym, uint32_t n, const uint64_t* seq_len, const uint32_t* assembly,
                        const uint32_t* cluster_weight, const uint8_t* trusted, double cutoff, uint32_t min_assemblies,
                        const uint16_t* cluster_nodes, uint32_t n_nodes, const uint16_t* manual, uint32_t n_manual, int device, ac_cluster_qc** out) {
    return guarded([&] {
        ClusterQcIndex ix;
        cluster_qc_prologue(t, asym, n, seq_len, assembly, cluster_weight, trusted, cutoff, manual, n_manual, out, &ix);
        (void)cluster_qc_nodes_checked(ix, cluster_nodes, n_nodes);      // (before a device is selected)
        auto h = std::make_unique<ac_cluster_qc>();
        ClusterQcDeviceStats st;
        if (n_manual) cluster_qc_nodes_host(ix, cluster_nodes, n_nodes, manual, n_manual, min_assemblies, ClusterQcEvaluate(), &h->r);
        else {
            DeviceCall call(device);
            cluster_qc_device(asym, n, ix.dfs_tip.data(), cutoff,
                              [&](const ClusterQcEvaluate& ev) { cluster_qc_nodes_host(ix, cluster_nodes, n_nodes, nullptr, 0, min_assemblies, ev, &h->r); }, &st);
        }
        h->publish(n, false, st);
        *out = h.release();
    });
}
int ac_cluster_qc_clusters(const ac_cluster_qc* q, const uint16_t** nodes, uint32_t* n_nodes) {
    return guarded([&] {
        if (!q || !nodes || !n_nodes) throw DeviceError("null pointer");
        *nodes = q->r.nodes.data(); *n_nodes = (uint32_t)q->r.nodes.size();
    });
}
int ac_cluster_qc_assignment(const ac_cluster_qc* q, const uint16_t** cluster_of_seq, uint32_t* n) {
    return guarded([&] {
        if (!q || !cluster_of_seq || !n) throw DeviceError("null pointer");
        *cluster_of_seq = q->r.cluster_of_seq.data(); *n = (uint32_t)q->r.cluster_of_seq.size();
    });
}
int ac_cluster_qc_records(const ac_cluster_qc* q, const ac_cluster_qc_record** records, uint32_t* n) {
    return guarded([&] {
        if (!q || !records || !n) throw DeviceError("null pointer");
        *records = q->records.data(); *n = (uint32_t)q->records.size();
    });
}
int ac_cluster_qc_metrics(const ac_cluster_qc* q, ac_clustering_metrics* out) {
    return guarded([&] {
        if (!q || !out) throw DeviceError("null pointer");
        *out = q->metrics;
    });
}
int ac_cluster_qc_trace(const ac_cluster_qc* q, const uint32_t** round_alternatives, uint32_t* n_rounds, const double** scores,
                        const uint8_t** accepted, uint64_t* n_scores) {
    return guarded([&] {
        if (!q || !round_alternatives || !n_rounds || !scores || !accepted || !n_scores) throw DeviceError("null pointer");
        *round_alternatives = q->r.round_alternatives.data(); *n_rounds = (uint32_t)q->r.round_alternatives.size();
        *scores = q->r.scores.data(); *accepted = q->r.accepted.data(); *n_scores = q->r.scores.size();
    });
}
size_t ac_cluster_qc_summary_get_sized(const ac_cluster_qc* q, ac_cluster_qc_summary* out, size_t out_size) {
    if (q && out) memcpy(out, &q->summary, std::min(out_size, sizeof(ac_cluster_qc_summary)));
    return sizeof(ac_cluster_qc_summary);
}
void ac_cluster_qc_free(ac_cluster_qc* q) { delete q; }
int ac_cluster_min_assemblies(const uint32_t* assembly, uint32_t n, uint32_t* out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer");
        if (n == 0) throw DeviceError("cluster: no sequences");
        *out = cluster_min_assemblies(cluster_assembly_count_checked(assembly, n));
    });
}
int ac_cluster_seq_inputs(const ac_graph* g, uint64_t* seq_len, uint32_t* assembly, uint32_t* cluster_weight, uint8_t* trusted, uint32_t* n_assemblies) {
    return guarded([&] {
        if (!g) throw DeviceError("null pointer");
        const size_t n = g->seq_ids.size();
        if (g->filenames.size() != n || g->headers.size() != n || g->seq_lens.size() != n)
            throw DeviceError("cluster: this graph carries no file names and headers (load it with ac_graph_from_gfa)");
        std::vector<uint32_t> number(n);
        const uint32_t distinct = cluster_number_assemblies(g->filenames, number.data());
        for (size_t i = 0; i < n; i++) {
            if (seq_len) seq_len[i] = g->seq_lens[i];
            if (assembly) assembly[i] = number[i];
            if (cluster_weight) cluster_weight[i] = cluster_header_weight(g->headers[i]);
            if (trusted) trusted[i] = cluster_header_trusted(g->headers[i]) ? 1 : 0;
        }
        if (n_assemblies) *n_assemblies = distinct;
    });
}

// ---- read-based unitig depths of `autocycler combine --reads` (depth.rs:45-76): the k-mer table and the read tally on the device
// (graph_depth.hip), the graph walks and the per-unitig arithmetic on the host (depth_host.cpp) ----
struct ac_depth {      // (every call on a handle makes the handle's own device current)
    int device = 0;
    std::unique_ptr<DepthEngine> e;
};
static void depth_begin(uint32_t k, const ac_depth_graph* graphs, uint32_t n_graphs, int device, ac_depth** out) {
    if (!out || (n_graphs && !graphs)) throw DeviceError("null pointer");
    *out = nullptr;
    if (k % 2 == 0 || k < 11 || k > 31) throw DeviceError("--kmer must be an odd number between 11 and 31 (inclusive) for read-based depths");
    std::vector<DepthGraphView> views(n_graphs);
    std::vector<DepthGraphPlan> plans(n_graphs);
    for (uint32_t g = 0; g < n_graphs; g++) {
        const ac_depth_graph& a = graphs[g];
        if ((a.n_unitigs && (!a.seq_bytes || !a.seq_begin || !a.seq_len)) || (a.n_links && !a.links)) throw DeviceError("null pointer in graph " + std::to_string(g + 1));
        static_assert(sizeof(ac_link) == 2 * sizeof(int32_t), "layout");
        views[g] = DepthGraphView{a.seq_bytes, a.seq_begin, a.seq_len, a.n_unitigs, (const int32_t*)a.links, a.n_links};
        depth_plan_graph(k, views[g], g, &plans[g]);
    }
    auto h = std::make_unique<ac_depth>();
    h->device = device;
    DeviceCall call(device);
    h->e = std::make_unique<DepthEngine>(k, views, std::move(plans));      // (a failure on the way frees what the engine already held)
    *out = h.release();
}
int ac_depth_begin(uint32_t k, const ac_depth_graph* graphs, uint32_t n_graphs, int device, ac_depth** out) {
    return guarded([&] { depth_begin(k, graphs, n_graphs, device, out); });
}
int ac_depth_begin_handles(uint32_t k, const ac_graph* const* graphs, uint32_t n_graphs, int device, ac_depth** out) {
    return guarded([&] {
        if (n_graphs && !graphs) throw DeviceError("null pointer");
        std::vector<ac_depth_graph> a(n_graphs);
        for (uint32_t g = 0; g < n_graphs; g++) {
            if (!graphs[g]) throw DeviceError("null pointer");
            memset(&a[g], 0, sizeof a[g]);
            if (ac_unitigs_bulk(graphs[g], &a[g].seq_bytes, &a[g].seq_begin, &a[g].seq_len, nullptr) || ac_links(graphs[g], &a[g].links, &a[g].n_links))
                throw DeviceError(last_error());
            a[g].n_unitigs = graphs[g]->g.n_unitigs;
        }
        depth_begin(k, a.data(), n_graphs, device, out);
    });
}
static void depth_check_offsets(const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads) {
    if (n_reads && !read_off) throw DeviceError("null pointer");
    for (uint64_t r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r]) throw DeviceError("read_off must ascend (read " + std::to_string(r + 1) + " ends before it starts)");
    if (n_reads && read_off[n_reads] > read_off[0] && !bases) throw DeviceError("null pointer");
}
int ac_depth_add_reads(ac_depth* d, const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads) {
    return guarded([&] {
        if (!d) throw DeviceError("null pointer");
        depth_check_offsets(bases, read_off, n_reads);
        DeviceCall call(d->device);
        d->e->add_reads(bases, read_off, n_reads);
    });
}
int ac_depth_add_fastq(ac_depth* d, const char* path) {
    return guarded([&] {
        if (!d || !path) throw DeviceError("null pointer");
        depth_read_fastq(path, (size_t)64 << 20, [&](const std::vector<uint8_t>& bases, const std::vector<uint64_t>& off) {
            DeviceCall call(d->device);
            d->e->add_reads(bases.data(), off.data(), off.size() - 1);
        });
    });
}
int ac_depth_totals_get(const ac_depth* d, ac_depth_totals* out) {
    return guarded([&] {
        if (!d || !out) throw DeviceError("null pointer");
        if (out->size < sizeof(uint64_t)) throw DeviceError("ac_depth_totals.size must hold the caller's sizeof(ac_depth_totals)");
        DeviceCall call(d->device);
        const DepthTotals t = d->e->totals();
        ac_depth_totals full;
        memset(&full, 0, sizeof full);
        full.size = sizeof full;
        full.reads = t.reads; full.rejected_reads = t.rejected_reads; full.read_bases = t.read_bases; full.span_bases = t.span_bases;
        full.span_kmers = t.span_kmers; full.hits = t.hits; full.distinct_kmers = t.distinct_kmers; full.repeat_kmers = t.repeat_kmers;
        full.table_slots = t.table_slots; full.batches = t.batches; full.launches = t.launches; full.seconds_device = t.seconds_device;
        memcpy(out, &full, std::min<size_t>((size_t)out->size, sizeof full));
    });
}
int ac_depth_kmer_counts(ac_depth* d, const uint64_t* kmers, uint64_t n, uint8_t* present, uint32_t* assembly_occurrences, uint32_t* read_count) {
    return guarded([&] {
        if (!d || (n && !kmers)) throw DeviceError("null pointer");
        DeviceCall call(d->device);
        d->e->kmer_counts(kmers, n, present, assembly_occurrences, read_count);
    });
}
int ac_depth_finish(ac_depth* d, uint32_t graph_index, double* depth, uint8_t* has_depth) {
    return guarded([&] {
        if (!d) throw DeviceError("null pointer");
        if (graph_index >= d->e->n_graphs()) throw DeviceError("graph index out of range");
        if (d->e->n_unitigs(graph_index) && (!depth || !has_depth)) throw DeviceError("null pointer");
        DeviceCall call(d->device);
        d->e->finish(graph_index, depth, has_depth);
    });
}
void ac_depth_free(ac_depth* d) {
    if (!d) return;
    std::lock_guard<std::mutex> lock(g_build_mutex);
    delete d;
}

// UnitigGraph::from_gfa_lines (unitig_graph.rs:55-174) for the GFAs `compress` writes: what `cluster` and `decompress` start from.
int ac_graph_from_gfa(const char* gfa_text, uint64_t len, ac_graph** out) {
    return guarded([&] {
        if (!gfa_text) throw DeviceError("no GFA text");
        auto h = std::make_unique<ac_graph>();
        std::vector<SeqMeta> meta;
        load_gfa(gfa_text, (size_t)len, &h->g, &meta);
        for (auto& m : meta) { h->seq_ids.push_back(m.id); h->seq_lens.push_back(m.length); h->filenames.push_back(m.filename); h->headers.push_back(m.contig_header); }
        *out = h.release();
    });
}
// reconstruct_original_sequences (unitig_graph.rs:362-388) for one sequence; out holds its LN bytes.
int ac_decompress_seq(const ac_graph* g, uint32_t seq_index, uint8_t* out) {
    return guarded([&] {
        if (seq_index >= g->seq_ids.size()) throw DeviceError("sequence index out of range");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        decompress_sequence(g->g, seq_index, (char*)out);
    });
}

// ---- the round-trip verifier behind the ABI (kernels_verify.inc) ------------------------------------------------------------------
static void fill_report(const VerifyReport& r, ac_verify_report* o) {
    memset(o, 0, sizeof *o);
    o->failed = r.failed;
    o->first_bad_unitig = r.first_bad_unitig; o->first_bad_link = r.first_bad_link; o->first_bad_path_entry = r.first_bad_path_entry;
    o->first_bad_sequence = r.first_bad_sequence; o->first_bad_base = r.first_bad_base;
    o->unitigs = r.unitigs; o->links = r.links; o->path_entries = r.path_entries; o->bases_checked = r.bases_checked;
    o->self_mirror_links = r.self_mirror_links; o->seconds = r.seconds;
    o->checks = r.checks; o->first_bad_junction = r.first_bad_junction;
}
int ac_verify_graph_device(const ac_graph* g, const void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                           uint32_t n_seqs, int device, ac_verify_report* report) {
    return guarded([&] {
        if (!g || !d_text || !seq_off || !seq_len || !report) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        if (n_seqs != g->seq_lens.size()) throw DeviceError("ac_verify_graph: the graph was built from " + std::to_string(g->seq_lens.size()) + " sequences, not " + std::to_string(n_seqs));
        DeviceCall call(device);
        std::vector<uint64_t> off(seq_off, seq_off + n_seqs);
        std::vector<uint32_t> len(seq_len, seq_len + n_seqs);
        VerifyReport r;
        verify_graph_device(g->g, (const uint8_t*)d_text, n_text, off, len, &r);
        fill_report(r, report);
    });
}
int ac_verify_graph(const ac_graph* g, const ac_seq_view* seqs, uint32_t n_seqs, int device, ac_verify_report* report) {
    return guarded([&] {
        if (!g || !seqs || !report) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        if (n_seqs != g->seq_lens.size()) throw DeviceError("ac_verify_graph: the graph was built from " + std::to_string(g->seq_lens.size()) + " sequences, not " + std::to_string(n_seqs));
        std::vector<SeqView> v(n_seqs);
        for (uint32_t i = 0; i < n_seqs; i++) {
            if (!seqs[i].fwd) throw DeviceError("null sequence");
            v[i] = SeqView{seqs[i].fwd, seqs[i].length};
        }
        std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<uint16_t> d1, d2;
        std::vector<uint8_t> text = layout_text(v, g->g.k, &off, &len, &d1, &d2);
        DeviceCall call(device);
        VerifyReport r;
        // (the text goes up through an allocation of its own: the verifier resets the arena for its working set)
#ifdef AC_EMU
        verify_graph_device(g->g, text.data(), text.size(), off, len, &r);
#else
        void* d_text = nullptr;
        AC_HIP_CHECK(hipMalloc(&d_text, text.size() + 64));
        struct Free { void* p; ~Free() { (void)hipFree(p); } } fr{d_text};
        AC_HIP_CHECK(hipMemcpy(d_text, text.data(), text.size(), hipMemcpyHostToDevice));
        verify_graph_device(g->g, (const uint8_t*)d_text, text.size(), off, len, &r);
#endif
        fill_report(r, report);
    });
}

// reconstruct_original_sequences for every sequence of the graph at once, on the device (kernels_verify.inc): out = sum of the sequence
// lengths bytes, sequence i at offset sum(length[0 .. i)).  What ac_decompress_seq does one sequence at a time on the host.
int ac_decompress_device(const ac_graph* g, int device, uint8_t* out, uint64_t out_bytes) {
    return guarded([&] {
        if (!g || !out) throw DeviceError("null pointer");
        if (!g->host_arrays || !g->host_paths) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
        uint64_t need = 0;
        for (uint32_t l : g->seq_lens) need += l;
        if (out_bytes < need) throw DeviceError("ac_decompress_device: the buffer holds " + std::to_string(out_bytes) + " bytes, the sequences need " + std::to_string(need));
        DeviceCall call(device);
        decompress_device(g->g, g->seq_lens, out);
    });
}
// The hand-written scan / radix sort / comparator sort (device_prims.hpp) against the host's std:: algorithms — test hook.
int ac_selftest_primitives(int device, uint64_t n, uint64_t seed, int end_bit, int key_kind) {
    return guarded([&] {
        if (end_bit < 1 || end_bit > 64) throw DeviceError("end_bit out of range");
        DeviceCall call(device);
        primitives_selftest(n, seed, end_bit, key_kind);
    });
}
// One primitive on the caller's arrays, its output handed back — test hooks (selftest_prims.inc).
int ac_selftest_scan(int device, int kind, const void* in, uint64_t n, int in_place, int misalign_in, int misalign_out, void* out) {
    return guarded([&] { DeviceCall call(device); selftest_scan(kind, in, n, in_place != 0, misalign_in, misalign_out, out); });
}
int ac_selftest_radix(int device, const uint64_t* keys, const void* vals, uint64_t n, int begin_bit, int end_bit, int val_kind, uint64_t prep_n, int prep_bits,
                      int prep_reuse, uint64_t* keys_out, void* vals_out) {
    return guarded([&] { DeviceCall call(device); selftest_radix(keys, vals, n, begin_bit, end_bit, val_kind, prep_n, prep_bits, prep_reuse != 0, keys_out, vals_out); });
}
int ac_selftest_segments(int device, int op, const uint32_t* seg, const uint64_t* vals, uint64_t n, uint64_t n_segments, int deferred_err, void* out, uint32_t* err_out) {
    return guarded([&] { DeviceCall call(device); selftest_segments(op, seg, vals, n, n_segments, deferred_err != 0, out, err_out); });
}
int ac_selftest_sort_cmp(int device, int form, const uint64_t* key_a, const uint32_t* key_b, const uint32_t* vals, uint64_t n, uint64_t* key_a_out, uint32_t* key_b_out,
                         uint32_t* vals_out) {
    return guarded([&] { DeviceCall call(device); selftest_sort_cmp(form, key_a, key_b, vals, n, key_a_out, key_b_out, vals_out); });
}
int ac_selftest_scan_pool(int device, int op, uint64_t value, uint64_t* out) {
    return guarded([&] { DeviceCall call(device); selftest_scan_pool(op, value, out); });
}
int ac_selftest_wave(int device, int program, const uint64_t* in_u64, const int32_t* aux_i32, const uint64_t* live_mask, uint64_t* out_u64) {
    return guarded([&] { DeviceCall call(device); selftest_wave(program, in_u64, aux_i32, live_mask, out_u64); });
}
// One facility of the device runtime on the caller's data — test hooks (selftest_runtime.inc).
int ac_selftest_fills(int device, const uint64_t* regions, uint64_t n_regions, int trigger, int mode, uint8_t* span, uint64_t span_bytes, uint32_t* launches_out) {
    return guarded([&] { DeviceCall call(device); selftest_fills(regions, n_regions, trigger, mode, span, span_bytes, launches_out); });
}
int ac_selftest_fill_order(int device, uint64_t n, int byte1, uint64_t w_lo, uint64_t w_hi, int w_val, uint64_t from2, int byte2, uint64_t upto3, int byte3, uint8_t* out) {
    return guarded([&] { DeviceCall call(device); selftest_fill_order(n, byte1, w_lo, w_hi, w_val, from2, byte2, upto3, byte3, out); });
}
int ac_selftest_readback(int device, const uint8_t* data, uint64_t n_data, int path, const uint64_t* items, uint64_t n_items, uint8_t* out, uint32_t* counters_out) {
    return guarded([&] { DeviceCall call(device); selftest_readback(data, n_data, path, items, n_items, out, counters_out); });
}
int ac_selftest_scalar_chain(int device, const uint64_t* values, uint64_t n, uint64_t* out, uint32_t* counters_out) {
    return guarded([&] { DeviceCall call(device); selftest_scalar_chain(values, n, out, counters_out); });
}
int ac_selftest_arena(int device, const uint64_t* ops, uint64_t n_ops, uint64_t* totals_out, uint64_t* allocs_out, const uint8_t* live, uint64_t* wrong_out) {
    return guarded([&] { DeviceCall call(device); selftest_arena(ops, n_ops, totals_out, allocs_out, live, wrong_out); });
}
int ac_selftest_launch(int device, int which, uint64_t n, uint64_t* slots_out, uint32_t* info_out) {
    return guarded([&] { DeviceCall call(device); selftest_launch(which, n, slots_out, info_out); });
}
int ac_selftest_atomics(int device, int op, uint64_t init, uint64_t expected, const uint64_t* operand, const uint32_t* target, uint32_t n_words, uint64_t* words_out,
                        uint64_t* returns_out) {
    return guarded([&] { DeviceCall call(device); selftest_atomics(op, init, expected, operand, target, n_words, words_out, returns_out); });
}
int ac_selftest_side_order(int device, int mode, int which, uint32_t seed, uint64_t n_words, uint32_t* out_words) {
    return guarded([&] { DeviceCall call(device); selftest_side_order(mode, which, seed, n_words, out_words); });
}
int ac_selftest_event_ring(int device, int op, const uint8_t* kinds, uint32_t n_more, uint64_t* out) {
    return guarded([&] { DeviceCall call(device); selftest_event_ring(op, kinds, n_more, out); });
}

int ac_random_access_ceilings_at(int device, uint64_t table_slots, double* cas_gops, double* read_gops) {
    return guarded([&] {
        DeviceCall call(device);
        random_access_ceilings(cas_gops, read_gops, table_slots);
    });
}
int ac_random_access_ceilings(int device, double* cas_gops, double* read_gops) { return ac_random_access_ceilings_at(device, (uint64_t)1 << 24, cas_gops, read_gops); }

}  // extern "C"
