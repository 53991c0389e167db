// C ABI, `autocycler combine` and `autocycler gfa2fasta` up to their texts: the order of the graphs, the offsets, the per-unitig end tests, topology()
// and the L-line order on the device (kernels_combine.inc); the loader, cluster_depth and the texts on the host (combine_host.cpp).  The two
// commands on files are in capi_command.cpp.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "capi_common.hpp"

using namespace ac;
using namespace ac::abi;

struct ac_combined {
    CombineResult r;
    ac_combined_summary summary;
    std::vector<uint8_t> seq_all;          // a copy of the caller's bytes when they were given: the texts need them
    std::vector<const char*> seq;          // per unitig in output order, into seq_all or into bytes the entry itself holds (text forms)
    bool has_seqs = false;
};
static_assert(sizeof(ac_combined_cluster) == sizeof(CombineClusterRecord) && offsetof(ac_combined_cluster, read_depth) == offsetof(CombineClusterRecord, read_depth) &&
              offsetof(ac_combined_cluster, topology) == offsetof(CombineClusterRecord, topology), "ac_combined_cluster is CombineClusterRecord");
static_assert(sizeof(ac_combined_unitig) == sizeof(CombineUnitigRecord) && offsetof(ac_combined_unitig, read_depth) == offsetof(CombineUnitigRecord, read_depth) &&
              offsetof(ac_combined_unitig, type) == offsetof(CombineUnitigRecord, type), "ac_combined_unitig is CombineUnitigRecord");

static char* text_out(const std::string& s, uint64_t* len) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) throw DeviceError("out of memory");
    memcpy(p, s.c_str(), s.size() + 1);
    if (len) *len = s.size();
    return p;
}

// seq_of(i): the bytes of unitig i of the concatenation, or nullptr.  The result's seq pointers are set in output order.
template <class SeqOf> static void combine_run(const CombineInput& in, int device, SeqOf seq_of, bool has_seqs, ac_combined* h) {
    combine_prepare(in);
    if (in.n_unitigs() == 0) combine_without_unitigs(in, &h->r);      // (nothing to launch: no device is asked for)
    else {
        DeviceCall call(device);
        combine_device(in, &h->r);
    }
    combine_finish(&h->r);
    const CombineResult& r = h->r;
    h->has_seqs = has_seqs;
    h->seq.assign(r.unitigs.size(), nullptr);
    if (has_seqs)
        for (size_t i = 0; i < r.unitigs.size(); i++) h->seq[i] = seq_of(in.unitig_off[r.unitigs[i].graph] + r.unitigs[i].index);
    ac_combined_summary& sm = h->summary;
    memset(&sm, 0, sizeof sm);
    sm.size = (uint32_t)sizeof sm; sm.graphs = in.n_graphs; sm.bases = r.bases; sm.unitigs = r.n_unitigs; sm.links = r.links.size();
    sm.fully_resolved = r.fully_resolved ? 1 : 0; sm.with_reads = r.with_reads ? 1 : 0; sm.launches = r.stats.launches; sm.read_backs = r.stats.read_backs;
    sm.seconds_device = r.stats.seconds_device;
}

// The cluster GFAs of a text entry, loaded and laid end to end as the array entry takes them; the bytes stay in the callers' texts.
struct CombineTexts {
    std::vector<CombineGfa> graphs;
    std::vector<const char*> text;
    std::vector<uint64_t> unitig_off, link_off;
    std::vector<uint32_t> number, len;
    std::vector<double> depth, read_depth;
    std::vector<uint8_t> type, has_read_depth;
    std::vector<Link> links;
    CombineInput in;
    void load(const char* const* texts, const uint64_t* lens, uint32_t n) {
        if (n == 0) throw DeviceError("combine: at least one graph is required");
        if (!texts || !lens) throw DeviceError("null pointer: texts and lens are required");
        graphs.resize(n); text.assign(texts, texts + n);
        unitig_off.assign(1, 0); link_off.assign(1, 0);
        for (uint32_t g = 0; g < n; g++) {
            combine_load_gfa(texts[g], lens[g], &graphs[g]);
            const CombineGfa& c = graphs[g];
            number.insert(number.end(), c.number.begin(), c.number.end()); len.insert(len.end(), c.len.begin(), c.len.end());
            depth.insert(depth.end(), c.depth.begin(), c.depth.end()); type.insert(type.end(), c.type.begin(), c.type.end());
            links.insert(links.end(), c.links.begin(), c.links.end());
            unitig_off.push_back(number.size()); link_off.push_back(links.size());
        }
        in.n_graphs = n; in.unitig_off = unitig_off.data(); in.link_off = link_off.data(); in.number = number.data(); in.len = len.data(); in.depth = depth.data();
        in.type = type.data(); in.links = links.data();
    }
    // per graph one array each (both lists or neither)
    void set_read_depths(const double* const* rd, const uint8_t* const* has) {
        if ((rd == nullptr) != (has == nullptr)) throw DeviceError("null pointer: read_depth and has_read_depth come together or not at all");
        if (!rd) return;
        read_depth.assign(number.size() + 1, 0.0); has_read_depth.assign(number.size() + 1, 0);
        for (uint32_t g = 0; g < in.n_graphs; g++) {
            const uint64_t a = unitig_off[g], b = unitig_off[g + 1];
            if (b > a && (!rd[g] || !has[g])) throw DeviceError("null pointer: read depths of graph " + std::to_string(g));
            for (uint64_t u = a; u < b; u++) { read_depth[u] = rd[g][u - a]; has_read_depth[u] = has[g][u - a] ? 1 : 0; }
        }
        in.read_depth = read_depth.data(); in.has_read_depth = has_read_depth.data();
    }
    const char* seq_of(uint64_t u) const {
        const size_t g = (size_t)(std::upper_bound(unitig_off.begin(), unitig_off.end() - 1, u) - unitig_off.begin()) - 1;
        return text[g] + graphs[g].seq_at[u - unitig_off[g]];
    }
};

extern "C" {

int ac_combine_graphs(uint32_t n_graphs, const uint64_t* unitig_off, const uint64_t* link_off, const uint32_t* number, const uint32_t* unitig_len, const double* depth,
                      const uint8_t* type, const ac_link* links, const double* read_depth, const uint8_t* has_read_depth, const uint8_t* seq_bytes,
                      const uint64_t* seq_begin, int device, ac_combined** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if ((seq_bytes == nullptr) != (seq_begin == nullptr)) throw DeviceError("null pointer: seq_bytes and seq_begin come together or not at all");
        CombineInput in;
        in.n_graphs = n_graphs; in.unitig_off = unitig_off; in.link_off = link_off; in.number = number; in.len = unitig_len; in.depth = depth; in.type = type;
        in.links = (const Link*)links; in.read_depth = read_depth; in.has_read_depth = has_read_depth;
        auto h = std::make_unique<ac_combined>();
        combine_prepare(in);
        if (seq_bytes) {
            uint64_t total = 0;
            for (uint64_t u = 0; u < in.n_unitigs(); u++) total = std::max<uint64_t>(total, seq_begin[u] + unitig_len[u]);
            h->seq_all.assign(seq_bytes, seq_bytes + total);
        }
        const ac_combined* hp = h.get();
        combine_run(in, device, [&](uint64_t u) { return (const char*)hp->seq_all.data() + seq_begin[u]; }, seq_bytes != nullptr, h.get());
        *out = h.release();
    });
}

int ac_combine_handles(const ac_graph* const* graphs, uint32_t n_graphs, const uint8_t* const* type, const double* const* read_depth, const uint8_t* const* has_read_depth,
                       int device, ac_combined** out) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (n_graphs == 0) throw DeviceError("combine: at least one graph is required");
        if (!graphs) throw DeviceError("null pointer: graphs");
        if ((read_depth == nullptr) != (has_read_depth == nullptr)) throw DeviceError("null pointer: read_depth and has_read_depth come together or not at all");
        std::vector<uint64_t> uoff(1, 0), loff(1, 0), seq_begin;
        std::vector<uint32_t> number, len;
        std::vector<double> depth, rd;
        std::vector<uint8_t> ty, has;
        std::vector<Link> links;
        auto h = std::make_unique<ac_combined>();
        for (uint32_t g = 0; g < n_graphs; g++) {
            if (!graphs[g]) throw DeviceError("null pointer: graph " + std::to_string(g));
            if (!graphs[g]->host_arrays) throw DeviceError("this rank kept no host arrays (sharded build, not the writing rank)");
            const FinalGraph& f = graphs[g]->g;
            if (read_depth && f.n_unitigs && (!read_depth[g] || !has_read_depth[g])) throw DeviceError("null pointer: read depths of graph " + std::to_string(g));
            for (uint32_t u = 0; u < f.n_unitigs; u++) {
                number.push_back(u + 1); len.push_back(f.seq_len[u]); depth.push_back(f.depth[u]); ty.push_back(type && type[g] ? type[g][u] : (uint8_t)MERGE_TYPE_OTHER);
                seq_begin.push_back(h->seq_all.size());
                h->seq_all.insert(h->seq_all.end(), (const uint8_t*)f.seq(u), (const uint8_t*)f.seq(u) + f.seq_len[u]);
                if (read_depth) { rd.push_back(read_depth[g][u]); has.push_back(has_read_depth[g][u] ? 1 : 0); }
            }
            links.insert(links.end(), f.links, f.links + f.n_links);
            uoff.push_back(number.size()); loff.push_back(links.size());
        }
        number.push_back(0); len.push_back(0); rd.push_back(0); has.push_back(0);      // (never empty: the pointers below are not null)
        CombineInput in;
        in.n_graphs = n_graphs; in.unitig_off = uoff.data(); in.link_off = loff.data(); in.number = number.data(); in.len = len.data(); in.depth = depth.data();
        in.type = ty.data(); in.links = links.data();
        if (read_depth) { in.read_depth = rd.data(); in.has_read_depth = has.data(); }
        const ac_combined* hp = h.get();
        combine_run(in, device, [&](uint64_t u) { return (const char*)hp->seq_all.data() + seq_begin[u]; }, true, h.get());
        *out = h.release();
    });
}

int ac_combined_clusters(const ac_combined* c, const ac_combined_cluster** clusters, uint32_t* n) {
    return guarded([&] {
        if (!c || !clusters || !n) throw DeviceError("null pointer");
        *clusters = (const ac_combined_cluster*)c->r.clusters.data(); *n = (uint32_t)c->r.clusters.size();
    });
}
int ac_combined_unitigs(const ac_combined* c, const ac_combined_unitig** unitigs, uint64_t* n) {
    return guarded([&] {
        if (!c || !unitigs || !n) throw DeviceError("null pointer");
        *unitigs = (const ac_combined_unitig*)c->r.unitigs.data(); *n = c->r.unitigs.size();
    });
}
int ac_combined_links(const ac_combined* c, const ac_link** links, uint64_t* n) {
    return guarded([&] {
        if (!c || !links || !n) throw DeviceError("null pointer");
        *links = (const ac_link*)c->r.links.data(); *n = c->r.links.size();
    });
}
size_t ac_combined_summary_get_sized(const ac_combined* c, ac_combined_summary* out, size_t out_size) {
    if (c && out) memcpy(out, &c->summary, std::min(out_size, sizeof(ac_combined_summary)));
    return sizeof(ac_combined_summary);
}
void ac_combined_free(ac_combined* c) { delete c; }

static const ac_combined& with_seqs(const ac_combined* c, char** out) {
    if (!out) throw DeviceError("null pointer: out");
    *out = nullptr;
    if (!c) throw DeviceError("null pointer");
    if (!c->has_seqs && c->r.bases) throw DeviceError("combine: missing sequences: the object was made without seq_bytes and seq_begin");
    return *c;
}
int ac_combined_gfa_string(const ac_combined* c, char** out, uint64_t* len) {
    return guarded([&] { const ac_combined& h = with_seqs(c, out); *out = text_out(combine_gfa_string(h.r, h.seq), len); });
}
int ac_combined_fasta_string(const ac_combined* c, char** out, uint64_t* len) {
    return guarded([&] { const ac_combined& h = with_seqs(c, out); *out = text_out(combine_fasta_string(h.r, h.seq), len); });
}
int ac_combined_yaml_string(const ac_combined* c, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!c) throw DeviceError("null pointer");
        *out = text_out(combine_yaml_string(c->r), len);
    });
}
int ac_combined_depth_lines(const ac_combined* c, char** out, uint64_t* len) {
    return guarded([&] {
        if (!out) throw DeviceError("null pointer: out");
        *out = nullptr;
        if (!c) throw DeviceError("null pointer");
        *out = text_out(combine_depth_lines(c->r), len);
    });
}

int ac_combine_gfas(const char* const* texts, const uint64_t* lens, uint32_t n, const double* const* read_depth, const uint8_t* const* has_read_depth, int device,
                    char** gfa, uint64_t* gfa_len, char** fasta, uint64_t* fasta_len, char** yaml, uint64_t* yaml_len, ac_combined_summary* summary) {
    return guarded([&] {
        if (!gfa || !fasta || !yaml) throw DeviceError("null pointer: out");
        *gfa = *fasta = *yaml = nullptr;
        CombineTexts t;
        t.load(texts, lens, n);
        t.set_read_depths(read_depth, has_read_depth);
        ac_combined h;
        combine_run(t.in, device, [&](uint64_t u) { return t.seq_of(u); }, true, &h);
        char* a = text_out(combine_gfa_string(h.r, h.seq), gfa_len);
        char* b = nullptr; char* c = nullptr;
        try { b = text_out(combine_fasta_string(h.r, h.seq), fasta_len); c = text_out(combine_yaml_string(h.r), yaml_len); }
        catch (...) { free(a); free(b); throw; }
        *gfa = a; *fasta = b; *yaml = c;
        if (summary) { const size_t want = summary->size ? std::min<size_t>(summary->size, sizeof h.summary) : sizeof h.summary; memcpy(summary, &h.summary, want); }
    });
}

// gfa2fasta.rs:56-83 from a text: the combine of one graph gives the flags; no offset, the file's own numbers and DP:f depths
int ac_gfa2fasta_string(const char* gfa_text, uint64_t len, int device, char** fasta, uint64_t* fasta_len, uint64_t* counts) {
    return guarded([&] {
        if (!fasta) throw DeviceError("null pointer: out");
        *fasta = nullptr;
        if (!gfa_text && len) throw DeviceError("null pointer: gfa_text");
        CombineTexts t;
        const char* texts[1] = {gfa_text ? gfa_text : ""};
        t.load(texts, &len, 1);
        ac_combined h;
        combine_run(t.in, device, [&](uint64_t u) { return t.seq_of(u); }, true, &h);
        std::vector<uint8_t> flags(h.r.unitigs.size());
        for (const CombineUnitigRecord& u : h.r.unitigs) flags[u.index] = u.flags;
        uint64_t c[3];
        *fasta = text_out(combine_gfa2fasta_string(t.graphs[0], texts[0], flags.data(), c), fasta_len);
        if (counts) { counts[0] = c[0]; counts[1] = c[1]; counts[2] = c[2]; }
    });
}

}  // extern "C"
