// Bounds check of kernels_combine.inc and of the flag stage of kernels_components.inc it calls: the CPU emulation (-DAC_EMU) linked into this
// stand-alone program under the address and undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2),
// from the per-level objects that `make kernel_bounds_check` builds.  `make combine_bounds_check` in autocycler_amd/csrc builds it;
// tests/test_combine_bounds_emu.py builds it the same way and feeds it.  CPU only.
//
//   combine_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                           writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "combine":
//   s: n_graphs
//   a: unitig_off u64, link_off u64, number u32, len u32, depth f64 (or empty), type u8 (or empty), links, read_depth f64, has_read_depth u8 (both
//      or both empty), seq_bytes u8, seq_begin u64 (both or both empty)
//   out: clusters (ac_combined_cluster) | unitigs (ac_combined_unitig) | links | the gfa | the fasta | the yaml | the depth lines |
//        u64 {launches, read_backs, bases, unitigs, fully_resolved}
// The input arrays are exact heap blocks: a read past one of them on the host side of a copy is the sanitizer's to see.
#include "../../include/autocycler_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
struct Call { std::string name; std::vector<int64_t> s; std::vector<Bytes> a; };
struct Out {
    std::vector<Bytes> a;
    void put(const void* p, size_t bytes) { a.emplace_back((const uint8_t*)p, (const uint8_t*)p + (p ? bytes : 0)); }
};
template <class T> static const T* arr(const Call& c, size_t i) { return c.a.at(i).empty() ? nullptr : (const T*)c.a[i].data(); }
#define TRY(expr) do { if ((expr) != 0) { fprintf(stderr, "%s: %s failed: %s\n", c.name.c_str(), #expr, ac_last_error()); return 1; } } while (0)

static int do_combine(const Call& c, Out& o) {
    const uint32_t n_graphs = (uint32_t)c.s.at(0);
    ac_combined* h = nullptr;
    TRY(ac_combine_graphs(n_graphs, arr<uint64_t>(c, 0), arr<uint64_t>(c, 1), arr<uint32_t>(c, 2), arr<uint32_t>(c, 3), arr<double>(c, 4), arr<uint8_t>(c, 5),
                          arr<ac_link>(c, 6), arr<double>(c, 7), arr<uint8_t>(c, 8), arr<uint8_t>(c, 9), arr<uint64_t>(c, 10), 0, &h));
    const ac_combined_cluster* clusters = nullptr; uint32_t nc = 0;
    TRY(ac_combined_clusters(h, &clusters, &nc));
    o.put(clusters, (size_t)nc * sizeof *clusters);
    const ac_combined_unitig* unitigs = nullptr; uint64_t nu = 0;
    TRY(ac_combined_unitigs(h, &unitigs, &nu));
    o.put(unitigs, (size_t)nu * sizeof *unitigs);
    const ac_link* links = nullptr; uint64_t nl = 0;
    TRY(ac_combined_links(h, &links, &nl));
    o.put(links, (size_t)nl * sizeof *links);
    const bool seqs = !c.a.at(10).empty() || nu == 0;
    int (*texts[4])(const ac_combined*, char**, uint64_t*) = {ac_combined_gfa_string, ac_combined_fasta_string, ac_combined_yaml_string, ac_combined_depth_lines};
    for (int t = 0; t < 4; t++) {
        if (t < 2 && !seqs) { o.put(nullptr, 0); continue; }
        char* text = nullptr; uint64_t len = 0;
        TRY(texts[t](h, &text, &len));
        o.put(text, (size_t)len);
        ac_string_free(text);
    }
    ac_combined_summary sm; memset(&sm, 0, sizeof sm);
    ac_combined_summary_get_sized(h, &sm, sizeof sm);
    const uint64_t counts[5] = {sm.launches, sm.read_backs, sm.bases, sm.unitigs, sm.fully_resolved};
    o.put(counts, sizeof counts);
    ac_combined_free(h);
    return 0;
}

struct Reader {
    FILE* f; bool ok = true;
    void raw(void* p, size_t n) { if (n && fread(p, 1, n, f) != n) ok = false; }
    uint32_t u32() { uint32_t v = 0; raw(&v, 4); return v; }
    uint64_t u64() { uint64_t v = 0; raw(&v, 8); return v; }
    std::string str() { std::string s(u32(), '\0'); raw(&s[0], s.size()); return s; }
};

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CALLS RESULTS\n", argv[0]); return 2; }
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
        for (uint32_t i = in.u32(); i-- > 0;) { in.str(); in.str(); }      // (no entry here reads the environment)
        for (uint32_t i = in.u32(); i-- > 0;) c.s.push_back((int64_t)in.u64());
        for (uint32_t i = in.u32(); i-- > 0;) { Bytes b(in.u64()); in.raw(b.data(), b.size()); c.a.push_back(std::move(b)); }
        if (!in.ok) { fprintf(stderr, "call %zu is cut short\n", done); return 2; }
        if (c.name != "combine") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_combine(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
        const uint32_t rc32 = (uint32_t)rc, na = (uint32_t)o.a.size();
        fwrite(&rc32, 4, 1, out); fwrite(&na, 4, 1, out);
        for (auto& b : o.a) { const uint64_t n = b.size(); fwrite(&n, 8, 1, out); if (n) fwrite(b.data(), 1, n, out); }
        fflush(out);
        if (rc != 0) { fprintf(stderr, "call %zu (%s) failed: nothing after it is run\n", done, c.name.c_str()); fclose(out); return 1; }
        done++;
    }
    fclose(out);
    fclose(in.f);
    ac_release_memory();
    printf("combine_bounds_check: %zu calls OK\n", done);
    return 0;
}
