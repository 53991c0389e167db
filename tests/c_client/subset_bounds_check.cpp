// Bounds check of kernels_subset.inc: the CPU emulation (-DAC_EMU) linked into this stand-alone program under the address and
// undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2), from the per-level objects that
// `make kernel_bounds_check` builds.  `make subset_bounds_check` in autocycler_amd/csrc builds it; tests/test_subset_bounds_emu.py builds it
// the same way and feeds it.  CPU only.
//
//   subset_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                          writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "subsets":
//   s: n_unitigs, n_links, n_seqs, n_clusters, merge (1: also the merge plan and the merged paths of every cluster)
//   a: links, unitig_len u32, alive u8 (or empty), path entries i32, path_off u64 (n_seqs + 1), labels u16
//   out: records | unitig_off | unitigs | fwd | rev | link_off | links | seq_off | seq_index | ends_off | path_ends | u64 {launches, read_backs}
//        then with merge, per cluster: chain members i32 | merged path_off u64 | merged entries i32
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

static int do_subsets(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), n_seqs = (uint32_t)c.s.at(2), nc = (uint32_t)c.s.at(3);
    const uint64_t n_links = (uint64_t)c.s.at(1);
    const int merge = (int)c.s.at(4);
    static const uint32_t no_len = 0; static const uint16_t no_label = 0;
    const uint32_t* len = n ? arr<uint32_t>(c, 1) : &no_len;
    const uint16_t* labels = n_seqs ? arr<uint16_t>(c, 5) : &no_label;
    ac_subsets* s = nullptr;
    TRY(ac_subsets_from_paths(n, arr<ac_link>(c, 0), n_links, len, arr<uint8_t>(c, 2), arr<int32_t>(c, 3), arr<uint64_t>(c, 4), n_seqs, labels, nc, 0, &s));
    const ac_subset_cluster* rec = nullptr; uint32_t got_nc = 0;
    TRY(ac_subsets_records(s, &rec, &got_nc));
    o.put(rec, (size_t)got_nc * sizeof *rec);
    const uint64_t* off = nullptr; const uint32_t *unitigs = nullptr, *fwd = nullptr, *rev = nullptr;
    TRY(ac_subsets_unitigs(s, &off, &unitigs, &fwd, &rev));
    o.put(off, ((size_t)nc + 1) * 8); o.put(unitigs, (size_t)off[nc] * 4); o.put(fwd, (size_t)off[nc] * 4); o.put(rev, (size_t)off[nc] * 4);
    const ac_link* links = nullptr;
    TRY(ac_subsets_links(s, &off, &links));
    o.put(off, ((size_t)nc + 1) * 8); o.put(links, (size_t)off[nc] * sizeof *links);
    const uint32_t* seq_index = nullptr;
    TRY(ac_subsets_seqs(s, &off, &seq_index));
    o.put(off, ((size_t)nc + 1) * 8); o.put(seq_index, (size_t)off[nc] * 4);
    const int32_t* ends = nullptr;
    TRY(ac_subsets_path_ends(s, &off, &ends));
    o.put(off, ((size_t)nc + 1) * 8); o.put(ends, (size_t)off[nc] * 8);
    ac_subsets_summary sm; memset(&sm, 0, sizeof sm);
    ac_subsets_summary_get_sized(s, &sm, sizeof sm);
    const uint64_t counts[2] = {sm.launches, sm.read_backs};
    o.put(counts, sizeof counts);
    for (uint32_t cl = 1; merge && cl <= nc; cl++) {
        {   // the densified arrays, exact blocks
            std::vector<uint8_t> alive(n); std::vector<uint32_t> f(n), r(n); std::vector<double> d(n);
            TRY(ac_subsets_dense(s, cl, alive.data(), f.data(), r.data(), d.data()));
        }
        ac_merge* plan = nullptr;
        TRY(ac_subsets_merge_plan(s, cl, nullptr, nullptr, 0, 0, &plan));
        const int32_t* members = nullptr; uint64_t n_members = 0;
        TRY(ac_merge_members(plan, &members, &n_members));
        o.put(members, (size_t)n_members * 4);
        ac_merged_paths* mp = nullptr;
        TRY(ac_subsets_merged_paths(s, cl, plan, 0, &mp));
        const uint32_t* mseq = nullptr; uint32_t n_mseq = 0; const uint64_t* moff = nullptr; const int32_t* ment = nullptr;
        TRY(ac_merged_paths_get(mp, &mseq, &n_mseq, &moff, &ment));
        o.put(moff, ((size_t)n_mseq + 1) * 8); o.put(ment, (size_t)moff[n_mseq] * 4);
        ac_merged_paths_free(mp);
        ac_merge_free(plan);
    }
    ac_subsets_free(s);
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
        if (c.name != "subsets") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_subsets(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
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
    printf("subset_bounds_check: %zu calls OK\n", done);
    return 0;
}
