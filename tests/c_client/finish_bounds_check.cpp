// Bounds check of kernels_finish.inc: the CPU emulation (-DAC_EMU) linked into this stand-alone program under the address and
// undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2), from the per-level objects that
// `make kernel_bounds_check` builds.  `make finish_bounds_check` in autocycler_amd/csrc builds it; tests/test_finish_bounds_emu.py builds it
// the same way and feeds it.  CPU only.
//
//   finish_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                          writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "finish":
//   s: n_unitigs, n_links, n_path_ends (pairs), renumber, n_seqs, n_clusters
//   a: links, unitig_len u32, alive u8 (or empty), depth f64 (or empty), type u8 (or empty), seq_bytes u8, seq_begin u64, path_ends i32,
//      path entries i32, path_off u64 (n_seqs + 1), labels u16
//   n_seqs == 0: ac_merge_plan_from_links, then ac_merge_finish without paths — one group of outputs
//   n_seqs > 0:  ac_subsets_from_paths, then per cluster its plan, its merged paths and ac_subsets_finish — one group per cluster
//   out, per group: unitig records | sequences | new_of_old u32 | links | path seq u32 | path_off u64 | path entries i32 | text |
//        u64 {launches, read_backs, tie_items}
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

static int put_finished(const Call& c, ac_finished* f, uint32_t cluster, Out& o) {
    const ac_finished_unitig* u = nullptr; uint32_t nu = 0;
    TRY(ac_finished_unitigs(f, &u, &nu));
    o.put(u, (size_t)nu * sizeof *u);
    const uint8_t* bytes = nullptr; uint64_t nb = 0;
    TRY(ac_finished_sequences(f, &bytes, &nb));
    o.put(bytes, (size_t)nb);
    const uint32_t* printed = nullptr; uint64_t np = 0;
    TRY(ac_finished_new_of_old(f, &printed, &np));
    o.put(printed, (size_t)np * 4);
    const ac_link* links = nullptr; uint64_t nl = 0;
    TRY(ac_finished_links(f, &links, &nl));
    o.put(links, (size_t)nl * sizeof *links);
    const uint32_t* pseq = nullptr; uint32_t n_pseq = 0; const uint64_t* poff = nullptr; const int32_t* pent = nullptr;
    TRY(ac_finished_paths(f, &pseq, &n_pseq, &poff, &pent));
    o.put(pseq, (size_t)n_pseq * 4); o.put(poff, ((size_t)n_pseq + 1) * 8); o.put(pent, (size_t)poff[n_pseq] * 4);
    // the text, with one record per P line in exact blocks
    std::vector<uint16_t> ids(n_pseq); std::vector<uint32_t> lens(n_pseq), tags(n_pseq, cluster);
    std::vector<std::string> names(n_pseq); std::vector<const char*> fn(n_pseq), hd(n_pseq);
    for (uint32_t i = 0; i < n_pseq; i++) { ids[i] = (uint16_t)(pseq[i] + 1); lens[i] = 100 + pseq[i]; names[i] = "seq_" + std::to_string(pseq[i]); fn[i] = hd[i] = names[i].c_str(); }
    char* text = nullptr; uint64_t len = 0;
    TRY(ac_finished_gfa_string(f, 5, ids.data(), lens.data(), fn.data(), hd.data(), tags.data(), 1, &text, &len));
    o.put(text, (size_t)len);
    ac_string_free(text);
    ac_finished_summary sm; memset(&sm, 0, sizeof sm);
    ac_finished_summary_get_sized(f, &sm, sizeof sm);
    const uint64_t counts[3] = {sm.launches, sm.read_backs, sm.tie_items};
    o.put(counts, sizeof counts);
    return 0;
}

static int do_finish(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), n_ends = (uint32_t)c.s.at(2), n_seqs = (uint32_t)c.s.at(4), nc = (uint32_t)c.s.at(5);
    const uint64_t n_links = (uint64_t)c.s.at(1);
    const int renumber = (int)c.s.at(3);
    static const uint32_t no_len = 0; static const uint16_t no_label = 0;
    const uint32_t* len = n ? arr<uint32_t>(c, 1) : &no_len;
    if (n_seqs == 0) {
        ac_merge* plan = nullptr;
        TRY(ac_merge_plan_from_links(n, arr<ac_link>(c, 0), n_links, len, arr<uint8_t>(c, 2), arr<int32_t>(c, 7), n_ends, arr<double>(c, 3), nullptr, nullptr,
                                     arr<uint8_t>(c, 4), arr<uint8_t>(c, 5), arr<uint64_t>(c, 6), 0, &plan));
        ac_finished* f = nullptr;
        TRY(ac_merge_finish(plan, n, arr<ac_link>(c, 0), n_links, len, arr<uint8_t>(c, 2), arr<double>(c, 3), arr<uint8_t>(c, 4), arr<uint8_t>(c, 5), arr<uint64_t>(c, 6),
                            nullptr, renumber, 0, &f));
        const int rc = put_finished(c, f, 0, o);
        ac_finished_free(f);
        ac_merge_free(plan);
        return rc;
    }
    const uint16_t* labels = arr<uint16_t>(c, 10) ? arr<uint16_t>(c, 10) : &no_label;
    ac_subsets* s = nullptr;
    TRY(ac_subsets_from_paths(n, arr<ac_link>(c, 0), n_links, len, arr<uint8_t>(c, 2), arr<int32_t>(c, 8), arr<uint64_t>(c, 9), n_seqs, labels, nc, 0, &s));
    for (uint32_t cl = 1; cl <= nc; cl++) {
        ac_merge* plan = nullptr;
        TRY(ac_subsets_merge_plan(s, cl, arr<uint8_t>(c, 5), arr<uint64_t>(c, 6), 1, 0, &plan));
        ac_merged_paths* mp = nullptr;
        TRY(ac_subsets_merged_paths(s, cl, plan, 0, &mp));
        ac_finished* f = nullptr;
        TRY(ac_subsets_finish(s, cl, plan, mp, arr<uint8_t>(c, 5), arr<uint64_t>(c, 6), renumber, 0, &f));
        const int rc = put_finished(c, f, cl, o);
        ac_finished_free(f);
        ac_merged_paths_free(mp);
        ac_merge_free(plan);
        if (rc) return rc;
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
        if (c.name != "finish") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_finish(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
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
    printf("finish_bounds_check: %zu calls OK\n", done);
    return 0;
}
