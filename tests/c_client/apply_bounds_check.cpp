// Bounds check of kernels_apply.inc: the CPU emulation (-DAC_EMU) linked into this stand-alone program under the address and
// undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2), from the per-level objects that
// `make kernel_bounds_check` builds.  `make apply_bounds_check` in autocycler_amd/csrc builds it; tests/test_apply_bounds_emu.py builds it
// the same way and feeds it.  CPU only.
//
//   apply_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                         writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "apply":
//   s: n_unitigs, n_links, n_anchors, n_bridges, n_best, n_distinct_paths, bridge_depth (the bits of the double), texts (0 / 1)
//   a: links, unitig_len u32, alive u8 (or empty), depth f64 (or empty), anchors u32, seq_bytes u8, seq_begin u64, bridges (ac_bridge),
//      best paths i32, distinct entries i32, distinct offsets u64, multiplicities u32, apply u8
//   out: len u32 | alive u8 | depth f64 | type u8 | bridge_of u32 | links | bridge sequences | bridge offsets u64 | 3_bridged's text |
//        the merged graph's text (ac_applied_merge_plan, ac_applied_finish with renumber = 1; empty with texts = 0) |
//        u64 {launches, launches_components, read_backs, removed_no_anchor, removed_zero_depth}
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

static int do_apply(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), n_anchors = (uint32_t)c.s.at(2), n_bridges = (uint32_t)c.s.at(3);
    const uint64_t n_links = (uint64_t)c.s.at(1), n_best = (uint64_t)c.s.at(4), n_paths = (uint64_t)c.s.at(5);
    double bridge_depth; const int64_t bits = c.s.at(6); memcpy(&bridge_depth, &bits, 8);
    const bool texts = c.s.at(7) != 0;
    static const uint32_t no_len = 0; static const uint64_t no_off = 0;
    const uint32_t* len = n ? arr<uint32_t>(c, 1) : &no_len;
    const uint64_t* dist_off = arr<uint64_t>(c, 10) ? arr<uint64_t>(c, 10) : &no_off;
    ac_applied* a = nullptr;
    TRY(ac_apply_bridges(n, arr<ac_link>(c, 0), n_links, len, arr<uint8_t>(c, 2), arr<double>(c, 3), arr<uint32_t>(c, 4), n_anchors, arr<uint8_t>(c, 5), arr<uint64_t>(c, 6),
                         arr<ac_bridge>(c, 7), n_bridges, arr<int32_t>(c, 8), n_best, arr<int32_t>(c, 9), dist_off, arr<uint32_t>(c, 11), n_paths, arr<uint8_t>(c, 12),
                         bridge_depth, 0, &a));
    uint32_t n_total = 0; const uint32_t* ulen = nullptr; const uint8_t* alive = nullptr; const double* depth = nullptr; const uint8_t* type = nullptr;
    TRY(ac_applied_unitigs(a, &n_total, &ulen, &alive, &depth, &type));
    o.put(ulen, (size_t)n_total * 4); o.put(alive, n_total); o.put(depth, (size_t)n_total * 8); o.put(type, n_total);
    const uint32_t* bridge_of = nullptr; uint32_t nq = 0;
    TRY(ac_applied_bridge_of(a, &bridge_of, &nq));
    o.put(bridge_of, (size_t)nq * 4);
    const ac_link* links = nullptr; uint64_t nl = 0;
    TRY(ac_applied_links(a, &links, &nl));
    o.put(links, (size_t)nl * sizeof *links);
    const uint8_t* bytes = nullptr; const uint64_t* off = nullptr; uint64_t nb = 0;
    TRY(ac_applied_bridge_sequences(a, &bytes, &off, &nb));
    o.put(bytes, (size_t)nb); o.put(off, ((size_t)nq + 1) * 8);
    char* text = nullptr; uint64_t text_len = 0;
    TRY(ac_applied_gfa_string(a, 7, 0, &text, &text_len));
    o.put(text, (size_t)text_len);
    ac_string_free(text);
    if (texts) {
        ac_merge* plan = nullptr;
        TRY(ac_applied_merge_plan(a, 1, 0, &plan));
        ac_finished* f = nullptr;
        TRY(ac_applied_finish(a, plan, 1, 0, &f));
        TRY(ac_finished_gfa_string(f, 7, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &text, &text_len));
        o.put(text, (size_t)text_len);
        ac_string_free(text);
        ac_finished_free(f);
        ac_merge_free(plan);
    } else o.put(nullptr, 0);
    ac_applied_summary sm; memset(&sm, 0, sizeof sm);
    ac_applied_summary_get_sized(a, &sm, sizeof sm);
    const uint64_t counts[5] = {sm.launches, sm.launches_components, sm.read_backs, sm.removed_no_anchor, sm.removed_zero_depth};
    o.put(counts, sizeof counts);
    ac_applied_free(a);
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
        if (c.name != "apply") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_apply(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
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
    printf("apply_bounds_check: %zu calls OK\n", done);
    return 0;
}
