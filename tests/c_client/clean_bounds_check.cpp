// Bounds check of kernels_clean.inc: the CPU emulation (-DAC_EMU) linked into this stand-alone program under the address and
// undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2), from the per-level objects that
// `make kernel_bounds_check` builds.  `make clean_bounds_check` in autocycler_amd/csrc builds it; tests/test_clean_bounds_emu.py builds it
// the same way and feeds it.  CPU only.
//
//   clean_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                         writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "clean":
//   s: n_unitigs, n_links, n_remove, n_duplicate, has_min_depth, min_depth (the bits of the double), texts (0: none, 1: the edited graph's,
//      2: the merged graph's too)
//   a: links, unitig_len u32, depth f64 (or empty), type u8 (or empty), alive u8 (or empty), seq_bytes u8, seq_begin u64, remove u32, duplicate u32
//   out: len u32 | alive u8 | depth f64 | type u8 | copy_of u32 | reason u8 | links | seq_begin u64 | the edited graph's text | the merged
//        graph's text (ac_cleaned_merge_plan, ac_cleaned_finish with renumber = 1, use_other_colour) | u64 {rounds, launches, read_backs}
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

static int do_clean(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), n_remove = (uint32_t)c.s.at(2), n_duplicate = (uint32_t)c.s.at(3);
    const uint64_t n_links = (uint64_t)c.s.at(1);
    const int has_min = (int)c.s.at(4);
    double min_depth; const int64_t bits = c.s.at(5); memcpy(&min_depth, &bits, 8);
    const int texts = (int)c.s.at(6);
    static const uint32_t no_len = 0;
    const uint32_t* len = n ? arr<uint32_t>(c, 1) : &no_len;
    ac_cleaned* h = nullptr;
    TRY(ac_clean_graph(n, arr<ac_link>(c, 0), n_links, len, arr<double>(c, 2), arr<uint8_t>(c, 3), arr<uint8_t>(c, 4), arr<uint8_t>(c, 5), arr<uint64_t>(c, 6),
                       arr<uint32_t>(c, 7), n_remove, arr<uint32_t>(c, 8), n_duplicate, has_min, min_depth, 0, &h));
    uint32_t n_out = 0; const uint32_t* ulen = nullptr; const uint8_t* alive = nullptr; const double* depth = nullptr; const uint8_t* type = nullptr;
    const uint64_t* seq_begin = nullptr; const uint32_t* copy_of = nullptr; const uint8_t* reason = nullptr;
    TRY(ac_cleaned_unitigs(h, &n_out, &ulen, &alive, &depth, &type, &seq_begin, &copy_of, &reason));
    o.put(ulen, (size_t)n_out * 4); o.put(alive, n_out); o.put(depth, (size_t)n_out * 8); o.put(type, n_out); o.put(copy_of, (size_t)n_out * 4); o.put(reason, n_out);
    const ac_link* links = nullptr; uint64_t nl = 0;
    TRY(ac_cleaned_links(h, &links, &nl));
    o.put(links, (size_t)nl * sizeof *links);
    o.put(seq_begin, (size_t)n_out * 8);
    char* text = nullptr; uint64_t text_len = 0;
    if (texts >= 1) {
        TRY(ac_cleaned_gfa_string(h, 7, 1, &text, &text_len));
        o.put(text, (size_t)text_len);
        ac_string_free(text);
    } else o.put(nullptr, 0);
    if (texts >= 2) {
        ac_merge* plan = nullptr;
        TRY(ac_cleaned_merge_plan(h, 1, 0, &plan));
        ac_finished* f = nullptr;
        TRY(ac_cleaned_finish(h, plan, 1, 0, &f));
        TRY(ac_finished_gfa_string(f, 7, nullptr, nullptr, nullptr, nullptr, nullptr, 1, &text, &text_len));
        o.put(text, (size_t)text_len);
        ac_string_free(text);
        ac_finished_free(f);
        ac_merge_free(plan);
    } else o.put(nullptr, 0);
    ac_cleaned_summary sm; memset(&sm, 0, sizeof sm);
    ac_cleaned_summary_get_sized(h, &sm, sizeof sm);
    const uint64_t counts[3] = {sm.rounds, sm.launches, sm.read_backs};
    o.put(counts, sizeof counts);
    ac_cleaned_free(h);
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
        if (c.name != "clean") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_clean(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
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
    printf("clean_bounds_check: %zu calls OK\n", done);
    return 0;
}
