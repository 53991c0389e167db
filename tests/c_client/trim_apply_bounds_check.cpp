// Bounds check of kernels_trim_apply.inc and of the subset stages it feeds: the CPU emulation (-DAC_EMU) linked into this stand-alone program
// under the address and undefined-behaviour sanitizers, with the guarded arena of csrc/device_rt.hpp (-DAC_ARENA_GUARD=1|2), from the per-level
// objects that `make kernel_bounds_check` builds.  `make trim_apply_bounds_check` in autocycler_amd/csrc builds it;
// tests/test_trim_apply_bounds_emu.py builds it the same way and feeds it.  CPU only.
//
//   trim_apply_bounds_check CALLS RESULTS      replays a call file in the format of kernel_bounds_check.cpp (tests/bounds_cases.py: Calls) and
//                                              writes every call's outputs to RESULTS; stops at the first call that fails
// The one entry, "trim_apply":
//   s: n_unitigs, n_links, n_seqs, chosen (AC_TRIM_CHOOSE_*), mad (the bits of the double), texts (0: none, 1: the finished graph's text too)
//   a: links, unitig_len u32, alive u8 (or empty), path entries i32, path_off u64, seq_length u32, results (ac_trim_result, or empty),
//      seq_bytes u8, seq_begin u64
//   out: records (ac_trimmed_record) | alive unitigs u32 | positions u32 | links | the text (ids 1.., file names hand_<s % 3>.fasta, headers
//        contig_<s>) | the yaml | u64 {launches, read_backs, median, mad, min_length, max_length, chosen}
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

static int do_trim_apply(const Call& c, Out& o) {
    const uint32_t n = (uint32_t)c.s.at(0), n_seqs = (uint32_t)c.s.at(2), chosen = (uint32_t)c.s.at(3);
    const uint64_t n_links = (uint64_t)c.s.at(1);
    double mad; const int64_t bits = c.s.at(4); memcpy(&mad, &bits, 8);
    const int texts = (int)c.s.at(5);
    ac_trimmed* h = nullptr;
    TRY(ac_trim_apply(n, arr<ac_link>(c, 0), n_links, arr<uint32_t>(c, 1), arr<uint8_t>(c, 2), nullptr, arr<int32_t>(c, 3), arr<uint64_t>(c, 4), arr<uint32_t>(c, 5), n_seqs,
                      arr<ac_trim_result>(c, 6), chosen, mad, 0, &h));
    const ac_trimmed_record* rec = nullptr; uint32_t nr = 0;
    TRY(ac_trimmed_records(h, &rec, &nr));
    o.put(rec, (size_t)nr * sizeof *rec);
    const ac_subsets* sub = ac_trimmed_subsets(h);
    const uint64_t* off = nullptr; const uint32_t* unitigs = nullptr; const uint32_t* fwd = nullptr;
    TRY(ac_subsets_unitigs(sub, &off, &unitigs, &fwd, nullptr));
    o.put(unitigs, (size_t)off[1] * 4); o.put(fwd, (size_t)off[1] * 4);
    const ac_link* links = nullptr;
    TRY(ac_subsets_links(sub, &off, &links));
    o.put(links, (size_t)off[1] * sizeof *links);
    if (texts) {
        ac_finished* f = nullptr;
        TRY(ac_trimmed_finish(h, arr<uint8_t>(c, 7), arr<uint64_t>(c, 8), 0, &f));
        std::vector<uint16_t> ids; std::vector<uint32_t> lengths; std::vector<std::string> fn, hd; std::vector<const char*> fnp, hdp;
        for (uint32_t s = 0; s < nr; s++)
            if (!rec[s].excluded) { ids.push_back((uint16_t)(s + 1)); lengths.push_back((uint32_t)rec[s].length); fn.push_back("hand_" + std::to_string(s % 3) + ".fasta"); hd.push_back("contig_" + std::to_string(s)); }
        for (size_t i = 0; i < fn.size(); i++) { fnp.push_back(fn[i].c_str()); hdp.push_back(hd[i].c_str()); }
        char* text = nullptr; uint64_t text_len = 0;
        TRY(ac_finished_gfa_string(f, 7, ids.data(), lengths.data(), fnp.data(), hdp.data(), nullptr, 0, &text, &text_len));
        o.put(text, (size_t)text_len);
        ac_string_free(text);
        ac_finished_free(f);
    } else o.put(nullptr, 0);
    char* yaml = nullptr; uint64_t yaml_len = 0;
    TRY(ac_trimmed_yaml_string(h, &yaml, &yaml_len));
    o.put(yaml, (size_t)yaml_len);
    ac_string_free(yaml);
    ac_trimmed_summary sm; memset(&sm, 0, sizeof sm);
    ac_trimmed_summary_get_sized(h, &sm, sizeof sm);
    const uint64_t counts[7] = {sm.launches, sm.read_backs, sm.median, sm.mad, sm.min_length, sm.max_length, sm.chosen};
    o.put(counts, sizeof counts);
    ac_trimmed_free(h);
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
        if (c.name != "trim_apply") { fprintf(stderr, "call %zu: no entry %s\n", done, c.name.c_str()); return 2; }
        Out o;
        int rc = 1;
        try { rc = do_trim_apply(c, o); } catch (const std::exception& e) { fprintf(stderr, "call %zu (%s): %s\n", done, c.name.c_str(), e.what()); }
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
    printf("trim_apply_bounds_check: %zu calls OK\n", done);
    return 0;
}
