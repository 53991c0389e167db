// finish_host.cpp on its own (no library, no device), with gfa_writer.cpp for the text: the input checks of finish_check_inputs and their
// texts, finish_check_result's refusal of arrays that do not fit together, finish_empty, and save_gfa's text with explicit numbers, colour
// tags, -0.0 and the CL:i tag.  A stand-alone program, so that it can be built with -fsanitize=address,undefined
// (tests/test_finish_bounds_emu.py does).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

#include "finish_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// five unitigs; 2 -> 3 is a chain (number 6), unitig 5 is dead
static MergeResult plan_of_five() {
    MergeResult p;
    p.n_unitigs = 5; p.links_in = 4;
    MergeChainRecord c; memset(&c, 0, sizeof c);
    c.number = 6; c.members = 2; c.length = 5; c.member_off = 0; c.seq_off = 0; c.depth = 2.5; c.type = MERGE_TYPE_CONSENTIG;
    p.chains.push_back(c);
    p.members = {2, 3};
    p.chain_of = {MERGE_NOT_MERGED, 0, 0, MERGE_NOT_MERGED, MERGE_NOT_MERGED};
    p.seq = {'A', 'C', 'G', 'T', 'A'};
    p.links = {Link{1, 6}, Link{-6, -1}};
    p.unitigs_after = 3;
    return p;
}
static const uint32_t LEN[] = {3, 2, 3, 1, 4};
static const uint8_t ALIVE[] = {1, 1, 1, 1, 0};
static const uint8_t SEQ[] = "AAACCGGGTCCCC";
static const uint64_t BEGIN[] = {0, 3, 5, 8, 9};

static std::string check_error(const MergeResult& p, FinishArrays a, bool renumber) {
    try { finish_check_inputs(p, a, renumber); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

int main() {
    const MergeResult plan = plan_of_five();
    FinishArrays a;
    a.n_unitigs = 5; a.unitig_len = LEN; a.alive = ALIVE; a.seq_bytes = SEQ; a.seq_begin = BEGIN; a.n_links = 4;
    CHECK(finish_check_inputs(plan, a, true) == 3);
    {   // the refusals, one at a time
        FinishArrays b = a; b.n_unitigs = 4;
        CHECK(has(check_error(plan, b, false), "the plan is over 5 unitigs, the call over 4"));
        b = a; b.n_links = 5;
        CHECK(has(check_error(plan, b, false), "the plan was made from 4 links, the call gives 5"));
        b = a; b.unitig_len = nullptr;
        CHECK(has(check_error(plan, b, false), "null pointer: unitig_len"));
        b = a; b.seq_begin = nullptr;
        CHECK(has(check_error(plan, b, false), "both or neither"));
        b = a; b.seq_begin = nullptr; b.seq_bytes = nullptr;
        CHECK(has(check_error(plan, b, false), "missing sequences: seq_bytes and seq_begin are needed (the unmerged unitigs have 4 bases)"));
        b = a; b.alive = nullptr;
        CHECK(has(check_error(plan, b, false), "4 unitigs are left, the plan has 3: it was made from another alive mask"));
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const double depth[] = {1.0, nan, nan, nan, nan};      // (merged members and dead unitigs take no part)
        b = a; b.depth = depth;
        CHECK(has(check_error(plan, b, true), "the depth of unitig 4 is NaN"));
        CHECK(check_error(plan, b, false).empty());      // without renumbering nothing compares depths
        MergeResult p2 = plan_of_five();
        p2.chains[0].depth = nan;
        CHECK(has(check_error(p2, a, true), "the depth of merged unitig 6 is NaN"));
        p2 = plan_of_five(); p2.seq.clear();
        CHECK(has(check_error(p2, a, false), "missing sequences: the plan was made without them (merged unitig 6 has 5 bases)"));
        p2 = plan_of_five(); p2.chains[0].seq_off = 1;
        CHECK(has(check_error(p2, a, false), "missing sequences"));
        p2 = plan_of_five(); p2.chain_of.pop_back();
        CHECK(has(check_error(p2, a, false), "contradict each other"));
    }
    // ---- a result as the device would return it, renumbered: 6 (5 bases), 1 (3 bases), 4 (1 base)
    FinishResult r;
    finish_empty(&r, true);
    CHECK(r.renumbered && r.path_off.size() == 1 && r.unitigs.empty());
    r.n_unitigs = 5; r.n_chains = 1;
    auto rec = [](uint32_t number, uint32_t source, uint64_t length, uint64_t off, double depth, uint8_t type) {
        FinishedUnitigRecord u; memset(&u, 0, sizeof u);
        u.number = number; u.source = source; u.length = length; u.seq_off = off; u.depth = depth; u.type = type;
        return u;
    };
    r.unitigs = {rec(1, 6, 5, 0, 2.5, MERGE_TYPE_CONSENTIG), rec(2, 1, 3, 5, -0.0, MERGE_TYPE_OTHER), rec(3, 4, 1, 8, 12.345, MERGE_TYPE_ANCHOR)};
    r.seq = {'A', 'C', 'G', 'T', 'A', 'A', 'A', 'A', 'T'};
    r.new_of_old = {2, 0, 0, 3, 0, 1};
    r.links = {Link{-1, -2}, Link{2, 1}};
    r.path_seq = {0, 2}; r.path_off = {0, 2, 3}; r.path_entries = {2, 1, -3};
    finish_check_result(r, plan, 3);
    {
        FinishResult bad = r; bad.links.pop_back();
        std::string what;
        try { finish_check_result(bad, plan, 3); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "1 links survive the merge, the plan has 2: the links are not the ones the plan was made from"));
        bad = r; bad.unitigs[1].seq_off = 4; what.clear();
        try { finish_check_result(bad, plan, 3); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "contradict each other"));
        bad = r; bad.new_of_old[0] = 3; what.clear();
        try { finish_check_result(bad, plan, 3); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "contradict each other"));
        bad = r; bad.seq.push_back('A'); what.clear();
        try { finish_check_result(bad, plan, 3); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "do not add up"));
        what.clear();
        try { finish_check_result(r, plan, 4); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "impossible sizes"));
    }
    // ---- the text
    std::vector<FinishSeqMeta> meta = {FinishSeqMeta{1, 8, "a.fasta", "contig_1 x", 4}, FinishSeqMeta{3, 1, "b.fasta", "contig_2", 0}};
    const std::string text = finish_gfa_string(r, 51, meta, false);
    const char* want =
        "H\tVN:Z:1.0\tKM:i:51\n"
        "S\t1\tACGTA\tDP:f:2.50\tCL:Z:steelblue\n"
        "S\t2\tAAA\tDP:f:-0.00\n"
        "S\t3\tT\tDP:f:12.35\tCL:Z:forestgreen\n"      // (12.345 is below the half in binary: 12.34 or 12.35 as printf says; checked below)
        "L\t1\t-\t2\t-\t0M\n"
        "L\t2\t+\t1\t+\t0M\n"
        "P\t1\t2+,1+\t*\tLN:i:8\tFN:Z:a.fasta\tHD:Z:contig_1 x\tCL:i:4\n"
        "P\t3\t3-\t*\tLN:i:1\tFN:Z:b.fasta\tHD:Z:contig_2\n";
    char depth_text[32];
    snprintf(depth_text, sizeof depth_text, "%.2f", 12.345);
    std::string expected = want;
    expected.replace(expected.find("12.35"), 5, depth_text);
    CHECK(text == expected);
    CHECK(has(finish_gfa_string(r, 51, meta, true), "S\t2\tAAA\tDP:f:-0.00\tCL:Z:orangered\n"));
    {
        std::string what;
        meta.pop_back();
        try { finish_gfa_string(r, 51, meta, false); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "1 sequence records for 2 P lines"));
    }
    CHECK(has(finish_nan_depth_message(7, false), "unitig 7") && has(finish_bad_path_entry_message(3, -9), "path entry 3 (-9)"));
    if (failures) { printf("finish_host_check: %d FAILED\n", failures); return 1; }
    printf("finish_host_check: OK\n");
    return 0;
}
