// clean_host.cpp on its own (no library, no device), with gfa_writer.cpp for the text: parse_tig_numbers, clean_prepare's refusals and their
// texts, the sequential duplication over gathered entries (a plain tig, a loop, a hairpin, two linked tigs, the refusals), the S-line types of a
// GFA text, clean_finish's counts and the edited graph's text.  A stand-alone program, so that it can be built with
// -fsanitize=address,undefined (tests/test_clean_bounds_emu.py does).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "clean_host.hpp"
#include "merge_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }
static bool same(const std::vector<Link>& got, std::initializer_list<Link> want) {
    if (got.size() != want.size()) return false;
    size_t i = 0;
    for (const Link& l : want) { if (got[i].a != l.a || got[i].b != l.b) return false; i++; }
    return true;
}
static std::string parse_error(const char* s) {
    try { clean_parse_tig_numbers(s); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
static std::string prepare_error(const CleanInput& in) {
    try { clean_prepare(in); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
static std::string edit_error(const CleanInput& in, const std::vector<Link>& gathered) {
    std::vector<Link> created;
    try { clean_duplicate_edit(in, gathered, &created); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

static const uint32_t LEN[] = {3, 2, 3, 1};
static const uint8_t SEQ[] = "AAACCGGGT";
static const uint64_t BEGIN[] = {0, 3, 5, 8};
static const Link LINKS[] = {{1, 2}, {2, 3}, {-2, -1}, {-3, -2}};

static CleanInput input() {
    CleanInput in;
    in.n_unitigs = 4; in.links = LINKS; in.n_links = 4; in.unitig_len = LEN; in.seq_bytes = SEQ; in.seq_begin = BEGIN; in.seq_total = 9;
    return in;
}

int main() {
    {   // parse_tig_numbers (clean.rs test_parse_tig_numbers and more)
        CHECK(clean_parse_tig_numbers(nullptr).empty());
        CHECK((clean_parse_tig_numbers("1,2,3") == std::vector<uint32_t>{1, 2, 3}));
        CHECK((clean_parse_tig_numbers("  5 , 10 ,15 ") == std::vector<uint32_t>{5, 10, 15}));
        CHECK((clean_parse_tig_numbers("9,+3,4294967295") == std::vector<uint32_t>{3, 9, 4294967295u}));
        CHECK(parse_error("") == "failed to parse '' as a node number");
        CHECK(parse_error("ABC") == "failed to parse 'ABC' as a node number");
        CHECK(parse_error("1,X,3") == "failed to parse 'X' as a node number");
        CHECK(parse_error("1,,3") == "failed to parse '' as a node number");
        CHECK(parse_error("4294967296") == "failed to parse '4294967296' as a node number");
        CHECK(parse_error("-1") == "failed to parse '-1' as a node number");
        CHECK(parse_error("+") == "failed to parse '+' as a node number");
        CHECK(parse_error("99999999999999999999999") == "failed to parse '99999999999999999999999' as a node number");
    }
    {   // clean_prepare's refusals, one at a time
        CHECK(prepare_error(input()).empty());
        CleanInput b = input(); b.seq_begin = nullptr;
        CHECK(has(prepare_error(b), "both or neither"));
        b = input(); b.unitig_len = nullptr;
        CHECK(has(prepare_error(b), "null pointer: unitig_len"));
        b = input(); b.n_remove = 1;
        CHECK(has(prepare_error(b), "n_remove > 0 without remove"));
        static const uint32_t FIVE[] = {5}, ZERO[] = {0}, DOWN[] = {3, 2}, TWICE[] = {2, 2}, THREE[] = {3};
        static const uint8_t ALIVE[] = {1, 1, 0, 1};
        b = input(); b.remove = FIVE; b.n_remove = 1; b.name = "in.gfa";
        CHECK(prepare_error(b) == "in.gfa does not contain tig 5");
        b = input(); b.duplicate = ZERO; b.n_duplicate = 1;
        CHECK(prepare_error(b) == "the graph does not contain tig 0");
        b = input(); b.remove = THREE; b.n_remove = 1; b.alive = ALIVE;
        CHECK(prepare_error(b) == "the graph does not contain tig 3");
        b = input(); b.remove = DOWN; b.n_remove = 2;
        CHECK(has(prepare_error(b), "must ascend"));
        b = input(); b.remove = TWICE; b.n_remove = 2;
        CHECK(prepare_error(b).empty());
        b = input(); b.n_unitigs = 0x7FFFFFFFu;
        CHECK(has(prepare_error(b), "more unitigs than a signed unitig number can name"));
    }
    {   // the duplication: 1 -> 2 -> 3, duplicate 2: copy 5 takes 2 -> 3, copy 6 takes 1 -> 2
        static const uint32_t TWO[] = {2};
        CleanInput in = input(); in.duplicate = TWO; in.n_duplicate = 1;
        std::vector<Link> created;
        clean_duplicate_edit(in, {LINKS, LINKS + 4}, &created);
        CHECK(same(created, {{5, 3}, {-3, -5}, {-6, -1}, {1, 6}}));
        // a loop is re-created from both strands' lists: twice per copy; the entries stand in creation order
        clean_duplicate_edit(in, {{1, 2}, {2, 2}, {2, 3}, {-2, -1}, {-2, -2}, {-3, -2}}, &created);
        CHECK(same(created, {{5, 5}, {-5, -5}, {6, 6}, {-6, -6}, {-5, -5}, {5, 5}, {-6, -6}, {6, 6}, {5, 3}, {-3, -5}, {-6, -1}, {1, 6}}));
        // a hairpin is its own mirror image: once per copy
        clean_duplicate_edit(in, {{1, 2}, {2, -2}, {3, 2}, {-2, -1}, {-2, -3}}, &created);
        CHECK(same(created, {{5, -5}, {6, -6}, {-5, -1}, {1, 5}, {-6, -3}, {3, 6}}));
        // the refusals
        CHECK(edit_error(in, {{1, 2}, {-2, -1}}) == "unitig 2 does not contain exactly two non-self links");
        CHECK(edit_error(in, {}) == "unitig 2 does not contain exactly two non-self links");
        static const uint32_t TWO_TWICE[] = {2, 2};
        in.duplicate = TWO_TWICE; in.n_duplicate = 2;
        CHECK(edit_error(in, {LINKS, LINKS + 4}) == "unitig 2 no longer exists: it was removed or duplicated earlier in the same call");
        in.duplicate = TWO; in.n_duplicate = 1; in.remove = TWO; in.n_remove = 1;
        CHECK(edit_error(in, {}) == "unitig 2 no longer exists: it was removed or duplicated earlier in the same call");
        // two linked tigs: duplicating 2 moves 3's entry for it to the end of 3's reverse list, and what it created for 3 goes when 3 is duplicated
        static const uint32_t TWO_THREE[] = {2, 3};
        static const Link CHAIN[] = {{1, 2}, {2, 3}, {-2, -1}, {3, 4}, {-3, -2}, {-4, -3}};
        in = input(); in.duplicate = TWO_THREE; in.n_duplicate = 2;
        clean_duplicate_edit(in, {CHAIN, CHAIN + 6}, &created);
        CHECK(same(created, {{-6, -1}, {1, 6}, {7, 4}, {-4, -7}, {-8, -5}, {5, 8}}));
    }
    {   // the S-line colours as types
        const std::string text = "H\tVN:Z:1.0\tKM:i:51\nS\t1\tACGT\tDP:f:1.00\tCL:Z:steelblue\nS\t2\tAC\tDP:f:2.00\nS\t3\tA\tDP:f:1.00\tCL:Z:pink\r\n"
                                 "S\t4\tA\tCL:Z:forestgreen\tDP:f:1.00\nS\t5\tA\tDP:f:1.00\tCL:Z:orangered\nL\t1\t+\t2\t+\t0M\nS\t6\tA\tDP:f:1.00\tCL:Z:pinkish";
        const std::vector<uint8_t> t = clean_gfa_types(text.data(), text.size());
        CHECK((t == std::vector<uint8_t>{MERGE_TYPE_CONSENTIG, MERGE_TYPE_OTHER, MERGE_TYPE_BRIDGE, MERGE_TYPE_ANCHOR, MERGE_TYPE_OTHER, MERGE_TYPE_OTHER}));
        CHECK(clean_gfa_types("", 0).empty());
        CHECK(clean_gfa_types(text.data(), 1).empty());
    }
    {   // the counts, the kept bytes and the text of an edited graph: 2 removed, copies of nothing
        CleanInput in = input();
        CleanResult r;
        r.n_unitigs = r.n_out = 4;
        r.len = {3, 2, 3, 1}; r.copy_of = {0, 0, 0, 0}; r.alive = {1, 0, 1, 1}; r.type = {0, 0, 3, 0}; r.reason = {CLEAN_KEPT, CLEAN_REMOVED, CLEAN_KEPT_DEAD_END, CLEAN_KEPT};
        r.depth = {1.0, 2.0, 0.5, 4.0}; r.seq_begin = {0, 3, 5, 8};
        clean_finish(in, &r);
        CHECK(r.count[CLEAN_KEPT] == 2 && r.count[CLEAN_REMOVED] == 1 && r.count[CLEAN_KEPT_DEAD_END] == 1 && r.count[CLEAN_LOW_DEPTH] == 0);
        CHECK(r.seq_all.size() == 10 && !memcmp(r.seq_all.data(), SEQ, 9));
        CHECK(clean_gfa_string(r, 9, true) == "H\tVN:Z:1.0\tKM:i:9\nS\t1\tAAA\tDP:f:1.00\tCL:Z:orangered\nS\t3\tGGG\tDP:f:0.50\tCL:Z:pink\nS\t4\tT\tDP:f:4.00\tCL:Z:orangered\n");
        in.seq_bytes = nullptr; in.seq_begin = nullptr;
        CleanResult bare = r; bare.seq_all.clear();
        clean_finish(in, &bare);
        std::string what;
        try { clean_gfa_string(bare, 9, true); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "missing sequences"));
        CleanResult none;
        clean_empty(&none);
        clean_finish(input(), &none);
        CHECK(none.n_out == 0 && none.seq_all.empty() && none.links.empty());
    }
    CHECK(has(clean_unordered_link_message(3, 1, 2, 2), "link entry 3 (1 -> 2) stands behind an entry that leaves 2"));
    if (failures) { printf("clean_host_check: %d FAILED\n", failures); return 1; }
    printf("clean_host_check: OK\n");
    return 0;
}
