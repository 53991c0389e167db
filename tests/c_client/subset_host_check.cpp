// subset_host.cpp on its own (no library, no device): the label and offset checks of subset_prepare with the sequence lists, path ends and
// the layout of the kept entries it makes; subset_finish's records and its refusal of arrays that do not fit together; subset_dense;
// subset_locate across sequences without entries; the error texts.  A stand-alone program, so that it can be built with
// -fsanitize=address,undefined (tests/test_subset_emu.py does).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "subset_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static std::string prepare_error(uint32_t n_seqs, const int32_t* path, const uint64_t* off, const uint16_t* labels, uint32_t nc) {
    SubsetPlan plan; SubsetResult r;
    try { subset_prepare(n_seqs, path, off, labels, nc, &plan, &r); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// five sequences over six unitigs, three clusters: 1 = {0, 3}, 2 = {}, 3 = {1 (empty path), 4}; sequence 2 is dropped
static const int32_t PATH[] = {1, 2, -3, /* 1: none */ 6, 6, /* 3 */ -3, 2, /* 4 */ 5};
static const uint64_t OFF[] = {0, 3, 3, 5, 7, 8};
static const uint16_t LABELS[] = {1, 3, 0, 1, 3};

int main() {
    // ---- subset_prepare
    SubsetPlan plan; SubsetResult r;
    r.n_unitigs = 6;
    subset_prepare(5, PATH, OFF, LABELS, 3, &plan, &r);
    CHECK((plan.kept_seq == std::vector<uint32_t>{0, 3, 1, 4}) && (plan.kept_label == std::vector<uint32_t>{1, 1, 3, 3}));
    CHECK((plan.kept_off == std::vector<uint64_t>{0, 3, 5, 5, 6}) && plan.kept_entries() == 6 && r.kept_entries == 6);
    CHECK((r.seq_off == std::vector<uint64_t>{0, 2, 2, 4}) && (r.seq_index == std::vector<uint32_t>{0, 3, 1, 4}));
    CHECK((r.ends_off == std::vector<uint64_t>{0, 2, 2, 3}) && (r.path_ends == std::vector<int32_t>{1, -3, -3, 2, 5, 5}));
    CHECK(r.n_clusters == 3 && r.n_seqs == 5);
    {   // no sequence at all, and every label 0
        SubsetPlan p2; SubsetResult r2;
        const uint64_t off0[] = {0};
        subset_prepare(0, nullptr, off0, LABELS, 2, &p2, &r2);
        CHECK(p2.kept_entries() == 0 && p2.kept_off.size() == 1 && r2.seq_off.size() == 3 && r2.path_ends.empty());
        const uint16_t zeros[] = {0, 0, 0, 0, 0};
        subset_prepare(5, PATH, OFF, zeros, 1, &p2, &r2);
        CHECK(p2.kept_seq.empty() && p2.kept_entries() == 0 && (r2.seq_off == std::vector<uint64_t>{0, 0}));
    }
    // the refusals, by their texts
    CHECK(has(prepare_error(5, PATH, OFF, LABELS, 2), "sequence 1 has label 3, above n_clusters = 2"));
    CHECK(has(prepare_error(5, PATH, OFF, LABELS, 0), "n_clusters is 0: it must be between 1 and 65535"));
    CHECK(has(prepare_error(5, PATH, OFF, LABELS, 65536), "n_clusters is 65536"));
    CHECK(prepare_error(5, PATH, OFF, LABELS, 65535).empty());
    CHECK(has(prepare_error(5, PATH, nullptr, LABELS, 3), "null pointer: path_off"));
    CHECK(has(prepare_error(5, PATH, OFF, nullptr, 3), "null pointer: cluster_of_seq"));
    CHECK(has(prepare_error(5, nullptr, OFF, LABELS, 3), "null pointer: path_entries"));
    {
        const uint64_t bad[] = {0, 3, 2, 5, 7, 8};
        CHECK(has(prepare_error(5, PATH, bad, LABELS, 3), "path_off decreases at sequence 1 (3 then 2)"));
    }
    // ---- subset_locate: entry 5 is the one entry of sequence 4, behind sequence 1, which has none
    {
        uint32_t seq = 9; uint64_t index = 9;
        subset_locate(plan, 0, &seq, &index); CHECK(seq == 0 && index == 0);
        subset_locate(plan, 2, &seq, &index); CHECK(seq == 0 && index == 2);
        subset_locate(plan, 3, &seq, &index); CHECK(seq == 3 && index == 0);
        subset_locate(plan, 4, &seq, &index); CHECK(seq == 3 && index == 1);
        subset_locate(plan, 5, &seq, &index); CHECK(seq == 4 && index == 0);
    }
    // ---- subset_finish on what the device would return: cluster 1 keeps 1, 2 and 3 (2 and 3 twice); cluster 3 keeps 5
    auto filled = [&] {
        SubsetResult x = r;
        x.unitig_off = {0, 3, 3, 4}; x.unitigs = {1, 2, 3, 5}; x.positions = {1, 2, 2, 1};
        x.length_at = {0, 10 + 20 + 30, 60, 110};
        x.link_off = {0, 2, 2, 2}; x.links = {Link{1, 2}, Link{-2, -1}};
        return x;
    };
    {
        SubsetResult x = filled();
        subset_finish(&x, plan);
        CHECK(x.records.size() == 3);
        CHECK(x.records[0].seqs == 2 && x.records[0].unitigs == 3 && x.records[0].entries == 5 && x.records[0].links == 2 && x.records[0].length == 60);
        CHECK(x.records[1].seqs == 0 && x.records[1].unitigs == 0 && x.records[1].entries == 0 && x.records[1].links == 0 && x.records[1].length == 0);
        CHECK(x.records[2].seqs == 2 && x.records[2].unitigs == 1 && x.records[2].entries == 1 && x.records[2].links == 0 && x.records[2].length == 50);
        // ---- subset_dense
        uint8_t alive[6]; uint32_t fwd[6], rev[6]; double depth[6];
        subset_dense(x, 1, alive, fwd, rev, depth);
        const uint8_t want_alive[6] = {1, 1, 1, 0, 0, 0}; const uint32_t want[6] = {1, 2, 2, 0, 0, 0};
        CHECK(!memcmp(alive, want_alive, 6) && !memcmp(fwd, want, sizeof want) && !memcmp(rev, want, sizeof want));
        for (int u = 0; u < 6; u++) CHECK(depth[u] == (double)want[u]);
        subset_dense(x, 2, alive, nullptr, nullptr, depth);
        for (int u = 0; u < 6; u++) CHECK(alive[u] == 0 && depth[u] == 0.0);
        subset_dense(x, 3, nullptr, fwd, nullptr, nullptr);
        CHECK(fwd[4] == 1 && fwd[0] == 0);
        for (uint32_t c : {0u, 4u}) {
            std::string text;
            try { subset_dense(x, c, alive, fwd, rev, depth); } catch (const std::runtime_error& e) { text = e.what(); }
            CHECK(has(text, "does not exist: clusters run from 1 to 3"));
        }
    }
    auto finish_throws = [&](SubsetResult x) {
        try { subset_finish(&x, plan); } catch (const std::runtime_error&) { return true; }
        return false;
    };
    { SubsetResult x = filled(); x.positions[1] = 3; CHECK(finish_throws(x)); }                 // the counts do not add up to the entries
    { SubsetResult x = filled(); x.unitig_off = {0, 3, 2, 4}; CHECK(finish_throws(x)); }        // descending offsets
    { SubsetResult x = filled(); x.links.pop_back(); CHECK(finish_throws(x)); }                 // links that do not fit their offsets
    { SubsetResult x = filled(); x.unitigs.pop_back(); CHECK(finish_throws(x)); }
    { SubsetResult x = filled(); x.length_at.pop_back(); CHECK(finish_throws(x)); }
    {   // nothing kept: the empty products finish
        SubsetPlan p2; SubsetResult r2;
        const uint16_t zeros[] = {0, 0, 0, 0, 0};
        subset_prepare(5, PATH, OFF, zeros, 2, &p2, &r2);
        subset_empty_products(&r2);
        subset_finish(&r2, p2);
        CHECK(r2.records.size() == 2 && r2.records[0].seqs == 0 && r2.records[1].unitigs == 0);
    }
    // ---- the texts
    CHECK(subset_bad_entry_message(3, 7, -9, 8) == "subsets: entry 7 of the path of sequence 3 (-9) names no unitig: unitig numbers run from 1 to 8");
    CHECK(subset_dead_entry_message(3, 7, -9) == "subsets: entry 7 of the path of sequence 3 (-9) enters a unitig that is not alive in the input");
    CHECK(has(merged_paths_inside_message(2, true, -4, 11), "the path of sequence 2 begins strictly inside chain 11 (entry -4)"));
    CHECK(has(merged_paths_inside_message(2, false, 4, 11), "the path of sequence 2 ends strictly inside chain 11 (entry 4)"));
    CHECK(has(merged_paths_length_message(5), "the path of sequence 5 changes its length over the merged unitigs"));
    if (failures) { printf("subset_host_check: %d FAILED\n", failures); return 1; }
    printf("subset_host_check: OK\n");
    return 0;
}
