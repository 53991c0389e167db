// merge_host.cpp on its own (no library, no device): the seeds of the fixed sets from path ends, the three depth rules of
// get_merge_path_depth (graph_simplification.rs:501-526) with the weighted mean as one sequential sum, the type rule, the totals of
// merge_finish and its refusal of arrays that do not fit together, the error texts.  A stand-alone program, so that it can be built with
// -fsanitize=address,undefined (tests/test_merge_emu.py does).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "merge_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static std::string seed_error(uint32_t n, const uint8_t* alive, std::vector<int32_t> ends) {
    std::vector<uint8_t> seed;
    try { merge_seed_fixed(n, alive, ends.data(), (uint32_t)(ends.size() / 2), &seed); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

// two chains over six unitigs: [1, -3] and [4, 5, -6]; unitig 2 stays
static MergeResult two_chains() {
    MergeResult r;
    r.n_unitigs = 6;
    r.chains.resize(2);
    r.chains[0].members = 2; r.chains[0].length = 10 + 30; r.chains[0].member_off = 0; r.chains[0].seq_off = 0;
    r.chains[1].members = 3; r.chains[1].length = 40 + 50 + 60; r.chains[1].member_off = 2; r.chains[1].seq_off = 40; r.chains[1].loop = 1;
    r.members = {1, -3, 4, 5, -6};
    r.chain_of = {0, MERGE_NOT_MERGED, 0, 1, 1, 1};
    r.fixed.assign(6, 0);
    return r;
}
static bool finish_throws(MergeResult r, const uint32_t* len) {
    try { merge_finish(&r, len, nullptr, nullptr, nullptr, nullptr, nullptr); } catch (const std::runtime_error&) { return true; }
    return false;
}

int main() {
    // ---- merge_seed_fixed: first entry + fixes the start, - the end; last entry + fixes the end, - the start
    {
        std::vector<uint8_t> seed;
        const int32_t ends[] = {1, 2, -3, -4, 5, 5, -6, 6};
        merge_seed_fixed(6, nullptr, ends, 4, &seed);
        CHECK(seed.size() == 6);
        CHECK(seed[0] == MERGE_FIXED_START && seed[1] == MERGE_FIXED_END && seed[2] == MERGE_FIXED_END && seed[3] == MERGE_FIXED_START);
        CHECK(seed[4] == (MERGE_FIXED_START | MERGE_FIXED_END) && seed[5] == MERGE_FIXED_END);
        merge_seed_fixed(3, nullptr, nullptr, 0, &seed);
        CHECK(seed.size() == 3 && seed[0] == 0 && seed[1] == 0 && seed[2] == 0);
        merge_seed_fixed(0, nullptr, nullptr, 0, &seed);
        CHECK(seed.empty());
        const uint8_t alive[] = {1, 0, 1};
        CHECK(seed_error(3, alive, {1, 3}).empty());
        CHECK(seed_error(3, alive, {1, -2}).find("last entry of sequence 0 (-2) names a unitig that is not alive") != std::string::npos);
        CHECK(seed_error(3, alive, {1, 3, 2, 3}).find("first entry of sequence 1 (2) names a unitig that is not alive") != std::string::npos);
        CHECK(seed_error(3, nullptr, {0, 1}).find("names no unitig") != std::string::npos);
        CHECK(seed_error(3, nullptr, {1, 4}).find("names no unitig: unitig numbers run from 1 to 3") != std::string::npos);
        CHECK(seed_error(3, nullptr, {-2147483647 - 1, 1}).find("names no unitig") != std::string::npos);
    }
    // ---- the depth rules
    const uint32_t len[] = {10, 20, 30, 40, 50, 60};
    const double depth[] = {1.5, 2.5, 0.1, 7.0, 0.3, 1e-3};
    {
        const int32_t path[] = {1, -3, 2};
        const uint32_t fwd[] = {4, 0, 0, 0, 0, 0}, rev[] = {0, 0, 9, 0, 0, 0};
        const uint8_t type[] = {MERGE_TYPE_OTHER, MERGE_TYPE_ANCHOR, MERGE_TYPE_ANCHOR, MERGE_TYPE_OTHER, MERGE_TYPE_BRIDGE, MERGE_TYPE_CONSENTIG};
        // rule 1: the first member's positions on its path strand
        CHECK(merge_path_depth(path, 3, len, depth, fwd, rev, type) == 4.0);
        const int32_t from_reverse[] = {-3, 1};
        CHECK(merge_path_depth(from_reverse, 2, len, depth, fwd, rev, type) == 9.0);
        // ... none on that strand: rule 2, the first anchor in path order
        const int32_t no_positions[] = {-1, -3, 2};
        CHECK(merge_path_depth(no_positions, 3, len, depth, fwd, rev, type) == 0.1);
        CHECK(merge_path_depth(path, 3, len, depth, nullptr, nullptr, type) == 0.1);
        const int32_t other_order[] = {1, 2, -3};
        CHECK(merge_path_depth(other_order, 3, len, depth, nullptr, nullptr, type) == 2.5);
        CHECK(merge_path_depth(other_order, 3, len, nullptr, nullptr, nullptr, type) == 0.0);
        // rule 3: the weighted mean, summed in path order (a bridge or consentig is no anchor)
        const int32_t tail[] = {4, 5, -6};
        double sum = 0.0;
        sum += 7.0 * 40.0; sum += 0.3 * 50.0; sum += 1e-3 * 60.0;
        CHECK(merge_path_depth(tail, 3, len, depth, nullptr, nullptr, type) == sum / 150.0);
        const int32_t tail_reversed[] = {6, -5, -4};
        double sum2 = 0.0;
        sum2 += 1e-3 * 60.0; sum2 += 0.3 * 50.0; sum2 += 7.0 * 40.0;
        CHECK(merge_path_depth(tail_reversed, 3, len, depth, nullptr, nullptr, type) == sum2 / 150.0);
        CHECK(merge_path_depth(tail, 3, len, depth, nullptr, nullptr, nullptr) == sum / 150.0);
        CHECK(merge_path_depth(tail, 3, len, nullptr, nullptr, nullptr, nullptr) == 0.0);
        CHECK(merge_path_depth(tail, 0, len, depth, nullptr, nullptr, nullptr) == 0.0);
        const uint32_t no_length[] = {0, 0, 0, 0, 0, 0};
        CHECK(std::isnan(merge_path_depth(tail, 3, no_length, depth, nullptr, nullptr, nullptr)));      // 0 / 0, as the reference computes it
        // ---- the type rule: Consentig if any member is Anchor or Consentig; a Bridge alone gives Other
        CHECK(merge_path_type(path, 3, type) == MERGE_TYPE_CONSENTIG);
        CHECK(merge_path_type(tail, 3, type) == MERGE_TYPE_CONSENTIG);
        const int32_t bridge_only[] = {4, 5, 1};
        CHECK(merge_path_type(bridge_only, 3, type) == MERGE_TYPE_OTHER);
        CHECK(merge_path_type(path, 3, nullptr) == MERGE_TYPE_OTHER);
    }
    // ---- merge_finish
    {
        MergeResult r = two_chains();
        const uint8_t alive[] = {1, 1, 1, 1, 1, 1};
        merge_finish(&r, len, alive, depth, nullptr, nullptr, nullptr);
        CHECK(r.chains[0].number == 7 && r.chains[1].number == 8);
        CHECK(r.alive == 6 && r.merged_unitigs == 5 && r.unitigs_after == 3 && r.bases_copied == 0);
        double s0 = 0.0; s0 += 1.5 * 10.0; s0 += 0.1 * 30.0;
        CHECK(r.chains[0].depth == s0 / 40.0 && r.chains[0].type == MERGE_TYPE_OTHER && r.chains[1].loop == 1);
        MergeResult with_seq = two_chains();
        with_seq.seq.assign(190, 'A');
        merge_finish(&with_seq, len, nullptr, depth, nullptr, nullptr, nullptr);
        CHECK(with_seq.bases_copied == 190 && with_seq.alive == 6);
        MergeResult bad = two_chains(); bad.seq.assign(189, 'A');
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chains[1].member_off = 3;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chains[1].seq_off = 41;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chains[0].length = 41;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chains[0].members = 1;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.members.push_back(2);
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.members[1] = 7;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.members[1] = 0;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chain_of[2] = 1;
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.chain_of.pop_back();
        CHECK(finish_throws(bad, len));
        bad = two_chains(); bad.members.resize(4);
        CHECK(finish_throws(bad, len));
        MergeResult empty;
        merge_finish(&empty, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        CHECK(empty.unitigs_after == 0 && empty.merged_unitigs == 0);
    }
    // ---- the error texts
    CHECK(merge_duplicate_link_message(3, -2, -1) == "link 3 (-2 -> -1) is a duplicate: the merge plan needs the links among alive unitigs as a set");
    CHECK(merge_unclosed_link_message(2, 2, 3).find("link 2 (2 -> 3) has no reverse complement (-3 -> -2)") == 0);
    CHECK(merge_unclosed_link_message(0, -2147483647 - 1, 1).find("(-1 -> 2147483648)") != std::string::npos);
    if (failures) { printf("merge_host_check: %d FAILED\n", failures); return 1; }
    printf("merge_host_check: OK\n");
    return 0;
}
