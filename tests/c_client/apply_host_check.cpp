// apply_host.cpp on its own (no library, no device), with gfa_writer.cpp for the text: apply_prepare's refusals and their texts, the numbering
// of the bridge unitigs and the layout of the work items, apply_finish's joined sequence array, apply_empty, the error texts and
// 3_bridged.gfa's text.  A stand-alone program, so that it can be built with -fsanitize=address,undefined
// (tests/test_apply_bounds_emu.py does).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "apply_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// four unitigs, anchors 1 and 2; bridge 0: 1 -> 2 over [3] (paths [3] twice, [4] once), bridge 1: 2 -> 1 direct, bridge 2: 1 -> -1 (status 2)
static const uint32_t LEN[] = {3, 2, 3, 1};
static const uint8_t SEQ[] = "AAACCGGGT";
static const uint64_t BEGIN[] = {0, 3, 5, 8};
static const uint32_t ANCHORS[] = {1, 2};
static const Link LINKS[] = {{1, 3}, {-3, -1}, {3, 2}, {-2, -3}, {2, 1}, {-1, -2}};
static const int32_t BEST[] = {3};
static const int32_t DIST[] = {3, 4};
static const uint64_t DIST_OFF[] = {0, 1, 2, 2};
static const uint32_t MULT[] = {2, 1, 3};
static const ApplyBridgeIn BRIDGES[] = {{1, 2, 0, 0, 1, 2, 0}, {2, 1, 1, 2, 0, 1, 0}, {1, -1, 1, 3, 0, 0, 2}};

static ApplyInput input(const uint8_t* apply) {
    ApplyInput in;
    in.n_unitigs = 4; in.links = LINKS; in.n_links = 6; in.unitig_len = LEN; in.anchors = ANCHORS; in.n_anchors = 2; in.seq_bytes = SEQ; in.seq_begin = BEGIN; in.seq_total = 9;
    in.bridges = BRIDGES; in.n_bridges = 3; in.apply = apply; in.best = BEST; in.n_best = 1; in.dist_entries = DIST; in.dist_off = DIST_OFF; in.dist_mult = MULT;
    in.n_dist_paths = 3; in.n_dist_entries = 2; in.bridge_depth = 3.0;
    return in;
}
static std::string prepare_error(const ApplyInput& in) {
    ApplyPlan plan;
    try { apply_prepare(in, &plan); } catch (const std::runtime_error& e) { return e.what(); }
    return "";
}

int main() {
    static const uint8_t FIRST_TWO[] = {1, 1, 0}, ALL[] = {1, 1, 1}, NONE[] = {0, 0, 0};
    const ApplyInput in = input(FIRST_TWO);
    ApplyPlan plan;
    apply_prepare(in, &plan);
    CHECK(plan.records.size() == 2 && plan.bridge_of.size() == 1 && plan.bridge_of[0] == 0 && plan.n_direct == 1);
    CHECK(plan.records[0].unitig == 0 && plan.records[0].created_off == 0 && plan.records[1].unitig == 0xFFFFFFFFu && plan.records[1].created_off == 4 && plan.n_created == 6);
    CHECK(plan.n_members == 1 && plan.q_begin.size() == 2 && plan.q_begin[1] == 1 && plan.q_best_off[0] == 0);
    CHECK(plan.n_visits == 2 && plan.vis_begin.size() == 3 && plan.vis_src[1] == 1 && plan.vis_mult[0] == 2 && plan.vis_mult[1] == 1);      // the direct link visits nothing
    {
        ApplyPlan none;
        apply_prepare(input(NONE), &none);
        CHECK(none.records.empty() && none.n_created == 0 && none.q_begin.size() == 1 && none.vis_begin.size() == 1);
    }
    {   // the refusals, one at a time
        CHECK(has(prepare_error(input(ALL)), "bridge 2 (1 -> -1) has status 2"));
        ApplyInput b = in; b.seq_begin = nullptr;
        CHECK(has(prepare_error(b), "both or neither"));
        b = in; b.unitig_len = nullptr;
        CHECK(has(prepare_error(b), "null pointer: unitig_len"));
        b = in; b.n_unitigs = 0x7FFFFFFFu;
        CHECK(has(prepare_error(b), "signed unitig number"));
        static const uint32_t one_anchor[] = {1}, unsorted[] = {2, 1}, beyond[] = {1, 9};
        b = in; b.anchors = one_anchor; b.n_anchors = 1;
        CHECK(has(prepare_error(b), "the end of bridge 0 (1 -> 2) is not among the anchors"));
        b = in; b.anchors = unsorted;
        CHECK(has(prepare_error(b), "the anchors must ascend"));
        b = in; b.anchors = beyond;
        CHECK(has(prepare_error(b), "anchor 9 names no unitig"));
        static const uint8_t dead_two[] = {1, 0, 1, 1};
        b = in; b.alive = dead_two;
        CHECK(has(prepare_error(b), "the end of bridge 0 (1 -> 2) names a unitig that is not alive"));
        ApplyBridgeIn moved[3]; memcpy(moved, BRIDGES, sizeof moved);
        moved[0].start = 0; b = in; b.bridges = moved;
        CHECK(has(prepare_error(b), "the start of bridge 0 (0 -> 2) is 0"));
        moved[0].start = 1; moved[0].end = -7;
        CHECK(has(prepare_error(b), "the end of bridge 0 (1 -> -7) is beyond n_unitigs (4)"));
        moved[0].end = 2; moved[0].best_off = 1;
        CHECK(has(prepare_error(b), "the best path of bridge 0 (1 -> 2) lies outside the best-path pool"));
        moved[0].best_off = 0; moved[0].first_distinct = 2; moved[0].n_distinct = 2;
        CHECK(has(prepare_error(b), "the distinct paths of bridge 0 (1 -> 2) lie outside the distinct-path pool"));
        static const uint64_t bad_off[] = {0, 2, 1, 2};
        b = in; b.dist_off = bad_off;
        CHECK(has(prepare_error(b), "offsets must ascend"));
    }
    // the error texts
    CHECK(apply_conflict_message(0, 1, 2, 5, -2, 7).find("bridge 0 (1 -> 2) and bridge 5 (-2 -> 7)") != std::string::npos);
    CHECK(has(apply_bad_entry_message(plan, in, true, 0), "entry 0 of the best-path pool (3), on a path of bridge 0 (1 -> 2)"));
    CHECK(has(apply_bad_entry_message(plan, in, false, 1), "entry 1 of the distinct-path pool (4), on a path of bridge 0 (1 -> 2)"));
    CHECK(has(apply_long_bridge_message(3, 5000000000ULL), "bridge 3 has 5000000000 bases"));
    {   // apply_finish and the text on a result as the device would leave it: unitig 5 = bridge 0 = "GGG"; 3 and 4 are gone
        ApplyResult r;
        r.n_unitigs = 4; r.n_total = 5;
        r.len = {3, 2, 3, 1, 3}; r.alive = {1, 1, 0, 0, 1}; r.type = {MERGE_TYPE_ANCHOR, MERGE_TYPE_ANCHOR, MERGE_TYPE_OTHER, MERGE_TYPE_OTHER, MERGE_TYPE_BRIDGE};
        r.depth = {4.0, 4.0, 1.0, 3.0, 3.0};
        r.links = {Link{1, 5}, Link{-1, -2}, Link{2, 1}, Link{-2, -5}, Link{5, 2}, Link{-5, -1}};
        r.bridge_seq = {'G', 'G', 'G'}; r.bridge_seq_off = {0, 3};
        apply_finish(in, plan, &r);
        CHECK(r.applied == 2 && r.direct == 1 && r.bridge_of.size() == 1 && r.seq_begin_all.size() == 5 && r.seq_begin_all[4] == 9 && r.seq_all.size() == 13);
        CHECK(memcmp(r.seq_all.data(), "AAACCGGGTGGG", 12) == 0);
        const std::string text = apply_gfa_string(r, 7, false);
        CHECK(text == "H\tVN:Z:1.0\tKM:i:7\nS\t1\tAAA\tDP:f:4.00\tCL:Z:forestgreen\nS\t2\tCC\tDP:f:4.00\tCL:Z:forestgreen\nS\t5\tGGG\tDP:f:3.00\tCL:Z:pink\n"
                      "L\t1\t+\t5\t+\t0M\nL\t1\t-\t2\t-\t0M\nL\t2\t+\t1\t+\t0M\nL\t2\t-\t5\t-\t0M\nL\t5\t+\t2\t+\t0M\nL\t5\t-\t1\t-\t0M\n");
        ApplyResult bare = r;
        bare.seq_all.clear(); bare.seq_begin_all.clear();
        std::string what;
        try { apply_gfa_string(bare, 7, false); } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(has(what, "missing sequences"));
    }
    {
        ApplyResult e;
        apply_empty(&e);
        CHECK(e.n_total == 0 && e.bridge_seq_off.size() == 1 && apply_gfa_string(e, 9, true) == "H\tVN:Z:1.0\tKM:i:9\n");
    }
    if (failures) { printf("apply_host_check: %d FAILED\n", failures); return 1; }
    printf("apply_host_check: OK\n");
    return 0;
}
