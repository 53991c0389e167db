// trim_apply_host.cpp alone, on the host, under the address and undefined-behaviour sanitizers (`make trim_apply_host_check` in
// autocycler_amd/csrc; tests/test_trim_apply_bounds_emu.py builds and runs it the same way): the choice of the kind, the slice table with its
// refusals, median / MAD (the reference's own answers, misc.rs:694-721), f64::round and `as usize`, the exclusion and the yaml.  CPU only.
#include "trim_apply_host.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)
template <class F> static std::string error_of(F&& f) {
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}
static TrimResult result(uint32_t se_status, uint32_t se_b, uint32_t se_e, uint32_t se_len, uint32_t hp_status = 0, uint32_t hp_b = 0, uint32_t hp_e = 0, uint32_t hp_len = 0) {
    TrimResult r;
    r.se = TrimSlice{se_status, se_b, se_e, se_len}; r.hp = TrimSlice{hp_status, hp_b, hp_e, hp_len};
    return r;
}

int main() {
    typedef std::vector<uint64_t> V;
    // the reference's answers
    CHECK(trim_apply_median(V{}) == 0 && trim_apply_median(V{0, 1, 2, 3, 4}) == 2 && trim_apply_median(V{4, 3, 2, 1, 0}) == 2);
    CHECK(trim_apply_median(V{0, 1, 2, 3, 4, 5}) == 2 && trim_apply_median(V{5, 4, 3, 2, 1, 0}) == 2);
    CHECK(trim_apply_median(V{0, 2, 4, 6, 8, 10}) == 5 && trim_apply_median(V{10, 8, 6, 4, 2, 0}) == 5);
    CHECK(trim_apply_mad(V{}) == 0 && trim_apply_mad(V{1, 1, 2, 2, 4, 6, 9}) == 1 && trim_apply_mad(V{4, 1, 9, 6, 1, 2, 2}) == 1);
    // f64::round and `as usize`
    CHECK(trim_apply_round_to_usize(14.5) == 15 && trim_apply_round_to_usize(15.5) == 16 && trim_apply_round_to_usize(2.4999) == 2);
    CHECK(trim_apply_round_to_usize(-0.5) == 0 && trim_apply_round_to_usize(-350.0) == 0 && trim_apply_round_to_usize(0.0) == 0);
    CHECK(trim_apply_round_to_usize(std::numeric_limits<double>::quiet_NaN()) == 0);
    CHECK(trim_apply_round_to_usize(std::numeric_limits<double>::infinity()) == ~0ULL && trim_apply_round_to_usize(1e30) == ~0ULL);
    CHECK(trim_apply_round_to_usize(-std::numeric_limits<double>::infinity()) == 0 && trim_apply_round_to_usize(4294967296.5) == 4294967297ULL);

    // the choice and the slices: two sequences over one array, the second one's slice lies back to back with nothing
    const int32_t path[] = {1, 2, 3, 4, 1, 1, 2, 3, 4};
    const uint64_t off[] = {0, 5, 9};
    const uint32_t seq_length[] = {23, 18};
    {
        TrimApplyPlan p;
        const TrimResult res[2] = {result(1, 0, 4, 18), result(0, 0, 4, 18, 1, 1, 3, 7)};
        trim_apply_choose(res, 2, path, off, seq_length, TRIM_CHOOSE_AUTO, &p);      // a tie: start-end
        CHECK(p.chosen == TRIM_KIND_START_END && p.c_se == 1 && p.c_hp == 1 && p.n_trimmed == 1 && p.rejected == 0);
        CHECK(p.seqs[0].begin == 0 && p.seqs[0].end == 4 && p.seqs[0].length == 18 && p.seqs[0].trimmed == 1);
        CHECK(p.seqs[1].begin == 0 && p.seqs[1].end == 4 && p.seqs[1].length == 18 && p.seqs[1].trimmed == 0);
        CHECK(p.sliced_off == V({0, 4, 8}) && p.sliced == std::vector<int32_t>({1, 2, 3, 4, 1, 2, 3, 4}));
        trim_apply_exclude(&p, 5.0);
        CHECK(p.median == 18 && p.mad == 0 && p.min_length == 18 && p.max_length == 18 && p.n_excluded == 0 && p.label == std::vector<uint16_t>({1, 1}));
        CHECK(trim_apply_yaml(p) == "trimmed_cluster_size: 2\ntrimmed_cluster_lengths:\n- 18\n- 18\ntrimmed_cluster_median: 18\ntrimmed_cluster_mad: 0\n");
        trim_apply_choose(res, 2, path, off, seq_length, TRIM_CHOOSE_HAIRPIN, &p);
        CHECK(p.chosen == TRIM_KIND_HAIRPIN && p.seqs[0].trimmed == 0 && p.seqs[0].length == 23 && p.seqs[1].begin == 1 && p.seqs[1].end == 3 && p.seqs[1].length == 7);
        CHECK(p.sliced == std::vector<int32_t>({1, 2, 3, 4, 1, 2, 3}));
        trim_apply_choose(res, 2, path, off, seq_length, TRIM_CHOOSE_NONE, &p);
        CHECK(p.chosen == TRIM_KIND_NONE && p.n_trimmed == 0 && p.sliced.size() == 9);
        trim_apply_choose(nullptr, 2, path, off, seq_length, TRIM_CHOOSE_NONE, &p);
        CHECK(p.chosen == TRIM_KIND_NONE && p.sliced.size() == 9);
    }
    {   // status 2 counts as not trimmed; more hairpins than start-ends
        TrimApplyPlan p;
        const TrimResult res[2] = {result(2, 0, 4, 18, 1, 0, 5, 23), result(0, 0, 4, 18, 1, 0, 0, 0)};
        trim_apply_choose(res, 2, path, off, seq_length, TRIM_CHOOSE_AUTO, &p);
        CHECK(p.chosen == TRIM_KIND_HAIRPIN && p.c_se == 0 && p.c_hp == 2 && p.rejected == 1);
        CHECK(error_of([&] { trim_apply_exclude(&p, 0.0); }).find("sequence 1 is kept with an empty slice") != std::string::npos);
        trim_apply_exclude(&p, 0.1);      // lengths 23 and 0: the range excludes both, the empty one included
        CHECK(p.n_excluded == 2 && p.label == std::vector<uint16_t>({0, 0}));
        CHECK(trim_apply_yaml(p) == "trimmed_cluster_size: 0\ntrimmed_cluster_lengths: []\ntrimmed_cluster_median: 0\ntrimmed_cluster_mad: 0\n");
    }
    {   // the refusals
        TrimApplyPlan p;
        const TrimResult late[2] = {result(1, 3, 2, 0), result(0, 0, 4, 18)}, beyond[2] = {result(0, 0, 5, 23), result(1, 0, 5, 18)};
        CHECK(error_of([&] { trim_apply_choose(late, 2, path, off, seq_length, TRIM_CHOOSE_AUTO, &p); }).find("begins at 3, after its end 2") != std::string::npos);
        CHECK(error_of([&] { trim_apply_choose(beyond, 2, path, off, seq_length, TRIM_CHOOSE_AUTO, &p); }).find("ends at 5, beyond its path of 4 entries") != std::string::npos);
        const uint64_t down[] = {0, 5, 4};
        CHECK(error_of([&] { trim_apply_choose(nullptr, 2, path, down, seq_length, TRIM_CHOOSE_NONE, &p); }).find("path offsets must ascend") != std::string::npos);
        CHECK(error_of([&] { trim_apply_choose(nullptr, 2, path, off, seq_length, TRIM_CHOOSE_AUTO, &p); }) == "null pointer: results");
        CHECK(error_of([&] { trim_apply_choose(nullptr, 0, path, off, seq_length, TRIM_CHOOSE_NONE, &p); }) == "trim apply: no sequences");
        CHECK(error_of([&] { trim_apply_choose(nullptr, 2, path, off, seq_length, 4, &p); }).find("chosen is 4") != std::string::npos);
        CHECK(error_of([&] { trim_apply_choose(nullptr, 2, nullptr, off, seq_length, TRIM_CHOOSE_NONE, &p); }) == "null pointer: path_entries");
        CHECK(error_of([&] { trim_apply_check_settings(1.5, 5.0); }) == "--min_identity must be between 0.0 and 1 (inclusive)");
        CHECK(error_of([&] { trim_apply_check_settings(std::nan(""), 5.0); }) == "--min_identity must be between 0.0 and 1 (inclusive)");
        CHECK(error_of([&] { trim_apply_check_settings(0.75, -0.1); }) == "--mad cannot be less than 0");
        CHECK(error_of([&] { trim_apply_check_settings(0.0, 0.0); trim_apply_check_settings(1.0, 5.0); }).empty());
    }
    {   // the range: half away from zero, saturation at 0, and no range at all for mad == 0
        TrimApplyPlan p;
        const int32_t one[] = {1, 2, 3};
        const uint64_t o3[] = {0, 1, 2, 3};
        const uint32_t a[] = {10, 20, 0}, b[] = {10, 100, 1000};
        trim_apply_choose(nullptr, 2, one, o3, a, TRIM_CHOOSE_NONE, &p);
        trim_apply_exclude(&p, 0.1);
        CHECK(p.median == 15 && p.mad == 5 && p.min_length == 15 && p.max_length == 16 && p.n_excluded == 2);
        trim_apply_choose(nullptr, 3, one, o3, b, TRIM_CHOOSE_NONE, &p);
        trim_apply_exclude(&p, 5.0);
        CHECK(p.median == 100 && p.mad == 90 && p.min_length == 0 && p.max_length == 550 && p.n_excluded == 1 && p.seqs[2].excluded == 1);
        trim_apply_exclude(&p, 0.0);
        CHECK(p.min_length == 0 && p.max_length == ~0ULL && p.n_excluded == 0 && p.seqs[2].excluded == 0);
        CHECK(trim_apply_yaml(p) == "trimmed_cluster_size: 3\ntrimmed_cluster_lengths:\n- 10\n- 100\n- 1000\ntrimmed_cluster_median: 100\ntrimmed_cluster_mad: 90\n");
    }
    if (failures) { fprintf(stderr, "trim_apply_host_check: %d check(s) failed\n", failures); return 1; }
    printf("trim_apply_host_check: OK\n");
    return 0;
}
