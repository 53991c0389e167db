// resolve_host.cpp on its own, with a CPU stub for the distances: the reference's known answers of Bridge::new, get_anchor_to_anchor_paths
// and consensus_weight through the host functions.  Meant to be built with sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I autocycler_amd/csrc tests/c_client/resolve_host_check.cpp autocycler_amd/csrc/resolve_host.cpp -o resolve_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "resolve_host.hpp"

using namespace ac;

static std::vector<uint32_t> g_w;
static uint32_t wt(int32_t u) { return g_w[(uint32_t)(u < 0 ? -u : u) - 1]; }
static uint32_t distance(const int32_t* a, uint64_t n, const int32_t* b, uint64_t m) {      // resolve.rs:387-418
    std::vector<uint32_t> prev(m + 1, 0), curr(m + 1, 0);
    for (uint64_t j = 1; j <= m; j++) prev[j] = prev[j - 1] + wt(b[j - 1]);
    for (uint64_t i = 1; i <= n; i++) {
        const uint32_t wi = wt(a[i - 1]);
        curr[0] = prev[0] + wi;
        for (uint64_t j = 1; j <= m; j++) {
            const uint32_t wj = wt(b[j - 1]), sub = prev[j - 1] + (a[i - 1] == b[j - 1] ? 0 : (wi > wj ? wi : wj));
            curr[j] = std::min(sub, std::min(prev[j] + wi, curr[j - 1] + wj));
        }
        prev.swap(curr);
    }
    return prev[m];
}
static void stub(const PathPool& pool, const std::vector<PathPair>& pairs, std::vector<uint32_t>& dist) {
    dist.resize(pairs.size());
    for (size_t q = 0; q < pairs.size(); q++) dist[q] = distance(pool.at(pairs[q].a), pool.len(pairs[q].a), pool.at(pairs[q].b), pool.len(pairs[q].b));
}
static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static ResolveResult run(const std::vector<std::vector<int32_t>>& seqs, const std::vector<uint32_t>& cw) {
    std::vector<int32_t> flat; std::vector<uint64_t> off{0};
    for (auto& s : seqs) { flat.insert(flat.end(), s.begin(), s.end()); off.push_back(flat.size()); }
    for (size_t s = 0; s < seqs.size(); s++) validate_resolve_path(flat.data() + off[s], off[s + 1] - off[s], (uint32_t)g_w.size(), "path");
    ResolveResult r;
    resolve_bridges_host(flat.data(), off.data(), (uint32_t)seqs.size(), nullptr, cw.data(), g_w.data(), (uint32_t)g_w.size(), stub, &r);
    return r;
}
static std::vector<int32_t> best_of(const ResolveResult& r, size_t b) {
    return std::vector<int32_t>(r.best_pool.begin() + r.bridges[b].best_off, r.bridges[b].best_off + r.bridges[b].best_len + r.best_pool.begin());
}

int main() {
    // test_consensus_weight
    CHECK(consensus_weight_of("c123") == 1); CHECK(consensus_weight_of("c123 other stuff") == 1);
    CHECK(consensus_weight_of("c123 Autocycler_consensus_weight=1") == 1); CHECK(consensus_weight_of("c123 AUTOCYCLER_CONSENSUS_WEIGHT=2") == 2);
    CHECK(consensus_weight_of("c123 other stuff Autocycler_consensus_weight=0 other stuff") == 0);
    CHECK(consensus_weight_of("c123 autocycler_consensus_weight=1234") == 1234); CHECK(consensus_weight_of("c123 Autocycler_consensus_weight=23.456") == 1);
    CHECK(consensus_weight_of("c123 Autocycler_consensus_weight=-1") == 1); CHECK(consensus_weight_of("c123 Autocycler_consensus_weight=abc") == 1);
    CHECK(consensus_weight_of("autocycler_consensus_weight=") == 1); CHECK(consensus_weight_of(nullptr) == 1);
    // test_best_path_1 / _2 (a sequence of weight 0 holding the two ends alone leaves only those as anchors)
    g_w.assign(123, 10);
    typedef std::vector<int32_t> P;
    const P x{1, 12, -23, -8, 41, 2}, y{1, 12, 17, 123, 41, 2};
    ResolveResult r = run({x, x, x, y, {1, 2}}, {1, 1, 1, 1, 0});
    CHECK(r.anchors == (std::vector<uint32_t>{1, 2}) && r.bridges.size() == 1 && r.bridges[0].depth == 4 && best_of(r, 0) == (P{12, -23, -8, 41}));
    r = run({y, x, x, y, {1, 2}}, {1, 1, 1, 1, 0});
    CHECK(r.bridges.size() == 1 && r.bridges[0].n_distinct == 2 && best_of(r, 0) == (P{12, -23, -8, 41}));
    // test_best_path_3
    g_w.assign(21, 10);
    std::vector<P> seqs;
    const P full{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    const int sub_at[] = {8, 4, 9, 5, 6, 2, 3, 7}, sub_to[] = {20, 16, 21, 17, 18, 14, 15, 19};
    for (int q = 0; q < 8; q++) { P p = full; p[sub_at[q]] = sub_to[q]; seqs.push_back(p); }
    seqs.push_back(P{1, 13, 12}); seqs.push_back(P{1, 13, 12}); seqs.push_back(full); seqs.push_back(P{1, 12});
    std::vector<uint32_t> cw(seqs.size(), 1); cw.back() = 0;
    r = run(seqs, cw);
    CHECK(r.bridges.size() == 1 && r.bridges[0].depth == 11 && best_of(r, 0) == (P{2, 3, 4, 5, 6, 7, 8, 9, 10, 11}));
    // test_get_anchor_to_anchor_paths / test_group_paths_by_start_end
    g_w.assign(12, 10);
    r = run({{1, -10, 4, 6, -5, -2, -9, 3, 8, -7}, {-2, -9, 12, 8, -7, 1, -10, 4, 6, -5}, {7, -8, -3, 9, 2, 11, -6, -4, 10, -1}, {1, 2, 6, 8}}, {1, 1, 1, 0});
    CHECK(r.anchors == (std::vector<uint32_t>{1, 2, 6, 8}) && r.bridges.size() == 4);
    CHECK(r.bridges[0].start == 1 && r.bridges[0].end == 6 && r.bridges[0].depth == 3 && r.bridges[0].n_distinct == 1);
    CHECK(r.bridges[1].start == -2 && r.bridges[1].end == 8 && r.bridges[1].depth == 3 && r.bridges[1].n_distinct == 2);
    CHECK(r.bridges[2].start == 6 && r.bridges[2].end == -2 && r.bridges[2].depth == 2 && r.bridges[2].n_distinct == 2);
    CHECK(r.bridges[3].start == 8 && r.bridges[3].end == 1 && r.bridges[3].depth == 1 && best_of(r, 3) == (P{-7}));
    // no sequences, one sequence, an overflowing bridge
    r = run({}, {});
    CHECK(r.anchors.size() == 12 && r.bridges.empty());
    g_w = {0x80000000u, 0x7FFFFFFFu, 1, 5, 5};
    r = run({{4, 1, 5}, {4, 2, 3, 5}, {4, 3, 5}}, {1, 1, 1});
    CHECK(r.bridges.size() == 1 && r.bridges[0].status == 2 && r.pairs_overflowing == 1 && r.best_pool.empty());
    printf(failures ? "resolve_host_check: %d FAILED\n" : "resolve_host_check: OK\n", failures);
    return failures ? 1 : 0;
}
