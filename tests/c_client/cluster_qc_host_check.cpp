// cluster_qc_host.cpp (+ cluster_host.cpp) on its own, with a plain loop over the matrix in place of the device's pair counts and verdict chain:
// the reference's known answers (split_clusters, cluster_assembly_count, set_min_assemblies, calculate_balance, calculate_tightness), the
// header parsing, and random trees on which generate_clusters through the plan (per-node facts, one evaluation per round) is held to a
// from-scratch qc_clusters per clustering built from cluster_assign and cluster_containment.  Meant to be built with sanitizers:
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -I autocycler_amd/csrc tests/c_client/cluster_qc_host_check.cpp
//       autocycler_amd/csrc/cluster_qc_host.cpp autocycler_amd/csrc/cluster_host.cpp -o cluster_qc_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cluster_qc_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)
typedef std::vector<uint16_t> V;
typedef std::vector<V> VV;

static ClusterTree tree_1() {      // (1:0.5,(2:0.3,(3:0.2,(4:0.1,5:0.1):0.1):0.1):0.2);
    const ClusterNode n[] = {{1, -1, -1, 0}, {2, -1, -1, 0}, {3, -1, -1, 0}, {4, -1, -1, 0}, {5, -1, -1, 0},
                             {6, 3, 4, 0.1}, {7, 2, 5, 0.2}, {8, 1, 6, 0.3}, {9, 0, 7, 0.5}};
    ClusterTree t;
    cluster_tree_from_nodes(n, 9, 8, &t);
    return t;
}
static ClusterTree tree_2() {      // (1:0.5,((2:0.1,3:0.1):0.2,(4:0.2,(5:0.1,6:0.1):0.1):0.1):0.2);
    const ClusterNode n[] = {{1, -1, -1, 0}, {2, -1, -1, 0}, {3, -1, -1, 0}, {4, -1, -1, 0}, {5, -1, -1, 0}, {6, -1, -1, 0},
                             {7, 1, 2, 0.1}, {8, 4, 5, 0.1}, {9, 3, 7, 0.2}, {10, 6, 8, 0.3}, {11, 0, 9, 0.5}};
    ClusterTree t;
    cluster_tree_from_nodes(n, 11, 10, &t);
    return t;
}

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

// ---- the stand-in for the device: the pair test by a loop over the matrix, the chain as the kernel runs it -----------------------
struct Matrix { const std::vector<double>* asym; uint32_t n; double cutoff; };
static bool contained(const Matrix& m, const ClusterQcIndex& ix, const ClusterQcEntity& x, const ClusterQcEntity& y) {
    uint64_t contain = 0;
    for (uint32_t p = x.lo; p < x.hi; p++)
        for (uint32_t q = y.lo; q < y.hi; q++) {
            const size_t a = ix.dfs_tip[p], b = ix.dfs_tip[q];
            const double ab = (*m.asym)[a * m.n + b], ba = (*m.asym)[b * m.n + a];
            if (ab < ba && ab < m.cutoff) contain++;
        }
    return 2 * contain > (uint64_t)(x.hi - x.lo) * (y.hi - y.lo);
}
static ClusterQcEvaluate stand_in(const Matrix& m, const ClusterQcIndex& ix, uint32_t* evaluations) {
    return [&m, &ix, evaluations](const ClusterQcPlan& plan, std::vector<uint32_t>* verdicts) {
        (*evaluations)++;
        verdicts->assign((size_t)plan.alts.size() * plan.stride(), 0xDEADu);
        for (uint32_t a = 0; a < plan.alts.size(); a++) {
            const uint32_t cnt = plan.count(a);
            uint32_t* v = verdicts->data() + (size_t)a * plan.stride();
            auto ent = [&](uint32_t j) { const uint32_t e = plan.entity(a, j); return e < plan.n ? plan.base[e] : plan.alts[a].child[e - plan.n]; };
            std::vector<uint8_t> pass(cnt);
            for (uint32_t j = 0; j < cnt; j++) { v[j] = ent(j).flags & 2u; pass[j] = v[j] == 0; }
            for (uint32_t c = 0; c < cnt; c++) {
                if (ent(c).flags & 1u) continue;
                for (uint32_t y = 0; y < cnt; y++)
                    if (y != c && pass[y] && contained(m, ix, ent(c), ent(y))) { v[c] |= 4u | ((y + 1) << 8); pass[c] = 0; break; }
            }
        }
    };
}

// ---- qc_clusters from scratch for one clustering: cluster_assign + cluster_containment, then the reference's loops -----------------
struct Scratch { std::vector<uint16_t> of_seq; std::vector<uint32_t> fail, container; ClusteringMetrics metrics; };
static Scratch from_scratch(const ClusterTree& t, const Matrix& m, const ClusterSeqInputs& in, const V& nodes, uint32_t min_assemblies) {
    Scratch s;
    const uint32_t n = in.n;
    s.of_seq.resize(n);
    std::vector<double> dist(nodes.size());
    const uint32_t top = cluster_assign(t, nodes.data(), (uint32_t)nodes.size(), in.seq_len, s.of_seq.data(), dist.data());
    std::vector<uint64_t> cc((size_t)top * top), tc((size_t)top * top);
    cluster_containment(m.asym->data(), n, s.of_seq.data(), top, m.cutoff, cc.data(), tc.data());
    s.fail.assign(top, 0); s.container.assign(top, 0);
    std::vector<uint8_t> trusted(top, 0);
    std::vector<ClusterQcItem> items(top);
    for (uint32_t c = 1; c <= top; c++) {
        std::vector<uint32_t> best(in.n_assemblies, 0), count(in.n_assemblies, 0);
        uint32_t size = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (s.of_seq[i] != c) continue;
            size++;
            if (in.trusted[i]) trusted[c - 1] = 1;
            if (count[in.assembly[i]]++ == 0 || in.cluster_weight[i] > best[in.assembly[i]]) best[in.assembly[i]] = in.cluster_weight[i];
        }
        uint64_t assemblies = 0; uint32_t ones = 0;
        for (uint32_t f = 0; f < in.n_assemblies; f++) { if (count[f]) assemblies += best[f]; if (count[f] == 1) ones++; }
        if (assemblies < min_assemblies && !trusted[c - 1]) s.fail[c - 1] |= 2;
        items[c - 1] = ClusterQcItem{size, ones, dist[c - 1], true};
    }
    for (uint32_t c = 1; c <= top; c++)
        for (uint32_t p = 1; p <= top; p++) {
            if (p == c || s.fail[p - 1]) continue;
            const size_t at = (size_t)(c - 1) * top + (p - 1);
            if ((double)cc[at] / (double)tc[at] > 0.5) {      // (the reference's quotient)
                if (!trusted[c - 1]) { s.fail[c - 1] |= 4; s.container[c - 1] = p; }
                break;
            }
        }
    for (uint32_t c = 0; c < top; c++) items[c].pass = s.fail[c] == 0;
    s.metrics = cluster_metrics(items.data(), top, in.n_assemblies);
    return s;
}
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static void random_case(uint64_t seed) {
    Rng r{seed * 977 + 5};
    const uint32_t S = 2 + r.below(30), F = 1u << r.below(3);
    std::vector<ClusterNode> nodes;
    std::vector<int32_t> roots;
    for (uint32_t i = 0; i < S; i++) { nodes.push_back(ClusterNode{(uint16_t)(i + 1), -1, -1, 0.0}); roots.push_back((int32_t)i); }
    for (uint32_t k = 0; roots.size() > 1; k++) {
        const uint32_t i = r.below((uint32_t)roots.size());
        uint32_t j = r.below((uint32_t)roots.size() - 1);
        if (j >= i) j++;
        nodes.push_back(ClusterNode{(uint16_t)(S + 1 + k), roots[i], roots[j], 0.0078125 * (double)(k + 1) / (double)S * 32.0});
        roots[i] = (int32_t)nodes.size() - 1;
        roots.erase(roots.begin() + j);
    }
    ClusterTree t;
    cluster_tree_from_nodes(nodes.data(), (uint32_t)nodes.size(), roots[0], &t);
    std::vector<double> asym((size_t)S * S, 0.0);
    for (uint32_t a = 0; a < S; a++)
        for (uint32_t b = 0; b < S; b++)
            if (a != b) asym[(size_t)a * S + b] = (double)(1 + r.below(8)) / 16.0;
    std::vector<uint64_t> len(S);
    std::vector<uint32_t> assembly(S), weight(S);
    std::vector<uint8_t> trusted(S);
    for (uint32_t i = 0; i < S; i++) { len[i] = 100 * (1 + r.below(4)); assembly[i] = i < F ? i : r.below(F); weight[i] = r.below(6) ? 1 : r.below(4); trusted[i] = r.below(12) == 0; }
    const ClusterSeqInputs in{len.data(), assembly.data(), weight.data(), trusted.data(), S, F};
    CHECK(cluster_assembly_count_checked(assembly.data(), S) == F);
    const double cutoffs[3] = {10.0, 0.3, 0.0};
    for (double cutoff : cutoffs) {
        const Matrix m{&asym, S, cutoff};
        const uint32_t min_assemblies = cluster_min_assemblies(F);
        ClusterQcIndex ix;
        cluster_qc_index(t, in, &ix);
        uint32_t evaluations = 0;
        ClusterQcResult res;
        cluster_generate_host(ix, cutoff, nullptr, 0, min_assemblies, stand_in(m, ix, &evaluations), &res);
        CHECK(evaluations == res.evaluations);
        // replay refine_auto_clusters with every clustering scored from scratch
        V best = cluster_cut(t, cutoff, nullptr, 0);
        double best_score = from_scratch(t, m, in, best, min_assemblies).metrics.overall_clustering_score;
        CHECK(same_bits(best_score, res.start_score));
        size_t at = 0, round = 0;
        for (bool improved = true; improved; round++) {
            improved = false;
            const VV alts = cluster_split_clusters(t, best);
            CHECK(round < res.round_alternatives.size() && res.round_alternatives[round] == alts.size());
            for (const V& alt : alts) {
                const double score = from_scratch(t, m, in, alt, min_assemblies).metrics.overall_clustering_score;
                const bool accept = score > best_score + 1e-12;
                CHECK(at < res.scores.size() && same_bits(res.scores[at], score) && (res.accepted[at] != 0) == accept);
                at++;
                if (accept) { best = alt; best_score = score; improved = true; }
            }
        }
        CHECK(round == res.round_alternatives.size() && at == res.scores.size());
        CHECK(best == res.nodes);
        const Scratch fin = from_scratch(t, m, in, best, min_assemblies);
        CHECK(fin.of_seq == res.cluster_of_seq && fin.fail.size() == res.records.size());
        for (size_t c = 0; c < res.records.size() && c < fin.fail.size(); c++)
            CHECK(res.records[c].fail == fin.fail[c] && res.records[c].container == fin.container[c]);
        CHECK(same_bits(fin.metrics.overall_clustering_score, res.metrics.overall_clustering_score));
        CHECK(same_bits(fin.metrics.cluster_balance_score, res.metrics.cluster_balance_score));
        CHECK(same_bits(fin.metrics.cluster_tightness_score, res.metrics.cluster_tightness_score));
        CHECK(fin.metrics.pass_cluster_count == res.metrics.pass_cluster_count && fin.metrics.fail_contig_count == res.metrics.fail_contig_count);
        // qc_clusters alone on a list in another order (the old number breaks ties), and with manual clusters
        V shuffled = best;
        for (size_t i = shuffled.size(); i > 1; i--) std::swap(shuffled[i - 1], shuffled[r.below((uint32_t)i)]);
        ClusterQcResult q;
        cluster_qc_nodes_host(ix, shuffled.data(), (uint32_t)shuffled.size(), nullptr, 0, min_assemblies, stand_in(m, ix, &evaluations), &q);
        const Scratch qs = from_scratch(t, m, in, shuffled, min_assemblies);
        CHECK(qs.of_seq == q.cluster_of_seq && same_bits(qs.metrics.overall_clustering_score, q.metrics.overall_clustering_score));
        for (size_t c = 0; c < q.records.size() && c < qs.fail.size(); c++) CHECK(q.records[c].fail == qs.fail[c] && q.records[c].container == qs.container[c]);
        ClusterQcResult man;
        const V manual{best[0]};
        cluster_qc_nodes_host(ix, best.data(), (uint32_t)best.size(), manual.data(), 1, min_assemblies, ClusterQcEvaluate(), &man);
        for (const ClusterQcRecord& rec : man.records) CHECK(rec.fail == (rec.node == best[0] ? 0u : 1u));
    }
}

template <class F> static bool throws(F&& f, const char* what) {
    try { f(); } catch (const ClusterError& e) { return strstr(e.what(), what) != nullptr; }
    return false;
}

int main() {
    // test_split_clusters
    const ClusterTree t1 = tree_1(), t2 = tree_2();
    CHECK((cluster_split_clusters(t1, V{1, 2, 3, 6}) == VV{V{1, 2, 3, 4, 5}}));
    CHECK((cluster_split_clusters(t1, V{1, 2, 7}) == VV{V{1, 2, 3, 6}}));
    CHECK((cluster_split_clusters(t1, V{1, 8}) == VV{V{1, 2, 7}}));
    CHECK((cluster_split_clusters(t1, V{9}) == VV{V{1, 8}}));
    CHECK((cluster_split_clusters(t2, V{1, 4, 5, 6, 7}) == VV{V{1, 2, 3, 4, 5, 6}}));
    CHECK((cluster_split_clusters(t2, V{1, 2, 3, 4, 8}) == VV{V{1, 2, 3, 4, 5, 6}}));
    CHECK((cluster_split_clusters(t2, V{1, 4, 7, 8}) == VV{V{1, 2, 3, 4, 8}, V{1, 4, 5, 6, 7}}));
    CHECK((cluster_split_clusters(t1, V{1, 2, 3, 4, 5}).empty()));
    // test_set_minpts: 12, 11, 9, 8, 7, 5, 4, 3, 2, 1 assemblies
    const uint32_t counts[] = {12, 11, 9, 8, 7, 5, 4, 3, 2, 1}, expected[] = {3, 3, 2, 2, 2, 2, 2, 2, 2, 1};
    for (int i = 0; i < 10; i++) CHECK(cluster_min_assemblies(counts[i]) == expected[i]);
    CHECK(cluster_min_assemblies(1000) == 250 && cluster_min_assemblies(0xFFFFFFFFu) == 0x40000000u);
    // Sequence::cluster_weight / is_trusted, the headers of test_cluster_assembly_count_2 / 3 among them
    CHECK(cluster_header_weight("contig_1 Autocycler_cluster_weight=3 other stuff") == 3 && cluster_header_weight("contig_2 other stuff autocycler_cluster_weight=6") == 6);
    CHECK(cluster_header_weight("contig_3") == 1 && cluster_header_weight("contig_2 AuToCyCleR_cluster_weight=0") == 0 && cluster_header_weight("") == 1);
    CHECK(cluster_header_weight("c autocycler_cluster_weight=x autocycler_cluster_weight=+4") == 4 && cluster_header_weight("c autocycler_cluster_weight=") == 1);
    CHECK(cluster_header_weight("c xautocycler_cluster_weight=5") == 1 && cluster_header_weight("c autocycler_cluster_weight=5x") == 1 && cluster_header_weight("c\tautocycler_cluster_weight=9") == 9);
    CHECK(cluster_header_weight("c autocycler_cluster_weight=99999999999999999999 autocycler_cluster_weight=2") == 2 && cluster_header_weight("c autocycler_cluster_weight=4294967297") == 0xFFFFFFFFu);
    CHECK(cluster_header_trusted("contig Autocycler_TRUSTED") && cluster_header_trusted("xautocycler_trustedx") && !cluster_header_trusted("autocycler_truste d") && !cluster_header_trusted(""));
    {
        uint32_t number[5];
        CHECK(cluster_number_assemblies({"b.fasta", "a.fasta", "b.fasta", "c.fasta", "a.fasta"}, number) == 3);
        CHECK(number[0] == 0 && number[1] == 1 && number[2] == 0 && number[3] == 2 && number[4] == 1);
    }
    // test_cluster_assembly_count_1 .. 3 through the per-node facts: the reference's clusters are nodes of a small tree
    {
        const ClusterNode n[] = {{1, -1, -1, 0}, {2, -1, -1, 0}, {3, -1, -1, 0}, {4, -1, -1, 0}, {5, -1, -1, 0},
                                 {6, 0, 3, 0.1}, {7, 2, 4, 0.1}, {8, 5, 1, 0.2}, {9, 7, 6, 0.3}};
        ClusterTree t;
        cluster_tree_from_nodes(n, 9, 8, &t);      // clusters {1, 4}, {2}, {3, 5}
        const uint64_t len[5] = {1, 1, 1, 1, 1};
        const uint8_t trusted[5] = {0, 0, 0, 0, 0};
        const uint32_t assembly[5] = {0, 0, 0, 1, 1};
        const uint32_t w1[5] = {1, 1, 1, 1, 1}, w2[5] = {3, 6, 1, 1, 0};
        ClusterQcIndex ix;
        cluster_qc_index(t, ClusterSeqInputs{len, assembly, w1, trusted, 5, 2}, &ix);
        CHECK(ix.node(5).assembly_count == 2 && ix.node(1).assembly_count == 1 && ix.node(6).assembly_count == 2);
        cluster_qc_index(t, ClusterSeqInputs{len, assembly, w2, trusted, 5, 2}, &ix);
        CHECK(ix.node(5).assembly_count == 4 && ix.node(1).assembly_count == 6 && ix.node(6).assembly_count == 1);
        ClusterTree u;
        const ClusterNode m[] = {{1, -1, -1, 0}, {2, -1, -1, 0}, {3, -1, -1, 0}, {4, -1, -1, 0}, {5, -1, -1, 0}, {6, 0, 1, 0.1}, {7, 5, 2, 0.1}, {8, 3, 4, 0.1}, {9, 6, 7, 0.3}};
        cluster_tree_from_nodes(m, 9, 8, &u);      // clusters {1, 2, 3}, {4, 5}
        const uint32_t w3[5] = {3, 1, 2, 1, 0};
        cluster_qc_index(u, ClusterSeqInputs{len, assembly, w3, trusted, 5, 2}, &ix);
        CHECK(ix.node(6).assembly_count == 3 && ix.node(7).assembly_count == 1 && ix.node(6).ones == 0 && ix.node(7).ones == 0 && ix.node(5).ones == 0);
        // check_complete_coverage and the other argument errors
        CHECK(throws([&] { cluster_qc_nodes_checked(ix, V{7, 8, 1}.data(), 3); }, "overlap"));
        CHECK(throws([&] { cluster_qc_nodes_checked(ix, V{7}.data(), 1); }, "cover 3 of 5"));
        CHECK(throws([&] { cluster_qc_nodes_checked(ix, V{7, 8, 77}.data(), 3); }, "does not contain a node with id 77"));
        CHECK(cluster_qc_nodes_checked(ix, V{8, 7}.data(), 2).size() == 2 && cluster_qc_nodes_checked(ix, V{9}.data(), 1).size() == 1);
        CHECK(throws([&] { ClusterQcIndex bad; cluster_qc_index(u, ClusterSeqInputs{len, assembly, w3, trusted, 4, 2}, &bad); }, "5 tips"));
        const uint32_t gap[3] = {0, 2, 2}, high[3] = {0, 1, 3};
        CHECK(throws([&] { cluster_assembly_count_checked(gap, 3); }, "not dense") && throws([&] { cluster_assembly_count_checked(high, 3); }, "not dense"));
        ClusterQcResult res;
        const V nested{9, 6};
        CHECK(throws([&] { cluster_generate_host(ix, 0.5, nested.data(), 2, 2, ClusterQcEvaluate(), &res); }, "manual clusters cannot be nested"));
    }
    // test_calculate_balance: six clusterings over files a .. f, by (ones, size) per cluster; strictly decreasing from 1.0
    {
        const ClusterQcItem c1[] = {{3, 3, 0, true}, {3, 3, 0, true}, {3, 3, 0, true}}, c2[] = {{3, 3, 0, true}, {4, 2, 0, true}, {3, 3, 0, true}},
                            c3[] = {{3, 3, 0, true}, {4, 2, 0, true}, {2, 2, 0, true}}, c4[] = {{3, 3, 0, true}, {4, 2, 0, true}, {1, 1, 0, true}},
                            c5[] = {{3, 3, 0, true}, {4, 2, 0, true}, {2, 0, 0, true}}, c6[] = {{3, 3, 0, true}, {2, 2, 0, true}, {1, 1, 0, true}};
        const double b[] = {cluster_metrics(c1, 3, 3).cluster_balance_score, cluster_metrics(c2, 3, 3).cluster_balance_score, cluster_metrics(c3, 3, 3).cluster_balance_score,
                            cluster_metrics(c4, 3, 3).cluster_balance_score, cluster_metrics(c5, 3, 3).cluster_balance_score, cluster_metrics(c6, 3, 6).cluster_balance_score};
        CHECK(std::fabs(b[0] - 1.0) < 1e-8);
        for (int i = 0; i + 1 < 6; i++) CHECK(b[i + 1] < b[i]);
    }
    // test_calculate_tightness_weights_by_cluster_size
    {
        const ClusterQcItem combined[] = {{4, 0, 0.0, true}, {8, 0, 0.25, true}}, split[] = {{1, 0, 0.0, true}, {1, 0, 0.0, true}, {1, 0, 0.0, true}, {1, 0, 0.0, true}, {8, 0, 0.25, true}};
        const ClusteringMetrics a = cluster_metrics(combined, 2, 2), b = cluster_metrics(split, 5, 2);
        CHECK(std::fabs(a.cluster_tightness_score - b.cluster_tightness_score) < 1e-8 && a.cluster_tightness_score == 8.0 / 12.0);
        const ClusterQcItem none[] = {{4, 0, 0.0, false}};
        CHECK(cluster_metrics(none, 1, 2).cluster_tightness_score == 0.0 && cluster_metrics(none, 1, 2).fail_contig_fraction == 1.0);
    }
    for (uint64_t seed = 0; seed < 60; seed++) random_case(seed);
    if (failures) { printf("cluster_qc_host_check: %d FAILED\n", failures); return 1; }
    printf("cluster_qc_host_check: OK\n");
    return 0;
}
