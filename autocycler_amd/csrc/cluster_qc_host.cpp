// The host side of cluster's QC, scores and refinement (cluster_qc_host.hpp).  As in cluster_host.cpp, every walk over the tree is a loop:
// a UPGMA tree of S tips may be a chain S deep.
#include "cluster_qc_host.hpp"

#include <algorithm>
#include <cmath>

namespace ac {

// ---- metrics --------------------------------------------------------------------------------------------------------------------------
ClusteringMetrics cluster_metrics(const ClusterQcItem* items, uint32_t n, uint32_t n_assemblies) {
    ClusteringMetrics m;
    uint64_t all_size = 0, pass_size = 0;
    double acc = 0.0, sum = 0.0;
    for (uint32_t c = 0; c < n; c++) {
        const ClusterQcItem& it = items[c];
        all_size += it.size;
        acc += ((double)it.ones / (double)n_assemblies) * (double)it.size;      // calculate_balance
        if (it.pass) {
            m.pass_cluster_count++; m.pass_contig_count += it.size;
            sum += (1.0 - std::sqrt(it.dist)) * (double)it.size;                // calculate_tightness
            pass_size += it.size;
        } else {
            m.fail_cluster_count++; m.fail_contig_count += it.size;
        }
    }
    const uint32_t total = m.pass_contig_count + m.fail_contig_count;
    if (total > 0) {      // calculate_fractions
        m.pass_contig_fraction = (double)m.pass_contig_count / (double)total;
        m.fail_contig_fraction = (double)m.fail_contig_count / (double)total;
    }
    m.cluster_balance_score = acc / (double)all_size;
    m.cluster_tightness_score = m.pass_cluster_count ? sum / (double)pass_size : 0.0;
    m.overall_clustering_score = (m.cluster_balance_score + m.cluster_tightness_score) / 2.0;
    return m;
}

// ---- the per-sequence inputs ----------------------------------------------------------------------------------------------------------
uint32_t cluster_min_assemblies(uint32_t n_assemblies) {
    if (n_assemblies == 1) return 1;
    return std::max<uint32_t>(2, (uint32_t)(((uint64_t)n_assemblies + 2) / 4));      // usize_division_rounded(count, 4)
}

uint32_t cluster_assembly_count_checked(const uint32_t* assembly, uint32_t n) {
    if (n && !assembly) throw ClusterError("null pointer");
    std::vector<uint8_t> seen(n, 0);
    uint32_t distinct = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (assembly[i] >= n) throw ClusterError("cluster: assembly index " + std::to_string(assembly[i]) + " of sequence " + std::to_string(i) + " is not dense (0 .. F - 1, every value in use)");
        if (!seen[assembly[i]]) { seen[assembly[i]] = 1; distinct++; }
    }
    for (uint32_t f = 0; f < distinct; f++)
        if (!seen[f]) throw ClusterError("cluster: the assembly indices are not dense (" + std::to_string(distinct) + " distinct values, but " + std::to_string(f) + " is not among them)");
    return distinct;
}

static std::string ascii_lower(const std::string& s) {
    std::string out = s;
    for (char& c : out) if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    return out;
}
bool cluster_header_trusted(const std::string& header) { return ascii_lower(header).find("autocycler_trusted") != std::string::npos; }

uint32_t cluster_header_weight(const std::string& header) {
    static const std::string prefix = "autocycler_cluster_weight=";
    const std::string h = ascii_lower(header);
    auto is_space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    size_t i = 0;
    while (i < h.size()) {
        while (i < h.size() && is_space(h[i])) i++;
        size_t e = i;
        while (e < h.size() && !is_space(h[e])) e++;
        if (e > i && e - i > prefix.size() && h.compare(i, prefix.size(), prefix) == 0) {      // usize::from_str: an optional '+', then digits only
            size_t d = i + prefix.size();
            if (h[d] == '+') d++;
            bool ok = d < e;
            uint64_t v = 0;
            for (size_t q = d; q < e && ok; q++) {
                if (h[q] < '0' || h[q] > '9') { ok = false; break; }
                const uint64_t digit = (uint64_t)(h[q] - '0');
                if (v > (0xFFFFFFFFFFFFFFFFull - digit) / 10) { ok = false; break; }      // beyond usize: the parse fails, the next token is tried
                v = v * 10 + digit;
            }
            if (ok) return (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull);
        }
        i = e;
    }
    return 1;
}

uint32_t cluster_number_assemblies(const std::vector<std::string>& filenames, uint32_t* assembly) {
    std::vector<std::pair<std::string, uint32_t>> sorted;      // (name, index), by name
    for (size_t i = 0; i < filenames.size(); i++) {
        auto it = std::lower_bound(sorted.begin(), sorted.end(), filenames[i], [](const std::pair<std::string, uint32_t>& a, const std::string& b) { return a.first < b; });
        if (it == sorted.end() || it->first != filenames[i]) it = sorted.insert(it, {filenames[i], (uint32_t)sorted.size()});
        assembly[i] = it->second;
    }
    return (uint32_t)sorted.size();
}

// ---- the tree's index -----------------------------------------------------------------------------------------------------------------
void cluster_qc_index(const ClusterTree& t, const ClusterSeqInputs& in, ClusterQcIndex* out) {
    ClusterQcIndex& ix = *out;
    const size_t n_nodes = t.nodes.size();
    if (t.tips.size() != in.n) throw ClusterError("cluster: the tree has " + std::to_string(t.tips.size()) + " tips, the call names " + std::to_string(in.n) + " sequences");
    if (in.n && (!in.seq_len || !in.assembly || !in.cluster_weight || !in.trusted)) throw ClusterError("null pointer");
    ix.t = &t; ix.in = in;
    ix.node_of_id.assign(65536, -1);
    for (size_t v = 0; v < n_nodes; v++) ix.node_of_id[t.nodes[v].id] = (int32_t)v;
    std::vector<int32_t> tip_rank(n_nodes, -1);
    for (size_t i = 0; i < t.tips.size(); i++) tip_rank[t.tips[i]] = (int32_t)i;
    ix.dfs_tip.clear();
    ix.lo.assign(n_nodes, 0); ix.hi.assign(n_nodes, 0);
    std::vector<int32_t> stack{t.root};
    while (!stack.empty()) {      // left first
        const int32_t v = stack.back();
        stack.pop_back();
        const ClusterNode& nd = t.nodes[v];
        if (nd.left < 0) { ix.lo[v] = (uint32_t)ix.dfs_tip.size(); ix.hi[v] = ix.lo[v] + 1; ix.dfs_tip.push_back((uint32_t)tip_rank[v]); }
        else { stack.push_back(nd.right); stack.push_back(nd.left); }
    }
    for (int32_t v : t.post_order) {
        const ClusterNode& nd = t.nodes[v];
        if (nd.left >= 0) { ix.lo[v] = ix.lo[nd.left]; ix.hi[v] = ix.hi[nd.right]; }
    }
    ix.facts.assign(n_nodes, ClusterNodeFacts());
    ix.scratch_max.assign(in.n_assemblies, 0); ix.scratch_count.assign(in.n_assemblies, 0);
}

const ClusterNodeFacts& ClusterQcIndex::node(int32_t v) {
    ClusterNodeFacts& f = facts[v];
    if (f.known) return f;
    f.lo = lo[v]; f.hi = hi[v];
    std::vector<uint64_t> lengths;
    lengths.reserve(f.hi - f.lo);
    for (uint32_t p = f.lo; p < f.hi; p++) {
        const uint32_t s = dfs_tip[p], file = in.assembly[s];
        lengths.push_back(in.seq_len[s]);
        if (in.trusted[s]) f.trusted = 1;
        if (scratch_count[file]++ == 0 || in.cluster_weight[s] > scratch_max[file]) scratch_max[file] = in.cluster_weight[s];
    }
    uint64_t count = 0;
    for (uint32_t p = f.lo; p < f.hi; p++) {      // (every file name of the node once: its count is reset on the way)
        const uint32_t file = in.assembly[dfs_tip[p]];
        if (!scratch_count[file]) continue;
        if (scratch_count[file] == 1) f.ones++;
        count += scratch_max[file];
        scratch_count[file] = 0; scratch_max[file] = 0;
    }
    f.assembly_count = (uint32_t)std::min<uint64_t>(count, 0xFFFFFFFFull);
    std::sort(lengths.begin(), lengths.end());      // median_usize
    const size_t len = lengths.size();
    f.median = len % 2 == 0 ? (lengths[len / 2 - 1] + lengths[len / 2]) / 2 : lengths[len / 2];
    f.dist = t->nodes[v].distance * 2.0;            // max_pairwise_distance
    f.known = 1;
    return f;
}

std::vector<int32_t> cluster_qc_nodes_checked(const ClusterQcIndex& ix, const uint16_t* ids, uint32_t n) {
    if (n && !ids) throw ClusterError("null pointer");
    std::vector<int32_t> nodes(n);
    std::vector<uint8_t> covered(ix.dfs_tip.size(), 0);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n; k++) {
        const int32_t v = ix.node_of_id[ids[k]];
        if (v < 0) throw ClusterError("clustering tree does not contain a node with id " + std::to_string(ids[k]));
        nodes[k] = v;
        for (uint32_t p = ix.lo[v]; p < ix.hi[v]; p++) {      // (stops at the first tip met twice: never more than one pass over the tips)
            if (covered[p]) throw ClusterError("cluster: the clusters overlap at node " + std::to_string(ids[k]) + " (every tip must be in exactly one cluster)");
            covered[p] = 1;
        }
        total += ix.hi[v] - ix.lo[v];
    }
    if (total != covered.size())
        throw ClusterError("cluster: the clusters cover " + std::to_string(total) + " of " + std::to_string(covered.size()) + " tips (every tip must be in exactly one cluster)");
    return nodes;
}

static std::vector<std::vector<uint16_t>> split_lists(const ClusterTree& t, const std::vector<int32_t>& node_of_id, const std::vector<uint16_t>& clusters,
                                                      std::vector<int32_t>* split_node) {
    std::vector<std::pair<std::vector<uint16_t>, int32_t>> lists;
    for (uint16_t c : clusters) {
        const int32_t v = node_of_id[c];
        const ClusterNode& nd = t.nodes[v];
        if (nd.left < 0) continue;
        std::vector<uint16_t> alt;
        alt.reserve(clusters.size() + 1);
        for (uint16_t other : clusters) if (other != c) alt.push_back(other);
        alt.push_back(t.nodes[nd.left].id); alt.push_back(t.nodes[nd.right].id);
        std::sort(alt.begin(), alt.end());
        lists.push_back({std::move(alt), v});
    }
    std::sort(lists.begin(), lists.end(), [](const std::pair<std::vector<uint16_t>, int32_t>& a, const std::pair<std::vector<uint16_t>, int32_t>& b) { return a.first < b.first; });
    std::vector<std::vector<uint16_t>> out;
    if (split_node) split_node->clear();
    for (auto& l : lists) { out.push_back(std::move(l.first)); if (split_node) split_node->push_back(l.second); }
    return out;
}

std::vector<std::vector<uint16_t>> cluster_split_clusters(const ClusterTree& t, const std::vector<uint16_t>& clusters) {
    std::vector<int32_t> node_of_id(65536, -1);
    for (size_t v = 0; v < t.nodes.size(); v++) node_of_id[t.nodes[v].id] = (int32_t)v;
    for (uint16_t c : clusters) if (node_of_id[c] < 0) throw ClusterError("clustering tree does not contain a node with id " + std::to_string(c));
    return split_lists(t, node_of_id, clusters, nullptr);
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------------
uint64_t ClusterQcPlan::pairs_counted() const {
    uint64_t p = (uint64_t)n * (n - 1);
    for (const ClusterQcAlt& a : alts) if (a.kpos != CLUSTER_QC_NONE) p += 4ull * (n - 1) + 2;
    return p;
}

namespace {
struct OrderKey { uint64_t median; uint32_t tie; };      // reorder_clusters: median descending, old number ascending
bool key_less(const OrderKey& a, const OrderKey& b) { return a.median != b.median ? a.median > b.median : a.tie < b.tie; }

ClusterQcEntity entity_of(const ClusterNodeFacts& f, uint32_t min_assemblies) {
    uint32_t flags = f.trusted ? 1u : 0u;
    if (!f.trusted && f.assembly_count < min_assemblies) flags |= 2u;
    return ClusterQcEntity{f.lo, f.hi, flags};
}

// nodes: the clustering in list order (cluster k + 1 = nodes[k]).  split_node empty: the clustering itself is the one alternative; else one
// alternative per entry (a node of `nodes`), in that order, and the list is sorted by id, so that the id stands in for the old number.
void build_plan(ClusterQcIndex& ix, const std::vector<int32_t>& nodes, const std::vector<int32_t>& split_node, uint32_t min_assemblies, ClusterQcPlan* plan) {
    ClusterQcPlan& p = *plan;
    const uint32_t n = (uint32_t)nodes.size();
    const bool by_id = !split_node.empty();
    p.n = n;
    std::vector<std::pair<OrderKey, int32_t>> order(n);
    for (uint32_t k = 0; k < n; k++) order[k] = {OrderKey{ix.node(nodes[k]).median, by_id ? (uint32_t)ix.t->nodes[nodes[k]].id : k}, nodes[k]};
    std::sort(order.begin(), order.end(), [](const std::pair<OrderKey, int32_t>& a, const std::pair<OrderKey, int32_t>& b) { return key_less(a.first, b.first); });
    p.base.resize(n); p.base_node.resize(n);
    std::vector<OrderKey> keys(n);
    for (uint32_t b = 0; b < n; b++) { p.base_node[b] = order[b].second; p.base[b] = entity_of(ix.node(order[b].second), min_assemblies); keys[b] = order[b].first; }
    p.alts.clear(); p.child_node.clear();
    if (!by_id) {
        ClusterQcAlt a{};
        a.kpos = a.ins0 = a.ins1 = CLUSTER_QC_NONE;
        p.alts.push_back(a); p.child_node.push_back({-1, -1});
        return;
    }
    for (int32_t v : split_node) {
        const ClusterNode& nd = ix.t->nodes[v];
        const OrderKey own{ix.node(v).median, nd.id};
        const uint32_t kpos = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), own, key_less) - keys.begin());
        int32_t child[2] = {nd.left, nd.right};
        OrderKey ck[2] = {OrderKey{ix.node(child[0]).median, ix.t->nodes[child[0]].id}, OrderKey{ix.node(child[1]).median, ix.t->nodes[child[1]].id}};
        if (key_less(ck[1], ck[0])) { std::swap(child[0], child[1]); std::swap(ck[0], ck[1]); }
        uint32_t at[2];
        for (int c = 0; c < 2; c++) {      // the clusters of the base, without the split one, that come before this child
            const uint32_t q = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), ck[c], key_less) - keys.begin());
            at[c] = q - (kpos < q ? 1u : 0u);
        }
        ClusterQcAlt a{};
        a.kpos = kpos; a.ins0 = at[0]; a.ins1 = at[1] + 1;
        a.child[0] = entity_of(ix.node(child[0]), min_assemblies); a.child[1] = entity_of(ix.node(child[1]), min_assemblies);
        p.alts.push_back(a); p.child_node.push_back({child[0], child[1]});
    }
}

// one alternative of an evaluated plan as a clustering with its verdicts
struct Scored {
    std::vector<int32_t> order;      // the node behind every reordered cluster
    std::vector<uint32_t> verdict;
    ClusteringMetrics metrics;
};
Scored score_alt(ClusterQcIndex& ix, const ClusterQcPlan& p, uint32_t a, const uint32_t* verdict) {
    Scored s;
    const uint32_t cnt = p.count(a);
    s.order.resize(cnt); s.verdict.assign(verdict, verdict + cnt);
    std::vector<ClusterQcItem> items(cnt);
    for (uint32_t j = 0; j < cnt; j++) {
        const int32_t v = p.node_at(a, j);
        const ClusterNodeFacts& f = ix.node(v);
        s.order[j] = v;
        items[j] = ClusterQcItem{f.hi - f.lo, f.ones, f.dist, (verdict[j] & 7u) == 0};
    }
    s.metrics = cluster_metrics(items.data(), cnt, ix.in.n_assemblies);
    return s;
}

void publish(ClusterQcIndex& ix, const Scored& s, ClusterQcResult* out) {
    out->metrics = s.metrics;
    out->records.resize(s.order.size());
    out->cluster_of_seq.assign(ix.in.n, 0);
    for (size_t j = 0; j < s.order.size(); j++) {
        const ClusterNodeFacts& f = ix.node(s.order[j]);
        ClusterQcRecord& r = out->records[j];
        r.node = ix.t->nodes[s.order[j]].id; r.size = f.hi - f.lo; r.median = f.median; r.assembly_count = f.assembly_count; r.trusted = f.trusted;
        r.cluster_dist = f.dist; r.fail = s.verdict[j] & 7u; r.container = (uint16_t)(s.verdict[j] >> 8);
        for (uint32_t q = f.lo; q < f.hi; q++) out->cluster_of_seq[ix.dfs_tip[q]] = (uint16_t)(j + 1);
    }
}

void check_answer(const ClusterQcPlan& p, const std::vector<uint32_t>& verdicts) {
    if (verdicts.size() != (size_t)p.alts.size() * p.stride()) throw ClusterError("cluster: the verdict chain answered " + std::to_string(verdicts.size()) + " words");
}
}  // namespace

// ---- qc_clusters and generate_clusters ------------------------------------------------------------------------------------------------
void cluster_qc_nodes_host(ClusterQcIndex& ix, const uint16_t* cluster_nodes, uint32_t n_nodes, const uint16_t* manual, uint32_t n_manual,
                           uint32_t min_assemblies, const ClusterQcEvaluate& evaluate, ClusterQcResult* out) {
    if (n_manual && !manual) throw ClusterError("null pointer");
    const std::vector<int32_t> nodes = cluster_qc_nodes_checked(ix, cluster_nodes, n_nodes);
    out->nodes.assign(cluster_nodes, cluster_nodes + n_nodes);
    ClusterQcPlan plan;
    build_plan(ix, nodes, {}, min_assemblies, &plan);
    std::vector<uint32_t> verdicts;
    if (n_manual) {      // the only failure there is: not among the manual clusters.  Nothing is asked of the matrix, and trust rescues nothing
        std::vector<uint8_t> is_manual(65536, 0);
        for (uint32_t i = 0; i < n_manual; i++) is_manual[manual[i]] = 1;
        verdicts.assign(plan.stride(), 0);
        for (uint32_t j = 0; j < plan.n; j++) verdicts[j] = is_manual[ix.t->nodes[plan.base_node[j]].id] ? 0u : (uint32_t)CLUSTER_QC_FAIL_MANUAL;
    } else {
        evaluate(plan, &verdicts);
        check_answer(plan, verdicts);
        out->evaluations++;
    }
    const Scored s = score_alt(ix, plan, 0, verdicts.data());
    out->start_score = s.metrics.overall_clustering_score;
    publish(ix, s, out);
}

void cluster_generate_host(ClusterQcIndex& ix, double cutoff, const uint16_t* manual, uint32_t n_manual, uint32_t min_assemblies,
                           const ClusterQcEvaluate& evaluate, ClusterQcResult* out) {
    std::vector<uint16_t> best = cluster_cut(*ix.t, cutoff, manual, n_manual);      // (nested manual clusters throw here)
    if (n_manual) { cluster_qc_nodes_host(ix, best.data(), (uint32_t)best.size(), manual, n_manual, min_assemblies, evaluate, out); return; }
    ClusterQcPlan plan;
    std::vector<uint32_t> verdicts;
    build_plan(ix, cluster_qc_nodes_checked(ix, best.data(), (uint32_t)best.size()), {}, min_assemblies, &plan);
    evaluate(plan, &verdicts);
    check_answer(plan, verdicts);
    out->evaluations++;
    Scored best_scored = score_alt(ix, plan, 0, verdicts.data());
    double best_score = best_scored.metrics.overall_clustering_score;
    out->start_score = best_score;
    for (bool improved = true; improved;) {      // refine_auto_clusters
        improved = false;
        std::vector<int32_t> split_node;
        std::vector<std::vector<uint16_t>> alts = split_lists(*ix.t, ix.node_of_id, best, &split_node);      // (all from the round's start)
        out->round_alternatives.push_back((uint32_t)alts.size());
        if (alts.empty()) break;
        build_plan(ix, cluster_qc_nodes_checked(ix, best.data(), (uint32_t)best.size()), split_node, min_assemblies, &plan);
        evaluate(plan, &verdicts);
        check_answer(plan, verdicts);
        out->evaluations++;
        for (uint32_t a = 0; a < alts.size(); a++) {
            Scored s = score_alt(ix, plan, a, verdicts.data() + (size_t)a * plan.stride());
            const double alt_score = s.metrics.overall_clustering_score;
            const bool accept = alt_score > best_score + 1e-12;
            out->scores.push_back(alt_score); out->accepted.push_back(accept ? 1 : 0);
            if (accept) { best = alts[a]; best_score = alt_score; best_scored = std::move(s); improved = true; }
        }
    }
    out->nodes = best;
    publish(ix, best_scored, out);
}

}  // namespace ac
