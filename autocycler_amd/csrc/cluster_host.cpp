// The host side of `autocycler cluster` (cluster_host.hpp).  Every walk over a tree is a loop over post_order (or its reverse): a UPGMA
// tree of S tips may be a chain S deep, and no recursion here depends on the depth.
#include "cluster_host.hpp"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdlib>

namespace ac {

void cluster_check_ids(const uint16_t* ids, uint32_t n) {
    if (n == 0) throw ClusterError("cluster: no sequences");
    if (!ids) throw ClusterError("null pointer");
    for (uint32_t i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1]) throw ClusterError("cluster: the sequence ids must ascend strictly (id " + std::to_string(ids[i]) + " follows " + std::to_string(ids[i - 1]) + ")");
    if ((uint64_t)ids[n - 1] + n - 1 > 65535)
        throw ClusterError("cluster: largest id " + std::to_string(ids[n - 1]) + " plus " + std::to_string(n - 1) + " internal nodes is beyond 65535 (the tree's u16 node numbers)");
}

// post_order and tips of a tree whose links are known to be in range; throws unless the links form one tree over all the nodes
static void index_tree(ClusterTree* t) {
    const size_t n = t->nodes.size();
    t->post_order.clear(); t->tips.clear();
    std::vector<uint8_t> seen(n, 0);
    std::vector<std::pair<int32_t, int>> stack{{t->root, 0}};
    seen[t->root] = 1;
    while (!stack.empty()) {
        const int32_t v = stack.back().first;
        const int stage = stack.back().second++;
        const ClusterNode& nd = t->nodes[v];
        if (nd.left < 0 || stage == 2) { t->post_order.push_back(v); stack.pop_back(); continue; }
        const int32_t c = stage == 0 ? nd.left : nd.right;
        if (seen[c]) throw ClusterError("cluster tree: node " + std::to_string(t->nodes[c].id) + " is reached twice");
        seen[c] = 1;
        stack.push_back({c, 0});
    }
    if (t->post_order.size() != n) throw ClusterError("cluster tree: " + std::to_string(n - t->post_order.size()) + " nodes are not below the root");
    for (size_t v = 0; v < n; v++) if (t->nodes[v].left < 0) t->tips.push_back((int32_t)v);
}

void cluster_tree_from_merges(const uint16_t* ids, uint32_t n, const std::vector<ClusterRowMerge>& merges, bool normalise, ClusterTree* out) {
    cluster_check_ids(ids, n);
    if (merges.size() != (size_t)n - 1) throw ClusterError("cluster: " + std::to_string(merges.size()) + " merges for " + std::to_string(n) + " sequences");
    ClusterTree& t = *out;
    t.nodes.clear(); t.merges.clear();
    std::vector<int32_t> node_of(n);      // the tree node of the cluster that carries this row's id
    for (uint32_t i = 0; i < n; i++) { t.nodes.push_back(ClusterNode{ids[i], -1, -1, 0.0}); node_of[i] = (int32_t)i; }
    uint16_t internal = ids[n - 1];
    for (const ClusterRowMerge& m : merges) {
        if (m.a >= m.b || m.b >= n || node_of[m.a] < 0 || node_of[m.b] < 0) throw ClusterError("cluster: the merge loop named a pair that is not two live clusters");
        internal++;
        t.nodes.push_back(ClusterNode{internal, node_of[m.a], node_of[m.b], m.distance / 2.0});
        node_of[m.a] = (int32_t)t.nodes.size() - 1;
        node_of[m.b] = -1;
        t.merges.push_back(ClusterMerge{ids[m.a], ids[m.b], m.distance});
    }
    t.root = (int32_t)t.nodes.size() - 1;
    if (normalise && t.nodes[t.root].distance > 0.5) {      // normalise_tree / scale_node_distance
        const double factor = 0.5 / t.nodes[t.root].distance;
        for (ClusterNode& nd : t.nodes) nd.distance *= factor;
    }
    index_tree(&t);
}

void cluster_tree_from_nodes(const ClusterNode* nodes, uint32_t n_nodes, int32_t root, ClusterTree* out) {
    if (n_nodes == 0 || !nodes) throw ClusterError("cluster tree: no nodes");
    if (root < 0 || (uint32_t)root >= n_nodes) throw ClusterError("cluster tree: the root index is out of range");
    ClusterTree& t = *out;
    t.nodes.assign(nodes, nodes + n_nodes);
    t.merges.clear();
    t.root = root;
    std::vector<uint8_t> used(65536, 0);
    for (const ClusterNode& nd : t.nodes) {
        if ((nd.left < 0) != (nd.right < 0)) throw ClusterError("cluster tree: node " + std::to_string(nd.id) + " has one child");
        if (nd.left >= (int32_t)n_nodes || nd.right >= (int32_t)n_nodes) throw ClusterError("cluster tree: a child index of node " + std::to_string(nd.id) + " is out of range");
        if (nd.left >= 0 && nd.left == nd.right) throw ClusterError("cluster tree: node " + std::to_string(nd.id) + " has the same child twice");
        if (used[nd.id]) throw ClusterError("cluster tree: two nodes with id " + std::to_string(nd.id));
        used[nd.id] = 1;
    }
    index_tree(&t);
}

std::vector<uint16_t> cluster_cut(const ClusterTree& t, double cutoff, const uint16_t* manual, uint32_t n_manual) {
    if (n_manual && !manual) throw ClusterError("null pointer");
    std::vector<uint8_t> is_manual(65536, 0);
    for (uint32_t i = 0; i < n_manual; i++) is_manual[manual[i]] = 1;
    std::vector<uint8_t> has_manual(t.nodes.size(), 0);      // has_manual_child
    for (int32_t v : t.post_order) {
        const ClusterNode& nd = t.nodes[v];
        const bool below = nd.left >= 0 && (has_manual[nd.left] || has_manual[nd.right]);
        if (n_manual && nd.left >= 0 && is_manual[nd.id] && below) throw ClusterError("manual clusters cannot be nested");      // check_consistency
        has_manual[v] = is_manual[nd.id] || below;
    }
    const double half = cutoff / 2.0;
    std::vector<uint16_t> clusters;
    std::vector<int32_t> stack{t.root};
    while (!stack.empty()) {      // collect_clusters
        const ClusterNode& nd = t.nodes[stack.back()];
        const bool manual_here = is_manual[nd.id], has = has_manual[stack.back()];
        stack.pop_back();
        if (manual_here || (nd.distance <= half && !has)) clusters.push_back(nd.id);
        else if (nd.left >= 0) { stack.push_back(nd.right); stack.push_back(nd.left); }
    }
    std::sort(clusters.begin(), clusters.end());
    return clusters;
}

static uint64_t median_u64(std::vector<uint64_t> v) {      // median_usize
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    const size_t len = v.size();
    return len % 2 == 0 ? (v[len / 2 - 1] + v[len / 2]) / 2 : v[len / 2];
}

uint32_t cluster_assign(const ClusterTree& t, const uint16_t* cluster_nodes, uint32_t n, const uint64_t* seq_len, uint16_t* cluster_of_seq,
                        double* cluster_dist) {
    const size_t n_tips = t.tips.size();
    if ((n && !cluster_nodes) || !seq_len || !cluster_of_seq || (n && !cluster_dist)) throw ClusterError("null pointer");
    if (n > 65535) throw ClusterError("cluster: more than 65535 clusters");
    std::vector<int32_t> node_of_id(65536, -1), tip_rank(t.nodes.size(), -1);
    for (size_t v = 0; v < t.nodes.size(); v++) node_of_id[t.nodes[v].id] = (int32_t)v;
    for (size_t i = 0; i < n_tips; i++) { tip_rank[t.tips[i]] = (int32_t)i; cluster_of_seq[i] = 0; }
    std::vector<double> dist_old(n);
    for (uint32_t k = 0; k < n; k++) {
        const int32_t v0 = node_of_id[cluster_nodes[k]];
        if (v0 < 0) throw ClusterError("clustering tree does not contain a node with id " + std::to_string(cluster_nodes[k]));
        std::vector<int32_t> stack{v0};      // assign_cluster_to_node
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            if (t.nodes[v].left < 0) cluster_of_seq[tip_rank[v]] = (uint16_t)(k + 1);
            else { stack.push_back(t.nodes[v].left); stack.push_back(t.nodes[v].right); }
        }
        dist_old[k] = t.nodes[v0].distance * 2.0;      // max_pairwise_distance
    }
    // reorder_clusters
    uint32_t max_cluster = 0;
    for (size_t i = 0; i < n_tips; i++) max_cluster = std::max<uint32_t>(max_cluster, cluster_of_seq[i]);
    std::vector<std::vector<uint64_t>> lengths(max_cluster + 1);
    for (size_t i = 0; i < n_tips; i++) lengths[cluster_of_seq[i]].push_back(seq_len[i]);
    std::vector<std::pair<uint64_t, uint32_t>> order;      // (median, old number)
    for (uint32_t c = 1; c <= max_cluster; c++) order.push_back({median_u64(lengths[c]), c});
    std::sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) {
        return x.first != y.first ? x.first > y.first : x.second < y.second;
    });
    std::vector<uint16_t> old_to_new(max_cluster + 1, 0);
    for (uint32_t i = 0; i < order.size(); i++) old_to_new[order[i].second] = (uint16_t)(i + 1);
    for (size_t i = 0; i < n_tips; i++) if (cluster_of_seq[i]) cluster_of_seq[i] = old_to_new[cluster_of_seq[i]];
    for (uint32_t k = 0; k < n; k++) cluster_dist[k] = -1.0;
    for (uint32_t c = 1; c <= max_cluster; c++) cluster_dist[old_to_new[c] - 1] = dist_old[c - 1];
    return max_cluster;
}

void cluster_containment(const double* asym, uint32_t n, const uint16_t* cluster_of_seq, uint32_t n_clusters, double cutoff,
                         uint64_t* contain_count, uint64_t* total_count) {
    if ((n && (!asym || !cluster_of_seq)) || (n_clusters && (!contain_count || !total_count))) throw ClusterError("null pointer");
    for (uint32_t i = 0; i < n; i++)
        if (cluster_of_seq[i] > n_clusters) throw ClusterError("cluster: sequence " + std::to_string(i) + " carries cluster " + std::to_string(cluster_of_seq[i]) + " of " + std::to_string(n_clusters));
    std::fill(contain_count, contain_count + (size_t)n_clusters * n_clusters, 0);
    std::fill(total_count, total_count + (size_t)n_clusters * n_clusters, 0);
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t ca = cluster_of_seq[a];
        if (!ca) continue;
        for (uint32_t b = 0; b < n; b++) {
            const uint32_t cb = cluster_of_seq[b];
            if (!cb || cb == ca) continue;
            const size_t at = (size_t)(ca - 1) * n_clusters + (cb - 1);
            total_count[at]++;
            const double ab = asym[(size_t)a * n + b], ba = asym[(size_t)b * n + a];
            if (ab < ba && ab < cutoff) contain_count[at]++;
        }
    }
}

// The shortest digits that read back as x (std::to_chars finds the ones Rust's formatter finds), written out without an exponent.  (to_chars'
// own fixed form is not that: from 2^53 on it prints the exact integer instead of the shortest digits followed by zeros.)
std::string cluster_format_f64(double x) {
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x < 0 ? "-inf" : "inf";
    char buf[64];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::scientific);
    const std::string sci(buf, r.ptr);      // [-]d[.ddd]e[+-]XX
    const size_t e = sci.find('e');
    std::string digits;
    for (size_t i = 0; i < e; i++) if (sci[i] >= '0' && sci[i] <= '9') digits += sci[i];
    const int exp10 = atoi(sci.c_str() + e + 1);
    const int nd = (int)digits.size();
    std::string out = sci[0] == '-' ? "-" : "";
    if (exp10 >= nd - 1) out += digits + std::string((size_t)(exp10 - (nd - 1)), '0');
    else if (exp10 >= 0) out += digits.substr(0, (size_t)exp10 + 1) + "." + digits.substr((size_t)exp10 + 1);
    else out += "0." + std::string((size_t)(-exp10 - 1), '0') + digits;
    return out;
}

std::string cluster_newick(const ClusterTree& t, const char* const* tip_names, bool file_form) {
    std::vector<std::string> text(t.nodes.size());
    std::vector<int32_t> tip_rank(t.nodes.size(), -1);
    for (size_t i = 0; i < t.tips.size(); i++) tip_rank[t.tips[i]] = (int32_t)i;
    for (int32_t v : t.post_order) {
        const ClusterNode& nd = t.nodes[v];
        if (nd.left < 0) {
            const char* name = tip_names ? tip_names[tip_rank[v]] : nullptr;
            text[v] = name ? std::string(name) : std::to_string(nd.id);
            continue;
        }
        std::string& l = text[nd.left];
        std::string& r = text[nd.right];
        std::string s;
        s.reserve(l.size() + r.size() + 64);
        s += '('; s += l; s += ':'; s += cluster_format_f64(nd.distance - t.nodes[nd.left].distance);
        s += ','; s += r; s += ':'; s += cluster_format_f64(nd.distance - t.nodes[nd.right].distance);
        s += ')'; s += std::to_string(nd.id);
        std::string().swap(l); std::string().swap(r);
        text[v].swap(s);
    }
    std::string& whole = text[t.root];
    if (!file_form) return whole;
    const double root_distance = t.nodes[t.root].distance;
    if (root_distance < 0.5) return "(" + whole + ":" + cluster_format_f64(0.5 - root_distance) + ");\n";
    return whole + ";\n";
}

}  // namespace ac
