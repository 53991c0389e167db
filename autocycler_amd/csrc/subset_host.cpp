// The host side of the sequence subsets (subset_host.hpp): checks, sequence lists, path ends, records, densify, error texts.
#include "subset_host.hpp"

#include <algorithm>
#include <stdexcept>

namespace ac {

void subset_prepare(uint32_t n_seqs, const int32_t* path_entries, const uint64_t* path_off, const uint16_t* cluster_of_seq, uint32_t n_clusters, SubsetPlan* plan,
                    SubsetResult* r) {
    if (n_clusters == 0 || n_clusters > 65535)
        throw std::runtime_error("subsets: n_clusters is " + std::to_string(n_clusters) + ": it must be between 1 and 65535");
    if (!path_off) throw std::runtime_error("null pointer: path_off");
    if (!cluster_of_seq) throw std::runtime_error("null pointer: cluster_of_seq");
    r->n_clusters = n_clusters; r->n_seqs = n_seqs;
    // a stable counting sort of the sequences by label: cluster after cluster, ascending index inside
    std::vector<uint64_t> count((size_t)n_clusters + 1, 0), ends((size_t)n_clusters + 1, 0);
    for (uint32_t s = 0; s < n_seqs; s++) {
        if (path_off[s + 1] < path_off[s])
            throw std::runtime_error("subsets: path_off decreases at sequence " + std::to_string(s) + " (" + std::to_string(path_off[s]) + " then " +
                                     std::to_string(path_off[s + 1]) + "): path offsets must ascend");
        const uint32_t c = cluster_of_seq[s];
        if (c > n_clusters)
            throw std::runtime_error("subsets: sequence " + std::to_string(s) + " has label " + std::to_string(c) + ", above n_clusters = " + std::to_string(n_clusters));
        if (c == 0) continue;
        count[c]++;
        if (path_off[s + 1] > path_off[s]) ends[c]++;
    }
    if (n_seqs && path_off[n_seqs] > path_off[0] && !path_entries) throw std::runtime_error("null pointer: path_entries");
    r->seq_off.assign((size_t)n_clusters + 1, 0); r->ends_off.assign((size_t)n_clusters + 1, 0);
    for (uint32_t c = 1; c <= n_clusters; c++) { r->seq_off[c] = r->seq_off[c - 1] + count[c]; r->ends_off[c] = r->ends_off[c - 1] + ends[c]; }
    const size_t n_kept = (size_t)r->seq_off[n_clusters];
    r->seq_index.assign(n_kept, 0); r->path_ends.assign(2 * (size_t)r->ends_off[n_clusters], 0);
    plan->kept_seq.assign(n_kept, 0); plan->kept_label.assign(n_kept, 0); plan->kept_off.assign(n_kept + 1, 0);
    std::vector<uint64_t> at(r->seq_off.begin(), r->seq_off.end() - 1), end_at(r->ends_off.begin(), r->ends_off.end() - 1);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint32_t c = cluster_of_seq[s];
        if (c == 0) continue;
        const size_t i = (size_t)at[c - 1]++;
        r->seq_index[i] = s; plan->kept_seq[i] = s; plan->kept_label[i] = c;
        plan->kept_off[i + 1] = path_off[s + 1] - path_off[s];      // (lengths now, offsets below)
        if (path_off[s + 1] > path_off[s]) {
            const size_t e = (size_t)end_at[c - 1]++;
            r->path_ends[2 * e] = path_entries[path_off[s]]; r->path_ends[2 * e + 1] = path_entries[path_off[s + 1] - 1];
        }
    }
    for (size_t i = 0; i < n_kept; i++) plan->kept_off[i + 1] += plan->kept_off[i];
    r->kept_entries = plan->kept_entries();
}

void subset_empty_products(SubsetResult* r) {
    const size_t c1 = (size_t)r->n_clusters + 1;
    r->unitig_off.assign(c1, 0); r->length_at.assign(c1, 0); r->link_off.assign(c1, 0);
    r->unitigs.clear(); r->positions.clear(); r->links.clear();
}

void subset_finish(SubsetResult* r, const SubsetPlan& plan) {
    const uint32_t nc = r->n_clusters;
    const size_t c1 = (size_t)nc + 1;
    if (r->unitig_off.size() != c1 || r->length_at.size() != c1 || r->link_off.size() != c1 || r->seq_off.size() != c1 || r->ends_off.size() != c1 ||
        r->unitig_off[0] != 0 || r->link_off[0] != 0 || r->unitig_off[nc] != r->unitigs.size() || r->unitigs.size() != r->positions.size() ||
        r->link_off[nc] != r->links.size())
        throw std::runtime_error("subsets: the result arrays do not fit together (internal error)");
    r->records.assign(nc, SubsetClusterRecord{0, 0, 0, 0, 0});
    uint64_t positions = 0;
    for (uint32_t c = 0; c < nc; c++) {
        if (r->unitig_off[c + 1] < r->unitig_off[c] || r->link_off[c + 1] < r->link_off[c] || r->length_at[c + 1] < r->length_at[c])
            throw std::runtime_error("subsets: an offsets array descends (internal error)");
        SubsetClusterRecord& rec = r->records[c];
        rec.seqs = (uint32_t)(r->seq_off[c + 1] - r->seq_off[c]);
        rec.unitigs = (uint32_t)(r->unitig_off[c + 1] - r->unitig_off[c]);
        rec.entries = plan.kept_off[(size_t)r->seq_off[c + 1]] - plan.kept_off[(size_t)r->seq_off[c]];
        rec.links = r->link_off[c + 1] - r->link_off[c];
        rec.length = r->length_at[c + 1] - r->length_at[c];
        uint64_t sum = 0;
        for (uint64_t p = r->unitig_off[c]; p < r->unitig_off[c + 1]; p++) sum += r->positions[(size_t)p];
        if (sum != rec.entries) throw std::runtime_error("subsets: the position counts of cluster " + std::to_string(c + 1) + " do not add up to its path entries (internal error)");
        positions += sum;
    }
    if (positions != r->kept_entries) throw std::runtime_error("subsets: the position counts do not add up to the kept entries (internal error)");
}

void subset_check_cluster(const SubsetResult& r, uint32_t cluster) {
    if (cluster == 0 || cluster > r.n_clusters)
        throw std::runtime_error("subsets: cluster " + std::to_string(cluster) + " does not exist: clusters run from 1 to " + std::to_string(r.n_clusters));
}

void subset_dense(const SubsetResult& r, uint32_t cluster, uint8_t* alive, uint32_t* fwd, uint32_t* rev, double* depth) {
    subset_check_cluster(r, cluster);
    const uint32_t n = r.n_unitigs;
    if (alive) std::fill(alive, alive + n, (uint8_t)0);
    if (fwd) std::fill(fwd, fwd + n, 0u);
    if (rev) std::fill(rev, rev + n, 0u);
    if (depth) std::fill(depth, depth + n, 0.0);
    for (uint64_t p = r.unitig_off[cluster - 1]; p < r.unitig_off[cluster]; p++) {
        const uint32_t u = r.unitigs[(size_t)p] - 1, count = r.positions[(size_t)p];
        if (alive) alive[u] = 1;
        if (fwd) fwd[u] = count;
        if (rev) rev[u] = count;
        if (depth) depth[u] = (double)count;      // recalculate_depth (unitig.rs:260-262): forward_positions.len() as f64
    }
}

void subset_locate(const SubsetPlan& plan, uint64_t j, uint32_t* seq, uint64_t* index) {
    // the last kept sequence whose entries begin at or before j (sequences without entries share their successor's offset)
    const size_t r = (size_t)(std::upper_bound(plan.kept_off.begin(), plan.kept_off.end() - 1, j) - plan.kept_off.begin()) - 1;
    *seq = plan.kept_seq[r]; *index = j - plan.kept_off[r];
}

std::string subset_bad_entry_message(uint32_t seq, uint64_t index, int32_t entry, uint32_t n) {
    return "subsets: entry " + std::to_string(index) + " of the path of sequence " + std::to_string(seq) + " (" + std::to_string(entry) +
           ") names no unitig: unitig numbers run from 1 to " + std::to_string(n);
}
std::string subset_dead_entry_message(uint32_t seq, uint64_t index, int32_t entry) {
    return "subsets: entry " + std::to_string(index) + " of the path of sequence " + std::to_string(seq) + " (" + std::to_string(entry) +
           ") enters a unitig that is not alive in the input";
}
std::string merged_paths_inside_message(uint32_t seq, bool begins, int32_t entry, uint32_t chain_number) {
    return "merged paths: the path of sequence " + std::to_string(seq) + (begins ? " begins" : " ends") + " strictly inside chain " + std::to_string(chain_number) +
           " (entry " + std::to_string(entry) + "): the plan was not made from these paths";
}
std::string merged_paths_length_message(uint32_t seq) {
    return "merged paths: the path of sequence " + std::to_string(seq) + " changes its length over the merged unitigs: the plan was not made from these paths";
}

}  // namespace ac
