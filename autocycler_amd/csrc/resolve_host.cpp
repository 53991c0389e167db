// Host side of ac_resolve_bridges (resolve_host.hpp): the reference's anchors, bridges, ambiguity and culling restated over plain arrays.
#include "resolve_host.hpp"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace ac {

uint32_t consensus_weight_of(const char* header) {
    static const char PREFIX[] = "autocycler_consensus_weight=";
    const size_t plen = sizeof PREFIX - 1;
    std::string h(header ? header : "");
    for (char& c : h) if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    auto is_space = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    size_t i = 0;
    while (i < h.size()) {
        while (i < h.size() && is_space(h[i])) i++;
        size_t j = i;
        while (j < h.size() && !is_space(h[j])) j++;
        if (j - i > plen && h.compare(i, plen, PREFIX) == 0) {
            // str::parse::<usize>: an optional '+', then digits only; a value beyond usize is an error and the search goes on
            size_t q = i + plen;
            if (h[q] == '+') q++;
            bool ok = q < j;
            unsigned __int128 v = 0;
            for (; ok && q < j; q++) {
                if (h[q] < '0' || h[q] > '9') ok = false;
                else { v = v * 10 + (unsigned)(h[q] - '0'); if (v > (unsigned __int128)UINT64_MAX) ok = false; }
            }
            if (ok) {
                if (v > 0xFFFFFFFFull) throw std::runtime_error("a consensus weight of 2^32 or more (" + h.substr(i, j - i) + ")");
                return (uint32_t)v;
            }
        }
        i = j;
    }
    return 1;
}

static uint32_t unitig_of(int32_t e) { return (uint32_t)(e < 0 ? -(int64_t)e : (int64_t)e); }

void validate_resolve_path(const int32_t* path, uint64_t n, uint32_t n_weights, const char* what) {
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t u = unitig_of(path[i]);
        if (u == 0 || u > n_weights)
            throw std::runtime_error(std::string(what) + ": entry " + std::to_string(i) + " (" + std::to_string(path[i]) + ") names no unitig of the " +
                                     std::to_string(n_weights) + " that have a weight");
    }
}

uint64_t path_weight(const int32_t* path, uint64_t n, const uint32_t* weights) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) sum += weights[unitig_of(path[i]) - 1];
    return sum;
}

int compare_paths(const int32_t* a, uint64_t n, const int32_t* b, uint64_t m) {
    const uint64_t c = std::min(n, m);
    for (uint64_t i = 0; i < c; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return n == m ? 0 : (n < m ? -1 : 1);
}

bool bridge_less(int32_t start_a, int32_t end_a, int32_t start_b, int32_t end_b) {
    const uint32_t sa = unitig_of(start_a), sb = unitig_of(start_b);
    if (sa != sb) return sa < sb;
    if (start_a != start_b) return start_b < start_a;      // other.start.cmp(&self.start): the forward strand first
    const uint32_t ea = unitig_of(end_a), eb = unitig_of(end_b);
    if (ea != eb) return ea < eb;
    return end_b < end_a;
}

// unitig.forward_positions holds one Position per occurrence of the unitig in a P line, on EITHER strand: from_gfa_lines adds the
// forward path's +u entries (unitig_graph.rs:155, :165-167) and, through the reversed path whose strands are flipped (:154, :156), the
// forward path's -u entries as +u.  find_anchor_unitigs compares the SORTED seq ids of those positions with the sorted ids of all sequences
// (resolve.rs:139-146): a multiset equality, i.e. per id as many occurrences as there are sequences of that id — once per sequence when the
// ids are distinct, which they are in every GFA the pipeline writes.
std::vector<uint32_t> find_anchors(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint16_t* seq_ids, uint32_t n_unitigs) {
    std::vector<uint32_t> order(n_seqs);
    std::iota(order.begin(), order.end(), 0u);
    if (seq_ids) std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return seq_ids[a] < seq_ids[b]; });
    std::vector<uint32_t> count(n_unitigs + 1, 0), groups_ok(n_unitigs + 1, 0), touched;
    std::vector<uint8_t> uneven(n_unitigs + 1, 0);      // occurs under some id, but not as often as there are sequences of that id
    uint32_t n_groups = 0;
    for (uint32_t g0 = 0; g0 < n_seqs;) {
        uint32_t g1 = g0 + 1;
        while (seq_ids && g1 < n_seqs && seq_ids[order[g1]] == seq_ids[order[g0]]) g1++;
        touched.clear();
        for (uint32_t q = g0; q < g1; q++)
            for (uint64_t i = off[order[q]]; i < off[order[q] + 1]; i++) {
                const uint32_t u = unitig_of(path[i]);
                if (count[u]++ == 0) touched.push_back(u);
            }
        for (uint32_t u : touched) {
            if (count[u] == g1 - g0) groups_ok[u]++; else uneven[u] = 1;
            count[u] = 0;
        }
        n_groups++;
        g0 = g1;
    }
    std::vector<uint32_t> anchors;
    for (uint32_t u = 1; u <= n_unitigs; u++)
        if (groups_ok[u] == n_groups && !uneven[u]) anchors.push_back(u);
    return anchors;
}

void anchor_to_anchor_paths(const int32_t* path, uint64_t n, const std::vector<uint8_t>& is_anchor, PathPool* out) {
    bool have = false;
    uint64_t last = 0;
    std::vector<int32_t> rev;
    for (uint64_t i = 0; i < n; i++) {
        if (!is_anchor[unitig_of(path[i])]) continue;
        if (have) {
            const int32_t* fwd = path + last;
            const uint64_t len = i - last + 1;
            rev.resize(len);
            for (uint64_t q = 0; q < len; q++) rev[q] = -fwd[len - 1 - q];
            if (compare_paths(fwd, len, rev.data(), len) > 0) out->add(fwd, len); else out->add(rev.data(), len);
        }
        have = true;
        last = i;
    }
}

void determine_ambiguity(const std::vector<ResolveBridge>& bridges, const std::vector<uint8_t>& alive, std::vector<uint8_t>* conflicting) {
    std::unordered_map<int32_t, uint32_t> start_count, end_count;
    for (size_t i = 0; i < bridges.size(); i++) {
        if (!alive[i]) continue;
        start_count[bridges[i].start]++; start_count[-bridges[i].end]++;      // start, rev_start
        end_count[bridges[i].end]++; end_count[-bridges[i].start]++;          // end, rev_end
    }
    conflicting->assign(bridges.size(), 0);
    for (size_t i = 0; i < bridges.size(); i++) {
        if (!alive[i]) continue;
        const ResolveBridge& b = bridges[i];
        (*conflicting)[i] = start_count[b.start] > 1 || start_count[-b.end] > 1 || end_count[b.end] > 1 || end_count[-b.start] > 1;
    }
}

void resolve_bridges_host(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint16_t* seq_ids, const uint32_t* consensus_weight,
                          const uint32_t* weights, uint32_t n_weights, const DistanceBatchFn& run, ResolveResult* out) {
    *out = ResolveResult();
    out->anchors = find_anchors(path, off, n_seqs, seq_ids, n_weights);
    std::vector<uint8_t> is_anchor(n_weights + 1, 0);
    for (uint32_t u : out->anchors) is_anchor[u] = 1;

    // create_bridges: a sequence's anchor-to-anchor paths count consensus-weight times (resolve.rs:174-178 repeats the whole path)
    PathPool all;
    std::vector<uint32_t> times;
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint32_t w = consensus_weight ? consensus_weight[s] : 1;
        if (w == 0) continue;
        anchor_to_anchor_paths(path + off[s], off[s + 1] - off[s], is_anchor, &all);
        times.resize(all.size(), w);
    }
    // group_paths_by_start_end, the bridges in Bridge::cmp order, and inside a bridge equal paths next to each other
    std::vector<uint32_t> order(all.size());
    std::iota(order.begin(), order.end(), 0u);
    auto first_of = [&](uint32_t p) { return all.at(p)[0]; };
    auto last_of = [&](uint32_t p) { return all.at(p)[all.len(p) - 1]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (first_of(a) != first_of(b) || last_of(a) != last_of(b)) return bridge_less(first_of(a), last_of(a), first_of(b), last_of(b));
        return compare_paths(all.at(a) + 1, all.len(a) - 2, all.at(b) + 1, all.len(b) - 2) < 0;      // (as stripped: the order of the distinct paths)
    });
    std::vector<uint64_t> weight_of_distinct;
    for (size_t q0 = 0; q0 < order.size();) {
        ResolveBridge br;
        br.start = first_of(order[q0]); br.end = last_of(order[q0]);
        br.first_distinct = out->distinct.size();
        uint64_t depth = 0;
        size_t q = q0;
        while (q < order.size() && first_of(order[q]) == br.start && last_of(order[q]) == br.end) {
            const uint32_t p = order[q];
            uint64_t mult = 0;
            while (q < order.size() && compare_paths(all.at(order[q]), all.len(order[q]), all.at(p), all.len(p)) == 0) mult += times[order[q++]];
            if (mult > 0xFFFFFFFFull) throw std::runtime_error("a bridge path occurs 2^32 times or more");
            out->distinct.add(all.at(p) + 1, all.len(p) - 2);      // (Bridge::new strips the two anchors)
            out->multiplicity.push_back((uint32_t)mult);
            weight_of_distinct.push_back(path_weight(all.at(p) + 1, all.len(p) - 2, weights));
            depth += mult;
        }
        if (depth > 0xFFFFFFFFull) throw std::runtime_error("a bridge of 2^32 paths or more");
        br.depth = (uint32_t)depth;
        br.n_distinct = (uint32_t)(out->distinct.size() - br.first_distinct);
        out->bridges.push_back(br);
        q0 = q;
    }

    // Bridge::new: every unordered pair of distinct paths is one distance job; copies of a path are at distance 0 from each other
    std::vector<PathPair> pairs;
    std::vector<uint64_t> first_pair(out->bridges.size() + 1, 0);
    for (size_t b = 0; b < out->bridges.size(); b++) {
        ResolveBridge& br = out->bridges[b];
        first_pair[b] = pairs.size();
        const uint64_t f = br.first_distinct, n = br.n_distinct;
        out->pairs += n * (n - 1) / 2;
        uint64_t big1 = 0, big2 = 0;      // the two heaviest paths: if that pair cannot overflow, none can
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t w = weight_of_distinct[f + i];
            if (w > big1) { big2 = big1; big1 = w; } else if (w > big2) big2 = w;
        }
        if (n >= 2 && pair_overflows(big1, big2)) {
            br.status = 2;
            for (uint64_t i = 0; i < n; i++)
                for (uint64_t j = i + 1; j < n; j++) out->pairs_overflowing += pair_overflows(weight_of_distinct[f + i], weight_of_distinct[f + j]);
            continue;
        }
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t j = i + 1; j < n; j++) pairs.push_back(PathPair{(uint32_t)(f + i), (uint32_t)(f + j)});
    }
    first_pair[out->bridges.size()] = pairs.size();
    if (out->distinct.size() > 0xFFFFFFFFull) throw std::runtime_error("2^32 distinct bridge paths or more");
    std::vector<uint32_t> dist;
    if (!pairs.empty()) {
        run(out->distinct, pairs, dist);
        if (dist.size() != pairs.size()) throw std::runtime_error("resolve: internal error (the distance batch lost jobs)");
    }

    // the path with the lowest sum of distances to all others; ties go to the smaller path (the distinct paths ascend: the first minimum)
    std::vector<uint64_t> total;
    for (size_t b = 0; b < out->bridges.size(); b++) {
        ResolveBridge& br = out->bridges[b];
        if (br.status != 0) continue;
        const uint64_t f = br.first_distinct, n = br.n_distinct;
        total.assign(n, 0);
        auto add = [&](uint64_t i, uint64_t x) { if (__builtin_add_overflow(total[i], x, &total[i])) total[i] = UINT64_MAX; };
        uint64_t q = first_pair[b];
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t j = i + 1; j < n; j++, q++) {
                add(i, (uint64_t)out->multiplicity[f + j] * dist[q]);
                add(j, (uint64_t)out->multiplicity[f + i] * dist[q]);
            }
        uint64_t best = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (total[i] >= 0xFFFFFFFFull) br.status = 2;      // (the reference adds in u32, from best_total = u32::MAX)
            if (total[i] < total[best]) best = i;
        }
        if (br.status != 0) continue;
        br.best_total = total[best];
        br.best_off = out->best_pool.size();
        br.best_len = (uint32_t)out->distinct.len(f + best);
        out->best_pool.insert(out->best_pool.end(), out->distinct.at(f + best), out->distinct.at(f + best) + br.best_len);
    }

    // determine_ambiguity, then cull_ambiguity: the conflicting bridge smallest by (depth, Bridge::cmp) goes, the flags are recomputed
    std::vector<uint8_t> alive(out->bridges.size(), 1), conflicting;
    determine_ambiguity(out->bridges, alive, &conflicting);
    for (size_t b = 0; b < out->bridges.size(); b++) out->bridges[b].conflicting = conflicting[b];
    for (uint32_t rank = 1;; rank++) {
        size_t pick = out->bridges.size();
        for (size_t b = 0; b < out->bridges.size(); b++) {      // (the bridges are in Bridge::cmp order: the first of the lowest depth)
            if (!alive[b] || !conflicting[b]) continue;
            if (pick == out->bridges.size() || out->bridges[b].depth < out->bridges[pick].depth) pick = b;
        }
        if (pick == out->bridges.size()) break;
        out->bridges[pick].culled = 1; out->bridges[pick].cull_rank = rank;
        alive[pick] = 0;
        determine_ambiguity(out->bridges, alive, &conflicting);
    }
}

}  // namespace ac
