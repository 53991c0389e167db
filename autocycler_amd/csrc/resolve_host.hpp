// `autocycler resolve` up to the point where the graph is edited: anchors (resolve.rs:134-163), bridges with their best paths
// (create_bridges :166-190, Bridge::new :430-462), ambiguity (:193-220) and culling (:285-313) — plain C++, no device code.
// The quadratic step, global_alignment_distance (:387-418) of every pair of a bridge's paths, is handed to the caller's batch
// function (the device: kernels_resolve.inc); everything here is O(path entries) plus the sorts.
// Not done here (the caller applies the bridges): apply_bridges, reduce_depths, merge_linear_paths.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

namespace ac {

// Paths one behind the other: path p = entries[off[p] .. off[p + 1]).
struct PathPool {
    std::vector<int32_t> entries;
    std::vector<uint64_t> off{0};
    size_t size() const { return off.size() - 1; }
    const int32_t* at(size_t p) const { return entries.data() + off[p]; }
    uint64_t len(size_t p) const { return off[p + 1] - off[p]; }
    void add(const int32_t* p, uint64_t n) { entries.insert(entries.end(), p, p + n); off.push_back(entries.size()); }
};
struct PathPair { uint32_t a, b; };      // two paths of a pool
// dist[i] = global_alignment_distance of pairs[i] (every pair handed over has passed pair_overflows)
typedef std::function<void(const PathPool&, const std::vector<PathPair>&, std::vector<uint32_t>&)> DistanceBatchFn;

// sequence.rs:104-109: the first whitespace-separated token of the lowercased header that starts with autocycler_consensus_weight= and
// whose rest parses as an unsigned integer; 1 without one.  (ASCII lowercasing and ASCII whitespace: the prefix is ASCII.)  Throws when
// the value is 2^32 or more.
uint32_t consensus_weight_of(const char* header);

// throws std::runtime_error: an entry that is 0 or names a unitig beyond the weights (weights[u - 1] = w(u), as for trim)
void validate_resolve_path(const int32_t* path, uint64_t n, uint32_t n_weights, const char* what);
uint64_t path_weight(const int32_t* path, uint64_t n, const uint32_t* weights);
// true: some cell of the reference's u32 matrix could overflow (the two paths' weights add up to 2^32 or more) — status 2, never launched
inline bool pair_overflows(uint64_t weight_a, uint64_t weight_b) { return weight_a + weight_b >= ((uint64_t)1 << 32); }
// Rust's Vec<i32> order: elementwise, then by length
int compare_paths(const int32_t* a, uint64_t n, const int32_t* b, uint64_t m);
// Bridge::cmp (resolve.rs:506-514) on (start, end): unique per bridge, so the best path never decides
bool bridge_less(int32_t start_a, int32_t end_a, int32_t start_b, int32_t end_b);

struct ResolveBridge {
    int32_t start = 0, end = 0;
    uint32_t depth = 0;                 // Bridge::depth: paths of the bridge, copies counted
    uint32_t n_distinct = 0;            // distinct paths; they are pool paths [first_distinct, first_distinct + n_distinct) of ResolveResult::distinct
    uint64_t first_distinct = 0;
    uint64_t best_off = 0;              // best path = best_pool[best_off .. best_off + best_len)
    uint32_t best_len = 0;
    uint64_t best_total = 0;            // sum of the distances from the best path to all others
    uint32_t status = 0;                // 0 fine; 2 the reference's u32 arithmetic would overflow: no best path
    uint32_t conflicting = 0;           // determine_ambiguity on all bridges
    uint32_t culled = 0, cull_rank = 0; // cull_ambiguity: culled as the cull_rank-th (1-based; 0: kept)
};
struct ResolveResult {
    std::vector<uint32_t> anchors;      // unitig numbers, ascending
    std::vector<ResolveBridge> bridges; // in Bridge::cmp order
    std::vector<int32_t> best_pool;
    PathPool distinct;                  // the bridges' distinct paths (start and end stripped), each bridge's in ascending path order
    std::vector<uint32_t> multiplicity; // per distinct path
    uint64_t pairs = 0, pairs_overflowing = 0;
};

// find_anchor_unitigs: unitigs whose occurrences (either strand) per sequence id are exactly the sequences' ids.  seq_ids may be null
// (every sequence its own id).
std::vector<uint32_t> find_anchors(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint16_t* seq_ids, uint32_t n_unitigs);
// get_anchor_to_anchor_paths (resolve.rs:344-365) of one path, appended to out
void anchor_to_anchor_paths(const int32_t* path, uint64_t n, const std::vector<uint8_t>& is_anchor, PathPool* out);
// determine_ambiguity (resolve.rs:193-220) over the bridges with alive[i] != 0
void determine_ambiguity(const std::vector<ResolveBridge>& bridges, const std::vector<uint8_t>& alive, std::vector<uint8_t>* conflicting);

// The whole of it.  consensus_weight may be null (all 1).  The paths must have passed validate_resolve_path.
void resolve_bridges_host(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint16_t* seq_ids, const uint32_t* consensus_weight,
                          const uint32_t* weights, uint32_t n_weights, const DistanceBatchFn& run, ResolveResult* out);

}  // namespace ac
