// The host side of the read-based unitig depths (depth.rs of `autocycler combine --reads`): the small graph walks that make the junction and
// context k-mers (extensions, depth.rs:252-279), the sequential arithmetic of a unitig's depth (tig_kmer_counts / clipped_mean, :317-360)
// and the FASTQ reader.  Plain C++ (no device code); the k-mer table and the read tally are kernels_depth.inc.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace ac {

// one consensus graph as the caller's arrays (ac_depth_graph); links = n_links pairs of signed unitig numbers in file order
struct DepthGraphView {
    const uint8_t* seq_bytes; const uint64_t* seq_begin; const uint32_t* seq_len; uint32_t n_unitigs;
    const int32_t* links; uint64_t n_links;
};
// context_kmers (depth.rs:187-232) of all unitigs of a graph, flattened: unitig u owns ctx[ctx_begin[u] .. ctx_begin[u + 1]), offsets
// ascending; an offset's alternatives are kmers[first .. first + count) in the order the reference finds them
struct DepthContext { int32_t offset; uint32_t count; uint64_t first; };
struct DepthGraphPlan {
    std::vector<uint64_t> junction;      // junction_kmers (depth.rs:101-134) of every unitig, one entry per occurrence
    std::vector<uint64_t> kmers;
    std::vector<DepthContext> ctx;
    std::vector<uint64_t> ctx_begin;
};
static const size_t DEPTH_MAX_WALK_STEPS = 10000;      // MAX_WALK_STEPS (depth.rs:42)

// Throws std::runtime_error for a link end that is 0 or beyond the graph.
void depth_plan_graph(uint32_t k, const DepthGraphView& g, uint32_t graph_index, DepthGraphPlan* out);

// clipped_mean (depth.rs:345-360): false = the reference's None
bool depth_clipped_mean(const std::vector<uint32_t>& counts, double* mean);

// Strict four-line FASTQ records, plain or gzip.  `sink` receives whole reads (bases one behind the other, off of n + 1 entries) whenever
// about flush_bytes of them have been collected, and once more at the end.  Throws std::runtime_error for a file that cannot be read or
// that ends inside a record.
void depth_read_fastq(const char* path, size_t flush_bytes,
                      const std::function<void(const std::vector<uint8_t>& bases, const std::vector<uint64_t>& off)>& sink);

}  // namespace ac
