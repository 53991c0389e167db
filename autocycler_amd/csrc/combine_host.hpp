// `autocycler combine` (combine.rs:28-54, 107-127, 144-224) and `autocycler gfa2fasta` (gfa2fasta.rs:56-83) — the host side: the input as the
// C ABI takes it, the loader of the cluster GFAs (segment numbers in any order and with holes, dangling L lines dropped, P lines ignored), the
// records the device fills, cluster_depth's literal sequential sum, the three texts and the error texts.  Plain C++, no device code; the
// ordering, the offsets, the per-unitig end tests and the L-line order are kernels_combine.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"

namespace ac {

// ac_combined_cluster, field for field: one per graph in output order (the device writes these records)
struct CombineClusterRecord {
    uint32_t input_index;         // the graph's place in the caller's list
    uint32_t unitigs;
    uint64_t length;              // total_length()
    uint64_t links;               // entries of the graph's link list (one per L line kept)
    uint64_t offset;              // what combine_clusters adds to the graph's numbers: the sum of the maxima before it
    uint32_t max_number;          // max_unitig_number(), 0 for an empty graph
    uint32_t topology;            // TOPO_* (components_host.hpp)
    uint32_t has_read_depth;      // cluster_depth is Some
    uint32_t reserved;
    double read_depth;            // cluster_depth (0 where it is None); the yaml prints it with one decimal
};
// ac_combined_unitig, field for field: one per unitig in output order
struct CombineUnitigRecord {
    uint32_t graph;               // the input index of its graph
    uint32_t index;               // its place in its graph's file order, from 0
    uint32_t number;              // printed: its own number + the graph's offset
    uint32_t length;
    double depth;                 // printed in DP:f: the caller's depth, or with read depths the read depth (0.0 where it is None)
    double read_depth;            // 0 where has_read_depth is 0
    uint8_t has_read_depth, flags /* CUF_* */, type /* MERGE_TYPE_* */, reserved[5];
};

struct CombineInput {
    uint32_t n_graphs = 0;
    const uint64_t* unitig_off = nullptr;      // n_graphs + 1
    const uint64_t* link_off = nullptr;        // n_graphs + 1
    const uint32_t* number = nullptr;          // per unitig of the concatenation: its own number
    const uint32_t* len = nullptr;
    const double* depth = nullptr;             // or nullptr = 0
    const uint8_t* type = nullptr;             // MERGE_TYPE_*, or nullptr = Other
    const Link* links = nullptr;               // signed 1-based file-order indices within their graph, in L-line order
    const double* read_depth = nullptr;        // both or neither: with them the result is `combine --reads`
    const uint8_t* has_read_depth = nullptr;
    uint64_t n_unitigs() const { return unitig_off[n_graphs]; }
    uint64_t n_links() const { return link_off[n_graphs]; }
};
struct CombineResult {
    std::vector<CombineClusterRecord> clusters;      // output order
    std::vector<CombineUnitigRecord> unitigs;        // output order
    std::vector<Link> links;                         // printed numbers, get_links_for_gfa order, graph after graph
    std::vector<uint64_t> link_off;                  // clusters.size() + 1: a cluster's links in `links`
    std::vector<uint64_t> unitig_off;                // clusters.size() + 1
    bool with_reads = false;
    uint64_t bases = 0, n_unitigs = 0;
    bool fully_resolved = true;
    StepStats stats;
};

// Null pointers, at least one graph, offsets that start at 0 and ascend, sizes the device's indices hold, the total of bases below 2^46.
// Throws std::runtime_error.
void combine_prepare(const CombineInput& in);
// the result for an input without any unitig (every graph empty): nothing is launched
void combine_without_unitigs(const CombineInput& in, CombineResult* out);
// link_off / unitig_off, cluster_depth (the literal sequential f64 sum in unitig order), the totals and fully_resolved
void combine_finish(CombineResult* r);

// Rust's {:.N} of an f64 (N = 1, 2): glibc's correctly rounded %.Nf for finite values, "NaN", "inf", "-inf" otherwise
std::string combine_fixed(double v, int decimals);
// what serde_yaml 0.9 prints for the f64 that the one-decimal text of v parses to
std::string combine_yaml_number(double v);

// One unitig's bytes for the texts: seq[i] points at unitig i (output order) of length unitigs[i].length
std::string combine_gfa_string(const CombineResult& r, const std::vector<const char*>& seq);
std::string combine_fasta_string(const CombineResult& r, const std::vector<const char*>& seq);
std::string combine_yaml_string(const CombineResult& r);
// combine.rs:94-104's lines: "Sequence depths:\n  N length=L depth=D\n..." (empty without reads)
std::string combine_depth_lines(const CombineResult& r);

// A cluster GFA as combine loads it (UnitigGraph::from_gfa_file): S lines in file order with their numbers, depths and colours, L lines in
// file order mapped to signed 1-based file-order indices, an L line naming a missing segment dropped; H and P lines ignored.  Two S lines
// with one number: a link naming it goes to the last, as the reference's index would have it (the combine itself then refuses the graph).
// The bytes stay in the text: seq_at[i] is the offset of unitig i's sequence.  Throws std::runtime_error with the reference's texts.
struct CombineGfa {
    std::vector<uint32_t> number, len;
    std::vector<double> depth;
    std::vector<uint8_t> type;
    std::vector<uint64_t> seq_at;
    std::vector<Link> links;
};
void combine_load_gfa(const char* text, uint64_t len, CombineGfa* g);
// gfa2fasta's text of one graph (no offset; unitigs with an empty sequence skipped) from its flags; counts: circular, linear, other
std::string combine_gfa2fasta_string(const CombineGfa& g, const char* text, const uint8_t* flags, uint64_t counts[3]);

std::string combine_duplicate_message(uint32_t graph, uint32_t number);
std::string combine_overflow_message(uint32_t graph, uint64_t offset, uint32_t max_number);
std::string combine_bad_link_message(uint32_t graph, uint64_t index, int32_t a, int32_t b, uint64_t n_unitigs);
std::string combine_bases_message(uint32_t graph);

}  // namespace ac
