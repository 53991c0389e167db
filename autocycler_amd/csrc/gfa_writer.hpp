// GFA text emission of the final graph — save_gfa (unitig_graph.rs:317-360), gfa_segment_line
// (unitig.rs:168-172).  One buffered pass instead of one writeln! syscall per line.
#pragma once
#include <string>
#include <vector>

#include "host_tail.hpp"

namespace ac {
struct SeqMeta { uint16_t id; uint32_t length; std::string filename; std::string contig_header; };
// parts: bit 0 = H, S and L lines, bit 1 = P lines (a sharded build can keep the P lines of each rank's sequences on that rank)
std::string gfa_string(const FinalGraph& g, const std::vector<SeqMeta>& seqs, int parts = 3);
// gfa_reader.cpp: the loader side (UnitigGraph::from_gfa_lines, unitig_graph.rs:55-174) and decompress's reconstruction
void load_gfa(const char* text, size_t len, FinalGraph* g, std::vector<SeqMeta>* seqs);
// the same for segment numbers in any order and with holes (mapped to 1..n in file order; *numbers: the table), with the P lines' CL:i tags
void load_gfa_any_numbers(const char* text, size_t len, FinalGraph* g, std::vector<SeqMeta>* seqs, std::vector<uint64_t>* numbers, std::vector<uint32_t>* cluster_tags);
void decompress_sequence(const FinalGraph& g, size_t seq_index, char* out);      // out: LN bytes
std::vector<std::string> gfa_chunks(const FinalGraph& g, const std::vector<SeqMeta>& seqs, int threads);
// The same text for a graph whose segments carry explicit numbers and types (a graph after merge_linear_paths): the S lines print `number`
// and colour_tag (unitig.rs:174-182), a P line whose cluster is above 0 ends in CL:i:<cluster> (unitig_graph.rs:357).
struct GfaSegmentView { uint32_t number; const char* seq; uint64_t length; double depth; uint8_t type; };      // type: 0 Other, 1 Anchor, 2 Consentig, 3 Bridge
struct GfaPathView { uint16_t id; const int32_t* entries; uint64_t n_entries; uint32_t length; const std::string* filename; const std::string* header; uint32_t cluster; };
std::string gfa_string_explicit(uint32_t k, const std::vector<GfaSegmentView>& segments, const Link* links, uint64_t n_links, const std::vector<GfaPathView>& paths,
                                bool use_other_colour);
}  // namespace ac
