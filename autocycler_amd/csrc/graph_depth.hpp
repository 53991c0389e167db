// Read-based unitig depths on the device (set_read_depths, depth.rs:45-76): the table of the consensus assembly's canonical k-mers, the
// two-pass tally of the reads' k-mers and the gathers the host arithmetic needs.  graph_depth.hip / kernels_depth.inc; the C ABI
// (ac_depth_*) holds one DepthEngine per handle.  The caller has selected the device and holds the build lock for every call.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "depth_host.hpp"

namespace ac {

struct DepthTotals {      // ReadTotals (depth.rs:446-453) and what the device did for them
    uint64_t reads = 0, rejected_reads = 0, read_bases = 0, span_bases = 0, span_kmers = 0, hits = 0;
    uint64_t distinct_kmers = 0, repeat_kmers = 0, table_slots = 0;
    uint32_t batches = 0, launches = 0;
    double seconds_device = 0;
};

class DepthEngine {
  public:
    // builds the table from every unitig of every graph plus the plans' junction k-mers; owns its device memory until destroyed
    DepthEngine(uint32_t k, const std::vector<DepthGraphView>& graphs, std::vector<DepthGraphPlan>&& plans);
    ~DepthEngine();
    DepthEngine(const DepthEngine&) = delete;
    DepthEngine& operator=(const DepthEngine&) = delete;
    void add_reads(const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads);
    DepthTotals totals();
    void kmer_counts(const uint64_t* kmers, uint64_t n, uint8_t* present, uint32_t* occurrences, uint32_t* read_count);
    uint32_t n_graphs() const;
    uint32_t n_unitigs(uint32_t graph_index) const;
    void finish(uint32_t graph_index, double* depth, uint8_t* has_depth);

  private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace ac
