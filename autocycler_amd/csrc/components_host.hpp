// Connected components and graph topology (UnitigGraph::connected_components, component_is_circular_loop, link_count, topology:
// unitig_graph.rs:478-545, 905-967; the per-unitig end tests of unitig.rs:197-215, 276-293) — the host side: the result as the C ABI
// hands it out, the totals, the topology chain and the error texts.  Plain C++, no device code; the analysis itself is
// kernels_components.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "graph_types.hpp"

namespace ac {

// ac_component, field for field (the device writes these records; capi_steps.cpp asserts the two layouts agree)
struct ComponentRecord {
    uint32_t first, unitigs;
    uint64_t length, links_all, links_one_way;
    uint32_t open_ends, marked;
    uint8_t circular_loop;
};
// per-unitig flag bits (ac_components_unitig_flags)
enum ComponentUnitigFlag { CUF_OPEN_START = 1, CUF_OPEN_END = 2, CUF_HAIRPIN_START = 4, CUF_HAIRPIN_END = 8, CUF_ISOLATED_CIRCULAR = 16, CUF_ISOLATED_LINEAR = 32 };
enum ComponentsTopology { TOPO_EMPTY = 0, TOPO_FRAGMENTED, TOPO_LINEAR_OPEN_OPEN, TOPO_CIRCULAR, TOPO_LINEAR_HAIRPIN_HAIRPIN, TOPO_LINEAR_OPEN_HAIRPIN, TOPO_OTHER, TOPO_COUNT };

struct ComponentsResult {
    uint32_t n_unitigs = 0;                   // the caller's n (alive or not)
    std::vector<ComponentRecord> records;     // in connected_components() order: by lowest member
    std::vector<uint32_t> component_of;       // n_unitigs; UINT32_MAX = not alive
    std::vector<uint64_t> member_off;         // records.size() + 1
    std::vector<uint32_t> members;            // unitig numbers, ascending inside a component
    std::vector<uint8_t> flags;               // n_unitigs; 0 for a unitig that is not alive
    // filled by components_finish
    uint32_t alive = 0, topology = TOPO_EMPTY;
    uint64_t links_all = 0, links_one_way = 0, total_length = 0;
    StepStats stats;                          // filled by the device driver
};

// topology() (unitig_graph.rs:527-545) from the number of alive unitigs, link_count().0 of the graph and, when exactly one unitig is
// alive, its flag bits
uint32_t components_topology(uint64_t alive, uint64_t links_all, uint8_t only_unitig_flags);
const char* components_topology_name(uint32_t topology);      // the reference's strings; nullptr beyond TOPO_OTHER
// the totals and the topology of a result whose arrays are filled; throws std::runtime_error when the arrays contradict each other
void components_finish(ComponentsResult* r);
// "link 7 (3 -> 0) names no unitig: ..."
std::string components_bad_link_message(uint64_t index, int32_t a, int32_t b, uint32_t n_unitigs);

}  // namespace ac
