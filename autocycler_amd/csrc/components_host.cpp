// The host side of the connected-components analysis (components_host.hpp): totals, the topology chain, error texts.
#include "components_host.hpp"

#include <stdexcept>

namespace ac {

uint32_t components_topology(uint64_t alive, uint64_t links_all, uint8_t f) {
    if (alive == 0) return TOPO_EMPTY;
    if (alive > 1) return TOPO_FRAGMENTED;
    if (links_all == 0) return TOPO_LINEAR_OPEN_OPEN;
    if (f & CUF_ISOLATED_CIRCULAR) return TOPO_CIRCULAR;
    if ((f & CUF_HAIRPIN_START) && (f & CUF_HAIRPIN_END)) return TOPO_LINEAR_HAIRPIN_HAIRPIN;
    if ((f & CUF_HAIRPIN_START) && (f & CUF_OPEN_END)) return TOPO_LINEAR_OPEN_HAIRPIN;
    if ((f & CUF_OPEN_START) && (f & CUF_HAIRPIN_END)) return TOPO_LINEAR_OPEN_HAIRPIN;
    return TOPO_OTHER;
}

const char* components_topology_name(uint32_t t) {
    static const char* const names[TOPO_COUNT] = {"empty", "fragmented", "linear-open-open", "circular", "linear-hairpin-hairpin", "linear-open-hairpin", "other"};
    return t < TOPO_COUNT ? names[t] : nullptr;
}

void components_finish(ComponentsResult* r) {
    const size_t nc = r->records.size();
    if (r->member_off.size() != nc + 1 || r->component_of.size() != r->n_unitigs || r->flags.size() != r->n_unitigs || r->member_off[0] != 0 ||
        r->member_off[nc] != r->members.size() || r->members.size() > r->n_unitigs)
        throw std::runtime_error("components: the result arrays do not fit together");
    r->alive = (uint32_t)r->members.size();
    r->links_all = r->links_one_way = r->total_length = 0;
    for (size_t c = 0; c < nc; c++) {
        const ComponentRecord& rec = r->records[c];
        if (r->member_off[c + 1] - r->member_off[c] != rec.unitigs || rec.unitigs == 0 || r->members[r->member_off[c]] != rec.first)
            throw std::runtime_error("components: a record does not fit its member list");
        r->links_all += rec.links_all; r->links_one_way += rec.links_one_way; r->total_length += rec.length;
    }
    const uint8_t f = r->alive == 1 ? r->flags[r->members[0] - 1] : 0;
    r->topology = components_topology(r->alive, r->links_all, f);
}

std::string components_bad_link_message(uint64_t index, int32_t a, int32_t b, uint32_t n_unitigs) {
    return "link " + std::to_string(index) + " (" + std::to_string(a) + " -> " + std::to_string(b) + ") names no unitig: unitig numbers run from 1 to " +
           std::to_string(n_unitigs) + " (link refers to nonexistent unitig)";
}

}  // namespace ac
