// components_host.cpp on its own (no library, no device): the topology chain of unitig_graph.rs:527-545 over every combination of flag
// bits, the names, the totals of components_finish and its refusal of arrays that do not fit together.  A stand-alone program, so that it
// can be built with -fsanitize=address,undefined (tests/test_components_emu.py does).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "components_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// the chain as the reference writes it, on booleans
static const char* reference_topology(uint64_t unitigs, uint64_t links_all, bool circ, bool hs, bool he, bool os, bool oe) {
    if (unitigs == 0) return "empty";
    if (unitigs > 1) return "fragmented";
    if (links_all == 0) return "linear-open-open";
    if (circ) return "circular";
    if (hs && he) return "linear-hairpin-hairpin";
    if (hs && oe) return "linear-open-hairpin";
    if (os && he) return "linear-open-hairpin";
    return "other";
}

static bool throws(ComponentsResult r) {
    try { components_finish(&r); } catch (const std::runtime_error&) { return true; }
    return false;
}

int main() {
    for (uint64_t unitigs = 0; unitigs < 3; unitigs++)
        for (uint64_t links = 0; links < 3; links++)
            for (unsigned f = 0; f < 64; f++) {
                const uint32_t t = components_topology(unitigs, links, (uint8_t)f);
                const char* want = reference_topology(unitigs, links, f & CUF_ISOLATED_CIRCULAR, f & CUF_HAIRPIN_START, f & CUF_HAIRPIN_END, f & CUF_OPEN_START, f & CUF_OPEN_END);
                CHECK(components_topology_name(t) && !strcmp(components_topology_name(t), want));
            }
    CHECK(components_topology_name(TOPO_COUNT) == nullptr && components_topology_name(0xFFFFFFFFu) == nullptr);
    CHECK(!strcmp(components_topology_name(TOPO_LINEAR_OPEN_HAIRPIN), "linear-open-hairpin"));

    ComponentsResult r;      // unitigs 1 .. 5, unitig 3 not alive: [1, 4], [2], [5]
    r.n_unitigs = 5;
    r.records = {{1, 2, 30, 2, 1, 2, 1, 0}, {2, 1, 7, 2, 1, 0, 0, 1}, {5, 1, 9, 0, 0, 2, 0, 0}};
    r.component_of = {0, 1, 0xFFFFFFFFu, 0, 2};
    r.member_off = {0, 2, 3, 4};
    r.members = {1, 4, 2, 5};
    r.flags = {0, 16, 0, 0, 35};
    {
        ComponentsResult ok = r;
        components_finish(&ok);
        CHECK(ok.alive == 4 && ok.links_all == 4 && ok.links_one_way == 2 && ok.total_length == 46 && ok.topology == TOPO_FRAGMENTED);
    }
    { ComponentsResult bad = r; bad.member_off[1] = 1; CHECK(throws(bad)); }
    { ComponentsResult bad = r; bad.members[0] = 4; CHECK(throws(bad)); }
    { ComponentsResult bad = r; bad.member_off.pop_back(); CHECK(throws(bad)); }
    { ComponentsResult bad = r; bad.flags.pop_back(); CHECK(throws(bad)); }
    { ComponentsResult bad = r; bad.members.push_back(3); CHECK(throws(bad)); }
    {
        ComponentsResult one;      // unitig 2 of 2 alone, with a circularising link
        one.n_unitigs = 2; one.records = {{2, 1, 7, 2, 1, 0, 0, 1}}; one.component_of = {0xFFFFFFFFu, 0}; one.member_off = {0, 1}; one.members = {2}; one.flags = {0, 16};
        components_finish(&one);
        CHECK(one.topology == TOPO_CIRCULAR && one.alive == 1);
    }
    {
        ComponentsResult none;
        none.member_off = {0};
        components_finish(&none);
        CHECK(none.topology == TOPO_EMPTY && none.alive == 0);
    }
    const std::string m = components_bad_link_message(7, 3, 0, 10);
    CHECK(m.find("link 7 (3 -> 0)") == 0 && m.find("names no unitig") != std::string::npos && m.find("1 to 10") != std::string::npos);
    if (failures) { printf("components_host_check: %d FAILED\n", failures); return 1; }
    printf("components_host_check: OK\n");
    return 0;
}
