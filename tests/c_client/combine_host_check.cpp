// combine_host.cpp alone under the address and undefined-behaviour sanitizers (CPU only; `make combine_host_check` in autocycler_amd/csrc, and
// tests/test_combine_bounds_emu.py builds it the same way): the input checks, the loader on whole and on cut-short texts held in exact heap
// blocks, the fixed-point and yaml number printing at their edges, cluster_depth's sum, the three texts and gfa2fasta's text.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "combine_host.hpp"
#include "components_host.hpp"
#include "merge_host.hpp"

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "combine_host_check: line %d: %s\n", __LINE__, #cond); failures++; } } while (0)
template <class F> static std::string error_of(F&& f) {
    try { f(); } catch (const std::exception& e) { return e.what(); }
    return "";
}
// the text in a heap block of exactly its size: a read past its end is the sanitizer's to see
static std::unique_ptr<char[]> exact(const std::string& s) {
    std::unique_ptr<char[]> p(new char[s.size() ? s.size() : 1]);
    memcpy(p.get(), s.data(), s.size());
    return p;
}

int main() {
    // the numbers
    CHECK(combine_fixed(0.125, 2) == "0.12" && combine_fixed(2.675, 2) == "2.67" && combine_fixed(0.05, 1) == "0.1" && combine_fixed(0.25, 1) == "0.2");
    CHECK(combine_fixed(std::nan(""), 1) == "NaN" && combine_fixed(INFINITY, 2) == "inf" && combine_fixed(-INFINITY, 1) == "-inf" && combine_fixed(-0.0, 1) == "-0.0");
    CHECK(combine_fixed(std::numeric_limits<double>::max(), 2).size() == 312 && combine_fixed(5e-324, 2) == "0.00");
    CHECK(combine_yaml_number(12.34) == "12.3" && combine_yaml_number(0.0) == "0.0" && combine_yaml_number(-0.04) == "-0.0" && combine_yaml_number(1e15) == "1000000000000000.0");
    CHECK(combine_yaml_number(1e16) == "1e16" && combine_yaml_number(1.5e20) == "1.5e20" && combine_yaml_number(123456789012345678.0) == "1.2345678901234568e17");
    CHECK(combine_yaml_number(std::nan("")) == ".nan" && combine_yaml_number(INFINITY) == ".inf" && combine_yaml_number(-INFINITY) == "-.inf");
    CHECK(combine_yaml_number(std::numeric_limits<double>::max()) == "1.7976931348623157e308" && combine_yaml_number(9007199254740993.0) == "9007199254740992.0");

    // the loader: numbers out of order, a repeated number, a dropped L line, colours, lines cut short at every byte
    const std::string text = "H\tVN:Z:1.0\tKM:i:51\nS\t7\tACGTA\tDP:f:2.50\tCL:Z:pink\nS\t2\t\tDP:f:1\nS\t7\tGG\tCL:Z:steelblue\tDP:f:0.125\nL\t7\t+\t2\t-\t0M\nL\t2\t+\t9\t+\t0M\n"
                             "P\t1\t7+\t*\tLN:i:5\nL\t2\t-\t2\t+\t0M\r\nS\t4294967295\tT\tDP:f:inf";
    {
        auto p = exact(text);
        CombineGfa g;
        combine_load_gfa(p.get(), text.size(), &g);
        CHECK(g.number == (std::vector<uint32_t>{7, 2, 7, 4294967295u}) && g.len == (std::vector<uint32_t>{5, 0, 2, 1}));
        CHECK(g.type == (std::vector<uint8_t>{MERGE_TYPE_BRIDGE, MERGE_TYPE_OTHER, MERGE_TYPE_CONSENTIG, MERGE_TYPE_OTHER}) && g.depth[2] == 0.125 && std::isinf(g.depth[3]));
        CHECK(g.links.size() == 2 && g.links[0].a == 3 && g.links[0].b == -2 && g.links[1].a == -2 && g.links[1].b == 2);      // 7 is its last S line
        CHECK(std::string(p.get() + g.seq_at[0], 5) == "ACGTA" && g.seq_at[1] <= text.size());
        for (size_t cut = 0; cut <= text.size(); cut++) {      // every prefix either loads or fails with a message
            auto q = exact(text.substr(0, cut));
            CombineGfa h;
            (void)error_of([&] { combine_load_gfa(q.get(), cut, &h); });
            for (size_t u = 0; u < h.number.size(); u++) CHECK(h.seq_at[u] + h.len[u] <= cut);
        }
    }
    auto load_error = [](const std::string& t) { return error_of([&] { auto p = exact(t); CombineGfa g; combine_load_gfa(p.get(), t.size(), &g); }); };
    CHECK(load_error("S\t1\tAC\n").find("Could not find a depth tag") == 0);
    CHECK(load_error("S\t1\tAC\tDP:f:x\n").find("Could not find a depth tag") == 0);
    CHECK(load_error("S\t-1\tAC\tDP:f:1\n") == "Unable to parse unitig number.");
    CHECK(load_error("S\t4294967296\tAC\tDP:f:1\n") == "Unable to parse unitig number.");
    CHECK(load_error("S\t1") == "Segment line does not have enough parts.");
    CHECK(load_error("L\t1\t+\t1\t+\t1M\n").find("non-zero overlap") == 0);
    CHECK(load_error("L\tx\t+\t1\t+\t0M\n") == "Error parsing segment 1 as integer");
    CHECK(load_error("L\t1\t+\t1\t+\n").find("non-zero overlap") == 0);
    CHECK(error_of([] { CombineGfa g; combine_load_gfa(nullptr, 3, &g); }) == "null pointer: gfa_text");
    { CombineGfa g; combine_load_gfa(nullptr, 0, &g); CHECK(g.number.empty() && g.links.empty()); }

    // the input checks
    {
        const uint64_t uoff[3] = {0, 2, 2}, loff[3] = {0, 1, 1}, bad[3] = {0, 2, 1};
        const uint32_t number[2] = {3, 1}, len[2] = {4, 6};
        const Link links[1] = {{1, -2}};
        const double rd[2] = {1.0, 2.0};
        CombineInput in;
        CHECK(error_of([&] { combine_prepare(in); }) == "combine: at least one graph is required");
        in.n_graphs = 2;
        CHECK(error_of([&] { combine_prepare(in); }) == "null pointer: unitig_off and link_off are required");
        in.unitig_off = uoff; in.link_off = loff;
        CHECK(error_of([&] { combine_prepare(in); }) == "null pointer: number and len are required");
        in.number = number; in.len = len;
        CHECK(error_of([&] { combine_prepare(in); }) == "null pointer: links");
        in.links = links;
        CHECK(error_of([&] { combine_prepare(in); }).empty());
        in.read_depth = rd;
        CHECK(error_of([&] { combine_prepare(in); }).find("read_depth and has_read_depth") != std::string::npos);
        in.read_depth = nullptr; in.unitig_off = bad;
        CHECK(error_of([&] { combine_prepare(in); }) == "combine: graph 1: unitig_off does not ascend");
        in.unitig_off = loff; in.link_off = bad;
        CHECK(error_of([&] { combine_prepare(in); }) == "combine: graph 1: link_off does not ascend");
        std::vector<uint32_t> many(20000, 0xFFFFFFFFu);
        const uint64_t big_u[3] = {0, 10000, 20000}, zero[3] = {0, 0, 0};
        in.unitig_off = big_u; in.link_off = zero; in.number = many.data(); in.len = many.data();
        CHECK(error_of([&] { combine_prepare(in); }) == combine_bases_message(1));
        // every graph empty: the records without a device
        const uint64_t none_l[3] = {0, 0, 1};
        in.unitig_off = zero; in.link_off = zero;
        CombineResult r;
        combine_without_unitigs(in, &r);
        combine_finish(&r);
        CHECK(r.clusters.size() == 2 && r.clusters[1].input_index == 1 && r.clusters[0].topology == TOPO_EMPTY && !r.fully_resolved && r.bases == 0);
        CHECK(combine_yaml_string(r) == "consensus_assembly_bases: 0\nconsensus_assembly_unitigs: 0\nconsensus_assembly_fully_resolved: false\nconsensus_assembly_clusters:\n"
                                        "- length: 0\n  unitigs: 0\n  topology: empty\n  read_depth: unavailable\n- length: 0\n  unitigs: 0\n  topology: empty\n  read_depth: unavailable\n");
        CHECK(combine_gfa_string(r, {}) == "H\tVN:Z:1.0\n" && combine_fasta_string(r, {}).empty());
        in.link_off = none_l;
        CHECK(error_of([&] { combine_without_unitigs(in, &r); }) == combine_bad_link_message(1, 0, 1, -2, 0));
    }

    // cluster_depth, the texts
    {
        CombineResult r;
        r.with_reads = true;
        CombineClusterRecord c; memset(&c, 0, sizeof c);
        c.input_index = 1; c.unitigs = 3; c.length = 12; c.links = 2; c.topology = TOPO_FRAGMENTED; c.max_number = 9;
        r.clusters.push_back(c);
        c.input_index = 0; c.unitigs = 1; c.length = 5; c.links = 0; c.topology = TOPO_LINEAR_OPEN_OPEN; c.offset = 9; c.max_number = 1;
        r.clusters.push_back(c);
        auto tig = [](uint32_t g, uint32_t i, uint32_t number, uint32_t length, double depth, bool has, double rd, uint8_t flags, uint8_t type) {
            CombineUnitigRecord t; memset(&t, 0, sizeof t);
            t.graph = g; t.index = i; t.number = number; t.length = length; t.depth = depth; t.has_read_depth = has; t.read_depth = rd; t.flags = flags; t.type = type;
            return t;
        };
        r.unitigs = {tig(1, 0, 9, 4, 0.1, true, 0.1, 0, MERGE_TYPE_ANCHOR), tig(1, 1, 2, 0, 0.0, false, 0.0, 0, MERGE_TYPE_OTHER), tig(1, 2, 5, 8, 0.7, true, 0.7, 0, MERGE_TYPE_BRIDGE),
                     tig(0, 0, 10, 5, 2.675, true, 2.675, CUF_ISOLATED_LINEAR | CUF_OPEN_START | CUF_OPEN_END, MERGE_TYPE_CONSENTIG)};
        r.links = {{9, 5}, {-5, -9}};
        combine_finish(&r);
        double total = 0.0;
        total += 0.1 * 4.0; total += 0.7 * 8.0;
        CHECK(r.clusters[0].has_read_depth && r.clusters[0].read_depth == total / 12.0 && r.clusters[1].read_depth == 2.675 && !r.fully_resolved && r.bases == 17);
        auto a = exact("ACGT"), b = exact("ACGTACGT"), d = exact("TTTTT");
        const std::vector<const char*> seq = {a.get(), nullptr, b.get(), d.get()};
        CHECK(combine_gfa_string(r, seq) == "H\tVN:Z:1.0\nS\t9\tACGT\tDP:f:0.10\tCL:Z:forestgreen\nS\t2\t\tDP:f:0.00\tCL:Z:orangered\nS\t5\tACGTACGT\tDP:f:0.70\tCL:Z:pink\n"
                                            "L\t9\t+\t5\t+\t0M\nL\t5\t-\t9\t-\t0M\nS\t10\tTTTTT\tDP:f:2.67\tCL:Z:steelblue\n");
        CHECK(combine_fasta_string(r, seq) == ">9 length=4 depth=0.1\nACGT\n>2 length=0 depth=unavailable\n\n>5 length=8 depth=0.7\nACGTACGT\n"
                                              ">10 length=5 depth=2.7 circular=false topology=linear\nTTTTT\n");
        CHECK(combine_depth_lines(r) == "Sequence depths:\n  9 length=4 depth=0.1\n  2 length=0 depth=unavailable\n  5 length=8 depth=0.7\n  10 length=5 depth=2.7\n");
        CHECK(combine_yaml_string(r).find("- length: 12\n  unitigs: 3\n  topology: fragmented\n  read_depth: 0.5\n- length: 5\n  unitigs: 1\n  topology: linear-open-open\n  read_depth: 2.7\n") != std::string::npos);
        CHECK(error_of([&] { combine_gfa_string(r, {a.get()}); }).find("one sequence per unitig") != std::string::npos);
        CHECK(error_of([&] { combine_fasta_string(r, {a.get(), nullptr, nullptr, d.get()}); }).find("missing sequences") != std::string::npos);
        r.links.pop_back();
        CHECK(error_of([&] { combine_finish(&r); }).find("disagree") != std::string::npos);
    }

    // gfa2fasta's text
    {
        const std::string t = "S\t3\tACG\tDP:f:0.25\nS\t1\t\tDP:f:9\nS\t8\tTT\tDP:f:7.05\n";
        auto p = exact(t);
        CombineGfa g;
        combine_load_gfa(p.get(), t.size(), &g);
        const uint8_t flags[3] = {CUF_ISOLATED_CIRCULAR, CUF_ISOLATED_LINEAR, 0};
        uint64_t counts[3];
        CHECK(combine_gfa2fasta_string(g, p.get(), flags, counts) == ">3 length=3 depth=0.2 circular=true topology=circular\nACG\n>8 length=2 depth=7.0\nTT\n");
        CHECK(counts[0] == 1 && counts[1] == 0 && counts[2] == 1);
    }
    if (failures) { fprintf(stderr, "combine_host_check: %d checks failed\n", failures); return 1; }
    printf("combine_host_check: OK\n");
    return 0;
}
