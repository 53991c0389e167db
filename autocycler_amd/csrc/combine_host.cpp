// The host side of combine and gfa2fasta (combine_host.hpp): the input checks, the cluster GFA loader, cluster_depth, the three texts, the error texts.
#include "combine_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <unordered_map>

#include "components_host.hpp"
#include "merge_host.hpp"

namespace ac {

std::string combine_duplicate_message(uint32_t graph, uint32_t number) {
    return "combine: graph " + std::to_string(graph) + ": unitig number " + std::to_string(number) + " occurs more than once";
}
std::string combine_overflow_message(uint32_t graph, uint64_t offset, uint32_t max_number) {
    return "combine: graph " + std::to_string(graph) + ": offset " + std::to_string(offset) + " + its highest unitig number " + std::to_string(max_number) +
           " does not fit 32 bits";
}
std::string combine_bad_link_message(uint32_t graph, uint64_t index, int32_t a, int32_t b, uint64_t n_unitigs) {
    return "combine: graph " + std::to_string(graph) + ": link " + std::to_string(index) + " (" + std::to_string(a) + " -> " + std::to_string(b) +
           ") names no unitig of its graph: its entries are 1-based file-order indices, " + std::to_string(n_unitigs) + " unitigs here";
}
std::string combine_bases_message(uint32_t graph) {
    return "combine: graph " + std::to_string(graph) + ": the total of bases reaches 2^46 with this graph";
}

void combine_prepare(const CombineInput& in) {
    if (in.n_graphs == 0) throw std::runtime_error("combine: at least one graph is required");
    if (!in.unitig_off || !in.link_off) throw std::runtime_error("null pointer: unitig_off and link_off are required");
    if ((in.read_depth == nullptr) != (in.has_read_depth == nullptr)) throw std::runtime_error("null pointer: read_depth and has_read_depth come together or not at all");
    if (in.unitig_off[0] != 0 || in.link_off[0] != 0) throw std::runtime_error("combine: unitig_off and link_off must start at 0");
    for (uint32_t g = 0; g < in.n_graphs; g++) {
        if (in.unitig_off[g + 1] < in.unitig_off[g]) throw std::runtime_error("combine: graph " + std::to_string(g) + ": unitig_off does not ascend");
        if (in.link_off[g + 1] < in.link_off[g]) throw std::runtime_error("combine: graph " + std::to_string(g) + ": link_off does not ascend");
    }
    const uint64_t n = in.n_unitigs(), nl = in.n_links();
    if (n > 0x7FFFFFF0ULL) throw std::runtime_error("combine: more unitigs than a signed entry can name");
    if (nl >= 0xFFFFFFE0ULL) throw std::runtime_error("combine: more than 2^32 links");
    if (n && (!in.number || !in.len)) throw std::runtime_error("null pointer: number and len are required");
    if (nl && !in.links) throw std::runtime_error("null pointer: links");
    uint64_t bases = 0;      // the device scan carries 46-bit totals
    for (uint32_t g = 0; g < in.n_graphs; g++)
        for (uint64_t u = in.unitig_off[g]; u < in.unitig_off[g + 1]; u++) {
            bases += in.len[u];
            if (bases >= (1ULL << 46)) throw std::runtime_error(combine_bases_message(g));
        }
}

void combine_without_unitigs(const CombineInput& in, CombineResult* out) {
    *out = CombineResult();
    out->with_reads = in.read_depth != nullptr;
    for (uint32_t g = 0; g < in.n_graphs; g++) {
        if (in.link_off[g + 1] != in.link_off[g]) {
            const Link& l = in.links[in.link_off[g]];
            throw std::runtime_error(combine_bad_link_message(g, 0, l.a, l.b, 0));
        }
        CombineClusterRecord c;
        memset(&c, 0, sizeof c);
        c.input_index = g; c.topology = TOPO_EMPTY;
        out->clusters.push_back(c);      // (equal totals: the stable sort keeps the input order)
    }
}

void combine_finish(CombineResult* r) {
    const size_t G = r->clusters.size();
    r->unitig_off.assign(G + 1, 0); r->link_off.assign(G + 1, 0);
    r->bases = 0; r->fully_resolved = true;
    for (size_t c = 0; c < G; c++) {
        CombineClusterRecord& k = r->clusters[c];
        r->unitig_off[c + 1] = r->unitig_off[c] + k.unitigs;
        r->link_off[c + 1] = r->link_off[c] + k.links;
        r->bases += k.length;
        if (k.unitigs != 1) r->fully_resolved = false;
        // cluster_depth (combine.rs:107-119): a sequential f64 sum in unitig order over the unitigs that have a depth
        double total = 0.0; uint64_t length = 0;
        for (uint64_t u = r->unitig_off[c]; u < r->unitig_off[c + 1]; u++) {
            const CombineUnitigRecord& t = r->unitigs[(size_t)u];
            if (!t.has_read_depth) continue;
            total += t.read_depth * (double)t.length;
            length += t.length;
        }
        k.has_read_depth = length > 0 ? 1 : 0;
        k.read_depth = length > 0 ? total / (double)length : 0.0;
    }
    r->n_unitigs = r->unitig_off[G];
    if (r->n_unitigs != r->unitigs.size() || r->link_off[G] != r->links.size()) throw std::runtime_error("combine: the records and the arrays disagree (internal error)");
}

std::string combine_fixed(double v, int decimals) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    std::string s(400, '\0');      // (1.8e308 has 309 digits before the point)
    const int n = snprintf(&s[0], s.size(), "%.*f", decimals, v);
    s.resize((size_t)n);
    return s;
}

// serde_yaml 0.9 prints a float with ryu: the shortest digits that read back, plain from 1e-5 up to 1e16 and with an exponent beyond,
// ".nan", ".inf", "-.inf".  The value is what its own one-decimal text parses to.
std::string combine_yaml_number(double v) {
    const std::string text = combine_fixed(v, 1);
    if (std::isnan(v)) return ".nan";
    if (std::isinf(v)) return v > 0 ? ".inf" : "-.inf";
    const double x = strtod(text.c_str(), nullptr);
    if (std::fabs(x) < 1e15) return text;      // (at most 15 digits before the point and one behind: the text is the shortest that reads back)
    char buf[64]; int prec = 1;
    for (; prec <= 17; prec++) { snprintf(buf, sizeof buf, "%.*e", prec - 1, x); if (strtod(buf, nullptr) == x) break; }
    std::string m(buf);
    const size_t e = m.find('e');
    std::string digits; const bool neg = m[0] == '-';
    for (size_t i = neg ? 1 : 0; i < e; i++) if (m[i] != '.') digits.push_back(m[i]);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int exp10 = atoi(m.c_str() + e + 1);
    std::string out = neg ? "-" : "";
    if (exp10 < 16) {
        std::string whole = digits;
        if ((int)whole.size() < exp10 + 1) whole.append((size_t)(exp10 + 1) - whole.size(), '0');
        out += whole.substr(0, (size_t)exp10 + 1) + "." + (whole.size() > (size_t)exp10 + 1 ? whole.substr((size_t)exp10 + 1) : "0");
    } else {
        out += digits.substr(0, 1);
        if (digits.size() > 1) out += "." + digits.substr(1);
        out += "e" + std::to_string(exp10);
    }
    return out;
}

static const char* colour_of(uint8_t type) {      // colour_tag(true): never empty
    switch (type) {
        case MERGE_TYPE_CONSENTIG: return "\tCL:Z:steelblue";
        case MERGE_TYPE_ANCHOR: return "\tCL:Z:forestgreen";
        case MERGE_TYPE_BRIDGE: return "\tCL:Z:pink";
        default: return "\tCL:Z:orangered";
    }
}
static const char* topology_words(uint8_t flags) {
    if (flags & CUF_ISOLATED_CIRCULAR) return " circular=true topology=circular";
    if (flags & CUF_ISOLATED_LINEAR) return " circular=false topology=linear";
    return "";
}
static void check_seqs(const CombineResult& r, const std::vector<const char*>& seq) {
    if (seq.size() != r.unitigs.size()) throw std::runtime_error("combine: one sequence per unitig is required for the texts");
    for (size_t i = 0; i < seq.size(); i++)
        if (!seq[i] && r.unitigs[i].length) throw std::runtime_error("combine: missing sequences: the texts need the unitigs' bytes");
}

std::string combine_gfa_string(const CombineResult& r, const std::vector<const char*>& seq) {
    check_seqs(r, seq);
    std::string out;
    out.reserve((size_t)r.bases + r.unitigs.size() * 48 + r.links.size() * 32 + 16);
    out += "H\tVN:Z:1.0\n";
    for (size_t c = 0; c < r.clusters.size(); c++) {
        for (uint64_t u = r.unitig_off[c]; u < r.unitig_off[c + 1]; u++) {
            const CombineUnitigRecord& t = r.unitigs[(size_t)u];
            out += "S\t"; out += std::to_string(t.number); out += '\t'; out.append(seq[(size_t)u] ? seq[(size_t)u] : "", t.length);
            out += "\tDP:f:"; out += combine_fixed(t.depth, 2); out += colour_of(t.type); out += '\n';
        }
        for (uint64_t i = r.link_off[c]; i < r.link_off[c + 1]; i++) {
            const Link& l = r.links[(size_t)i];
            out += "L\t"; out += std::to_string(l.na()); out += l.a_fwd() ? "\t+\t" : "\t-\t"; out += std::to_string(l.nb()); out += l.b_fwd() ? "\t+\t0M\n" : "\t-\t0M\n";
        }
    }
    return out;
}

std::string combine_fasta_string(const CombineResult& r, const std::vector<const char*>& seq) {
    check_seqs(r, seq);
    std::string out;
    out.reserve((size_t)r.bases + r.unitigs.size() * 96);
    for (size_t u = 0; u < r.unitigs.size(); u++) {
        const CombineUnitigRecord& t = r.unitigs[u];
        out += ">"; out += std::to_string(t.number); out += " length="; out += std::to_string(t.length);
        if (r.with_reads) out += t.has_read_depth ? " depth=" + combine_fixed(t.read_depth, 1) : std::string(" depth=unavailable");
        out += topology_words(t.flags); out += '\n';
        out.append(seq[u] ? seq[u] : "", t.length); out += '\n';
    }
    return out;
}

std::string combine_yaml_string(const CombineResult& r) {
    std::string y = "consensus_assembly_bases: " + std::to_string(r.bases) + "\n";
    y += "consensus_assembly_unitigs: " + std::to_string((uint32_t)r.n_unitigs) + "\n";
    y += std::string("consensus_assembly_fully_resolved: ") + (r.fully_resolved ? "true" : "false") + "\n";
    y += "consensus_assembly_clusters:\n";      // (at least one graph: never the empty list)
    for (const CombineClusterRecord& c : r.clusters) {
        y += "- length: " + std::to_string(c.length) + "\n";
        y += "  unitigs: " + std::to_string(c.unitigs) + "\n";
        y += std::string("  topology: ") + components_topology_name(c.topology) + "\n";
        y += "  read_depth: " + (c.has_read_depth ? combine_yaml_number(c.read_depth) : std::string("unavailable")) + "\n";
    }
    return y;
}

std::string combine_depth_lines(const CombineResult& r) {
    if (!r.with_reads) return std::string();
    std::string s = "Sequence depths:\n";
    for (const CombineUnitigRecord& t : r.unitigs)
        s += "  " + std::to_string(t.number) + " length=" + std::to_string(t.length) + " depth=" + (t.has_read_depth ? combine_fixed(t.read_depth, 1) : std::string("unavailable")) + "\n";
    return s;
}

namespace {
struct Field { const char* p; size_t n; bool is(const char* s) const { return n == strlen(s) && !memcmp(p, s, n); } };
std::vector<Field> fields_of(const char* s, size_t n) {
    std::vector<Field> out;
    size_t a = 0;
    for (size_t i = 0; i <= n; i++)
        if (i == n || s[i] == '\t') { out.push_back(Field{s + a, i - a}); a = i + 1; }
    return out;
}
bool parse_u32(const Field& f, uint32_t* v) {      // str::parse::<u32>: an optional '+', digits, no overflow
    size_t i = f.n && f.p[0] == '+' ? 1 : 0;
    if (i == f.n) return false;
    uint64_t x = 0;
    for (; i < f.n; i++) {
        if (f.p[i] < '0' || f.p[i] > '9') return false;
        x = x * 10 + (uint64_t)(f.p[i] - '0');
        if (x > 0xFFFFFFFFULL) return false;
    }
    *v = (uint32_t)x;
    return true;
}
}  // namespace

void combine_load_gfa(const char* text, uint64_t len, CombineGfa* g) {
    *g = CombineGfa();
    if (!text && len) throw std::runtime_error("null pointer: gfa_text");
    struct RawLink { uint32_t a, b; bool fa, fb; };
    std::vector<RawLink> raw;
    std::unordered_map<uint32_t, uint32_t> index_of;      // number -> 1-based file-order index; a repeated number keeps the last
    uint64_t a = 0;
    while (a < len) {
        uint64_t e = a;
        while (e < len && text[e] != '\n') e++;
        uint64_t ll = e - a;
        if (ll && text[a + ll - 1] == '\r') ll--;
        const std::vector<Field> f = fields_of(text + a, (size_t)ll);
        if (f[0].is("S")) {
            if (f.size() < 3) throw std::runtime_error("Segment line does not have enough parts.");
            uint32_t number = 0;
            if (!parse_u32(f[1], &number)) throw std::runtime_error("Unable to parse unitig number.");
            if (f[2].n > 0xFFFFFFFFULL) throw std::runtime_error("combine: a unitig longer than 2^32 bases");
            bool has_depth = false; double depth = 0;
            bool consentig = false, anchor = false, bridge = false;
            for (const Field& t : f) {
                if (!has_depth && t.n >= 5 && !memcmp(t.p, "DP:f:", 5)) {      // find(): the first such part decides; it must parse
                    const std::string v(t.p + 5, t.n - 5);
                    char* end = nullptr;
                    depth = strtod(v.c_str(), &end);
                    if (v.empty() || *end || v[0] == ' ') throw std::runtime_error("Could not find a depth tag (e.g. DP:f:10.00) in the GFA segment line.\nAre you sure this is an Autocycler-generated GFA file?");
                    has_depth = true;
                }
                consentig |= t.is("CL:Z:steelblue"); anchor |= t.is("CL:Z:forestgreen"); bridge |= t.is("CL:Z:pink");
            }
            if (!has_depth) throw std::runtime_error("Could not find a depth tag (e.g. DP:f:10.00) in the GFA segment line.\nAre you sure this is an Autocycler-generated GFA file?");
            g->number.push_back(number); g->len.push_back((uint32_t)f[2].n); g->depth.push_back(depth);
            g->type.push_back(consentig ? MERGE_TYPE_CONSENTIG : anchor ? MERGE_TYPE_ANCHOR : bridge ? MERGE_TYPE_BRIDGE : MERGE_TYPE_OTHER);
            g->seq_at.push_back((uint64_t)(f[2].p - text));
            if (g->number.size() > 0x7FFFFFF0ULL) throw std::runtime_error("combine: more unitigs than a signed entry can name");
            index_of[number] = (uint32_t)g->number.size();
        } else if (f[0].is("L")) {
            if (f.size() < 6 || !f[5].is("0M")) throw std::runtime_error("non-zero overlap found on the GFA link line.\nAre you sure this is an Autocycler-generated GFA file?");
            RawLink r;
            if (!parse_u32(f[1], &r.a)) throw std::runtime_error("Error parsing segment 1 as integer");
            if (!parse_u32(f[3], &r.b)) throw std::runtime_error("Error parsing segment 2 as integer");
            r.fa = f[2].is("+"); r.fb = f[4].is("+");
            raw.push_back(r);
        }
        a = e + 1;
    }
    for (const RawLink& r : raw) {
        const auto ia = index_of.find(r.a), ib = index_of.find(r.b);
        if (ia == index_of.end() || ib == index_of.end()) continue;      // an L line that names a segment the file lacks
        g->links.push_back(Link{r.fa ? (int32_t)ia->second : -(int32_t)ia->second, r.fb ? (int32_t)ib->second : -(int32_t)ib->second});
    }
}

std::string combine_gfa2fasta_string(const CombineGfa& g, const char* text, const uint8_t* flags, uint64_t counts[3]) {
    std::string out;
    counts[0] = counts[1] = counts[2] = 0;
    for (size_t u = 0; u < g.number.size(); u++) {
        if (g.len[u] == 0) continue;
        const uint8_t f = flags[u];
        if (f & CUF_ISOLATED_CIRCULAR) counts[0]++; else if (f & CUF_ISOLATED_LINEAR) counts[1]++; else counts[2]++;
        out += ">"; out += std::to_string(g.number[u]); out += " length="; out += std::to_string(g.len[u]); out += " depth="; out += combine_fixed(g.depth[u], 1);
        out += topology_words(f); out += '\n';
        out.append(text + g.seq_at[u], g.len[u]); out += '\n';
    }
    return out;
}

}  // namespace ac
