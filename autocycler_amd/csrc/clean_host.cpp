// The host side of `autocycler clean` (clean_host.hpp): the number lists, the checks, the sequential duplication over the gathered links, the
// S-line types of a GFA text, the text and the error texts.
#include "clean_host.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "gfa_writer.hpp"
#include "merge_host.hpp"

namespace ac {

std::string clean_unordered_link_message(uint64_t index, int32_t a, int32_t b, int32_t prev_a) {
    return "clean: link entry " + std::to_string(index) + " (" + std::to_string(a) + " -> " + std::to_string(b) + ") stands behind an entry that leaves " +
           std::to_string(prev_a) + ": the links must be in L-line order (unitigs ascending, the forward strand's links before the reverse strand's)";
}
std::string clean_no_tig_message(const std::string& name, uint32_t tig) { return name + " does not contain tig " + std::to_string(tig); }
std::string clean_gone_message(uint32_t tig) {
    return "unitig " + std::to_string(tig) + " no longer exists: it was removed or duplicated earlier in the same call";
}
std::string clean_not_two_links_message(uint32_t tig) { return "unitig " + std::to_string(tig) + " does not contain exactly two non-self links"; }

std::vector<uint32_t> clean_parse_tig_numbers(const char* s) {
    std::vector<uint32_t> out;
    if (!s) return out;
    std::string t;
    for (const char* p = s; *p; p++) if (*p != ' ') t.push_back(*p);
    size_t a = 0;
    for (size_t i = 0; i <= t.size(); i++) {
        if (i < t.size() && t[i] != ',') continue;
        const std::string piece = t.substr(a, i - a);
        a = i + 1;
        // str::parse::<u32>: an optional '+', then decimal digits only, no overflow
        size_t d = !piece.empty() && piece[0] == '+' ? 1 : 0;
        uint64_t v = 0;
        bool ok = d < piece.size();
        for (; ok && d < piece.size(); d++) {
            if (piece[d] < '0' || piece[d] > '9') { ok = false; break; }
            v = v * 10 + (uint64_t)(piece[d] - '0');
            if (v > 0xFFFFFFFFULL) ok = false;
        }
        if (!ok) throw std::runtime_error("failed to parse '" + piece + "' as a node number");
        out.push_back((uint32_t)v);
    }
    std::sort(out.begin(), out.end());
    return out;
}

void clean_prepare(const CleanInput& in) {
    const uint32_t n = in.n_unitigs;
    if (n > 0x7FFFFFFEu) throw std::runtime_error("clean: more unitigs than a signed unitig number can name");
    if (n && !in.unitig_len) throw std::runtime_error("null pointer: unitig_len");
    if (in.n_links && !in.links) throw std::runtime_error("null pointer: n_links > 0 without links");
    if ((in.seq_bytes == nullptr) != (in.seq_begin == nullptr)) throw std::runtime_error("seq_bytes and seq_begin: both or neither");
    if (in.n_remove && !in.remove) throw std::runtime_error("null pointer: n_remove > 0 without remove");
    if (in.n_duplicate && !in.duplicate) throw std::runtime_error("null pointer: n_duplicate > 0 without duplicate");
    if ((uint64_t)n + 2ULL * in.n_duplicate > 0x7FFFFFFEULL)
        throw std::runtime_error("clean: " + std::to_string(n) + " unitigs and " + std::to_string(in.n_duplicate) + " duplications: more than a signed unitig number can name");
    for (uint32_t i = 1; i < in.n_remove; i++)
        if (in.remove[i] < in.remove[i - 1]) throw std::runtime_error("clean: the numbers to remove must ascend (" + std::to_string(in.remove[i]) + ")");
    for (uint32_t i = 1; i < in.n_duplicate; i++)
        if (in.duplicate[i] < in.duplicate[i - 1]) throw std::runtime_error("clean: the numbers to duplicate must ascend (" + std::to_string(in.duplicate[i]) + ")");
    auto valid = [&](const uint32_t* v, uint32_t count) {
        for (uint32_t i = 0; i < count; i++)
            if (v[i] == 0 || v[i] > n || (in.alive && !in.alive[v[i] - 1])) throw std::runtime_error(clean_no_tig_message(in.name, v[i]));
    };
    valid(in.remove, in.n_remove);
    valid(in.duplicate, in.n_duplicate);
}

void clean_duplicate_edit(const CleanInput& in, const std::vector<Link>& gathered, std::vector<Link>* created) {
    // One list of entries stands for all four lists of every unitig: the gathered entries in input order, then what create_link pushes, in
    // time order.  A unitig strand's next list is the entries that leave it, in this order — the loader fills a list in input order,
    // create_link_one_way pushes at its end, and the deletions (delete_dangling_links: retain) keep the order of what stays.  The prev lists
    // hold the same entries; duplicate_unitig_by_number reads only the next lists.
    struct Entry { int32_t a, b; bool there; };
    std::vector<Entry> e;
    e.reserve(gathered.size() + 16 * (size_t)in.n_duplicate);
    for (const Link& l : gathered) e.push_back(Entry{l.a, l.b, true});
    const size_t n_gathered = e.size();
    auto number = [](int32_t v) { return v < 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)v; };
    auto create_link = [&](int32_t start, int32_t end) {
        e.push_back(Entry{start, end, true});
        if (start != -end) e.push_back(Entry{-end, -start, true});
    };
    for (uint32_t i = 0; i < in.n_duplicate; i++) {
        const uint32_t d = in.duplicate[i];
        if (std::binary_search(in.remove, in.remove + in.n_remove, d) || (i && in.duplicate[i - 1] == d)) throw std::runtime_error(clean_gone_message(d));
        std::vector<Link> forward_next, reverse_next;
        for (const Entry& x : e) {
            if (!x.there) continue;
            if (x.a == (int32_t)d) forward_next.push_back(Link{x.a, x.b});
            else if (x.a == -(int32_t)d) reverse_next.push_back(Link{x.a, x.b});
        }
        std::vector<Link> non_self;
        for (const Link& l : forward_next) if (number(l.b) != d) non_self.push_back(l);
        for (const Link& l : reverse_next) if (number(l.b) != d) non_self.push_back(l);
        if (non_self.size() != 2) throw std::runtime_error(clean_not_two_links_message(d));
        const int32_t a_num = (int32_t)(in.n_unitigs + 1 + 2 * i), b_num = a_num + 1;
        for (Entry& x : e) if (number(x.a) == d || number(x.b) == d) x.there = false;      // remove_unitigs_by_number with delete_dangling_links
        for (const Link& l : forward_next)
            if (number(l.b) == d) { create_link(a_num, l.b > 0 ? a_num : -a_num); create_link(b_num, l.b > 0 ? b_num : -b_num); }
        for (const Link& l : reverse_next)
            if (number(l.b) == d) { create_link(-a_num, l.b > 0 ? a_num : -a_num); create_link(-b_num, l.b > 0 ? b_num : -b_num); }
        create_link(non_self[0].a > 0 ? a_num : -a_num, non_self[0].b);
        create_link(non_self[1].a > 0 ? b_num : -b_num, non_self[1].b);
    }
    created->clear();
    for (size_t j = n_gathered; j < e.size(); j++) if (e[j].there) created->push_back(Link{e[j].a, e[j].b});
}

void clean_empty(CleanResult* r) { *r = CleanResult(); }

void clean_finish(const CleanInput& in, CleanResult* r) {
    for (uint64_t& c : r->count) c = 0;
    for (uint8_t code : r->reason) if (code < CLEAN_REASONS) r->count[code]++;
    if (!in.seq_bytes || r->n_out == 0) return;      // (an empty graph keeps no bytes: there is no seq_begin to go with them)
    r->seq_all.resize(in.seq_total + 1);      // (+ 1: never an empty array behind a pointer)
    if (in.seq_total) memcpy(r->seq_all.data(), in.seq_bytes, in.seq_total);
}

std::vector<uint8_t> clean_gfa_types(const char* text, uint64_t len) {
    std::vector<uint8_t> types;
    uint64_t a = 0;
    while (a < len) {
        uint64_t e = a;
        while (e < len && text[e] != '\n') e++;
        uint64_t ll = e - a;
        if (ll && text[a + ll - 1] == '\r') ll--;
        if (ll >= 2 && text[a] == 'S' && text[a + 1] == '\t') {
            bool consentig = false, anchor = false, bridge = false;
            uint64_t f = a;
            for (uint64_t i = a; i <= a + ll; i++) {
                if (i < a + ll && text[i] != '\t') continue;
                const std::string part(text + f, i - f);
                consentig |= part == "CL:Z:steelblue"; anchor |= part == "CL:Z:forestgreen"; bridge |= part == "CL:Z:pink";
                f = i + 1;
            }
            types.push_back(consentig ? MERGE_TYPE_CONSENTIG : anchor ? MERGE_TYPE_ANCHOR : bridge ? MERGE_TYPE_BRIDGE : MERGE_TYPE_OTHER);
        }
        a = e + 1;
    }
    return types;
}

std::string clean_gfa_string(const CleanResult& r, uint32_t k, bool use_other_colour) {
    std::vector<GfaSegmentView> segs;
    for (uint32_t u = 0; u < r.n_out; u++) {
        if (!r.alive[u]) continue;
        if (r.len[u] && r.seq_all.empty()) throw std::runtime_error("clean: missing sequences: the edit was made without seq_bytes and seq_begin");
        segs.push_back(GfaSegmentView{u + 1, r.seq_all.empty() ? "" : (const char*)r.seq_all.data() + r.seq_begin[u], r.len[u], r.depth[u], r.type[u]});
    }
    return gfa_string_explicit(k, segs, r.links.data(), r.links.size(), std::vector<GfaPathView>(), use_other_colour);
}

}  // namespace ac
