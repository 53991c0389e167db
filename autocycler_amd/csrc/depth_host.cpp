// Host side of the read-based unitig depths: see depth_host.hpp.  Every loop here keeps the reference's order (links as given, walks as
// found, offsets ascending): the step budget decides which walks exist once it runs out, and the f64 sums depend on their order.
#include "depth_host.hpp"

#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <unordered_set>
#include <zlib.h>

namespace ac {
namespace {

inline int base_bits(uint8_t b) {      // base_to_bits (depth.rs:434-442)
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}
inline uint8_t complement_base(uint8_t b) {      // misc.rs:358-367: anything but an upper-case base becomes N
    switch (b) {
        case 'A': return 'T';
        case 'T': return 'A';
        case 'G': return 'C';
        case 'C': return 'G';
        case '.': return '.';
        default: return 'N';
    }
}
std::string reverse_complement(const std::string& s) {
    std::string r(s.size(), 'N');
    for (size_t i = 0; i < s.size(); i++) r[i] = (char)complement_base((uint8_t)s[s.size() - 1 - i]);
    return r;
}

// each_kmer (depth.rs:161-184)
template <class F> void each_kmer(const std::string& seq, uint32_t k, F&& f) {
    if (seq.size() < k) return;
    const uint64_t mask = (1ULL << (2 * k)) - 1;
    const unsigned shift = 2 * (k - 1);
    uint64_t fwd = 0, rev = 0; size_t valid = 0;
    for (size_t i = 0; i < seq.size(); i++) {
        const int bits = base_bits((uint8_t)seq[i]);
        if (bits < 0) { fwd = 0; rev = 0; valid = 0; continue; }
        fwd = ((fwd << 2) | (uint64_t)bits) & mask;
        rev = (rev >> 2) | ((uint64_t)(3 - bits) << shift);
        valid++;
        if (valid >= k) f(i + 1 - k, fwd < rev ? fwd : rev);
    }
}

struct Walker {
    const DepthGraphView& g;
    std::vector<std::vector<int32_t>> fwd_next, rev_next;      // by unitig index, in link order
    explicit Walker(const DepthGraphView& gv) : g(gv), fwd_next(gv.n_unitigs), rev_next(gv.n_unitigs) {}
    const std::vector<int32_t>& next(int32_t strand) const { return strand > 0 ? fwd_next[(size_t)strand - 1] : rev_next[(size_t)(-(int64_t)strand) - 1]; }
    uint32_t len(int32_t strand) const { return g.seq_len[(size_t)(strand > 0 ? strand : -(int64_t)strand) - 1]; }
    const uint8_t* fwd(int32_t strand) const { return g.seq_bytes + g.seq_begin[(size_t)(strand > 0 ? strand : -(int64_t)strand) - 1]; }
    // the bases [from, from + n) of a strand's sequence (reverse strand: Unitig::reverse_seq = reverse_complement(forward_seq))
    std::string slice(int32_t strand, size_t from, size_t n) const {
        const uint8_t* s = fwd(strand); const size_t L = len(strand);
        std::string r(n, 'N');
        if (strand > 0) memcpy(&r[0], s + from, n);
        else for (size_t i = 0; i < n; i++) r[i] = (char)complement_base(s[L - 1 - (from + i)]);
        return r;
    }
    // extensions (depth.rs:252-279)
    std::vector<std::string> extensions(const std::vector<int32_t>& nx, size_t length, size_t* steps) const {
        std::vector<std::string> seqs;
        for (int32_t strand : nx) {
            if (*steps == 0) break;
            --*steps;
            const size_t take = std::min<size_t>(length, len(strand));
            std::string seq = slice(strand, 0, take);
            if (seq.size() == length) { seqs.push_back(std::move(seq)); continue; }
            std::vector<std::string> further = extensions(next(strand), length - seq.size(), steps);
            if (further.empty()) seqs.push_back(std::move(seq));
            else for (auto& f : further) seqs.push_back(seq + f);
        }
        return seqs;
    }
};

}  // namespace

void depth_plan_graph(uint32_t k, const DepthGraphView& g, uint32_t graph_index, DepthGraphPlan* out) {
    Walker w(g);
    for (uint64_t i = 0; i < g.n_links; i++) {
        const int32_t a = g.links[2 * i], b = g.links[2 * i + 1];
        const int64_t ua = a < 0 ? -(int64_t)a : a, ub = b < 0 ? -(int64_t)b : b;
        if (ua == 0 || ub == 0 || ua > (int64_t)g.n_unitigs || ub > (int64_t)g.n_unitigs)
            throw std::runtime_error("link " + std::to_string(i + 1) + " of graph " + std::to_string(graph_index + 1) + " has an end that is 0 or beyond the graph's " +
                                     std::to_string(g.n_unitigs) + " unitigs");
        (a > 0 ? w.fwd_next : w.rev_next)[(size_t)ua - 1].push_back(b);
    }
    out->junction.clear(); out->kmers.clear(); out->ctx.clear();
    out->ctx_begin.assign((size_t)g.n_unitigs + 1, 0);
    const size_t K = k;
    for (uint32_t u = 0; u < g.n_unitigs; u++) {
        const int32_t num = (int32_t)(u + 1);
        const size_t n = g.seq_len[u];
        // junction_kmers (depth.rs:101-134): a fresh budget per strand
        for (int32_t strand : {num, -num}) {
            size_t steps = DEPTH_MAX_WALK_STEPS;
            const std::vector<std::string> walks = w.extensions(w.next(strand), K - 1, &steps);
            if (walks.empty()) continue;
            const size_t s0 = n > K - 1 ? n - (K - 1) : 0;
            const std::string tail = w.slice(strand, s0, n - s0);
            for (size_t start = s0; start < n; start++) {
                const size_t needed = K - (n - start);
                for (const std::string& walk : walks) {
                    if (needed > walk.size()) continue;
                    const std::string km = tail.substr(start - s0) + walk.substr(0, needed);
                    uint64_t fwd = 0, rev = 0; bool ok = true;
                    for (size_t i = 0; i < K && ok; i++) {
                        const int bits = base_bits((uint8_t)km[i]);
                        if (bits < 0) { ok = false; break; }
                        fwd = (fwd << 2) | (uint64_t)bits;
                        rev = (rev >> 2) | ((uint64_t)(3 - bits) << (2 * (K - 1)));
                    }
                    if (ok && fwd < rev) out->junction.push_back(fwd);
                }
            }
        }
        // context_kmers (depth.rs:187-232): one budget, left then right
        size_t steps = DEPTH_MAX_WALK_STEPS;
        std::vector<std::string> left = w.extensions(w.next(-num), K - 1, &steps);
        std::vector<std::string> right = w.extensions(w.next(num), K - 1, &steps);
        for (auto& s : left) s = reverse_complement(s);
        if (left.empty()) left.emplace_back();
        if (right.empty()) right.emplace_back();
        struct Variants { std::vector<uint64_t> order; std::unordered_set<uint64_t> have; };      // (the set only answers `contains`)
        std::map<int32_t, Variants> found;
        const int64_t last_inside = (int64_t)n - (int64_t)K;
        auto add = [&](const std::string& context, int64_t first_offset) {      // add_context_kmers (depth.rs:235-249)
            each_kmer(context, k, [&](size_t i, uint64_t kmer) {
                const int64_t offset = first_offset + (int64_t)i;
                if (offset < 0 || offset > last_inside) {
                    Variants& v = found[(int32_t)offset];
                    if (v.have.insert(kmer).second) v.order.push_back(kmer);
                }
            });
        };
        if (n >= K) {
            const std::string head = w.slice(num, 0, K - 1), tail = w.slice(num, n - K + 1, K - 1);
            for (const std::string& s : left) add(s + head, -(int64_t)s.size());
            for (const std::string& s : right) add(tail + s, (int64_t)(n - K + 1));
        } else {
            const std::string whole = w.slice(num, 0, n);
            for (const std::string& l : left)
                for (const std::string& r : right) add(l + whole + r, -(int64_t)l.size());
        }
        for (auto& kv : found) {
            out->ctx.push_back(DepthContext{kv.first, (uint32_t)kv.second.order.size(), (uint64_t)out->kmers.size()});
            out->kmers.insert(out->kmers.end(), kv.second.order.begin(), kv.second.order.end());
        }
        out->ctx_begin[u + 1] = out->ctx.size();
    }
}

bool depth_clipped_mean(const std::vector<uint32_t>& counts, double* mean_out) {
    if (counts.empty()) return false;
    const double count = (double)counts.size();
    double sum = 0.0;
    for (uint32_t c : counts) sum += (double)c;
    const double mean = sum / count;
    const double six = 6.0 * std::sqrt(mean);
    const double a = mean + six, b = 2.0 * mean;
    const double limit = a > b ? a : b;
    double clipped = 0.0;
    for (uint32_t c : counts) { const double v = (double)c; clipped += v < limit ? v : limit; }
    *mean_out = clipped / count;
    return true;
}

namespace {
struct GzLines {
    gzFile f; std::string path; std::vector<char> buf; size_t at = 0, have = 0; bool eof = false;
    GzLines(const char* p) : f(gzopen(p, "rb")), path(p), buf((size_t)4 << 20) {
        if (!f) throw std::runtime_error("unable to read " + path);
        gzbuffer(f, 1 << 20);
    }
    ~GzLines() { if (f) gzclose(f); }
    void fill() {
        const int got = gzread(f, buf.data(), (unsigned)buf.size());
        if (got < 0) { int e = 0; const char* m = gzerror(f, &e); throw std::runtime_error("truncated FASTQ: unable to read " + path + ": " + (m ? m : "read error")); }
        at = 0; have = (size_t)got;
        if (got == 0) {
            eof = true;
            int e = 0; (void)gzerror(f, &e);
            if (e != Z_OK && e != Z_STREAM_END) throw std::runtime_error("truncated FASTQ: " + path + " ends inside its compressed stream");
        }
    }
    // false at the end of the file with nothing read; *complete = the line ended with a newline
    bool line(std::string* out, bool* complete) {
        out->clear(); *complete = false;
        bool any = false;
        for (;;) {
            if (at == have) { if (eof) break; fill(); if (eof) break; }
            const char* s = buf.data() + at;
            const char* nl = (const char*)memchr(s, '\n', have - at);
            any = true;
            if (nl) { out->append(s, (size_t)(nl - s)); at += (size_t)(nl - s) + 1; *complete = true; break; }
            out->append(s, have - at); at = have;
        }
        if (!out->empty() && out->back() == '\r') out->pop_back();
        return any;
    }
};
}  // namespace

void depth_read_fastq(const char* path, size_t flush_bytes,
                      const std::function<void(const std::vector<uint8_t>&, const std::vector<uint64_t>&)>& sink) {
    GzLines in(path);
    if (gzdirect(in.f) == 0) { /* gzip: a stream that ends early is reported by gzread */ }
    std::vector<uint8_t> bases; std::vector<uint64_t> off(1, 0);
    std::string head, seq, plus, qual; bool c = false;
    uint64_t record = 0;
    auto bad = [&](const char* what) {
        throw std::runtime_error("truncated FASTQ: " + std::string(path) + ", record " + std::to_string(record + 1) + ": " + what);
    };
    for (;;) {
        if (!in.line(&head, &c)) break;
        if (head.empty()) continue;      // blank lines between records / at the end
        if (head[0] != '@') bad("the header line does not start with '@'");
        if (!in.line(&seq, &c) || !c) bad("the file ends after the header line");
        if (!in.line(&plus, &c) || !c) bad("the file ends inside the sequence");
        if (plus.empty() || plus[0] != '+') bad("the third line does not start with '+'");
        if (!in.line(&qual, &c)) bad("the file ends before the quality line");
        if (qual.size() != seq.size()) bad("the quality line is not as long as the sequence");
        bases.insert(bases.end(), seq.begin(), seq.end());
        off.push_back(bases.size());
        record++;
        if (bases.size() >= flush_bytes) { sink(bases, off); bases.clear(); off.assign(1, 0); }
    }
    if (off.size() > 1) sink(bases, off);
}

}  // namespace ac
