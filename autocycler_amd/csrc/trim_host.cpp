// Host side of ac_trim_paths (trim_host.hpp): the reference's post-processing of the overlap alignments, restated over plain arrays.
#include "trim_host.hpp"

#include <cmath>
#include <stdexcept>
#include <string>

namespace ac {

static uint32_t wt(const uint32_t* weights, int32_t u) { return weights[(uint32_t)(u < 0 ? -(int64_t)u : (int64_t)u) - 1]; }

void validate_trim_path(const int32_t* path, uint64_t n, const uint32_t* weights, uint32_t n_weights, const char* what) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        const int64_t p = path[i], u = p < 0 ? -p : p;
        if (u == 0 || u > (int64_t)n_weights)
            throw std::runtime_error(std::string(what) + ": entry " + std::to_string(i) + " (" + std::to_string(p) + ") names no unitig of the " + std::to_string(n_weights) + " that have a weight");
        sum += weights[u - 1];
    }
    if (sum >= ((uint64_t)1 << 32)) throw std::runtime_error(std::string(what) + ": the weights of the path add up to 2^32 or more");
}

std::vector<int32_t> reverse_path(const int32_t* p, uint64_t n) {
    std::vector<int32_t> r(n);
    for (uint64_t i = 0; i < n; i++) r[i] = -p[n - 1 - i];
    return r;
}

bool alignment_passes(AlignOut* o, double min_identity) {
    if (o->status != 0) { o->pieces.clear(); return false; }
    // (the reference's expression, trim.rs:470-473, from the three integer sums)
    const double mean_length = ((double)o->len_a + (double)o->len_b) / 2.0;
    const double alignment_identity = (double)o->matches / mean_length;
    if (alignment_identity < min_identity) { o->pieces.clear(); return false; }
    return true;
}

// find_midpoint (trim.rs:482-507)
static size_t find_midpoint(const std::vector<AlignPiece>& al, const uint32_t* weights) {
    uint64_t total = 0;
    for (const AlignPiece& p : al) {
        if (p.a_unitig != 0) total += wt(weights, p.a_unitig);
        if (p.b_unitig != 0) total += wt(weights, p.b_unitig);
    }
    uint64_t cum = 0;
    size_t best = 0;
    double best_closeness = 1.0;
    for (size_t i = 0; i < al.size(); i++) {
        const AlignPiece& p = al[i];
        if (p.a_unitig != 0) cum += wt(weights, p.a_unitig);
        if (p.b_unitig != 0) cum += wt(weights, p.b_unitig);
        const double closeness = std::fabs(0.5 - ((double)cum / (double)total));
        if (p.a_unitig == p.b_unitig && closeness < best_closeness) { best = i; best_closeness = closeness; }
    }
    return best;
}

// The loop of trim_path_hairpin_end (trim.rs:304-315) over an alignment that passed.  false: one of the reference's own checks
// (the assertion of :310, or the unwrap of an empty front before it) would have stopped the program.
static bool hairpin_end_of(const std::vector<AlignPiece>& al, uint32_t* end) {
    size_t lo = 0, hi = al.size();
    *end = 0;
    while (lo < hi) {
        while (lo < hi && al[lo].a_unitig == 0) lo++;          // trim_gaps_a_front
        while (lo < hi && al[hi - 1].b_unitig == 0) hi--;      // trim_gaps_b_back
        if (lo == hi) break;
        const AlignPiece& back = al[--hi];
        if (lo == hi) return false;
        if ((int64_t)back.b_unitig != -(int64_t)al[lo].a_unitig) return false;
        if (back.a_unitig != 0) *end = back.b_index;
        lo++;
    }
    return true;
}

static uint32_t slice_length(const int32_t* p, uint32_t b, uint32_t e, const uint32_t* weights) {
    uint64_t s = 0;
    for (uint32_t i = b; i < e; i++) s += wt(weights, p[i]);
    return (uint32_t)s;
}

void trim_paths_host(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint32_t* weights, double min_identity,
                     uint32_t max_unitigs, const AlignBatchFn& run, TrimResult* out, TrimSummary* summary) {
    *summary = TrimSummary();
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint32_t n = (uint32_t)(off[s + 1] - off[s]);
        out[s] = TrimResult();
        out[s].se.end = out[s].hp.end = n;
        out[s].se.length = out[s].hp.length = slice_length(path + off[s], 0, n, weights);
    }
    if (max_unitigs == 0 || n_seqs == 0) return;      // (trim.rs:106, :141: trimming disabled)
    // phase 1: start-end (the path against itself, diagonal skipped) and hairpin start (= hairpin end of the reversed path)
    std::vector<AlignJob> jobs((size_t)2 * n_seqs);
    std::vector<AlignOut> outs;
    for (uint32_t s = 0; s < n_seqs; s++) {
        const int32_t* p = path + off[s];
        const uint64_t n = off[s + 1] - off[s];
        jobs[2 * s].a.assign(p, p + n); jobs[2 * s].b = jobs[2 * s].a; jobs[2 * s].skip_diagonal = true;
        jobs[2 * s + 1].a.assign(p, p + n); jobs[2 * s + 1].b = reverse_path(p, n);      // rev(rev(P)) against rev(P)
    }
    run(jobs, outs);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const int32_t* p = path + off[s];
        const uint32_t n = (uint32_t)(off[s + 1] - off[s]);
        TrimResult& r = out[s];
        if (alignment_passes(&outs[2 * s], min_identity) && !outs[2 * s].pieces.empty()) {      // trim_path_start_end (trim.rs:288-296)
            const AlignPiece& m = outs[2 * s].pieces[find_midpoint(outs[2 * s].pieces, weights)];
            if (m.a_index == ALIGN_NONE || m.b_index == ALIGN_NONE || m.a_index > m.b_index || m.b_index > n) r.se.status = 2;      // path[start..end] would panic
            else { r.se.status = 1; r.se.begin = m.a_index; r.se.end = m.b_index; r.se.length = slice_length(p, r.se.begin, r.se.end, weights); }
        }
        if (alignment_passes(&outs[2 * s + 1], min_identity) && !outs[2 * s + 1].pieces.empty()) {      // trim_path_hairpin_start (:320-326)
            uint32_t end = 0;
            if (!hairpin_end_of(outs[2 * s + 1].pieces, &end) || end > n) r.hp.status = 2;
            else { r.hp_start = 1; r.hp.begin = n - end; }      // rev(rev(P)[..end]) = P[n - end ..]
        }
    }
    // phase 2: hairpin end of the start-trimmed paths
    jobs.assign(n_seqs, AlignJob());
    for (uint32_t s = 0; s < n_seqs; s++) {
        if (out[s].hp.status == 2) continue;      // (an empty job: no alignment)
        const int32_t* q = path + off[s] + out[s].hp.begin;
        const uint64_t m = (off[s + 1] - off[s]) - out[s].hp.begin;
        jobs[s].a = reverse_path(q, m); jobs[s].b.assign(q, q + m);
    }
    run(jobs, outs);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const int32_t* p = path + off[s];
        TrimResult& r = out[s];
        if (r.hp.status != 2 && alignment_passes(&outs[s], min_identity) && !outs[s].pieces.empty()) {
            uint32_t end = 0;
            if (!hairpin_end_of(outs[s].pieces, &end) || end > r.hp.end - r.hp.begin) r.hp.status = 2;
            else { r.hp_end = 1; r.hp.end = r.hp.begin + end; }
        }
        if (r.hp.status == 2) { r.hp_start = r.hp_end = 0; r.hp.begin = 0; r.hp.end = (uint32_t)(off[s + 1] - off[s]); }
        else if (r.hp_start || r.hp_end) r.hp.status = 1;
        r.hp.length = slice_length(p, r.hp.begin, r.hp.end, weights);
        if (r.se.status == 1) summary->c_se++;
        if (r.hp.status == 1) summary->c_hp++;
    }
    // choose_trim_type (trim.rs:189-211)
    summary->chosen = (summary->c_se == 0 && summary->c_hp == 0) ? 0u : (summary->c_se >= summary->c_hp ? 1u : 2u);
}

}  // namespace ac
