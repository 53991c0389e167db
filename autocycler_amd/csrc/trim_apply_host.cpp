// The host side of trim's edit (trim_apply_host.hpp): the choice of the kind, the slice table, the exclusion's arithmetic, the yaml, the error texts.
#include "trim_apply_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace ac {

void trim_apply_choose(const TrimResult* results, uint32_t n_seqs, const int32_t* path, const uint64_t* path_off, const uint32_t* seq_length, uint32_t request,
                       TrimApplyPlan* plan) {
    if (request > TRIM_CHOOSE_HAIRPIN) throw std::runtime_error("trim apply: chosen is " + std::to_string(request) + ": it must be 0 (auto), 1 (none), 2 (start-end) or 3 (hairpin)");
    if (n_seqs == 0) throw std::runtime_error("trim apply: no sequences");
    if (n_seqs > 32767) throw std::runtime_error("trim apply: " + std::to_string(n_seqs) + " sequences: a graph holds at most 32767");
    if (!path_off) throw std::runtime_error("null pointer: path_off");
    if (!seq_length) throw std::runtime_error("null pointer: seq_length");
    if (!results && request != TRIM_CHOOSE_NONE) throw std::runtime_error("null pointer: results");
    plan->c_se = plan->c_hp = plan->rejected = plan->n_trimmed = plan->n_excluded = 0;
    for (uint32_t s = 0; results && s < n_seqs; s++) {      // (status 2 counts as not trimmed, as in trim_paths_host's summary)
        if (results[s].se.status == 1) plan->c_se++;
        if (results[s].hp.status == 1) plan->c_hp++;
        if (results[s].se.status == 2 || results[s].hp.status == 2) plan->rejected++;
    }
    if (request == TRIM_CHOOSE_AUTO)
        plan->chosen = (plan->c_se == 0 && plan->c_hp == 0) ? TRIM_KIND_NONE : plan->c_se >= plan->c_hp ? TRIM_KIND_START_END : TRIM_KIND_HAIRPIN;
    else
        plan->chosen = request - 1;
    plan->seqs.assign(n_seqs, TrimApplyRecord{0, 0, 0, 0, 0});
    plan->sliced_off.assign((size_t)n_seqs + 1, 0);
    for (uint32_t s = 0; s < n_seqs; s++) {
        if (path_off[s + 1] < path_off[s])
            throw std::runtime_error("trim apply: path_off decreases at sequence " + std::to_string(s) + " (" + std::to_string(path_off[s]) + " then " +
                                     std::to_string(path_off[s + 1]) + "): path offsets must ascend");
        const uint64_t n = path_off[s + 1] - path_off[s];
        if (n > 0xFFFFFFFFull) throw std::runtime_error("trim apply: the path of sequence " + std::to_string(s) + " has more than 2^32 entries");
        TrimApplyRecord& r = plan->seqs[s];
        const TrimSlice* t = plan->chosen == TRIM_KIND_START_END ? &results[s].se : plan->chosen == TRIM_KIND_HAIRPIN ? &results[s].hp : nullptr;
        if (t && t->status == 1) {
            if (t->begin > t->end)
                throw std::runtime_error("trim apply: the slice of sequence " + std::to_string(s) + " begins at " + std::to_string(t->begin) + ", after its end " +
                                         std::to_string(t->end));
            if (t->end > n)
                throw std::runtime_error("trim apply: the slice of sequence " + std::to_string(s) + " ends at " + std::to_string(t->end) + ", beyond its path of " +
                                         std::to_string(n) + " entries");
            r.begin = t->begin; r.end = t->end; r.length = t->length; r.trimmed = 1;
            plan->n_trimmed++;
        } else {
            r.begin = 0; r.end = (uint32_t)n; r.length = seq_length[s];
        }
        plan->sliced_off[s + 1] = plan->sliced_off[s] + (r.end - r.begin);
    }
    if (plan->sliced_off[n_seqs] && !path) throw std::runtime_error("null pointer: path_entries");
    plan->sliced.resize((size_t)plan->sliced_off[n_seqs]);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const TrimApplyRecord& r = plan->seqs[s];
        if (r.end > r.begin) memcpy(plan->sliced.data() + plan->sliced_off[s], path + path_off[s] + r.begin, (size_t)(r.end - r.begin) * 4);
    }
}

uint64_t trim_apply_median(std::vector<uint64_t> v) {
    if (v.empty()) return 0;
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    // ((a + b) / 2 of two values below 2^63, as isize holds them: no overflow in u64)
    return n % 2 == 0 ? (v[n / 2 - 1] + v[n / 2]) / 2 : v[n / 2];
}

uint64_t trim_apply_mad(const std::vector<uint64_t>& v) {
    if (v.empty()) return 0;
    const uint64_t m = trim_apply_median(v);
    std::vector<uint64_t> dev(v.size());
    for (size_t i = 0; i < v.size(); i++) dev[i] = v[i] >= m ? v[i] - m : m - v[i];
    return trim_apply_median(dev);
}

uint64_t trim_apply_round_to_usize(double x) {
    const double r = std::round(x);      // half away from zero, as f64::round
    if (!(r > 0.0)) return 0;            // negative and NaN
    if (r >= 18446744073709551616.0) return ~0ULL;
    return (uint64_t)r;
}

void trim_apply_check_settings(double min_identity, double mad) {
    if (!(min_identity >= 0.0 && min_identity <= 1.0)) throw std::runtime_error("--min_identity must be between 0.0 and 1 (inclusive)");
    if (mad < 0.0) throw std::runtime_error("--mad cannot be less than 0");
}

std::string trim_apply_empty_message(uint32_t seq) {
    return "trim apply: sequence " + std::to_string(seq) + " is kept with an empty slice: it has no starting unitig";
}
std::string trim_apply_mismatch_message(uint32_t seq, uint64_t sum, uint64_t expected) {
    return "trim apply: Position calculation mismatch: the unitigs of the slice of sequence " + std::to_string(seq) + " add up to " + std::to_string(sum) +
           " bases, its new length is " + std::to_string(expected);
}

void trim_apply_exclude(TrimApplyPlan* plan, double mad) {
    if (mad < 0.0) throw std::runtime_error("--mad cannot be less than 0");
    std::vector<uint64_t> lengths(plan->seqs.size());
    for (size_t s = 0; s < lengths.size(); s++) lengths[s] = plan->seqs[s].length;
    plan->median = trim_apply_median(lengths); plan->mad = trim_apply_mad(lengths);
    plan->min_length = 0; plan->max_length = ~0ULL;
    if (mad != 0.0) {      // (NaN excludes by a range of 0-0, as the reference's comparison and casts would)
        plan->min_length = trim_apply_round_to_usize((double)plan->median - (double)plan->mad * mad);
        plan->max_length = trim_apply_round_to_usize((double)plan->median + (double)plan->mad * mad);
    }
    plan->n_excluded = 0;
    plan->label.assign(plan->seqs.size(), 1);
    for (size_t s = 0; s < plan->seqs.size(); s++) {
        TrimApplyRecord& r = plan->seqs[s];
        r.excluded = (plan->min_length <= r.length && r.length <= plan->max_length) ? 0 : 1;
        if (r.excluded) { plan->label[s] = 0; plan->n_excluded++; }
        else if (r.begin == r.end) throw std::runtime_error(trim_apply_empty_message((uint32_t)s));
    }
}

std::string trim_apply_yaml(const TrimApplyPlan& plan) {
    std::vector<uint64_t> kept;
    for (const TrimApplyRecord& r : plan.seqs) if (!r.excluded) kept.push_back(r.length);
    std::string y = "trimmed_cluster_size: " + std::to_string((uint32_t)kept.size()) + "\n";
    if (kept.empty()) y += "trimmed_cluster_lengths: []\n";
    else {
        y += "trimmed_cluster_lengths:\n";
        for (uint64_t v : kept) y += "- " + std::to_string(v) + "\n";
    }
    y += "trimmed_cluster_median: " + std::to_string((uint32_t)trim_apply_median(kept)) + "\n";      // (`as u32`, metrics.rs:225-226)
    y += "trimmed_cluster_mad: " + std::to_string((uint32_t)trim_apply_mad(kept)) + "\n";
    return y;
}

}  // namespace ac
