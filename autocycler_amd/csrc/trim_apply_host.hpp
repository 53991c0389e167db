// `autocycler trim` after the alignments (trim.rs:189-269): choose_trim_type, the slices with create_sequence_and_positions' length check,
// exclude_outliers_in_length and what clean_up_graph starts from — the host side: the choice and the slice table, median / MAD / range with
// Rust's round and `as usize`, the keep flags, 2_trimmed.yaml, the error texts.  Plain C++, no device code; everything that grows with the
// path entries is kernels_trim_apply.inc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "trim_host.hpp"

namespace ac {

static const uint32_t TRIM_CHOOSE_AUTO = 0, TRIM_CHOOSE_NONE = 1, TRIM_CHOOSE_START_END = 2, TRIM_CHOOSE_HAIRPIN = 3;
static const uint32_t TRIM_KIND_NONE = 0, TRIM_KIND_START_END = 1, TRIM_KIND_HAIRPIN = 2;      // ac_trim_summary.chosen's values

// ac_trimmed_record, field for field
struct TrimApplyRecord {
    uint32_t begin, end;      // the slice of the sequence's path that stays
    uint64_t length;          // its new length
    uint32_t trimmed, excluded;
};

struct TrimApplyPlan {
    uint32_t chosen = 0, c_se = 0, c_hp = 0, rejected = 0, n_trimmed = 0, n_excluded = 0;
    uint64_t median = 0, mad = 0, min_length = 0, max_length = 0;      // of the new lengths; the range is [0, 2^64 - 1] when nothing is excluded by rule (mad == 0)
    std::vector<TrimApplyRecord> seqs;
    std::vector<int32_t> sliced;            // the slices back to back
    std::vector<uint64_t> sliced_off;       // n_seqs + 1
    std::vector<uint16_t> label;            // 1 kept, 0 excluded: subset_prepare's cluster_of_seq
};

// choose_trim_type (trim.rs:189-226) and the slices.  `request`: TRIM_CHOOSE_*.  results may be null when nothing is to be trimmed
// (TRIM_CHOOSE_NONE).  Throws std::runtime_error: begin > end, end beyond the path, descending offsets.
void trim_apply_choose(const TrimResult* results, uint32_t n_seqs, const int32_t* path, const uint64_t* path_off, const uint32_t* seq_length, uint32_t request,
                       TrimApplyPlan* plan);
// median_isize / mad_isize (misc.rs:433-457) of unsigned values; 0 for an empty list, as median_usize is
uint64_t trim_apply_median(std::vector<uint64_t> v);
uint64_t trim_apply_mad(const std::vector<uint64_t>& v);
// Rust's f64::round (half away from zero) followed by `as usize` (saturating; NaN = 0)
uint64_t trim_apply_round_to_usize(double x);
// exclude_outliers_in_length (trim.rs:229-257): fills median, mad, the range, excluded and label.  Throws on mad < 0 (trim.rs:60) and on a kept
// sequence with an empty slice (find_starting_unitig's assertion, unitig_graph.rs:423).
void trim_apply_exclude(TrimApplyPlan* plan, double mad);
void trim_apply_check_settings(double min_identity, double mad);
// TrimmedClusterMetrics (metrics.rs:213-230) as serde_yaml 0.9 prints it
std::string trim_apply_yaml(const TrimApplyPlan& plan);

std::string trim_apply_mismatch_message(uint32_t seq, uint64_t sum, uint64_t expected);
std::string trim_apply_empty_message(uint32_t seq);

}  // namespace ac
