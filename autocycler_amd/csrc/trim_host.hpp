// `autocycler trim`: what the host does around the device's overlap alignments (kernels_trim.inc) — plain C++, no device code.
// The alignments of all sequences go to the device in two batches (start-end + hairpin start, then hairpin end on the start-trimmed
// paths); everything here is O(alignment length): the identity test (trim.rs:468-475), find_midpoint (:482-507), the hairpin
// bookkeeping (:299-326) and choose_trim_type's count (:189-211).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

namespace ac {

static const uint32_t ALIGN_NONE = 0xFFFFFFFFu;      // AlignmentPiece index of a gap (usize::MAX in the reference); GAP itself is unitig 0
struct AlignPiece { int32_t a_unitig; uint32_t a_index; int32_t b_unitig; uint32_t b_index; };
struct AlignJob { std::vector<int32_t> a, b; bool skip_diagonal = false; };      // |a| == |b|
// What the traceback kernel hands back.  status: 0 = the traceback reached the top edge, 1 = the best right-edge score is <= 0,
// 2 = the traceback ended on the left edge (1 and 2: pieces is empty).  matches / len_a / len_b: summed weights of equal pairs / non-gap a / non-gap b.
struct AlignOut { uint32_t status = 1; uint64_t matches = 0, len_a = 0, len_b = 0; std::vector<AlignPiece> pieces; };
typedef std::function<void(const std::vector<AlignJob>&, std::vector<AlignOut>&)> AlignBatchFn;

// trim.rs:468-475: true when the alignment is kept (pieces is emptied otherwise)
bool alignment_passes(AlignOut* o, double min_identity);

struct TrimSlice { uint32_t status = 0, begin = 0, end = 0, length = 0; };      // status: 0 not trimmed, 1 trimmed, 2 the reference would have panicked
struct TrimResult { TrimSlice se, hp; uint32_t hp_start = 0, hp_end = 0; };
struct TrimSummary { uint32_t c_se = 0, c_hp = 0, chosen = 0; };

// throws std::runtime_error: an entry that is 0 or names a unitig beyond the weights, a path whose weights add up to 2^32 or more
void validate_trim_path(const int32_t* path, uint64_t n, const uint32_t* weights, uint32_t n_weights, const char* what);
std::vector<int32_t> reverse_path(const int32_t* p, uint64_t n);      // reversed and negated (misc.rs reverse_path)

// trim_start_end_overlap + trim_harpin_overlap + the counts of choose_trim_type for n_seqs paths (path[off[s] .. off[s + 1])).
void trim_paths_host(const int32_t* path, const uint64_t* off, uint32_t n_seqs, const uint32_t* weights, double min_identity,
                     uint32_t max_unitigs, const AlignBatchFn& run, TrimResult* out, TrimSummary* summary);

}  // namespace ac
