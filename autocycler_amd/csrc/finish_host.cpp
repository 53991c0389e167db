// The host side of a finished graph (finish_host.hpp): input checks, consistency checks, the text.  Built with -ffp-contract=off like the
// other host files whose numbers are compared with the reference's.
#include "finish_host.hpp"

#include <cmath>
#include <stdexcept>

#include "gfa_writer.hpp"

namespace ac {

std::string finish_nan_depth_message(uint32_t number, bool chain) {
    return std::string("finish: the depth of ") + (chain ? "merged unitig " : "unitig ") + std::to_string(number) +
           " is NaN: renumber_unitigs' comparator is no total order there";
}
std::string finish_bad_path_entry_message(uint64_t index, int32_t entry) {
    return "finish: path entry " + std::to_string(index) + " (" + std::to_string(entry) + ") names no unitig of the graph after the merge";
}

uint64_t finish_check_inputs(const MergeResult& plan, const FinishArrays& in, bool renumber) {
    const uint32_t n = in.n_unitigs;
    if (plan.n_unitigs != n)
        throw std::runtime_error("finish: the plan is over " + std::to_string(plan.n_unitigs) + " unitigs, the call over " + std::to_string(n));
    if (plan.links_in != in.n_links)
        throw std::runtime_error("finish: the plan was made from " + std::to_string(plan.links_in) + " links, the call gives " + std::to_string(in.n_links));
    if (n && !in.unitig_len) throw std::runtime_error("null pointer: unitig_len");
    if ((in.seq_bytes == nullptr) != (in.seq_begin == nullptr)) throw std::runtime_error("seq_bytes and seq_begin: both or neither");
    if (plan.chain_of.size() != n) throw std::runtime_error("finish: the plan's arrays contradict each other (internal error)");
    uint64_t survivors = 0, bases = 0, merged_bases = 0;
    for (uint32_t u = 0; u < n; u++) {
        if (in.alive && !in.alive[u]) continue;
        if (plan.chain_of[u] != MERGE_NOT_MERGED) continue;
        survivors++; bases += in.unitig_len[u];
        if (renumber && in.depth && std::isnan(in.depth[u])) throw std::runtime_error(finish_nan_depth_message(u + 1, false));
    }
    for (size_t c = 0; c < plan.chains.size(); c++) {
        const MergeChainRecord& rec = plan.chains[c];
        if (renumber && std::isnan(rec.depth)) throw std::runtime_error(finish_nan_depth_message(rec.number, true));
        if (rec.length && (plan.seq.empty() || rec.seq_off > plan.seq.size() || rec.length > plan.seq.size() - rec.seq_off))
            throw std::runtime_error("finish: missing sequences: the plan was made without them (merged unitig " + std::to_string(rec.number) + " has " +
                                     std::to_string(rec.length) + " bases)");
        merged_bases += rec.length;
    }
    if (bases && !in.seq_bytes) throw std::runtime_error("finish: missing sequences: seq_bytes and seq_begin are needed (the unmerged unitigs have " + std::to_string(bases) + " bases)");
    if (bases + merged_bases >= (1ULL << 46)) throw std::runtime_error("finish: 2^46 bases or more");
    const uint64_t after = survivors + plan.chains.size();
    if (after != plan.unitigs_after)
        throw std::runtime_error("finish: " + std::to_string(after) + " unitigs are left, the plan has " + std::to_string(plan.unitigs_after) +
                                 ": it was made from another alive mask");
    return after;
}

void finish_empty(FinishResult* r, bool renumber) {
    *r = FinishResult();
    r->renumbered = renumber;
    r->path_off.assign(1, 0);
}

void finish_check_result(const FinishResult& r, const MergeResult& plan, uint64_t unitigs_after) {
    if (r.unitigs.size() != unitigs_after || r.new_of_old.size() != (size_t)plan.n_unitigs + plan.chains.size())
        throw std::runtime_error("finish: the device returned arrays of impossible sizes (internal error)");
    if (r.links.size() != plan.links.size())
        throw std::runtime_error("finish: " + std::to_string(r.links.size()) + " links survive the merge, the plan has " + std::to_string(plan.links.size()) +
                                 ": the links are not the ones the plan was made from");
    uint64_t at = 0;
    for (const FinishedUnitigRecord& u : r.unitigs) {
        if (u.seq_off != at || u.number == 0 || u.source == 0 || u.source > r.new_of_old.size() || r.new_of_old[u.source - 1] != u.number)
            throw std::runtime_error("finish: the device returned records that contradict each other (internal error)");
        at += u.length;
    }
    if (at != r.seq.size()) throw std::runtime_error("finish: the gathered sequences do not add up (internal error)");
}

std::string finish_gfa_string(const FinishResult& r, uint32_t k, const std::vector<FinishSeqMeta>& meta, bool use_other_colour) {
    if (meta.size() != r.path_seq.size())
        throw std::runtime_error("finish: " + std::to_string(meta.size()) + " sequence records for " + std::to_string(r.path_seq.size()) + " P lines");
    std::vector<GfaSegmentView> segs(r.unitigs.size());
    for (size_t i = 0; i < segs.size(); i++) {
        const FinishedUnitigRecord& u = r.unitigs[i];
        segs[i] = GfaSegmentView{u.number, (const char*)r.seq.data() + u.seq_off, u.length, u.depth, u.type};
    }
    std::vector<GfaPathView> paths(meta.size());
    for (size_t s = 0; s < paths.size(); s++)
        paths[s] = GfaPathView{meta[s].id, r.path_entries.data() + r.path_off[s], r.path_off[s + 1] - r.path_off[s], meta[s].length, &meta[s].filename, &meta[s].header,
                               meta[s].cluster};
    return gfa_string_explicit(k, segs, r.links.data(), r.links.size(), paths, use_other_colour);
}

}  // namespace ac
