// The host side of apply_bridges (apply_host.hpp): the checks on the bridge records, the numbering of the bridge unitigs, the layout of the
// device's work items, the text and the error texts.
#include "apply_host.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "gfa_writer.hpp"

namespace ac {

std::string apply_bridge_name(uint32_t bridge, int32_t start, int32_t end) {
    return "bridge " + std::to_string(bridge) + " (" + std::to_string(start) + " -> " + std::to_string(end) + ")";
}
std::string apply_conflict_message(uint32_t bridge_a, int32_t start_a, int32_t end_a, uint32_t bridge_b, int32_t start_b, int32_t end_b) {
    return "apply bridges: the applied bridges conflict: " + apply_bridge_name(bridge_a, start_a, end_a) + " and " + apply_bridge_name(bridge_b, start_b, end_b) +
           " share a start or an end (apply where determine_ambiguity left no flag, or where cull_ambiguity kept the bridge)";
}
std::string apply_long_bridge_message(uint32_t bridge, uint64_t bytes) {
    return "apply bridges: the best path of bridge " + std::to_string(bridge) + " has " + std::to_string(bytes) + " bases: more than a unitig length can hold";
}
std::string apply_bad_entry_message(const ApplyPlan& plan, const ApplyInput& in, bool best, uint64_t at) {
    const int32_t e = best ? in.best[at] : in.dist_entries[at];
    std::string where = "an applied bridge";
    if (best) {
        for (size_t q = 0; q < plan.bridge_of.size(); q++)
            if (plan.q_best_off[q] <= at && at - plan.q_best_off[q] < plan.q_begin[q + 1] - plan.q_begin[q]) {
                const ApplyBridgeIn& b = in.bridges[plan.bridge_of[q]];
                where = apply_bridge_name(plan.bridge_of[q], b.start, b.end);
            }
    } else {
        for (size_t p = 0; p < plan.vis_src.size(); p++)
            if (plan.vis_src[p] <= at && at - plan.vis_src[p] < plan.vis_begin[p + 1] - plan.vis_begin[p]) {
                const ApplyBridgeIn& b = in.bridges[plan.vis_bridge[p]];
                where = apply_bridge_name(plan.vis_bridge[p], b.start, b.end);
            }
    }
    const uint64_t u = e < 0 ? (uint64_t)(-(int64_t)e) : (uint64_t)e;
    const char* why = u == 0 ? "is 0" : u > in.n_unitigs ? "is beyond n_unitigs" : "names a unitig that is not alive";
    return std::string("apply bridges: entry ") + std::to_string(at) + " of the " + (best ? "best-path" : "distinct-path") + " pool (" + std::to_string(e) + "), on a path of " +
           where + ", " + why;
}

static void check_anchor_end(const ApplyInput& in, uint32_t b, int32_t v, const char* what) {
    const ApplyBridgeIn& br = in.bridges[b];
    const uint64_t u = v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v;
    const std::string name = std::string("apply bridges: the ") + what + " of " + apply_bridge_name(b, br.start, br.end);
    if (u == 0) throw std::runtime_error(name + " is 0");
    if (u > in.n_unitigs) throw std::runtime_error(name + " is beyond n_unitigs (" + std::to_string(in.n_unitigs) + ")");
    if (in.alive && !in.alive[u - 1]) throw std::runtime_error(name + " names a unitig that is not alive");
    if (!std::binary_search(in.anchors, in.anchors + in.n_anchors, (uint32_t)u)) throw std::runtime_error(name + " is not among the anchors");
}

void apply_prepare(const ApplyInput& in, ApplyPlan* plan) {
    *plan = ApplyPlan();
    const uint32_t n = in.n_unitigs;
    if (n > 0x7FFFFFFEu) throw std::runtime_error("apply bridges: more unitigs than a signed unitig number can name");
    if (n && !in.unitig_len) throw std::runtime_error("null pointer: unitig_len");
    if (in.n_links && !in.links) throw std::runtime_error("null pointer: n_links > 0 without links");
    if ((in.seq_bytes == nullptr) != (in.seq_begin == nullptr)) throw std::runtime_error("seq_bytes and seq_begin: both or neither");
    if (in.n_anchors && !in.anchors) throw std::runtime_error("null pointer: n_anchors > 0 without anchors");
    if (in.n_bridges && (!in.bridges || !in.apply)) throw std::runtime_error("null pointer: n_bridges > 0 without bridges or apply");
    if (in.n_dist_paths && (!in.dist_off || !in.dist_mult)) throw std::runtime_error("null pointer: distinct paths without offsets or multiplicities");
    for (uint32_t i = 0; i < in.n_anchors; i++) {
        if (in.anchors[i] == 0 || in.anchors[i] > n) throw std::runtime_error("apply bridges: anchor " + std::to_string(in.anchors[i]) + " names no unitig");
        if (i && in.anchors[i] <= in.anchors[i - 1]) throw std::runtime_error("apply bridges: the anchors must ascend (anchor " + std::to_string(in.anchors[i]) + ")");
    }
    for (uint64_t p = 0; p < in.n_dist_paths; p++)
        if (in.dist_off[p + 1] < in.dist_off[p] || in.dist_off[p + 1] > in.n_dist_entries) throw std::runtime_error("apply bridges: the distinct-path offsets must ascend inside the pool");
    plan->q_begin.push_back(0); plan->vis_begin.push_back(0);
    for (uint32_t b = 0; b < in.n_bridges; b++) {
        if (!in.apply[b]) continue;
        const ApplyBridgeIn& br = in.bridges[b];
        if (br.status == 2)
            throw std::runtime_error("apply bridges: " + apply_bridge_name(b, br.start, br.end) + " has status 2 (the reference's own arithmetic would overflow on it): it has no best path to apply");
        check_anchor_end(in, b, br.start, "start");
        check_anchor_end(in, b, br.end, "end");
        if (br.best_off > in.n_best || br.best_len > in.n_best - br.best_off || (br.best_len && !in.best))
            throw std::runtime_error("apply bridges: the best path of " + apply_bridge_name(b, br.start, br.end) + " lies outside the best-path pool");
        if (br.first_distinct > in.n_dist_paths || br.n_distinct > in.n_dist_paths - br.first_distinct || (br.n_distinct && !in.dist_entries && in.n_dist_entries))
            throw std::runtime_error("apply bridges: the distinct paths of " + apply_bridge_name(b, br.start, br.end) + " lie outside the distinct-path pool");
        ApplyRecord rec;
        rec.start = br.start; rec.end = br.end; rec.bridge = b; rec.unitig = 0xFFFFFFFFu; rec.created_off = plan->n_created;
        if (br.best_len) {
            rec.unitig = (uint32_t)plan->bridge_of.size();
            plan->bridge_of.push_back(b);
            plan->q_best_off.push_back(br.best_off);
            plan->n_members += br.best_len;
            plan->q_begin.push_back(plan->n_members);
            plan->n_created += 4;
            for (uint64_t p = br.first_distinct; p < br.first_distinct + br.n_distinct; p++) {      // reduce_depths: all of the bridge's paths, the copies included
                plan->vis_src.push_back(in.dist_off[p]); plan->vis_mult.push_back(in.dist_mult[p]); plan->vis_bridge.push_back(b);
                plan->n_visits += in.dist_off[p + 1] - in.dist_off[p];
                plan->vis_begin.push_back(plan->n_visits);
            }
        } else {
            plan->n_direct++;
            plan->n_created += br.start == -br.end ? 1 : 2;
        }
        plan->records.push_back(rec);
    }
    if ((uint64_t)n + plan->bridge_of.size() > 0x7FFFFFFEULL)
        throw std::runtime_error("apply bridges: " + std::to_string(n) + " unitigs and " + std::to_string(plan->bridge_of.size()) +
                                 " bridge unitigs: more than a signed unitig number can name");
    if (plan->records.size() >= 0xFFFFFFFFULL) throw std::runtime_error("apply bridges: more than 2^32 applied bridges");
}

void apply_empty(ApplyResult* r) {
    *r = ApplyResult();
    r->bridge_seq_off.assign(1, 0);
}

void apply_finish(const ApplyInput& in, const ApplyPlan& plan, ApplyResult* r) {
    r->bridge_of = plan.bridge_of;
    r->applied = (uint32_t)plan.records.size(); r->direct = plan.n_direct;
    if (r->bridge_seq_off.empty()) r->bridge_seq_off.assign(plan.bridge_of.size() + 1, 0);
    if (!in.seq_bytes) return;
    const uint32_t n = in.n_unitigs;
    r->seq_all.resize(in.seq_total + r->bridge_seq.size() + 1);      // (+ 1: never an empty array behind a pointer)
    if (in.seq_total) memcpy(r->seq_all.data(), in.seq_bytes, in.seq_total);
    if (!r->bridge_seq.empty()) memcpy(r->seq_all.data() + in.seq_total, r->bridge_seq.data(), r->bridge_seq.size());
    r->seq_begin_all.resize(r->n_total);
    for (uint32_t u = 0; u < n; u++) r->seq_begin_all[u] = in.seq_begin[u];
    for (size_t q = 0; q < plan.bridge_of.size(); q++) r->seq_begin_all[n + q] = in.seq_total + r->bridge_seq_off[q];
}

std::string apply_gfa_string(const ApplyResult& r, uint32_t k, bool use_other_colour) {
    std::vector<GfaSegmentView> segs;
    for (uint32_t u = 0; u < r.n_total; u++) {
        if (!r.alive[u]) continue;
        if (r.len[u] && r.seq_all.empty()) throw std::runtime_error("apply bridges: missing sequences: the edit was made without seq_bytes and seq_begin");
        segs.push_back(GfaSegmentView{u + 1, r.seq_all.empty() ? "" : (const char*)r.seq_all.data() + r.seq_begin_all[u], r.len[u], r.depth[u], r.type[u]});
    }
    return gfa_string_explicit(k, segs, r.links.data(), r.links.size(), std::vector<GfaPathView>(), use_other_colour);
}

}  // namespace ac
