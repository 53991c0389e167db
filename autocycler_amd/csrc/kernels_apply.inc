// apply_bridges with what follows it — reduce_depths, delete_unitigs_not_connected_to_anchor, remove_zero_depth_unitigs (resolve.rs:223-282
// over unitig_graph.rs:795-893, 547-592) — as an edit ON THE DEVICE: part of graph_extras.hip (included inside namespace ac; not a translation
// unit of its own).  The host side (apply_host.cpp) checks the bridge records, numbers the bridge unitigs and lays the work items out.
//
// The reference's loop is sequential: per bridge that is not skipped, in Bridge::cmp order, delete_outgoing_links(start),
// delete_incoming_links(end), then create_link(start, end) (empty best path) or a new unitig B = max number + 1 with create_link(start, B),
// create_link(B, end) and reduce_depths.  Call the bridges the loop does not skip the APPLIED bridges, and
//   S_out = {start_i} u {-end_i},  S_in = {end_i} u {-start_i}      (signed numbers; a node as in kernels_merge.inc: merge_node)
// The order-free form that runs here holds where no two applied bridges share a value of S_out and no two share a value of S_in — what
// determine_ambiguity (:193-220) says of the bridges it leaves unflagged: it counts start and -end in one table, end and -start in the other,
// and flags every bridge whose value was counted twice — and where the link entries among alive unitigs are a duplicate-free set closed under
// reverse complement (the merge plan's requirement, checked by its own functor).  Both are checked, not assumed.  Then:
//   deletions   delete_outgoing_links(s) removes every entry (s, x) and, through delete_link's second half (:821-824), its mirror (-x, -s);
//               delete_incoming_links(e) every (p, e) and (-e, -p).  Over all applied bridges an input entry (a, b) is deleted iff a = s or
//               b = -s or b = e or a = -e for some bridge: iff a is in S_out or b is in S_in.  delete_link_one_way (:826-865) removes by value
//               from two lists and leaves the order of what stays alone, so the survivors keep their relative order inside every list.
//   creations   create_link (:867-872) pushes (x, y) and, unless x = -y, (-y, -x); create_link_one_way (:874-893) pushes at the END of x's next
//               list and y's prev list.  The next lists pushed to are those of s, -e, B and -B.  B's are new.  s's next list was emptied by
//               this bridge's delete_outgoing_links; -e's by its delete_incoming_links (the mirrors).  Could a LATER bridge j delete a created
//               entry?  It deletes entries whose source is in {s_j, -e_j} or whose target is in {e_j, -s_j}.  The created entries have sources
//               s, -e (and B, -B: no anchor) and targets e, -s (and B, -B).  s or -e in {s_j, -e_j} is a shared value of S_out, e or -s in
//               {e_j, -s_j} one of S_in: excluded.  Could an EARLIER-created entry be a duplicate of a survivor?  A survivor has its source
//               outside S_out, a created entry from an anchor has its source inside.  So every list is pushed to only after it was emptied, no
//               created entry is deleted, and the edited entries are: the survivors in input order, then the created ones.  One bridge alone
//               may push twice to one list: start = -end with a best path pushes B and then -B to start's next list; the created entries are
//               written in an order that keeps this (below), and with an empty best path the second push is the one create_link leaves out.
//   numbers     max_unitig_number() + 1 at the i-th applied bridge with a best path is n_unitigs + 1 + i when the highest number is alive (the
//               library numbers from n_unitigs + 1 always, as the merge plan does for its chains).
//   depths      reduce_depths (:261-270) runs for applied bridges with a best path only, over all_paths (copies included): c[u] visits, each
//               reduce_depth_by_one (unitig.rs:269-274): d -= 1.0; if d < 0.0 { d = 0.0 }.  Closed form: apply_reduced_depth below.
//   removal     connected_components() runs on the edited lists over the unitigs in the graph then — alive at entry plus the bridge unitigs,
//               zero depth or not; components without an Anchor die; then retain(depth > 0.0) (a NaN dies); then delete_dangling_links.
//
// The L-line order.  get_links_for_gfa (:333-350) walks graph.unitigs — the alive originals ascending, then the bridge unitigs in creation
// order — and per unitig its forward_next, then its reverse_next.  The created entries are written per bridge as
//   start -> B,  B -> end,  -B -> -start,  -end -> -B
// so that among the entries whose source is a bridge unitig the order is already the final one (B's forward list, B's reverse list, bridge
// after bridge), and start -> B stays before start -> -B where start = -end.  A stable radix sort by min(source node, 2 n_unitigs) then puts
// the original sources in place and keeps the bridge sources behind them: its key width does not grow with the number of bridges.
//
// Stages.  Phase A, stream 0, nothing read by the host in between:
//   marks       per applied bridge: atomic-min of its index onto out_mark[start], out_mark[-end], in_mark[end], in_mark[-start]
//   check       per applied bridge: a mark that holds a lower index is the "applied bridges conflict" error: the smallest such pair
//   visits      per entry of the applied bridges' distinct paths (a binary search finds its path): range / alive check, atomic add of the
//               path's multiplicity onto c[unitig]
//   depths      per unitig: apply_reduced_depth
//   members     per entry of the applied best paths: range / alive check, the member list and the member lengths; scan -> member offsets
//   bridges     per bridge unitig: where its bytes begin; the total
//   flags       per input entry: range check, alive filter, the merge plan's key, survives = a not in S_out and b not in S_in
//   radix sort  the keys; MergeLinkCheckFunctor (kernels_merge.inc): duplicates and missing mirror images
//   scan        the flags; compact: the survivors in input order; create: the created entries behind them
//   (header read-back: errors, survivors, bases)
//   copy        MergeCopyFunctor (kernels_merge.inc) as it stands: members = the applied best paths, member offsets = the scan above
// components_device (kernels_components.inc) on the edited entries, marked = the anchors; it takes host arrays, so the edited entries cross
// once, and starts its own arena session.  Phase B, a new session:
//   alive       per unitig: in the graph, its component holds an anchor, depth > 0; the two removal counts by ballot; the types
//   keys        per edited entry: both ends alive -> min(source node, 2 n), else dropped; stable radix sort; gather
//   (header read-back: links out, removal counts)
// No launch count depends on the number of bridges, the length of a path or a bridge, or the number of components.
static const u32 APPLY_NONE = 0xFFFFFFFFu;
enum { APPLY_BAD_DUPLICATE = 0, APPLY_BAD_UNCLOSED = 1, APPLY_BAD_LINK = 2, APPLY_BAD_BEST = 3, APPLY_BAD_VISIT = 4, APPLY_BAD_CONFLICT = 5, APPLY_BAD_WORDS = 6 };
struct ApplyCounts { u64 n_survive, n_bases, n_links_out, removed_no_anchor, removed_zero_depth, alive_after, reserved[2]; };      // zeroed

// c visits of reduce_depth_by_one on d, bit for bit.  Let step(d) = (d - 1.0 < 0.0) ? 0.0 : d - 1.0 in f64.
//   NaN         d - 1.0 is NaN, NaN < 0.0 is false: NaN stays.  Below: NaN >= 2^53 is false, r is NaN, r < 0.0 is false: NaN.
//   +inf        inf - 1.0 = inf: a fixed point, found by the first round of the loop.  -inf and every d < 1.0 (negative, -0.0, 0.5): the first
//               step gives a negative number (the difference of two numbers on a common grid is no 0 unless they are equal) or, for
//               d = 1.0 ... no: d < 1.0 gives d - 1.0 < 0 -> 0.0, and 0.0 stays 0.0 (0.0 - 1.0 = -1.0 -> 0.0).  Below: d - c with c >= 1 is
//               negative for d < 1.0 (same argument), so 0.0.
//   0 <= d < 2^53   ulp(d) <= 1, so every integer is a multiple of ulp(d) and d - 1.0 is a multiple of ulp(d) of smaller magnitude:
//               representable, the subtraction is exact.  By induction the value after j <= d steps is the real number d - j, and the first
//               step that leaves it negative clamps to 0.0, where it stays.  d - (double)c: for c <= d the real d - c is a multiple of ulp(d)
//               below d, representable, so the one rounded subtraction is exact too and equal; for c > d the real difference is a nonzero
//               negative multiple of a power of two that is at least the smallest subnormal, which rounds to a negative number: 0.0 both
//               ways.  (c >= 2^53 > d: (double)c may be rounded but stays above d.)
//   d >= 2^53, finite   ulp(d) >= 2.  2^53 - 1.0 is exact and falls into the case above.  For 2^53 < d < 2^54, d - 1.0 lies halfway between
//               d - 2 and d and goes to the one with the even mantissa: an odd d / 2 drops by 2 once and is even then; an even one stays.
//               For d >= 2^54 the difference rounds back to d.  So at most two steps change d before it is either a fixed point or below
//               2^53: the loop runs them literally (four rounds bound it) and the closed form takes over from there.
AC_D double apply_reduced_depth(double d, u64 c) {
    for (int it = 0; it < 4 && c > 0 && d >= 9007199254740992.0; it++) {
        const double r = d - 1.0;
        if (r == d) return d;      // a fixed point: every further visit leaves it
        d = r; c--;
    }
    if (c == 0) return d;
    const double r = d - (double)c;
    return r < 0.0 ? 0.0 : r;
}

// the largest p < n with begin[p] <= i (begin[0] = 0, ascending, begin[n] = the number of items; empty ranges are passed over)
AC_D u64 apply_find_range(const u64* begin, u64 n, u64 i) {
    u64 lo = 0, hi = n;
    for (int it = 0; it < 64 && hi - lo > 1; it++) {
        const u64 mid = lo + (hi - lo) / 2;
        if (begin[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

struct ApplyMarkFunctor {
    const ApplyRecord* rec; u32* out_mark; u32* in_mark;
    AC_D void operator()(u64 j) const {
        const int32_t s = rec[j].start, e = rec[j].end;
        atomic_min32(&out_mark[merge_node(s)], (u32)j); atomic_min32(&out_mark[merge_node(-e)], (u32)j);
        atomic_min32(&in_mark[merge_node(e)], (u32)j); atomic_min32(&in_mark[merge_node(-s)], (u32)j);
    }
};
// every mark holds the lowest index that claimed it: a bridge that finds another one there shares a value of S_out or S_in with it
struct ApplyMarkCheckFunctor {
    const ApplyRecord* rec; const u32* out_mark; const u32* in_mark; u64* first_bad;
    AC_D void operator()(u64 j) const {
        const int32_t s = rec[j].start, e = rec[j].end;
        u32 m = out_mark[merge_node(s)];
        const u32 m1 = out_mark[merge_node(-e)], m2 = in_mark[merge_node(e)], m3 = in_mark[merge_node(-s)];
        m = m1 < m ? m1 : m; m = m2 < m ? m2 : m; m = m3 < m ? m3 : m;
        if (m != (u32)j) atomic_min64(&first_bad[APPLY_BAD_CONFLICT], ((u64)m << 32) | (u64)j);
    }
};

struct ApplyVisitFunctor {
    const u64* vis_begin; const u64* vis_src; const u32* vis_mult; u64 n_vis; const int32_t* entries; u32 n; const u8* alive; u64* visits; u64* first_bad;
    AC_D void operator()(u64 i) const {
        const u64 p = apply_find_range(vis_begin, n_vis, i);
        const u64 at = vis_src[p] + (i - vis_begin[p]);
        const int64_t e = entries[at];
        const int64_t u = e < 0 ? -e : e;
        if (u == 0 || u > (int64_t)n || (alive && !alive[u - 1])) { atomic_min64(&first_bad[APPLY_BAD_VISIT], at); return; }
        atomic_add64(&visits[u - 1], (u64)vis_mult[p]);
    }
};
struct ApplyDepthFunctor {
    const double* depth; const u64* visits; double* out;
    AC_D void operator()(u64 u) const { out[u] = apply_reduced_depth(depth ? depth[u] : 0.0, visits[u]); }
};

// member m of the applied best paths, bridge unitig after bridge unitig; m == n_members: the sentinel behind the last length
struct ApplyMemberFunctor {
    const u64* q_begin; const u64* q_best_off; u64 n_q; u64 n_members; const int32_t* best; u32 n; const u8* alive; const u32* unitig_len;
    int32_t* members; u64* member_len; u64* first_bad;
    AC_D void operator()(u64 m) const {
        if (m == n_members) { member_len[m] = 0; return; }
        const u64 q = apply_find_range(q_begin, n_q, m);
        const u64 at = q_best_off[q] + (m - q_begin[q]);
        const int64_t e = best[at];
        const int64_t u = e < 0 ? -e : e;
        members[m] = (int32_t)e; member_len[m] = 0;
        if (u == 0 || u > (int64_t)n || (alive && !alive[u - 1])) { atomic_min64(&first_bad[APPLY_BAD_BEST], at); return; }
        member_len[m] = unitig_len[u - 1];
    }
};
// bridge unitig q: the first byte of its sequence; q == n_q: the total
struct ApplyBridgeOffFunctor {
    const u64* q_begin; const u64* member_seq_off; u64 n_q; u64* bridge_seq_off; ApplyCounts* counts;
    AC_D void operator()(u64 q) const {
        bridge_seq_off[q] = member_seq_off[q_begin[q]];
        if (q == n_q) counts->n_bases = bridge_seq_off[q];
    }
};

struct ApplyFlagFunctor {
    const Link* links; u32 n; const u8* alive; const u32* out_mark; const u32* in_mark; int key_bits; u32* flag; u64* key; u32* key_index; u64* first_bad;
    AC_D void operator()(u64 i) const {
        key[i] = link_key_dropped(key_bits); key_index[i] = (u32)i; flag[i] = 0;
        LinkEnds e;
        const int ends = link_ends(links[i], n, alive, &e);
        if (ends == LINK_NO_UNITIG) { atomic_min64(&first_bad[APPLY_BAD_LINK], i); return; }
        if (ends == LINK_DEAD) return;
        key[i] = merge_key(links[i].a, links[i].b, n, key_bits);
        flag[i] = out_mark[merge_node(links[i].a)] == APPLY_NONE && in_mark[merge_node(links[i].b)] == APPLY_NONE ? 1u : 0u;
    }
};
struct ApplyCompactFunctor {
    const Link* links; const u32* flag; const u32* pos; u64 n_links; Link* out; ApplyCounts* counts;
    AC_D void operator()(u64 i) const {
        if (flag[i]) out[pos[i]] = links[i];
        if (i + 1 == n_links) counts->n_survive = (u64)pos[i] + flag[i];
    }
};
struct ApplyCreateFunctor {
    const ApplyRecord* rec; const ApplyCounts* counts; u32 n; Link* out;
    AC_D void operator()(u64 j) const {
        const int32_t s = rec[j].start, e = rec[j].end;
        Link* o = out + counts->n_survive + rec[j].created_off;
        if (rec[j].unitig != APPLY_NONE) {
            const int32_t b = (int32_t)(n + 1u + rec[j].unitig);
            o[0] = Link{s, b}; o[1] = Link{b, e}; o[2] = Link{-b, -s}; o[3] = Link{-e, -b};
        } else {
            o[0] = Link{s, e};
            if (s != -e) o[1] = Link{-e, -s};
        }
    }
};

// ---- phase B ----
struct ApplyAliveFunctor {
    u32 n, n_total; const u8* alive_in; const u32* component_of; const u8* comp_anchor; const double* depth; const u8* marked;
    u8* alive_out; u8* type_out; ApplyCounts* counts;
    AC_D void operator()(u64 u, bool valid) const {
        bool no_anchor = false, zero = false, stays = false;
        if (valid) {
            const bool in = u >= n || !alive_in || alive_in[u];
            const u32 c = component_of[u];
            no_anchor = in && (c == COMP_DEAD || !comp_anchor[c]);
            zero = in && !no_anchor && !(depth[u] > 0.0);
            stays = in && !no_anchor && !zero;
            alive_out[u] = stays ? 1 : 0;
            type_out[u] = u >= n ? (u8)MERGE_TYPE_BRIDGE : (marked && marked[u]) ? (u8)MERGE_TYPE_ANCHOR : (u8)MERGE_TYPE_OTHER;
        }
        const u64 b0 = wv::ballot(no_anchor), b1 = wv::ballot(zero), b2 = wv::ballot(stays);
        if (wv::lane() == 0) {
            if (b0) atomic_add64(&counts->removed_no_anchor, (u64)prim_popc64(b0));
            if (b1) atomic_add64(&counts->removed_zero_depth, (u64)prim_popc64(b1));
            if (b2) atomic_add64(&counts->alive_after, (u64)prim_popc64(b2));
        }
    }
};
struct ApplyLinkKeyFunctor {
    const Link* links; u32 n; const u8* alive; u64 dropped; u64* key; u32* val;
    AC_D void operator()(u64 i) const {
        const u32 ua = links[i].na() - 1, ub = links[i].nb() - 1;      // (the edited entries name unitigs of [1, n_total]: range-checked survivors and what create wrote)
        const u64 node = merge_node(links[i].a);
        key[i] = alive[ua] && alive[ub] ? (node < 2ULL * n ? node : 2ULL * n) : dropped;
        val[i] = (u32)i;
    }
};
struct ApplyGatherFunctor {
    const u64* key; const u32* val; u64 n_links; u64 dropped; const Link* links; Link* out; ApplyCounts* counts;
    AC_D void operator()(u64 j) const {
        if (key[j] == dropped) return;
        out[j] = links[val[j]];
        if (j + 1 == n_links || key[j + 1] == dropped) counts->n_links_out = j + 1;
    }
};

void apply_bridges_device(const ApplyInput& in, const ApplyPlan& plan, ApplyResult* out) {
    const u32 n = in.n_unitigs;
    const u64 nl = in.n_links;
    const u64 na = plan.records.size(), nq = plan.bridge_of.size(), nm = plan.n_members, nv = plan.vis_src.size(), n_items = plan.n_visits;
    const u32 n_total = n + (u32)nq;      // (apply_prepare has refused a sum above what a signed number can name)
    if (nl >= 0xFFFFFFF0ULL - plan.n_created) throw DeviceError("apply bridges: more than 2^32 links");
    const bool with_seq = in.seq_bytes != nullptr;
    StepMeter meter;
    double seconds_device = 0;
    out->n_unitigs = n; out->n_total = n_total; out->links_in = nl;

    // ---- phase A ----
    Arena& arena = Arena::device();
    arena.reset();
    const int key_bits = bit_width(2 * (u64)n);
    const u64 nodes = 2 * (u64)n, ne_max = nl + plan.n_created;
    DBuf<Link> d_links(nl), d_edit(ne_max);
    DBuf<u32> d_len(n), d_out_mark(nodes), d_in_mark(nodes), d_flag(nl), d_pos(nl), d_key_index(nl), d_vis_mult(nv);
    DBuf<u8> d_alive(in.alive ? n : 0);
    DBuf<double> d_depth(in.depth ? n : 0), d_depth_out(n);
    DBuf<ApplyRecord> d_rec(na);
    DBuf<u64> d_vis_begin(nv + 1), d_vis_src(nv), d_visits(n), d_q_begin(nq + 1), d_q_best_off(nq), d_member_len(nm + 1), d_member_seq_off(nm + 1), d_bridge_seq_off(nq + 1);
    DBuf<u64> d_key(nl), d_first_bad(APPLY_BAD_WORDS);
    DBuf<int32_t> d_entries(nv ? in.n_dist_entries : 0), d_best(nq ? in.n_best : 0), d_members(nm);
    DBuf<ApplyCounts> d_counts(1);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    copy_h2d(d_len.ptr(), in.unitig_len, (u64)n * 4);
    if (in.alive) copy_h2d(d_alive.ptr(), in.alive, n);
    if (in.depth) copy_h2d(d_depth.ptr(), in.depth, (u64)n * 8);
    copy_h2d(d_rec.ptr(), plan.records.data(), na * sizeof(ApplyRecord));
    copy_h2d(d_vis_begin.ptr(), plan.vis_begin.data(), (nv + 1) * 8);
    copy_h2d(d_vis_src.ptr(), plan.vis_src.data(), nv * 8);
    copy_h2d(d_vis_mult.ptr(), plan.vis_mult.data(), nv * 4);
    copy_h2d(d_q_begin.ptr(), plan.q_begin.data(), (nq + 1) * 8);
    copy_h2d(d_q_best_off.ptr(), plan.q_best_off.data(), nq * 8);
    if (nv) copy_h2d(d_entries.ptr(), in.dist_entries, in.n_dist_entries * 4);
    if (nq) copy_h2d(d_best.ptr(), in.best, in.n_best * 4);
    const u8* p_alive = in.alive ? d_alive.ptr() : nullptr;
    d_out_mark.fill_bytes(0xFF); d_in_mark.fill_bytes(0xFF); d_visits.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_counts.fill_bytes(0);
    d_member_seq_off.fill_bytes(0); d_bridge_seq_off.fill_bytes(0);
    RadixScratch sort_links;
    sort_links.prepare(nl, 2 * key_bits);

    meter.begin();
    launch(na, ApplyMarkFunctor{d_rec.ptr(), d_out_mark.ptr(), d_in_mark.ptr()});
    launch(na, ApplyMarkCheckFunctor{d_rec.ptr(), d_out_mark.ptr(), d_in_mark.ptr(), d_first_bad.ptr()});
    launch(n_items, ApplyVisitFunctor{d_vis_begin.ptr(), d_vis_src.ptr(), d_vis_mult.ptr(), nv, d_entries.ptr(), n, p_alive, d_visits.ptr(), d_first_bad.ptr()});
    launch(n, ApplyDepthFunctor{in.depth ? d_depth.ptr() : nullptr, d_visits.ptr(), d_depth_out.ptr()});
    if (nq) {
        launch(nm + 1, ApplyMemberFunctor{d_q_begin.ptr(), d_q_best_off.ptr(), nq, nm, d_best.ptr(), n, p_alive, d_len.ptr(), d_members.ptr(), d_member_len.ptr(),
                                          d_first_bad.ptr()});
        exclusive_scan_u64(d_member_len.ptr(), d_member_seq_off.ptr(), nm + 1);
        launch(nq + 1, ApplyBridgeOffFunctor{d_q_begin.ptr(), d_member_seq_off.ptr(), nq, d_bridge_seq_off.ptr(), d_counts.ptr()});
    }
    if (nl) {
        launch(nl, ApplyFlagFunctor{d_links.ptr(), n, p_alive, d_out_mark.ptr(), d_in_mark.ptr(), key_bits, d_flag.ptr(), d_key.ptr(), d_key_index.ptr(), d_first_bad.ptr()});
        sort_pairs_u64_u32(d_key, d_key_index, nl, 2 * key_bits, 0, 0, &sort_links);
        launch(nl, MergeLinkCheckFunctor{d_key.ptr(), d_key_index.ptr(), nl, n, key_bits, d_first_bad.ptr()});
        exclusive_scan_u32(d_flag.ptr(), d_pos.ptr(), nl);
        launch(nl, ApplyCompactFunctor{d_links.ptr(), d_flag.ptr(), d_pos.ptr(), nl, d_edit.ptr(), d_counts.ptr()});
    }
    launch(na, ApplyCreateFunctor{d_rec.ptr(), d_counts.ptr(), n, d_edit.ptr()});
    meter.end();
    ApplyCounts h; u64 first_bad[APPLY_BAD_WORDS];
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad);
        rb.run();
    }
    if (first_bad[APPLY_BAD_LINK] < nl) {
        const u64 i = first_bad[APPLY_BAD_LINK];
        throw DeviceError(components_bad_link_message(i, in.links[i].a, in.links[i].b, n));
    }
    if (first_bad[APPLY_BAD_DUPLICATE] < nl) throw DeviceError(merge_duplicate_link_message(first_bad[0], in.links[first_bad[0]].a, in.links[first_bad[0]].b));
    if (first_bad[APPLY_BAD_UNCLOSED] < nl) throw DeviceError(merge_unclosed_link_message(first_bad[1], in.links[first_bad[1]].a, in.links[first_bad[1]].b));
    if (first_bad[APPLY_BAD_CONFLICT] != ~0ULL) {
        const u64 a = first_bad[APPLY_BAD_CONFLICT] >> 32, b = first_bad[APPLY_BAD_CONFLICT] & 0xFFFFFFFFULL;
        if (a >= na || b >= na) throw DeviceError("apply bridges: the device returned an impossible header (internal error)");
        throw DeviceError(apply_conflict_message(plan.records[a].bridge, plan.records[a].start, plan.records[a].end, plan.records[b].bridge, plan.records[b].start,
                                                 plan.records[b].end));
    }
    if (first_bad[APPLY_BAD_BEST] != ~0ULL) {
        const u64 at = first_bad[APPLY_BAD_BEST];
        if (at >= in.n_best) throw DeviceError("apply bridges: the device returned an impossible header (internal error)");
        throw DeviceError(apply_bad_entry_message(plan, in, true, at));
    }
    if (first_bad[APPLY_BAD_VISIT] != ~0ULL) {
        const u64 at = first_bad[APPLY_BAD_VISIT];
        if (at >= in.n_dist_entries) throw DeviceError("apply bridges: the device returned an impossible header (internal error)");
        throw DeviceError(apply_bad_entry_message(plan, in, false, at));
    }
    if (h.n_survive > nl) throw DeviceError("apply bridges: the device returned an impossible header (internal error)");
    const u64 ne = h.n_survive + plan.n_created, n_bases = h.n_bases;
    out->bridge_seq_off.assign(nq + 1, 0);
    if (with_seq && n_bases) {
        DBuf<u8> d_seq(in.seq_total), d_out(n_bases);
        DBuf<u64> d_seq_begin(n);
        copy_h2d(d_seq.ptr(), in.seq_bytes, in.seq_total);
        copy_h2d(d_seq_begin.ptr(), in.seq_begin, (u64)n * 8);
        meter.begin();      // the copy kernel alone: seconds_copy
        launch_full((n_bases + MERGE_COPY_WAVE_BYTES - 1) / MERGE_COPY_WAVE_BYTES * 64,
                    MergeCopyFunctor{d_member_seq_off.ptr(), d_members.ptr(), nm, n_bases, d_seq.ptr(), d_seq_begin.ptr(), d_len.ptr(), d_out.ptr()});
        meter.end();
        out->bridge_seq.resize(n_bases);
        copy_d2h_async(out->bridge_seq.data(), d_out.ptr(), n_bases);
    }
    std::vector<Link> edited((size_t)ne);
    std::vector<double> depth_total(n_total, in.bridge_depth);
    copy_d2h_async(edited.data(), d_edit.ptr(), ne * sizeof(Link));
    copy_d2h_async(depth_total.data(), d_depth_out.ptr(), (u64)n * 8);
    if (nq) copy_d2h_async(out->bridge_seq_off.data(), d_bridge_seq_off.ptr(), (nq + 1) * 8);
    meter.sync_copies();
    out->seconds_copy = meter.seconds(1);
    seconds_device += meter.take();
    out->bases_copied = out->bridge_seq.size();

    // the per-unitig arrays over 1 .. n_total
    out->len.assign(n_total, 0);
    for (u32 u = 0; u < n; u++) out->len[u] = in.unitig_len[u];
    for (u64 q = 0; q < nq; q++) {
        const u64 bytes = out->bridge_seq_off[q + 1] - out->bridge_seq_off[q];
        if (out->bridge_seq_off[q + 1] < out->bridge_seq_off[q] || bytes > 0xFFFFFFFFULL)
            throw DeviceError(apply_long_bridge_message(plan.bridge_of[q], bytes));
        out->len[n + q] = (u32)bytes;
    }
    std::vector<u8> in_graph(n_total, 1), marked(n_total, 0);
    if (in.alive) for (u32 u = 0; u < n; u++) in_graph[u] = in.alive[u] ? 1 : 0;
    for (u32 i = 0; i < in.n_anchors; i++) marked[in.anchors[i] - 1] = 1;

    // ---- the components of the edited graph, before any zero-depth removal ----
    ComponentsResult comp;
    components_device(n_total, edited.data(), ne, out->len.data(), in_graph.data(), marked.data(), &comp);
    out->stats_components = comp.stats;
    std::vector<u8> comp_anchor(comp.records.size() + 1, 0);
    for (size_t c = 0; c < comp.records.size(); c++) comp_anchor[c] = comp.records[c].marked ? 1 : 0;

    // ---- phase B ----
    arena.reset();
    {
        const u64 dropped = 2 * (u64)n + 1;
        const int bits_b = bit_width(dropped);
        DBuf<Link> d_edit_b(ne), d_out_links(ne);
        DBuf<u32> d_component_of(n_total), d_val(ne);
        DBuf<u8> d_in(n_total), d_comp_anchor(comp_anchor.size()), d_marked(n_total), d_alive_out(n_total), d_type(n_total);
        DBuf<double> d_depth_b(n_total);
        DBuf<u64> d_key_b(ne);
        DBuf<ApplyCounts> d_counts_b(1);
        copy_h2d(d_edit_b.ptr(), edited.data(), ne * sizeof(Link));
        copy_h2d(d_component_of.ptr(), comp.component_of.data(), (u64)n_total * 4);
        copy_h2d(d_in.ptr(), in_graph.data(), n_total);
        copy_h2d(d_comp_anchor.ptr(), comp_anchor.data(), comp_anchor.size());
        copy_h2d(d_marked.ptr(), marked.data(), n_total);
        copy_h2d(d_depth_b.ptr(), depth_total.data(), (u64)n_total * 8);
        d_counts_b.fill_bytes(0);
        RadixScratch sort_b;
        sort_b.prepare(ne, bits_b);
        meter.begin();
        launch_full(n_total, ApplyAliveFunctor{n, n_total, d_in.ptr(), d_component_of.ptr(), d_comp_anchor.ptr(), d_depth_b.ptr(), d_marked.ptr(), d_alive_out.ptr(),
                                               d_type.ptr(), d_counts_b.ptr()});
        if (ne) {
            launch(ne, ApplyLinkKeyFunctor{d_edit_b.ptr(), n, d_alive_out.ptr(), dropped, d_key_b.ptr(), d_val.ptr()});
            sort_pairs_u64_u32(d_key_b, d_val, ne, bits_b, 0, 0, &sort_b);
            launch(ne, ApplyGatherFunctor{d_key_b.ptr(), d_val.ptr(), ne, dropped, d_edit_b.ptr(), d_out_links.ptr(), d_counts_b.ptr()});
        }
        meter.end();
        ApplyCounts hb;
        {
            ReadBatch rb;
            rb.add(&hb, d_counts_b.ptr(), sizeof hb);
            rb.run();
        }
        if (hb.n_links_out > ne || hb.alive_after + hb.removed_no_anchor + hb.removed_zero_depth > n_total)
            throw DeviceError("apply bridges: the device returned an impossible header (internal error)");
        out->links.resize((size_t)hb.n_links_out); out->alive.resize(n_total); out->type.resize(n_total);
        copy_d2h_async(out->links.data(), d_out_links.ptr(), hb.n_links_out * sizeof(Link));
        copy_d2h_async(out->alive.data(), d_alive_out.ptr(), n_total);
        copy_d2h_async(out->type.data(), d_type.ptr(), n_total);
        meter.sync_copies();
        seconds_device += meter.take();
        out->removed_no_anchor = hb.removed_no_anchor; out->removed_zero_depth = hb.removed_zero_depth; out->alive_after = hb.alive_after;
    }
    out->depth = std::move(depth_total);
    out->stats = meter.stats();
    out->stats.seconds_device = seconds_device + comp.stats.seconds_device;
}
