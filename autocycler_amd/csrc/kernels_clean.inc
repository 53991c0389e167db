// `autocycler clean` (clean.rs:23-45): remove_unitigs_by_number, duplicate_unitig_by_number and remove_low_depth_unitigs
// (unitig_graph.rs:588-721) as an edit ON THE DEVICE: part of graph_extras.hip (included inside namespace ac; not a translation unit of its
// own).  The host side (clean_host.cpp) checks the number lists and runs the literal duplication over the few links the device gathers for it.
//
// Lists as one array.  A unitig strand's next list is the entries that leave it, in input order (L-line order: checked), then what create_link
// pushed, in time order; deletions keep the order of what stays.  So "the survivors in input order, then the created entries in creation order",
// stably sorted by source node over the n_out = n + 2 * duplications unitigs, is every next list in its order and get_links_for_gfa's walk at
// once: the originals ascending, then the copies a, b of one duplication after the other, forward_next before reverse_next.  The prev lists
// hold the same entries; only their membership is ever read (below), never their order.
//
// Removal.  alive1 = alive at entry and not named by remove; an entry with a dead end is gone (delete_dangling_links).
// Duplication.  Every entry duplicate_unitig_by_number deletes or creates touches a duplicated unitig or a copy.  The entries among alive1
// unitigs split into those without an end in the duplicate set — survivors, whatever the loop does — and the rest, which are compacted in
// input order and handed to clean_duplicate_edit; what it created comes back behind the survivors.  Every duplicated original dies.
// Low depth.  The reference walks `unitigs` from the last to the first — descending index here, the copies first, b before a — and decides
// each unitig whose depth is not above min_depth against the graph as the earlier deletions left it: u goes iff every neighbour it leads to,
// and every neighbour that leads to it, keeps an entry on that side whose number is not u (:685-715).  With the link multiset closed under
// reverse complement the entering list of a node t is the mirror image of the next list of -t, and forward_prev of u that of u's reverse_next:
//   u goes iff for x in {u+, u-}, for every t in next(x) with |t| != u (alive): next(-t) holds an alive w with |w| != u.
// That reads the next lists of u and of its neighbours, i.e. the alive flags of unitigs within distance two.  Round form: every undecided
// candidate writes (round, index) with an atomic max into a slot per member of its closed neighbourhood N[u] (taken over the edited links,
// dead neighbours included: a superset only delays); u is READY iff all slots of N[u] hold u.  Two candidates within distance two share a
// slot, which holds the larger: a ready u has no undecided candidate of larger index within distance two — all that the walk decided before u
// and that u's decision reads are decided — and none of smaller index within distance two is ready in the same round.  So the ready
// candidates of a round are pairwise further than two apart, none reads a flag another writes, and each sees what the walk would show it: they
// are decided in one launch, in place.  The largest undecided index is always ready: every round decides at least one.  A chain of n candidates
// takes n rounds; the slots carry the round, so nothing is reset.  Cost per round: the degrees of the undecided candidates (marks), plus for the
// ready ones their neighbours' lists up to the first witness.
//
// Stages, stream 0.  Phase A: marks (remove and duplicate, one launch) · unitigs (alive1) · links (range, L-line order, the merge plan's key, survivor /
// gathered flags) · radix sort + MergeLinkCheckFunctor · two scans · compact · (read-back: errors, counts) · (the gathered entries to the host).
// Phase B: created entries up · unitigs (all per-unitig outputs, candidate flags) · scan · candidates into work list 0 · source-node keys ·
// radix sort · gather · node offsets · (read-back: candidates).  Rounds in batches of CLEAN_ROUNDS_PER_BATCH: batch init · per round mark,
// decide (the undecided into the other work list, one atomic per wavefront) · (read-back per batch: what is left, rounds used); the launches of
// a batch are sized by what was left before it, and a round that finds its list empty exits at once.  Then: alive-link flags · scan · compact ·
// (read-back: links out) · the arrays to the host.  No launch count follows the unitigs, links, candidates, removals or duplications.
enum { CLEAN_BAD_DUPLICATE = 0, CLEAN_BAD_UNCLOSED = 1, CLEAN_BAD_LINK = 2, CLEAN_BAD_ORDER = 3, CLEAN_BAD_WORDS = 4 };
struct CleanCounts { u64 n_survive, n_gathered, n_candidates, n_links_out, left, rounds, reserved[2]; };      // zeroed

// one item per number of remove, then of duplicate, and one that does nothing: the launch is there whatever the lists hold.  Bytes, not
// bits: a number may stand in both lists, and two items never modify one byte (clean_prepare: 1 <= number <= n; a number listed twice stores
// the same byte twice)
struct CleanMarkFunctor {
    const u32* remove; u32 n_remove; const u32* duplicate; u32 n_duplicate; u8* mark_remove; u8* mark_duplicate;
    AC_D void operator()(u64 i) const {
        if (i < n_remove) mark_remove[remove[i] - 1] = 1;
        else if (i < (u64)n_remove + n_duplicate) mark_duplicate[duplicate[i - n_remove] - 1] = 1;
    }
};
struct CleanAlive1Functor {
    const u8* alive_in; const u8* mark_remove; u8* alive1;
    AC_D void operator()(u64 u) const { alive1[u] = (!alive_in || alive_in[u]) && !mark_remove[u] ? 1 : 0; }
};
struct CleanLinkFlagFunctor {
    const Link* links; u32 n; const u8* alive_in; const u8* alive1; const u8* mark_duplicate; int key_bits;
    u32* flag_survive; u32* flag_gather; u64* key; u32* key_index; u64* first_bad;
    AC_D void operator()(u64 i) const {
        key[i] = link_key_dropped(key_bits); key_index[i] = (u32)i; flag_survive[i] = 0; flag_gather[i] = 0;
        LinkEnds e;
        const int ends = link_ends(links[i], n, alive_in, &e);
        if (ends == LINK_NO_UNITIG) { atomic_min64(&first_bad[CLEAN_BAD_LINK], i); return; }
        if (i > 0) {
            const Link p = links[i - 1];
            if (p.a != 0 && p.na() <= n && merge_node(p.a) > merge_node(links[i].a)) atomic_min64(&first_bad[CLEAN_BAD_ORDER], i);
        }
        if (ends == LINK_DEAD) return;
        key[i] = merge_key(links[i].a, links[i].b, n, key_bits);
        if (!alive1[e.ua] || !alive1[e.ub]) return;
        const bool touches = (mark_duplicate[e.ua] | mark_duplicate[e.ub]) != 0;
        flag_survive[i] = touches ? 0u : 1u; flag_gather[i] = touches ? 1u : 0u;
    }
};
struct CleanCompactFunctor {
    const Link* links; const u32* flag_survive; const u32* pos_survive; const u32* flag_gather; const u32* pos_gather; u64 n_links;
    Link* survive; Link* gathered; CleanCounts* counts;
    AC_D void operator()(u64 i) const {
        if (flag_survive[i]) survive[pos_survive[i]] = links[i];
        if (flag_gather[i]) gathered[pos_gather[i]] = links[i];
        if (i + 1 == n_links) { counts->n_survive = (u64)pos_survive[i] + flag_survive[i]; counts->n_gathered = (u64)pos_gather[i] + flag_gather[i]; }
    }
};

// ---- phase B ----
// every per-unitig output over 1 .. n_out; copies a, b of duplicate[i] are unitigs n + 1 + 2 i and n + 2 + 2 i
struct CleanUnitigFunctor {
    u32 n; const u32* duplicate; const u8* alive_in; const u8* mark_remove; const u8* mark_duplicate; const u32* len_in; const double* depth_in; const u8* type_in; const u64* seq_begin_in;
    int has_min; double min_depth;
    u8* alive; u8* reason; u32* len; double* depth; u8* type; u64* seq_begin; u32* copy_of; u32* candidate;
    AC_D void operator()(u64 u) const {
        const u32 src = u < n ? (u32)u : duplicate[(u - n) / 2] - 1u;
        const double d = depth_in ? depth_in[src] : 0.0;
        u8 code = CLEAN_KEPT;
        if (u < n) {
            if (alive_in && !alive_in[u]) code = CLEAN_ABSENT;
            else if (mark_remove[u]) code = CLEAN_REMOVED;
            else if (mark_duplicate[u]) code = CLEAN_DUPLICATED;
        }
        const double d_out = u < n ? d : d / 2.0;
        const bool low = code == CLEAN_KEPT && has_min && !(d_out > min_depth);      // (a NaN on either side is low: unitig_graph.rs:682)
        if (low) code = CLEAN_KEPT_DEAD_END;                                         // until a round decides otherwise
        alive[u] = code == CLEAN_KEPT || code == CLEAN_KEPT_DEAD_END ? 1 : 0;
        reason[u] = code; len[u] = len_in[src]; depth[u] = d_out; type[u] = type_in ? type_in[src] : (u8)MERGE_TYPE_OTHER;
        if (seq_begin) seq_begin[u] = seq_begin_in[src];
        copy_of[u] = u < n ? 0u : src + 1u;
        candidate[u] = low ? 1u : 0u;
    }
};
// the candidates ascending into work list 0; left = their number (the round counters' carry: counter[CLEAN_ROUNDS_PER_BATCH])
struct CleanCandidateFunctor {
    const u32* candidate; const u32* pos; u64 n_out; u32* work; u32* counter; CleanCounts* counts;
    AC_D void operator()(u64 u) const {
        if (candidate[u]) work[pos[u]] = (u32)u;
        if (u + 1 == n_out) { const u32 c = pos[u] + candidate[u]; counter[CLEAN_ROUNDS_PER_BATCH] = c; counts->n_candidates = c; counts->left = c; }
    }
};
struct CleanSourceKeyFunctor {
    const Link* edit; u64* key; u32* val;
    AC_D void operator()(u64 i) const { key[i] = merge_node(edit[i].a); val[i] = (u32)i; }      // (range-checked survivors and what the host created)
};
struct CleanGatherFunctor {
    const Link* edit; const u32* val; Link* sorted;
    AC_D void operator()(u64 j) const { sorted[j] = edit[val[j]]; }
};
// off[x] = the first sorted entry whose source node is at least x, x in [0, 2 n_out]
struct CleanNodeOffsetFunctor {
    const u64* key; u64 n_edit; u32* off;
    AC_D void operator()(u64 x) const {
        u64 lo = 0, hi = n_edit;
        for (int it = 0; it < 64 && lo < hi; it++) {
            const u64 mid = lo + (hi - lo) / 2;
            if (key[mid] < x) lo = mid + 1; else hi = mid;
        }
        off[x] = (u32)lo;
    }
};

// ---- the rounds ----
// counter[r]: the length of the work list round r of the batch reads (list r & 1); counter[CLEAN_ROUNDS_PER_BATCH] carries over to the next batch
struct CleanBatchInitFunctor {
    u32* counter;
    AC_D void operator()(u64) const {
        const u32 c = counter[CLEAN_ROUNDS_PER_BATCH];
        counter[0] = c;
        for (u32 r = 1; r <= CLEAN_ROUNDS_PER_BATCH; r++) counter[r] = 0;
    }
};
AC_D u64 clean_tag(u32 round, u32 u) { return ((u64)(round + 1u) << 32) | (u64)(u + 1u); }
struct CleanRoundMarkFunctor {
    const u32* work; const u32* count; u32 round; const Link* sorted; const u32* off; u64* slot;
    AC_D void operator()(u64 i) const {
        if (i >= *count) return;
        const u32 u = work[i];
        const u64 tag = clean_tag(round, u);
        atomic_max64(&slot[u], tag);
        for (u32 j = off[2 * u]; j < off[2 * u + 2]; j++) atomic_max64(&slot[sorted[j].nb() - 1], tag);
    }
};
struct CleanRoundDecideFunctor {
    const u32* work; const u32* count; u32 round; const Link* sorted; const u32* off; const u64* slot;
    u8* alive; u8* reason; u32* work_next; u32* count_next; CleanCounts* counts;
    AC_D void operator()(u64 i, bool valid) const {
        const u32 c = *count;
        bool undecided = false;
        u32 u = 0;
        if (valid && i < c) {
            u = work[i];
            const u64 tag = clean_tag(round, u);
            const u32 j0 = off[2 * u], j1 = off[2 * u + 2];
            bool ready = slot[u] == tag;
            for (u32 j = j0; ready && j < j1; j++) ready = slot[sorted[j].nb() - 1] == tag;
            if (ready) {
                bool ok = true;
                for (u32 j = j0; ok && j < j1; j++) {
                    const int32_t t = sorted[j].b;
                    const u32 v = sorted[j].nb() - 1;
                    if (v == u || !alive[v]) continue;
                    const u32 m = merge_node(-t);
                    bool has_other = false;
                    for (u32 jj = off[m]; !has_other && jj < off[m + 1]; jj++) {
                        const u32 w = sorted[jj].nb() - 1;
                        has_other = w != u && alive[w];
                    }
                    ok = has_other;
                }
                if (ok) { alive[u] = 0; reason[u] = CLEAN_LOW_DEPTH; }
            } else undecided = true;
            if (i == 0) counts->rounds += 1;      // (one thread of one launch at a time)
        }
        const u32 at = wave_alloc32(count_next, undecided ? 1u : 0u);
        if (undecided) work_next[at] = u;
    }
};
struct CleanLeftFunctor {
    const u32* counter; CleanCounts* counts;
    AC_D void operator()(u64) const { counts->left = counter[CLEAN_ROUNDS_PER_BATCH]; }
};

struct CleanOutFlagFunctor {
    const Link* sorted; const u8* alive; u32* flag;
    AC_D void operator()(u64 j) const { flag[j] = alive[sorted[j].na() - 1] && alive[sorted[j].nb() - 1] ? 1u : 0u; }
};
struct CleanOutCompactFunctor {
    const Link* sorted; const u32* flag; const u32* pos; u64 n_edit; Link* out; CleanCounts* counts;
    AC_D void operator()(u64 j) const {
        if (flag[j]) out[pos[j]] = sorted[j];
        if (j + 1 == n_edit) counts->n_links_out = (u64)pos[j] + flag[j];
    }
};

void clean_device(const CleanInput& in, CleanResult* out) {
    const u32 n = in.n_unitigs, nd = in.n_duplicate;
    const u32 n_out = n + 2 * nd;      // (clean_prepare has refused a sum above what a signed number can name)
    const u64 nl = in.n_links;
    if (nl >= 0xFFFFFFF0ULL - 16ULL * nd) throw DeviceError("clean: more than 2^32 links");
    const bool with_seq = in.seq_bytes != nullptr;
    StepMeter meter;
    double seconds_device = 0;
    out->n_unitigs = n; out->n_out = n_out; out->links_in = nl;

    // ---- phase A ----
    Arena& arena = Arena::device();
    arena.reset();
    const int key_bits = bit_width(2 * (u64)n);
    DBuf<Link> d_links(nl), d_survive(nl), d_gathered(nl);
    DBuf<u32> d_remove(in.n_remove), d_duplicate(nd), d_flag_s(nl), d_flag_g(nl), d_pos_s(nl), d_pos_g(nl), d_key_index(nl);
    DBuf<u8> d_alive_in(in.alive ? n : 0), d_mark_remove(n), d_mark_duplicate(n), d_alive1(n);
    DBuf<u64> d_key(nl), d_first_bad(CLEAN_BAD_WORDS);
    DBuf<CleanCounts> d_counts(1);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    copy_h2d(d_remove.ptr(), in.remove, (u64)in.n_remove * 4);
    copy_h2d(d_duplicate.ptr(), in.duplicate, (u64)nd * 4);
    if (in.alive) copy_h2d(d_alive_in.ptr(), in.alive, n);
    const u8* p_alive_in = in.alive ? d_alive_in.ptr() : nullptr;
    d_mark_remove.fill_bytes(0); d_mark_duplicate.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_counts.fill_bytes(0);
    RadixScratch sort_links;
    sort_links.prepare(nl, 2 * key_bits);

    meter.begin();
    launch((u64)in.n_remove + nd + 1, CleanMarkFunctor{d_remove.ptr(), in.n_remove, d_duplicate.ptr(), nd, d_mark_remove.ptr(), d_mark_duplicate.ptr()});
    launch(n, CleanAlive1Functor{p_alive_in, d_mark_remove.ptr(), d_alive1.ptr()});
    if (nl) {
        launch(nl, CleanLinkFlagFunctor{d_links.ptr(), n, p_alive_in, d_alive1.ptr(), d_mark_duplicate.ptr(), key_bits, d_flag_s.ptr(), d_flag_g.ptr(), d_key.ptr(), d_key_index.ptr(),
                                        d_first_bad.ptr()});
        sort_pairs_u64_u32(d_key, d_key_index, nl, 2 * key_bits, 0, 0, &sort_links);
        launch(nl, MergeLinkCheckFunctor{d_key.ptr(), d_key_index.ptr(), nl, n, key_bits, d_first_bad.ptr()});
        exclusive_scan_u32(d_flag_s.ptr(), d_pos_s.ptr(), nl);
        exclusive_scan_u32(d_flag_g.ptr(), d_pos_g.ptr(), nl);
        launch(nl, CleanCompactFunctor{d_links.ptr(), d_flag_s.ptr(), d_pos_s.ptr(), d_flag_g.ptr(), d_pos_g.ptr(), nl, d_survive.ptr(), d_gathered.ptr(), d_counts.ptr()});
    }
    meter.end();
    CleanCounts h; u64 first_bad[CLEAN_BAD_WORDS];
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad);
        rb.run();
    }
    if (first_bad[CLEAN_BAD_LINK] < nl) {
        const u64 i = first_bad[CLEAN_BAD_LINK];
        throw DeviceError(components_bad_link_message(i, in.links[i].a, in.links[i].b, n));
    }
    if (first_bad[CLEAN_BAD_ORDER] < nl && first_bad[CLEAN_BAD_ORDER] > 0) {
        const u64 i = first_bad[CLEAN_BAD_ORDER];
        throw DeviceError(clean_unordered_link_message(i, in.links[i].a, in.links[i].b, in.links[i - 1].a));
    }
    if (first_bad[CLEAN_BAD_DUPLICATE] < nl) throw DeviceError(merge_duplicate_link_message(first_bad[0], in.links[first_bad[0]].a, in.links[first_bad[0]].b));
    if (first_bad[CLEAN_BAD_UNCLOSED] < nl) throw DeviceError(merge_unclosed_link_message(first_bad[1], in.links[first_bad[1]].a, in.links[first_bad[1]].b));
    if (h.n_survive > nl || h.n_gathered > nl - h.n_survive) throw DeviceError("clean: the device returned an impossible header (internal error)");
    const u64 ns = h.n_survive;
    std::vector<Link> gathered((size_t)h.n_gathered), created;
    if (h.n_gathered) {
        copy_d2h_async(gathered.data(), d_gathered.ptr(), h.n_gathered * sizeof(Link));
        meter.sync_copies();
    }
    seconds_device += meter.take();
    clean_duplicate_edit(in, gathered, &created);      // (throws: a number that is gone, or not exactly two non-self links)
    const u64 nc = created.size(), ne = ns + nc;
    // (per duplication at most: a loop from each strand's list, 2 x 2 create_link of two entries; two hairpins, 2 x 2 of one; two links of two)
    if (nc > 16ULL * nd) throw DeviceError("clean: the duplication created more entries than it can (internal error)");

    // ---- phase B: the buffers of phase A stay (no reset); the edited entries = the survivors, then the created ones ----
    const u64 nodes = 2 * (u64)n_out;
    const int node_bits = bit_width(nodes ? nodes - 1 : 0);
    DBuf<Link> d_edit(ne), d_sorted(ne), d_out_links(ne);
    DBuf<u32> d_len_in(n), d_len(n_out), d_copy_of(n_out), d_candidate(n_out), d_cand_pos(n_out), d_work0(n_out), d_work1(n_out), d_val(ne), d_off(nodes + 1),
        d_counter(CLEAN_ROUNDS_PER_BATCH + 1), d_flag_out(ne), d_pos_out(ne);
    DBuf<u8> d_type_in(in.type ? n : 0), d_alive(n_out), d_reason(n_out), d_type(n_out);
    DBuf<double> d_depth_in(in.depth ? n : 0), d_depth(n_out);
    DBuf<u64> d_seq_begin_in(with_seq ? n : 0), d_seq_begin(with_seq ? n_out : 0), d_node_key(ne), d_slot(n_out);
    copy_d2d(d_edit.ptr(), d_survive.ptr(), ns * sizeof(Link));
    copy_h2d(d_edit.ptr() + ns, created.data(), nc * sizeof(Link));
    copy_h2d(d_len_in.ptr(), in.unitig_len, (u64)n * 4);
    if (in.type) copy_h2d(d_type_in.ptr(), in.type, n);
    if (in.depth) copy_h2d(d_depth_in.ptr(), in.depth, (u64)n * 8);
    if (with_seq) copy_h2d(d_seq_begin_in.ptr(), in.seq_begin, (u64)n * 8);
    d_slot.fill_bytes(0); d_counter.fill_bytes(0);
    RadixScratch sort_nodes;
    sort_nodes.prepare(ne, node_bits);

    meter.begin();
    launch(n_out, CleanUnitigFunctor{n, d_duplicate.ptr(), p_alive_in, d_mark_remove.ptr(), d_mark_duplicate.ptr(), d_len_in.ptr(), in.depth ? d_depth_in.ptr() : nullptr, in.type ? d_type_in.ptr() : nullptr,
                                     with_seq ? d_seq_begin_in.ptr() : nullptr, in.has_min_depth ? 1 : 0, in.min_depth, d_alive.ptr(), d_reason.ptr(), d_len.ptr(),
                                     d_depth.ptr(), d_type.ptr(), with_seq ? d_seq_begin.ptr() : nullptr, d_copy_of.ptr(), d_candidate.ptr()});
    exclusive_scan_u32(d_candidate.ptr(), d_cand_pos.ptr(), n_out);
    launch(n_out, CleanCandidateFunctor{d_candidate.ptr(), d_cand_pos.ptr(), n_out, d_work0.ptr(), d_counter.ptr(), d_counts.ptr()});
    if (ne) {
        launch(ne, CleanSourceKeyFunctor{d_edit.ptr(), d_node_key.ptr(), d_val.ptr()});
        sort_pairs_u64_u32(d_node_key, d_val, ne, node_bits, 0, 0, &sort_nodes);
        launch(ne, CleanGatherFunctor{d_edit.ptr(), d_val.ptr(), d_sorted.ptr()});
    }
    launch(nodes + 1, CleanNodeOffsetFunctor{d_node_key.ptr(), ne, d_off.ptr()});
    meter.end();
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h);
        rb.run();
    }
    if (h.n_candidates > n_out || h.left != h.n_candidates) throw DeviceError("clean: the device returned an impossible header (internal error)");
    seconds_device += meter.take();

    // ---- the rounds of the low-depth step ----
    u64 left = h.left;
    u32 round = 0;
    while (left) {
        meter.begin();
        launch(1, CleanBatchInitFunctor{d_counter.ptr()});
        for (u32 r = 0; r < CLEAN_ROUNDS_PER_BATCH; r++, round++) {
            u32* const work = (r & 1) ? d_work1.ptr() : d_work0.ptr();
            u32* const work_next = (r & 1) ? d_work0.ptr() : d_work1.ptr();
            launch(left, CleanRoundMarkFunctor{work, d_counter.ptr() + r, round, d_sorted.ptr(), d_off.ptr(), d_slot.ptr()});
            launch_full(left, CleanRoundDecideFunctor{work, d_counter.ptr() + r, round, d_sorted.ptr(), d_off.ptr(), d_slot.ptr(), d_alive.ptr(), d_reason.ptr(), work_next,
                                                      d_counter.ptr() + r + 1, d_counts.ptr()});
        }
        launch(1, CleanLeftFunctor{d_counter.ptr(), d_counts.ptr()});
        meter.end();
        const u64 before = left;
        {
            ReadBatch rb;
            rb.add(&h, d_counts.ptr(), sizeof h);
            rb.run();
        }
        seconds_device += meter.take();
        left = h.left;
        if (left >= before || (left && before - left < CLEAN_ROUNDS_PER_BATCH))      // (every round with work decides at least one candidate)
            throw DeviceError("clean: the low-depth rounds made no progress (internal error)");
    }
    out->rounds = (u32)h.rounds;

    // ---- the links among what is alive now ----
    meter.begin();
    if (ne) {
        launch(ne, CleanOutFlagFunctor{d_sorted.ptr(), d_alive.ptr(), d_flag_out.ptr()});
        exclusive_scan_u32(d_flag_out.ptr(), d_pos_out.ptr(), ne);
        launch(ne, CleanOutCompactFunctor{d_sorted.ptr(), d_flag_out.ptr(), d_pos_out.ptr(), ne, d_out_links.ptr(), d_counts.ptr()});
    }
    meter.end();
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h);
        rb.run();
    }
    if (h.n_links_out > ne) throw DeviceError("clean: the device returned an impossible header (internal error)");
    out->links.resize((size_t)h.n_links_out); out->alive.resize(n_out); out->reason.resize(n_out); out->type.resize(n_out); out->len.resize(n_out);
    out->copy_of.resize(n_out); out->depth.resize(n_out); out->seq_begin.resize(with_seq ? n_out : 0);
    copy_d2h_async(out->links.data(), d_out_links.ptr(), h.n_links_out * sizeof(Link));
    copy_d2h_async(out->alive.data(), d_alive.ptr(), n_out);
    copy_d2h_async(out->reason.data(), d_reason.ptr(), n_out);
    copy_d2h_async(out->type.data(), d_type.ptr(), n_out);
    copy_d2h_async(out->len.data(), d_len.ptr(), (u64)n_out * 4);
    copy_d2h_async(out->copy_of.data(), d_copy_of.ptr(), (u64)n_out * 4);
    copy_d2h_async(out->depth.data(), d_depth.ptr(), (u64)n_out * 8);
    if (with_seq) copy_d2h_async(out->seq_begin.data(), d_seq_begin.ptr(), (u64)n_out * 8);
    meter.sync_copies();
    seconds_device += meter.take();
    out->stats = meter.stats();
    out->stats.seconds_device = seconds_device;
}
