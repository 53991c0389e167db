// Sequence subsets of a graph — what save_cluster_gfa (cluster.rs:794-806), clean_up_graph (trim.rs:260-269) and resolve.rs:248 do to the graph
// before merge_linear_paths: drop sequences, recount the positions, remove the unitigs nobody visits any more with their links — for EVERY
// cluster of sequences in one call, as a read-only analysis ON THE DEVICE; and the paths of one cluster over the merged unitigs of a plan.
// Part of graph_extras.hip (included inside namespace ac; not a translation unit of its own).  The host side is subset_host.cpp.
//
// create_sequence_and_positions (unitig_graph.rs:151-174) walks a path forwards and its reverse backwards, so every entry of a kept path,
// on whichever strand, adds one position to its unitig's forward list and one to its reverse list: both lengths are the number of entries
// that name the unitig, and the unitig is alive in cluster c iff some kept path of c names it (depth = forward_positions.len() > 0).
//
// Stages of subsets_device, all on stream 0.  The entries of the kept sequences lie cluster after cluster (subset_prepare's order):
//   key         per kept entry: its sequence by a binary search of the kept offsets, key = (cluster - 1) * n + (unitig - 1); an entry that
//               names no unitig, or one that is not alive in the input, is recorded (lowest index) instead
//   radix sort  the keys: one run per (cluster, unitig) pair that occurs.  No atomic per entry: a unitig of a 1000-assembly graph is named
//               by 1000 sequences, which would all hit one address
//   heads       run-length: flag the first key of every run, scan, compact -> per pair its key and where its run begins
//   pairs       per pair: the unitig, the run's length = the position count, the unitig's length, and one bit in the unitig's row of cluster
//               bits (n x ceil(n_clusters / 64) words — the only memory that grows with n_clusters x n_unitigs)
//   scan        the lengths: total length per cluster is a difference of two prefixes
//   link count  per link: popcount of the AND of its two rows = the clusters that keep it; scan
//   (header read-back: errors, pairs, kept links)
//   link keys   per link, per common bit ascending: (cluster << 32) | link index, at the scanned offset: ascending link index per cluster...
//   radix sort  ...made cluster-major by a stable sort on the cluster bits alone: the input's order survives inside each cluster
//   decode      the links themselves
//   offsets     per cluster: where its unitigs and its links begin (binary searches), and the length prefix there
// The number of launches depends on the key widths alone — not on n_clusters, n_seqs or how the labels are spread.
struct SubsetCounts { u64 n_pairs, reserved; };
static const int SUBSET_BAD_ENTRY = 0, SUBSET_DEAD_ENTRY = 1, SUBSET_BAD_LINK = 2;      // first_bad[]: lowest index, ~0 = none

// the last r in [0, n_off) with off[r] <= j (off[0] = 0 <= j)
AC_D u64 subset_last_at_or_before(const u64* off, u64 n_off, u64 j) {
    u64 lo = 0, hi = n_off;
    for (int it = 0; it < 64 && hi - lo > 1; it++) {
        const u64 mid = lo + (hi - lo) / 2;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}
// the first p in [0, n) with key[p] >= k (n when none)
AC_D u64 subset_lower_bound(const u64* key, u64 n, u64 k, int shift) {
    u64 lo = 0, hi = n;
    for (int it = 0; it < 64 && lo < hi; it++) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((key[mid] >> shift) < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct SubsetKeyFunctor {
    const int32_t* path; const u64* kept_off; const u32* kept_label; u64 n_kept; u32 n; const u8* alive; u64* key; u32* val; u64* first_bad;
    AC_D void operator()(u64 j) const {
        const u64 r = subset_last_at_or_before(kept_off, n_kept, j);
        const int64_t e = path[j];
        const int64_t u = e < 0 ? -e : e;
        key[j] = 0; val[j] = 0;      // (a refused entry: the call fails, its key is never looked at)
        if (u == 0 || u > (int64_t)n) { atomic_min64(&first_bad[SUBSET_BAD_ENTRY], j); return; }
        if (alive && !alive[u - 1]) { atomic_min64(&first_bad[SUBSET_DEAD_ENTRY], j); return; }
        key[j] = (u64)(kept_label[r] - 1u) * n + (u64)(u - 1);
    }
};

struct SubsetHeadFunctor {
    const u64* key; u32* head;
    AC_D void operator()(u64 j) const { head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u; }
};

// pair_start has n_entries + 1 words: the run of pair p is [pair_start[p], pair_start[p + 1])
struct SubsetCompactFunctor {
    const u64* key; const u32* head; const u32* rank; u64 n_entries; u64* pair_key; u32* pair_start; SubsetCounts* counts;
    AC_D void operator()(u64 j) const {
        if (j + 1 == n_entries) { counts->n_pairs = (u64)rank[j] + head[j]; pair_start[rank[j] + head[j]] = (u32)n_entries; }
        if (!head[j]) return;
        pair_key[rank[j]] = key[j]; pair_start[rank[j]] = (u32)j;
    }
};

struct SubsetPairFunctor {
    const SubsetCounts* counts; const u64* pair_key; const u32* pair_start; u32 n; u32 n_clusters; u32 words; const u32* unitig_len;
    u32* unit; u32* count; u64* len64; u64* bits;
    AC_D void operator()(u64 p) const {
        len64[p] = 0;
        if (p >= counts->n_pairs) return;
        const u64 k = pair_key[p];
        const u64 c = k / n, u = k % n;
        if (c >= n_clusters) return;      // (cannot happen: the labels were checked)
        unit[p] = (u32)u + 1u; count[p] = pair_start[p + 1] - pair_start[p]; len64[p] = unitig_len[u];
        atomic_or64(&bits[u * words + (c >> 6)], 1ULL << (c & 63));
    }
};

struct SubsetLinkCountFunctor {
    const Link* links; u32 n; u32 words; const u64* bits; u64* kept; u64* first_bad;
    AC_D void operator()(u64 i) const {
        LinkEnds e;
        kept[i] = 0;
        if (link_ends(links[i], n, nullptr, &e) != LINK_OK) { atomic_min64(&first_bad[SUBSET_BAD_LINK], i); return; }
        const u64* ra = bits + (u64)e.ua * words; const u64* rb = bits + (u64)e.ub * words;
        u64 total = 0;
        for (u32 w = 0; w < words; w++) total += (u64)prim_popc64(ra[w] & rb[w]);
        kept[i] = total;
    }
};

struct SubsetLinkKeyFunctor {
    const Link* links; u32 n; u32 words; const u64* bits; const u64* kept_off; u64 n_out; u64* key; u32* val;
    AC_D void operator()(u64 i) const {
        LinkEnds e;
        if (link_ends(links[i], n, nullptr, &e) != LINK_OK) return;
        const u64* ra = bits + (u64)e.ua * words; const u64* rb = bits + (u64)e.ub * words;
        u64 at = kept_off[i];
        for (u32 w = 0; w < words; w++) {
            u64 m = ra[w] & rb[w];
            for (int it = 0; it < 64 && m; it++) {
                const u64 c = (u64)w * 64 + (u64)ctz64(m);
                m &= m - 1;
                if (at >= n_out) return;      // (cannot happen: the offsets are the scan of these very counts)
                key[at] = (c << 32) | i; val[at] = 0;
                at++;
            }
        }
    }
};

struct SubsetLinkDecodeFunctor {
    const u64* key; const Link* links; u64 n_links; Link* out;
    AC_D void operator()(u64 j) const {
        const u64 i = key[j] & 0xFFFFFFFFULL;
        out[j] = i < n_links ? links[i] : Link{0, 0};
    }
};

// cluster c in [0, n_clusters]: where its unitigs and links begin (c = n_clusters: where they end)
struct SubsetOffsetsFunctor {
    const SubsetCounts* counts; const u64* pair_key; const u64* len_prefix; u32 n; const u64* link_key; u64 n_out; u64* unit_off; u64* length_at; u64* link_off;
    AC_D void operator()(u64 c) const {
        const u64 p = subset_lower_bound(pair_key, counts->n_pairs, c * (u64)n, 0);
        unit_off[c] = p; length_at[c] = len_prefix[p];
        link_off[c] = n_out ? subset_lower_bound(link_key, n_out, c, 32) : 0;
    }
};

// the entries of kept sequences [first, first + count) of the plan, one copy per run of sequences that lie back to back in the caller's array
static void subset_upload_entries(const SubsetPlan& plan, size_t first, size_t count, const int32_t* path, const u64* path_off, int32_t* d_path) {
    size_t i = first;
    const u64 base = plan.kept_off[first];
    while (i < first + count) {
        size_t j = i;
        while (j + 1 < first + count && path_off[plan.kept_seq[j] + 1] == path_off[plan.kept_seq[j + 1]]) j++;
        const u64 from = path_off[plan.kept_seq[i]], upto = path_off[plan.kept_seq[j] + 1];
        copy_h2d(d_path + (plan.kept_off[i] - base), path + from, (upto - from) * 4);
        i = j + 1;
    }
}

// what subsets_device has put on the device before its stages run: the kept sequences' entries, cluster after cluster, and the input's arrays
struct SubsetResident { const int32_t* path; const u64* kept_off; const u32* kept_label; const u32* unitig_len; const u8* alive; const Link* links; };
static void subset_stages(const SubsetInput& in, const SubsetResident& d, StepMeter& meter, SubsetResult* out);

static void subset_check_sizes(u32 n, u64 ne, u64 nl) {
    if (n == 0 || n > 0x7FFFFFFEu) throw DeviceError("subsets: the number of unitigs must be between 1 and 2^31 - 2 here");
    if (ne == 0) throw DeviceError("subsets: no kept entry (internal error)");
    if (ne >= 0xFFFFFFF0ULL) throw DeviceError("subsets: more than 2^32 path entries in the kept sequences");
    if (nl >= 0xFFFFFFF0ULL) throw DeviceError("subsets: more than 2^32 links");
}

// the upload, then the stages
void subsets_device(const SubsetInput& in, SubsetResult* out) {
    const u32 n = in.n_unitigs;
    const u64 nl = in.n_links;
    const SubsetPlan& plan = *in.plan;
    const u64 ne = plan.kept_entries(), n_kept = plan.kept_seq.size();
    subset_check_sizes(n, ne, nl);
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    DBuf<int32_t> d_path(ne);
    DBuf<u64> d_kept_off(n_kept + 1);
    DBuf<u32> d_kept_label(n_kept), d_len(n);
    DBuf<u8> d_alive(in.alive ? n : 0);
    DBuf<Link> d_links(nl);
    subset_upload_entries(plan, 0, n_kept, in.path, in.path_off, d_path.ptr());
    copy_h2d(d_kept_off.ptr(), plan.kept_off.data(), (n_kept + 1) * 8);
    copy_h2d(d_kept_label.ptr(), plan.kept_label.data(), n_kept * 4);
    copy_h2d(d_len.ptr(), in.unitig_len, (u64)n * 4);
    if (in.alive) copy_h2d(d_alive.ptr(), in.alive, n);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    subset_stages(in, SubsetResident{d_path.ptr(), d_kept_off.ptr(), d_kept_label.ptr(), d_len.ptr(), in.alive ? d_alive.ptr() : nullptr, d_links.ptr()}, meter, out);
}

// The stages on entries that are on the device already (in.path / in.path_off: the host's copy, read for an error's text alone).  The arena
// session and the meter are the caller's: trim_apply_device (kernels_trim_apply.inc) runs them on the entries its own stage left there.
static void subset_stages(const SubsetInput& in, const SubsetResident& d, StepMeter& meter, SubsetResult* out) {
    const u32 n = in.n_unitigs, nc = in.n_clusters;
    const u64 nl = in.n_links;
    const SubsetPlan& plan = *in.plan;
    const u64 ne = plan.kept_entries(), n_kept = plan.kept_seq.size();
    subset_check_sizes(n, ne, nl);
    const u32 words = (nc + 63) / 64;
    // (the links' sort always runs over all 16 bits a label can have: two passes whatever n_clusters, so that the launches follow the entry keys' width alone)
    const int key_bits = bit_width((u64)nc * n - 1), cluster_bits = 16;
    const u8* p_alive = d.alive;

    DBuf<u64> d_key(ne), d_pair_key(ne), d_len64(ne + 1), d_len_prefix(ne + 1), d_bits((u64)n * words), d_link_kept(nl + 1), d_link_kept_off(nl + 1), d_first_bad(3);
    DBuf<u32> d_val(ne), d_head(ne), d_rank(ne), d_pair_start(ne + 1), d_unit(ne), d_count(ne);
    DBuf<u64> d_unit_off((u64)nc + 1), d_length_at((u64)nc + 1), d_link_off((u64)nc + 1);
    DBuf<SubsetCounts> d_counts(1);
    d_len64.fill_bytes(0); d_bits.fill_bytes(0); d_link_kept.fill_bytes(0); d_link_kept_off.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_counts.fill_bytes(0);
    d_pair_start.fill_bytes(0); d_pair_key.fill_bytes(0);
    RadixScratch sort_keys;
    sort_keys.prepare(ne, key_bits);

    meter.begin();
    launch(ne, SubsetKeyFunctor{d.path, d.kept_off, d.kept_label, n_kept, n, p_alive, d_key.ptr(), d_val.ptr(), d_first_bad.ptr()});
    sort_pairs_u64_u32(d_key, d_val, ne, key_bits, 0, 0, &sort_keys);
    launch(ne, SubsetHeadFunctor{d_key.ptr(), d_head.ptr()});
    exclusive_scan_u32(d_head.ptr(), d_rank.ptr(), ne);
    launch(ne, SubsetCompactFunctor{d_key.ptr(), d_head.ptr(), d_rank.ptr(), ne, d_pair_key.ptr(), d_pair_start.ptr(), d_counts.ptr()});
    launch(ne, SubsetPairFunctor{d_counts.ptr(), d_pair_key.ptr(), d_pair_start.ptr(), n, nc, words, d.unitig_len, d_unit.ptr(), d_count.ptr(), d_len64.ptr(), d_bits.ptr()});
    exclusive_scan_u64(d_len64.ptr(), d_len_prefix.ptr(), ne + 1);
    if (nl) {
        launch(nl, SubsetLinkCountFunctor{d.links, n, words, d_bits.ptr(), d_link_kept.ptr(), d_first_bad.ptr()});
        exclusive_scan_u64(d_link_kept.ptr(), d_link_kept_off.ptr(), nl + 1);
    }
    meter.end();
    // the header: errors, the pairs and the kept links — what sizes the second half and the bulk copy
    SubsetCounts h; u64 first_bad[3] = {~0ULL, ~0ULL, ~0ULL}; u64 n_out = 0;
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad); rb.add(&n_out, d_link_kept_off.ptr() + nl, 8);
        rb.run();
    }
    if (first_bad[SUBSET_BAD_ENTRY] < ne || first_bad[SUBSET_DEAD_ENTRY] < ne) {
        const bool bad = first_bad[SUBSET_BAD_ENTRY] <= first_bad[SUBSET_DEAD_ENTRY];      // (the earlier of the two)
        u32 seq = 0; u64 index = 0;
        subset_locate(plan, bad ? first_bad[SUBSET_BAD_ENTRY] : first_bad[SUBSET_DEAD_ENTRY], &seq, &index);
        const int32_t e = in.path[in.path_off[seq] + index];
        throw DeviceError(bad ? subset_bad_entry_message(seq, index, e, n) : subset_dead_entry_message(seq, index, e));
    }
    if (first_bad[SUBSET_BAD_LINK] < nl) { const u64 i = first_bad[SUBSET_BAD_LINK]; throw DeviceError(components_bad_link_message(i, in.links[i].a, in.links[i].b, n)); }
    if (h.n_pairs == 0 || h.n_pairs > ne || n_out > nl * (u64)nc) throw DeviceError("subsets: the device returned an impossible header (internal error)");
    if (n_out >= 0xFFFFFFF0ULL) throw DeviceError("subsets: more than 2^32 kept links over all clusters");
    const u64 np = h.n_pairs;
    DBuf<u64> d_link_key(n_out);
    DBuf<u32> d_link_val(n_out);
    DBuf<Link> d_links_out(n_out);
    meter.begin();
    if (n_out) {
        launch(nl, SubsetLinkKeyFunctor{d.links, n, words, d_bits.ptr(), d_link_kept_off.ptr(), n_out, d_link_key.ptr(), d_link_val.ptr()});
        sort_pairs_u64_u32(d_link_key, d_link_val, n_out, 32 + cluster_bits, 0, 32);
        launch(n_out, SubsetLinkDecodeFunctor{d_link_key.ptr(), d.links, nl, d_links_out.ptr()});
    }
    launch((u64)nc + 1, SubsetOffsetsFunctor{d_counts.ptr(), d_pair_key.ptr(), d_len_prefix.ptr(), n, d_link_key.ptr(), n_out, d_unit_off.ptr(), d_length_at.ptr(),
                                             d_link_off.ptr()});
    meter.end();
    const size_t c1 = (size_t)nc + 1;
    out->unitig_off.resize(c1); out->length_at.resize(c1); out->link_off.resize(c1);
    out->unitigs.resize((size_t)np); out->positions.resize((size_t)np); out->links.resize((size_t)n_out);
    copy_d2h_async(out->unitig_off.data(), d_unit_off.ptr(), c1 * 8);
    copy_d2h_async(out->length_at.data(), d_length_at.ptr(), c1 * 8);
    copy_d2h_async(out->link_off.data(), d_link_off.ptr(), c1 * 8);
    copy_d2h_async(out->unitigs.data(), d_unit.ptr(), np * 4);
    copy_d2h_async(out->positions.data(), d_count.ptr(), np * 4);
    copy_d2h_async(out->links.data(), d_links_out.ptr(), n_out * sizeof(Link));
    meter.sync_copies();
    out->stats = meter.stats();
}

// ---- the paths of one cluster over the merged unitigs ------------------------------------------------------------------------------------------
// After merge_linear_paths the reference rebuilds a path by walking positions (get_unitig_path_for_sequence, unitig_graph.rs:407-465); the merged
// unitig carries its first member's forward and its last member's reverse positions (merge_path, graph_simplification.rs:414-415).  The members
// inside a chain have one way in and one way out and path ends are fixed, so a path that touches a chain runs through all of it: the walk equals
// the old path with every traversal of a chain collapsed into the chain's number, + along the chain, - against it.
//   members     per member of the plan's member list: its index in its chain and its chain strand, by unitig
//   flags       per entry: outside a chain it stays; along its chain strand it is emitted at index 0, against it at the last index (a loop
//               walked several times: once per lap); its own length, and the length it has in the new path: the chain's where emitted
//   scans       the flags: where every kept entry goes; the two lengths: every sequence's must add up to the same (two sums, not one of
//               differences: the device scan carries 46-bit values)
//   sequences   per sequence: its new offset, the invariant, and that it neither begins nor ends strictly inside a chain
//   scatter     the kept entries
struct MergedPathsView { u32 n; const u32* chain_of; const u32* pos_in; const u8* strand_in; const MergeChainRecord* chains; u64 n_chains; };
// is entry e in a chain, and where in its traversal: bit 0 in a chain, bit 1 at the traversal's first member, bit 2 at its last, bit 3 along the chain
AC_D u32 merged_paths_classify(const MergedPathsView& v, int64_t e, u32* chain) {
    const int64_t u = e < 0 ? -e : e;
    if (u == 0 || u > (int64_t)v.n) return 0;
    const u32 ch = v.chain_of[u - 1];
    if (ch == MERGE_NONE || (u64)ch >= v.n_chains) return 0;
    *chain = ch;
    const bool along = (v.strand_in[u - 1] != 0) == (e < 0);
    const u32 pos = v.pos_in[u - 1], last = v.chains[ch].members - 1u;
    const bool first_here = along ? pos == 0 : pos == last, last_here = along ? pos == last : pos == 0;
    return 1u | (first_here ? 2u : 0u) | (last_here ? 4u : 0u) | (along ? 8u : 0u);
}

struct MergedPathsMemberFunctor {
    const int32_t* members; u32 n; const u32* chain_of; const MergeChainRecord* chains; u64 n_chains; u32* pos_in; u8* strand_in; u32* err;
    AC_D void operator()(u64 m) const {
        const int64_t e = members[m];
        const int64_t u = e < 0 ? -e : e;
        if (u == 0 || u > (int64_t)n) { atomic_or32(err, 1u); return; }
        const u32 ch = chain_of[u - 1];
        if ((u64)ch >= n_chains || m < chains[ch].member_off || m - chains[ch].member_off >= chains[ch].members) { atomic_or32(err, 1u); return; }
        pos_in[u - 1] = (u32)(m - chains[ch].member_off); strand_in[u - 1] = e < 0 ? 1 : 0;
    }
};

struct MergedPathsFlagFunctor {
    const int32_t* path; MergedPathsView v; const u32* unitig_len; u32* flag; int32_t* entry_out; u64* len_old; u64* len_new;
    AC_D void operator()(u64 j) const {
        const int64_t e = path[j];
        const int64_t u = e < 0 ? -e : e;
        u32 ch = 0;
        const u32 cls = merged_paths_classify(v, e, &ch);
        const u64 own = (u != 0 && u <= (int64_t)v.n) ? (u64)unitig_len[u - 1] : 0;
        len_old[j] = own;
        if (!(cls & 1u)) { flag[j] = 1; entry_out[j] = (int32_t)e; len_new[j] = own; return; }
        const bool emit = (cls & 2u) != 0;
        const int64_t number = (int64_t)v.n + 1 + (int64_t)ch;
        flag[j] = emit ? 1u : 0u; entry_out[j] = (int32_t)((cls & 8u) ? number : -number);
        len_new[j] = emit ? v.chains[ch].length : 0ULL;
    }
};

// sequence r in [0, n_seqs]: its offset among the new entries (r = n_seqs: their number)
struct MergedPathsSeqFunctor {
    const int32_t* path; MergedPathsView v; const u64* seq_off; u64 n_seqs; const u32* rank; const u64* old_prefix; const u64* new_prefix; u64* new_off; u64* first_bad;
    AC_D void operator()(u64 r) const {
        const u64 b = seq_off[r];
        new_off[r] = rank[b];
        if (r == n_seqs) return;
        const u64 e = seq_off[r + 1];
        if (e == b) return;
        u32 ch = 0;
        const u32 first = merged_paths_classify(v, path[b], &ch), last = merged_paths_classify(v, path[e - 1], &ch);
        if ((first & 1u) && !(first & 2u)) atomic_min64(&first_bad[0], r);
        if ((last & 1u) && !(last & 4u)) atomic_min64(&first_bad[1], r);
        if (old_prefix[e] - old_prefix[b] != new_prefix[e] - new_prefix[b]) atomic_min64(&first_bad[2], r);
    }
};

struct MergedPathsScatterFunctor {
    const u32* flag; const u32* rank; const int32_t* entry_out; u64 n_out_max; int32_t* out;
    AC_D void operator()(u64 j) const { if (flag[j] && (u64)rank[j] < n_out_max) out[rank[j]] = entry_out[j]; }
};

void merged_paths_device(const MergedPathsInput& in, MergedPathsResult* out) {
    const u32 n = in.n_unitigs;
    const SubsetPlan& plan = *in.plan;
    const MergeResult& mr = *in.merge;
    const size_t ns = in.kept_count;
    const u64 base = plan.kept_off[in.kept_first], ne = plan.kept_off[in.kept_first + ns] - base;
    const u64 n_chains = mr.chains.size(), nm = mr.members.size();
    if (n == 0 || ne == 0) throw DeviceError("merged paths: nothing to launch (internal error)");
    if (ne >= 0xFFFFFFF0ULL) throw DeviceError("merged paths: more than 2^32 path entries in the cluster");
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    std::vector<u64> seq_off(ns + 1);
    for (size_t i = 0; i <= ns; i++) seq_off[i] = plan.kept_off[in.kept_first + i] - base;

    DBuf<int32_t> d_path(ne + 1), d_members(nm), d_entry(ne), d_out(ne);
    DBuf<u64> d_seq_off(ns + 1), d_len_old(ne + 1), d_len_new(ne + 1), d_old_prefix(ne + 1), d_new_prefix(ne + 1), d_new_off(ns + 1), d_first_bad(3);
    DBuf<u32> d_len(n), d_chain_of(n), d_pos_in(n), d_flag(ne + 1), d_rank(ne + 1), d_err(2);
    DBuf<u8> d_strand_in(n);
    DBuf<MergeChainRecord> d_chains(n_chains);
    subset_upload_entries(plan, in.kept_first, ns, in.path, in.path_off, d_path.ptr());
    copy_h2d(d_seq_off.ptr(), seq_off.data(), (ns + 1) * 8);
    copy_h2d(d_len.ptr(), in.unitig_len, (u64)n * 4);
    copy_h2d(d_chain_of.ptr(), mr.chain_of.data(), (u64)n * 4);
    copy_h2d(d_members.ptr(), mr.members.data(), nm * 4);
    copy_h2d(d_chains.ptr(), mr.chains.data(), n_chains * sizeof(MergeChainRecord));
    d_pos_in.fill_bytes(0); d_strand_in.fill_bytes(0); d_flag.fill_bytes(0); d_len_old.fill_bytes(0); d_len_new.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_err.fill_bytes(0);
    const MergedPathsView view{n, d_chain_of.ptr(), d_pos_in.ptr(), d_strand_in.ptr(), d_chains.ptr(), n_chains};

    meter.begin();
    if (nm) launch(nm, MergedPathsMemberFunctor{d_members.ptr(), n, d_chain_of.ptr(), d_chains.ptr(), n_chains, d_pos_in.ptr(), d_strand_in.ptr(), d_err.ptr()});
    launch(ne, MergedPathsFlagFunctor{d_path.ptr(), view, d_len.ptr(), d_flag.ptr(), d_entry.ptr(), d_len_old.ptr(), d_len_new.ptr()});
    exclusive_scan_u32(d_flag.ptr(), d_rank.ptr(), ne + 1);
    exclusive_scan_u64(d_len_old.ptr(), d_old_prefix.ptr(), ne + 1);
    exclusive_scan_u64(d_len_new.ptr(), d_new_prefix.ptr(), ne + 1);
    launch((u64)ns + 1, MergedPathsSeqFunctor{d_path.ptr(), view, d_seq_off.ptr(), ns, d_rank.ptr(), d_old_prefix.ptr(), d_new_prefix.ptr(), d_new_off.ptr(), d_first_bad.ptr()});
    launch(ne, MergedPathsScatterFunctor{d_flag.ptr(), d_rank.ptr(), d_entry.ptr(), ne, d_out.ptr()});
    meter.end();
    u32 total = 0, err[2] = {0, 0}; u64 first_bad[3] = {~0ULL, ~0ULL, ~0ULL};
    {
        ReadBatch rb;
        rb.add(&total, d_rank.ptr() + ne, 4); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad); rb.add(err, d_err.ptr(), sizeof err);
        rb.run();
    }
    if (err[0]) throw DeviceError("merged paths: the plan's member list does not fit its chains");
    for (int which = 0; which < 2; which++)
        if (first_bad[which] < ns && first_bad[which] <= first_bad[1 - which]) {
            const u32 seq = plan.kept_seq[in.kept_first + (size_t)first_bad[which]];
            const int32_t e = which == 0 ? in.path[in.path_off[seq]] : in.path[in.path_off[seq + 1] - 1];
            const uint32_t u = e < 0 ? (uint32_t)(-(int64_t)e) : (uint32_t)e;
            throw DeviceError(merged_paths_inside_message(seq, which == 0, e, n + 1 + mr.chain_of[u - 1]));
        }
    if (first_bad[2] < ns) throw DeviceError(merged_paths_length_message(plan.kept_seq[in.kept_first + (size_t)first_bad[2]]));
    if ((u64)total > ne) throw DeviceError("merged paths: the device returned an impossible header (internal error)");
    out->entries.resize(total); out->path_off.resize(ns + 1);
    copy_d2h_async(out->entries.data(), d_out.ptr(), (u64)total * 4);
    copy_d2h_async(out->path_off.data(), d_new_off.ptr(), (ns + 1) * 8);
    meter.sync_copies();
    out->entries_before = ne;
    out->stats = meter.stats();
}
