// `autocycler trim` after the alignments — choose_trim_type's slices, exclude_outliers_in_length and the first half of clean_up_graph
// (trim.rs:189-269) — ON THE DEVICE: the slices' entries go up once and stay there, from create_sequence_and_positions' length check through to the
// subset stages of kernels_subset.inc, which recount the positions and drop the unitigs and links nobody visits any more.
// Part of graph_extras.hip (included inside namespace ac; not a translation unit of its own).  The host side is trim_apply_host.cpp.
//
// Stages of trim_apply_device, all on stream 0:
//   entry       per entry of a slice: it must name a unitig in 1..n that is alive (lowest bad index recorded otherwise); its length as a u64
//   scan        the lengths
//   sequence    per sequence: the sum of its slice = a difference of two prefixes (64-bit: an untrimmed sequence may be as long as u32 allows,
//               and the sum of a wrong table longer); it must equal the new length ("Position calculation mismatch", unitig_graph.rs:173):
//               the lowest mismatching sequence is recorded
//   (read-back: the sums and the error slots; the host computes median, MAD, range and keep flags: trim_apply_exclude)
//   compaction  only when somebody was excluded: per entry its sequence's keep flag (a binary search of the slice offsets), scan, scatter: the
//               kept sequences' entries move to the front of a second array in their order.  Nobody excluded: the entries are used as they lie
//   subsets     subset_stages with one cluster on the resident entries
// The number of launches depends on the key width and on whether anything was excluded — not on the number of sequences or the slice sizes.
static const int TRIM_APPLY_BAD_ENTRY = 0, TRIM_APPLY_DEAD_ENTRY = 1, TRIM_APPLY_MISMATCH = 2;      // first_bad[]: lowest index, ~0 = none

struct TrimApplyEntryFunctor {
    const int32_t* path; u32 n; const u32* unitig_len; const u8* alive; u64* len64; u64* first_bad;
    AC_D void operator()(u64 j) const {
        const int64_t e = path[j];
        const int64_t u = e < 0 ? -e : e;
        len64[j] = 0;
        if (u == 0 || u > (int64_t)n) { atomic_min64(&first_bad[TRIM_APPLY_BAD_ENTRY], j); return; }
        if (alive && !alive[u - 1]) { atomic_min64(&first_bad[TRIM_APPLY_DEAD_ENTRY], j); return; }
        len64[j] = unitig_len[u - 1];
    }
};

// prefix has n_entries + 1 words
struct TrimApplySeqFunctor {
    const u64* off; const u64* prefix; const u64* expected; u64* sum; u64* first_bad;
    AC_D void operator()(u64 s) const {
        const u64 v = prefix[off[s + 1]] - prefix[off[s]];
        sum[s] = v;
        if (v != expected[s]) atomic_min64(&first_bad[TRIM_APPLY_MISMATCH], s);
    }
};

// flag has n_entries + 1 words: the last one is 0, so that the scan's last word is the number of kept entries
struct TrimApplyFlagFunctor {
    const u64* off; u64 n_seqs; u64 n_entries; const u8* keep; u32* flag;
    AC_D void operator()(u64 j) const { flag[j] = (j < n_entries && keep[subset_last_at_or_before(off, n_seqs, j)]) ? 1u : 0u; }
};

struct TrimApplyScatterFunctor {
    const int32_t* path; const u32* flag; const u32* rank; u64 n_out; int32_t* out;
    AC_D void operator()(u64 j) const { if (flag[j] && (u64)rank[j] < n_out) out[rank[j]] = path[j]; }
};

// the slices' entries, one copy per run of slices that lie back to back in the caller's array
static void trim_apply_upload_entries(const TrimApplyPlan& tp, const int32_t* path, const u64* path_off, int32_t* d_path) {
    const size_t ns = tp.seqs.size();
    size_t i = 0;
    while (i < ns) {
        size_t j = i;
        while (j + 1 < ns && path_off[j] + tp.seqs[j].end == path_off[j + 1] + tp.seqs[j + 1].begin) j++;
        const u64 from = path_off[i] + tp.seqs[i].begin, upto = path_off[j] + tp.seqs[j].end;
        copy_h2d(d_path + tp.sliced_off[i], path + from, (upto - from) * 4);
        i = j + 1;
    }
}

void trim_apply_device(const TrimApplyInput& in, TrimApplyPlan* tp, SubsetPlan* plan, SubsetResult* out) {
    const u32 n = in.n_unitigs;
    const u64 nl = in.n_links, ns = tp->seqs.size(), ne = tp->sliced_off[ns];
    if (n == 0 || n > 0x7FFFFFFEu) throw DeviceError("trim apply: the number of unitigs must be between 1 and 2^31 - 2 here");
    if (ne == 0) throw DeviceError("trim apply: no entry in any slice (internal error)");
    if (ne >= 0xFFFFFFF0ULL) throw DeviceError("trim apply: more than 2^32 path entries in the slices");
    if (nl >= 0xFFFFFFF0ULL) throw DeviceError("trim apply: more than 2^32 links");
    {   // the device scan carries 46-bit totals: no table of lengths may reach that, whatever the entries name
        u32 longest = 0;
        for (u32 u = 0; u < n; u++) longest = std::max(longest, in.unitig_len[u]);
        if ((double)longest * (double)ne >= 70368744177664.0) throw DeviceError("trim apply: the slices could add up to 2^46 bases or more");
    }
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    std::vector<u64> expected(ns);
    for (u64 s = 0; s < ns; s++) expected[s] = tp->seqs[s].length;

    DBuf<int32_t> d_path(ne);
    DBuf<u64> d_off(ns + 1), d_expected(ns);
    DBuf<u32> d_len(n);
    DBuf<u8> d_alive(in.alive ? n : 0);
    DBuf<Link> d_links(nl);
    trim_apply_upload_entries(*tp, in.path, in.path_off, d_path.ptr());
    copy_h2d(d_off.ptr(), tp->sliced_off.data(), (ns + 1) * 8);
    copy_h2d(d_expected.ptr(), expected.data(), ns * 8);
    copy_h2d(d_len.ptr(), in.unitig_len, (u64)n * 4);
    if (in.alive) copy_h2d(d_alive.ptr(), in.alive, n);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    const u8* p_alive = in.alive ? d_alive.ptr() : nullptr;

    DBuf<u64> d_len64(ne + 1), d_prefix(ne + 1), d_sum(ns), d_first_bad(3);
    d_len64.fill_bytes(0); d_first_bad.fill_bytes(0xFF);
    meter.begin();
    launch(ne, TrimApplyEntryFunctor{d_path.ptr(), n, d_len.ptr(), p_alive, d_len64.ptr(), d_first_bad.ptr()});
    exclusive_scan_u64(d_len64.ptr(), d_prefix.ptr(), ne + 1);
    launch(ns, TrimApplySeqFunctor{d_off.ptr(), d_prefix.ptr(), d_expected.ptr(), d_sum.ptr(), d_first_bad.ptr()});
    meter.end();
    std::vector<u64> sum(ns, 0); u64 first_bad[3] = {~0ULL, ~0ULL, ~0ULL};
    {
        ReadBatch rb;
        rb.add(sum.data(), d_sum.ptr(), ns * 8); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad);
        rb.run();
    }
    if (first_bad[TRIM_APPLY_BAD_ENTRY] < ne || first_bad[TRIM_APPLY_DEAD_ENTRY] < ne) {
        const bool bad = first_bad[TRIM_APPLY_BAD_ENTRY] <= first_bad[TRIM_APPLY_DEAD_ENTRY];      // (the earlier of the two)
        const u64 j = bad ? first_bad[TRIM_APPLY_BAD_ENTRY] : first_bad[TRIM_APPLY_DEAD_ENTRY];
        const size_t s = (size_t)(std::upper_bound(tp->sliced_off.begin(), tp->sliced_off.end() - 1, j) - tp->sliced_off.begin()) - 1;
        const u64 index = tp->seqs[s].begin + (j - tp->sliced_off[s]);      // (within the caller's path, not the slice)
        const int32_t e = tp->sliced[(size_t)j];
        throw DeviceError(bad ? subset_bad_entry_message((u32)s, index, e, n) : subset_dead_entry_message((u32)s, index, e));
    }
    if (first_bad[TRIM_APPLY_MISMATCH] < ns) {
        const u64 s = first_bad[TRIM_APPLY_MISMATCH];
        throw DeviceError(trim_apply_mismatch_message((u32)s, sum[(size_t)s], expected[(size_t)s]));
    }
    trim_apply_exclude(tp, in.mad);
    out->n_unitigs = n;
    subset_prepare((u32)ns, tp->sliced.data(), tp->sliced_off.data(), tp->label.data(), 1, plan, out);
    const u64 n_kept = plan->kept_seq.size(), ne_kept = plan->kept_entries();
    if (ne_kept == 0) {      // (everyone excluded: the graph is empty, nothing more is launched)
        subset_empty_products(out);
        out->stats = meter.stats();
        return;
    }
    const int32_t* p_path = d_path.ptr();
    DBuf<int32_t> d_compact(tp->n_excluded ? ne_kept : 0);
    if (tp->n_excluded) {
        std::vector<u8> keep(ns);
        for (u64 s = 0; s < ns; s++) keep[s] = tp->label[s] ? 1 : 0;
        DBuf<u8> d_keep(ns);
        DBuf<u32> d_flag(ne + 1), d_rank(ne + 1);
        copy_h2d(d_keep.ptr(), keep.data(), ns);
        meter.begin();
        launch(ne + 1, TrimApplyFlagFunctor{d_off.ptr(), ns, ne, d_keep.ptr(), d_flag.ptr()});
        exclusive_scan_u32(d_flag.ptr(), d_rank.ptr(), ne + 1);
        launch(ne, TrimApplyScatterFunctor{d_path.ptr(), d_flag.ptr(), d_rank.ptr(), ne_kept, d_compact.ptr()});
        meter.end();
        p_path = d_compact.ptr();
    }
    DBuf<u64> d_kept_off(n_kept + 1);
    DBuf<u32> d_kept_label(n_kept);
    copy_h2d(d_kept_off.ptr(), plan->kept_off.data(), (n_kept + 1) * 8);
    copy_h2d(d_kept_label.ptr(), plan->kept_label.data(), n_kept * 4);
    SubsetInput sin;
    sin.n_unitigs = n; sin.links = in.links; sin.n_links = nl; sin.unitig_len = in.unitig_len; sin.alive = in.alive; sin.path = tp->sliced.data();
    sin.path_off = tp->sliced_off.data(); sin.n_clusters = 1; sin.plan = plan;
    StepStats total = meter.stats();
    StepMeter stage_meter;
    subset_stages(sin, SubsetResident{p_path, d_kept_off.ptr(), d_kept_label.ptr(), d_len.ptr(), p_alive, d_links.ptr()}, stage_meter, out);
    total += out->stats;
    out->stats = total;
}
