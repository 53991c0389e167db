// `autocycler combine` (combine.rs:144-224) ON THE DEVICE: load_clusters' stable sort by total length, combine_clusters' running offset, the
// per-unitig end tests its FASTA headers print, topology() of every graph and get_links_for_gfa's order — for all graphs at once, on their
// concatenation.  Part of graph_extras.hip (included inside namespace ac; not a translation unit of its own).  The host side is combine_host.cpp.
//
// The reference's loop carries one number from graph to graph (offset += max_unitig_number()) and prints as it goes.  Here nothing is
// carried: a graph's place is its rank in a stable sort, its offset a prefix sum over the maxima in rank order, a unitig's output slot its
// graph's base plus its place in the file, and a link's place the rank of (slot of its source, strand) in a stable sort.
//
// Stages of combine_device, all on stream 0, nothing read by the host in between:
//   unitig      per unitig: its graph (binary search of unitig_off), its length as a u64, the printed depth (the caller's, or with read depths
//               the read depth / 0.0), the graph's highest number: an atomic max per (wavefront, run of one graph)
//   scan        the lengths; a graph's total is a difference of two prefixes
//   graph       per graph: the total, the sort key ~total (46 bits) with the input index as value; one more key behind all of them, so that
//               the sort has two items even for one graph
//   radix sort  stable: rank order, ties in input order
//   rank        per rank: the graph's maximum and unitig count in rank order
//   2 scans     the offsets and the bases of the output slots
//   offsets     per rank: offset and base back under the graph's input index; the first rank whose offset + maximum leaves u32 is recorded
//   link        per link: its graph (binary search of link_off), the range check of both ends (lowest bad index recorded), the entry with
//               global indices for the flag stage, the sort key (slot of |a|) * 2 + (a < 0); two more keys behind all of them
//   flags       CompInit, CompCensus and CompRoots of kernels_components.inc as they stand, on the concatenation: the end tests are local, so
//               every graph gets its own answers.  (The census also hooks its trees; nothing here reads them, and the root pass's "tree not
//               flat" word goes to a slot nobody looks at: the jump rounds between the two are the components' own business.)
//   printed     per unitig: the printed number as a sort key (32 bits), one more key behind
//   radix sort  the printed numbers; graphs own disjoint ranges, so two neighbours with one key and one graph are a duplicate
//   duplicates  the lowest (graph, number) that occurs twice
//   records     per graph: unitigs, links, topology() from the only unitig's flags
//   unitig out  per unitig: its record into its output slot
//   radix sort  the links by their key, limited to the bits 2 n + 1 needs
//   link out    both ends rewritten to printed numbers
// The number of launches depends on the key width of the link sort (the bits of 2 n) and on nothing else.  The bases never come here: no
// decision reads them.
static const int COMBINE_BAD_LINK = 0, COMBINE_DUPLICATE = 1, COMBINE_OVERFLOW = 2;      // err[]: lowest offender, ~0 = none
static const u64 COMBINE_TOTAL_MAX = (1ULL << 46) - 1;

// the highest value over the lanes of this lane's run up to this lane
AC_D u32 combine_run_max32(u32 v, u32 run, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = (u32)wv::shfl_up((int)v, o);
        const u32 tr = (u32)wv::shfl_up((int)run, o);
        if (lane >= o && tr == run && t > v) v = t;
    }
    return v;
}

// topology() (unitig_graph.rs:527-545) of a graph from its unitig count, its link count and its only unitig's flags
AC_D u32 combine_topology(u64 unitigs, u64 links, u8 f) {
    if (unitigs == 0) return TOPO_EMPTY;
    if (unitigs > 1) return TOPO_FRAGMENTED;
    if (links == 0) return TOPO_LINEAR_OPEN_OPEN;
    if (f & CUF_ISOLATED_CIRCULAR) return TOPO_CIRCULAR;
    if ((f & CUF_HAIRPIN_START) && (f & CUF_HAIRPIN_END)) return TOPO_LINEAR_HAIRPIN_HAIRPIN;
    if ((f & CUF_HAIRPIN_START) && (f & CUF_OPEN_END)) return TOPO_LINEAR_OPEN_HAIRPIN;
    if ((f & CUF_OPEN_START) && (f & CUF_HAIRPIN_END)) return TOPO_LINEAR_OPEN_HAIRPIN;
    return TOPO_OTHER;
}

// len64 has n + 1 words (the last one stays 0)
struct CombineUnitigFunctor {
    const u64* unitig_off; u32 n_graphs; u64 n; const u32* number; const u32* len; const double* depth; const double* read_depth; const u8* has_read_depth;
    u32* graph_of; u64* len64; double* printed_depth; u32* max_number;
    AC_D void operator()(u64 u, bool valid) const {
        const int lane = wv::lane();
        u32 g = 0xFFFFFFFFu, num = 0;
        if (valid) {
            g = (u32)subset_last_at_or_before(unitig_off, (u64)n_graphs, u);      // (empty graphs share their offset with the next: the last of them at or before u owns it)
            graph_of[u] = g; len64[u] = len[u]; num = number[u];
            printed_depth[u] = read_depth ? (has_read_depth[u] ? read_depth[u] : 0.0) : (depth ? depth[u] : 0.0);
        }
        const u32 run = comp_run_id(g, lane);
        num = combine_run_max32(num, run, lane);
        const u32 next_run = (u32)wv::shfl_down((int)run, 1);
        if (valid && (lane == 63 || next_run != run) && num) atomic_max32(&max_number[g], num);
    }
};

// g < n_graphs: the graph's key; g == n_graphs: the key behind them all
struct CombineGraphFunctor {
    const u64* unitig_off; u32 n_graphs; const u64* prefix; u64* total; u64* key; u32* val;
    AC_D void operator()(u64 g) const {
        val[g] = (u32)g;
        if (g == n_graphs) { key[g] = 1ULL << 46; return; }
        const u64 t = prefix[unitig_off[g + 1]] - prefix[unitig_off[g]];
        total[g] = t;
        key[g] = COMBINE_TOTAL_MAX - (t & COMBINE_TOTAL_MAX);      // Reverse(total_length())
    }
};

// r < n_graphs: the graph at rank r; r == n_graphs: the word whose prefix is the sum
struct CombineRankFunctor {
    const u32* order; u32 n_graphs; const u64* unitig_off; const u32* max_number; u64* max_ranked; u64* count_ranked;
    AC_D void operator()(u64 r) const {
        if (r == n_graphs) { max_ranked[r] = 0; count_ranked[r] = 0; return; }
        const u32 g = order[r];
        max_ranked[r] = max_number[g];
        count_ranked[r] = unitig_off[g + 1] - unitig_off[g];
    }
};

struct CombineOffsetsFunctor {
    const u32* order; const u64* max_ranked; const u64* offset_ranked; const u64* base_ranked; u32* rank_of; u64* offset_of; u64* base_of; u64* err;
    AC_D void operator()(u64 r) const {
        const u32 g = order[r];
        rank_of[g] = (u32)r; offset_of[g] = offset_ranked[r]; base_of[g] = base_ranked[r];
        if (offset_ranked[r] + max_ranked[r] > 0xFFFFFFFFULL) atomic_min64(&err[COMBINE_OVERFLOW], r);
    }
};

// i < n_links: a link; beyond: the keys behind them all, entries that name no unitig
struct CombineLinkFunctor {
    const Link* links; u64 n_links; const u64* link_off; const u64* unitig_off; u32 n_graphs; u64 n; const u64* base_of;
    Link* global; u32* link_graph; u64* key; u32* val; u64* err;
    AC_D void operator()(u64 i) const {
        val[i] = (u32)i; key[i] = 2 * n; global[i] = Link{0, 0};
        if (i >= n_links) return;
        const u32 g = (u32)subset_last_at_or_before(link_off, (u64)n_graphs, i);
        link_graph[i] = g;
        const u64 first = unitig_off[g], count = unitig_off[g + 1] - first;
        const Link l = links[i];
        const u64 na = l.na(), nb = l.nb();
        if (na == 0 || nb == 0 || na > count || nb > count) { atomic_min64(&err[COMBINE_BAD_LINK], i); return; }
        const int32_t ga = (int32_t)(first + na), gb = (int32_t)(first + nb);      // (n is below 2^31)
        global[i] = Link{l.a > 0 ? ga : -ga, l.b > 0 ? gb : -gb};
        key[i] = (base_of[g] + (na - 1)) * 2 + (l.a < 0 ? 1 : 0);
    }
};

// u < n: a unitig; u == n: the key behind them all (it belongs to no graph)
struct CombinePrintedFunctor {
    u64 n; const u32* number; const u32* graph_of; const u64* offset_of; u64* key; u32* val;
    AC_D void operator()(u64 u) const {
        val[u] = (u32)u;
        key[u] = u == n ? 0xFFFFFFFFULL : (((u64)number[u] + offset_of[graph_of[u]]) & 0xFFFFFFFFULL);      // (beyond 32 bits the call fails with the overflow)
    }
};

struct CombineDuplicateFunctor {
    u64 n; const u64* key; const u32* val; const u32* graph_of; const u32* number; u64* err;
    AC_D void operator()(u64 j) const {
        if (j == 0) return;
        const u32 a = val[j - 1], b = val[j];
        if ((u64)a >= n || (u64)b >= n || key[j - 1] != key[j]) return;
        if (graph_of[a] != graph_of[b] || number[a] != number[b]) return;      // (number 0 of one graph prints as the maximum of the graph before)
        atomic_min64(&err[COMBINE_DUPLICATE], ((u64)graph_of[a] << 32) | (u64)number[a]);
    }
};

struct CombineRecordsFunctor {
    const u32* order; const u64* unitig_off; const u64* link_off; const u64* total; const u32* max_number; const u64* offset_of; const u8* flags;
    CombineClusterRecord* records;
    AC_D void operator()(u64 r) const {
        const u32 g = order[r];
        CombineClusterRecord& c = records[r];      // (the buffer was zeroed: the padding and the host's fields stay 0)
        c.input_index = g; c.unitigs = (u32)(unitig_off[g + 1] - unitig_off[g]); c.length = total[g]; c.links = link_off[g + 1] - link_off[g];
        c.offset = offset_of[g]; c.max_number = max_number[g];
        c.topology = combine_topology(c.unitigs, c.links, c.unitigs == 1 ? flags[unitig_off[g]] : (u8)0);
    }
};

struct CombineUnitigOutFunctor {
    const u64* unitig_off; const u32* graph_of; const u32* number; const u32* len; const double* printed_depth; const double* read_depth; const u8* has_read_depth;
    const u8* type; const u8* flags; const u64* offset_of; const u64* base_of; u64 n; CombineUnitigRecord* out;
    AC_D void operator()(u64 u) const {
        const u32 g = graph_of[u];
        const u64 local = u - unitig_off[g], slot = base_of[g] + local;
        if (slot >= n) return;      // (cannot happen: the bases are a prefix sum of the counts)
        CombineUnitigRecord& t = out[slot];      // (zeroed)
        t.graph = g; t.index = (u32)local; t.number = (u32)((u64)number[u] + offset_of[g]); t.length = len[u];
        t.depth = printed_depth[u];
        t.has_read_depth = read_depth && has_read_depth[u] ? 1 : 0;
        t.read_depth = t.has_read_depth ? read_depth[u] : 0.0;
        t.flags = flags[u]; t.type = type ? type[u] : (u8)0;
    }
};

// sorted[j] = the j-th link in output order
struct CombineLinkOutFunctor {
    const u32* sorted; const Link* links; const u32* link_graph; const u64* unitig_off; const u32* number; const u64* offset_of; u64 n_links; Link* out;
    AC_D void operator()(u64 j) const {
        const u32 i = sorted[j];
        if (j >= n_links || (u64)i >= n_links) return;      // (the keys behind sort behind)
        const u32 g = link_graph[i];
        const Link l = links[i];
        const u64 first = unitig_off[g], count = unitig_off[g + 1] - first;
        out[j] = Link{0, 0};
        if (l.na() == 0 || l.nb() == 0 || l.na() > count || l.nb() > count) return;      // (a refused entry: the call fails, nobody reads this)
        const int32_t pa = (int32_t)(u32)((u64)number[first + l.na() - 1] + offset_of[g]), pb = (int32_t)(u32)((u64)number[first + l.nb() - 1] + offset_of[g]);
        out[j] = Link{l.a > 0 ? pa : -pa, l.b > 0 ? pb : -pb};
    }
};

void combine_device(const CombineInput& in, CombineResult* out) {
    *out = CombineResult();
    out->with_reads = in.read_depth != nullptr;
    const u32 G = in.n_graphs;
    const u64 n = in.n_unitigs(), nl = in.n_links(), nlp = nl + 2;
    if (n == 0) throw DeviceError("combine: no unitig in any graph (internal error)");
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    const int link_bits = bit_width(2 * n);

    DBuf<u64> d_uoff((u64)G + 1), d_loff((u64)G + 1);
    DBuf<u32> d_number(n), d_len(n);
    DBuf<double> d_depth(in.depth ? n : 0), d_rd(in.read_depth ? n : 0);
    DBuf<u8> d_has(in.read_depth ? n : 0), d_type(in.type ? n : 0);
    DBuf<Link> d_links(nlp);
    copy_h2d(d_uoff.ptr(), in.unitig_off, ((u64)G + 1) * 8);
    copy_h2d(d_loff.ptr(), in.link_off, ((u64)G + 1) * 8);
    copy_h2d(d_number.ptr(), in.number, n * 4);
    copy_h2d(d_len.ptr(), in.len, n * 4);
    if (in.depth) copy_h2d(d_depth.ptr(), in.depth, n * 8);
    if (in.read_depth) { copy_h2d(d_rd.ptr(), in.read_depth, n * 8); copy_h2d(d_has.ptr(), in.has_read_depth, n); }
    if (in.type) copy_h2d(d_type.ptr(), in.type, n);
    if (nl) copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    const double* p_depth = in.depth ? d_depth.ptr() : nullptr;
    const double* p_rd = in.read_depth ? d_rd.ptr() : nullptr;
    const u8* p_has = in.read_depth ? d_has.ptr() : nullptr;
    const u8* p_type = in.type ? d_type.ptr() : nullptr;

    DBuf<u32> d_graph_of(n), d_max(G), d_gval((u64)G + 1), d_rank_of(G), d_link_graph(nlp), d_lval(nlp), d_pval(n + 1);
    DBuf<u64> d_len64(n + 1), d_prefix(n + 1), d_total(G), d_gkey((u64)G + 1), d_max_ranked((u64)G + 1), d_count_ranked((u64)G + 1), d_offset_ranked((u64)G + 1),
        d_base_ranked((u64)G + 1), d_offset_of(G), d_base_of(G), d_lkey(nlp), d_pkey(n + 1), d_err(3);
    DBuf<double> d_printed(n);
    DBuf<Link> d_global(nlp), d_links_out(nl);
    DBuf<CombineClusterRecord> d_records(G);
    DBuf<CombineUnitigRecord> d_unitigs_out(n);
    // the flag stage's arrays (kernels_components.inc)
    const u32 n32 = (u32)n;
    const int comp_key_bits = bit_width(2 * n);
    DBuf<u32> d_deg(4 * n), d_notself(n), d_parent(n), d_cerr(2), d_roots_err(1), d_is_root(n), d_ckey_unitig(nlp);
    DBuf<int32_t> d_target(4 * n);
    DBuf<u64> d_ckey(nlp);
    DBuf<u8> d_flags(n);
    DBuf<CompHeader> d_hdr(1);
    d_max.fill_bytes(0); d_len64.fill_bytes(0); d_err.fill_bytes(0xFF); d_records.fill_bytes(0); d_unitigs_out.fill_bytes(0); d_link_graph.fill_bytes(0);
    d_deg.fill_bytes(0); d_notself.fill_bytes(0); d_cerr.fill_bytes(0); d_roots_err.fill_bytes(0); d_target.fill_bytes(0); d_hdr.fill_bytes(0xFF);
    RadixScratch sort_graphs, sort_printed, sort_links;
    sort_graphs.prepare((u64)G + 1, 47);
    sort_printed.prepare(n + 1, 32);
    sort_links.prepare(nlp, link_bits);

    meter.begin();
    launch_full(n, CombineUnitigFunctor{d_uoff.ptr(), G, n, d_number.ptr(), d_len.ptr(), p_depth, p_rd, p_has, d_graph_of.ptr(), d_len64.ptr(), d_printed.ptr(), d_max.ptr()});
    exclusive_scan_u64(d_len64.ptr(), d_prefix.ptr(), n + 1);
    launch((u64)G + 1, CombineGraphFunctor{d_uoff.ptr(), G, d_prefix.ptr(), d_total.ptr(), d_gkey.ptr(), d_gval.ptr()});
    sort_pairs_u64_u32(d_gkey, d_gval, (u64)G + 1, 47, 0, 0, &sort_graphs);
    launch((u64)G + 1, CombineRankFunctor{d_gval.ptr(), G, d_uoff.ptr(), d_max.ptr(), d_max_ranked.ptr(), d_count_ranked.ptr()});
    exclusive_scan_u64(d_max_ranked.ptr(), d_offset_ranked.ptr(), (u64)G + 1);
    exclusive_scan_u64(d_count_ranked.ptr(), d_base_ranked.ptr(), (u64)G + 1);
    launch(G, CombineOffsetsFunctor{d_gval.ptr(), d_max_ranked.ptr(), d_offset_ranked.ptr(), d_base_ranked.ptr(), d_rank_of.ptr(), d_offset_of.ptr(), d_base_of.ptr(), d_err.ptr()});
    launch(nlp, CombineLinkFunctor{d_links.ptr(), nl, d_loff.ptr(), d_uoff.ptr(), G, n, d_base_of.ptr(), d_global.ptr(), d_link_graph.ptr(), d_lkey.ptr(), d_lval.ptr(), d_err.ptr()});
    launch(n, CompInitFunctor{d_parent.ptr()});
    launch(nlp, CompCensusFunctor{d_global.ptr(), n32, nullptr, comp_key_bits, d_deg.ptr(), d_target.ptr(), d_notself.ptr(), d_parent.ptr(), d_ckey.ptr(), d_ckey_unitig.ptr(),
                                  d_cerr.ptr(), d_hdr.ptr()});
    launch(n, CompRootsFunctor{d_parent.ptr(), nullptr, n32, d_deg.ptr(), d_target.ptr(), d_notself.ptr(), d_is_root.ptr(), d_flags.ptr(), d_roots_err.ptr()});
    launch(n + 1, CombinePrintedFunctor{n, d_number.ptr(), d_graph_of.ptr(), d_offset_of.ptr(), d_pkey.ptr(), d_pval.ptr()});
    sort_pairs_u64_u32(d_pkey, d_pval, n + 1, 32, 0, 0, &sort_printed);
    launch(n + 1, CombineDuplicateFunctor{n, d_pkey.ptr(), d_pval.ptr(), d_graph_of.ptr(), d_number.ptr(), d_err.ptr()});
    launch(G, CombineRecordsFunctor{d_gval.ptr(), d_uoff.ptr(), d_loff.ptr(), d_total.ptr(), d_max.ptr(), d_offset_of.ptr(), d_flags.ptr(), d_records.ptr()});
    launch(n, CombineUnitigOutFunctor{d_uoff.ptr(), d_graph_of.ptr(), d_number.ptr(), d_len.ptr(), d_printed.ptr(), p_rd, p_has, p_type, d_flags.ptr(), d_offset_of.ptr(),
                                      d_base_of.ptr(), n, d_unitigs_out.ptr()});
    sort_pairs_u64_u32(d_lkey, d_lval, nlp, link_bits, 0, 0, &sort_links);
    launch(nlp, CombineLinkOutFunctor{d_lval.ptr(), d_links.ptr(), d_link_graph.ptr(), d_uoff.ptr(), d_number.ptr(), d_offset_of.ptr(), nl, d_links_out.ptr()});
    meter.end();

    u64 err[3] = {~0ULL, ~0ULL, ~0ULL};
    out->clusters.resize(G);
    {
        ReadBatch rb;
        rb.add(err, d_err.ptr(), sizeof err); rb.add(out->clusters.data(), d_records.ptr(), (u64)G * sizeof(CombineClusterRecord));
        rb.run();
    }
    if (err[COMBINE_BAD_LINK] < nl) {
        const u64 i = err[COMBINE_BAD_LINK];
        const u32 g = (u32)(std::upper_bound(in.link_off, in.link_off + G + 1, i) - in.link_off) - 1;
        throw DeviceError(combine_bad_link_message(g, i - in.link_off[g], in.links[i].a, in.links[i].b, in.unitig_off[g + 1] - in.unitig_off[g]));
    }
    if (err[COMBINE_DUPLICATE] != ~0ULL) throw DeviceError(combine_duplicate_message((u32)(err[COMBINE_DUPLICATE] >> 32), (u32)err[COMBINE_DUPLICATE]));
    if (err[COMBINE_OVERFLOW] < G) {
        const CombineClusterRecord& c = out->clusters[(size_t)err[COMBINE_OVERFLOW]];
        throw DeviceError(combine_overflow_message(c.input_index, c.offset, c.max_number));
    }
    out->unitigs.resize(n); out->links.resize(nl);
    copy_d2h_async(out->unitigs.data(), d_unitigs_out.ptr(), n * sizeof(CombineUnitigRecord));
    copy_d2h_async(out->links.data(), d_links_out.ptr(), nl * sizeof(Link));
    meter.sync_copies();
    out->stats = meter.stats();
}
