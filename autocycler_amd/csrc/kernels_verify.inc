// ac_verify_graph: the size-independent properties of a finished unitig graph, checked ON THE DEVICE behind the C ABI (SURVEY.md §8 row
// f-4: "round-trip verifier at scale") — part of graph_build.hip (included inside namespace ac; not a translation unit of its own).
//
// What the reference's own tests hold a compress result to (tests.rs:108-127: save -> load -> save, decompress == input) plus the
// invariants it asserts at run time, restated as data-parallel checks over the result arrays:
//   * reconstruct_original_sequences (unitig_graph.rs:362-400, decompress.rs:83-105): every path spells its input sequence base for base
//     (forward entries read the unitig left to right, reverse entries its reverse complement: unitig.rs:174-182);
//   * check_links (unitig_graph.rs:752-793): every link has its reverse-complement mirror (b- -> a-), no link twice; every step of every
//     path is a link (get_unitig_path_for_sequence only ever moves along forward_next / reverse_next, unitig_graph.rs:447-465);
//   * depth == number of path occurrences (unitig.rs:149-156; from_gfa_lines recomputes it that way, unitig_graph.rs:151-174);
//   * renumber_unitigs order (unitig_graph.rs:295-315): length descending, forward sequence ascending, depth descending — a total
//     order, so the adjacent pairs decide;
//   * the printed statistics (unitig_graph.rs:474-516): total_length == sum of lengths, link_count().1 == (links + self-mirror links) / 2.
// Round 6 — the three ORDER-SENSITIVE guarantees of the reference, so that a graph too large for the oracle is checked as "the reference's
// graph", not only as "lossless and consistent":
//   * maximality (unitig_graph.rs:192-223): a unitig only ends where the walk had to stop.  For a link a -> b that is a's only successor and
//     b's only predecessor the stop must be one of the walk's break cases: the end of a / the start of b lies on a sequence-strand end
//     (first_position of rc X / of Y: a path ends with a or starts with -a; a path starts with b or ends with -b), or the `seen` test
//     (Y = rc X: b == -a; the walk meeting its own seed: b == a).  Anything else is a unitig cut in two.
//   * expand_repeats at its fixed point (graph_simplification.rs:26-40 loops until a pass shifts nothing): every junction is re-evaluated
//     with the reference's candidate test (get_exclusive_inputs / _outputs :233-280, the fixed starts / ends :190-230) and clamps
//     (avoid_zero_len_unitigs :145-161, avoid_start_of_path :164-181) and must shift 0.  In closed form a junction would still shift iff
//     the sources' facing bases all agree, (shortest source - 1) / (1 or 2 with a unitig on both strands) >= 1, and the destination's
//     smallest position on that strand is >= 2; the positions are those from_gfa_lines rebuilds from the paths (unitig_graph.rs:151-174).
//   * L-line order = get_links_for_gfa (unitig_graph.rs:333-350): unitigs ascending, forward_next before reverse_next, and inside a list
//     create_links' push order (:248-286): forward_next b+ .. then b- ..; reverse_next a'- (seed a' <= a), b+ .., a'- (seed a' > a), each
//     class ascending in SEED number.  The seed numbers come with a built graph (FinalGraph::seed_index); a graph reloaded from a GFA has
//     none, and only the part of the order that does not need them is checked (report.checks says which).
// The graph's arrays come from the host blocks of the handle (a verifier reads what the caller would write to the GFA, not the
// builder's device state: it also checks graphs loaded from a GFA, ac_graph_from_gfa).
enum VerifyFlag : u32 {
    VF_UNITIG = 1, VF_ORDER = 2, VF_LINK_RANGE = 4, VF_LINK_DUP = 8, VF_LINK_MIRROR = 16, VF_PATH_RANGE = 32, VF_PATH_STEP = 64,
    VF_PATH_LEN = 128, VF_SPELL = 256, VF_DEPTH = 512, VF_STATS = 1024, VF_LINK_ORDER = 2048, VF_MAXIMAL = 4096, VF_EXPAND = 8192
};
// report.checks: which of the round-6 checks ran (the topology checks need links in range; the fixed-point check needs valid unitig ranges and
// paths that add up; the in-class part of the link order needs seed numbers)
enum VerifyCheck : u32 { VC_LINK_ORDER = 1, VC_LINK_ORDER_SEEDS = 2, VC_MAXIMAL = 4, VC_EXPAND = 8 };
// err[0] = flags; err[1 + c] = smallest index that failed check class c (unitig, link, path entry, sequence, base, junction = 2 * unitig + side) — all ones: none
struct VerifyErr {
    u64* w;
    AC_D void fail(u32 flag, int cls, u64 index) const { atomic_or64(&w[0], (u64)flag); atomic_min64(&w[1 + cls], index); }
};
struct VerifyUnitigFunctor {      // lengths, sequence ranges, renumber_unitigs order (adjacent pairs)
    const u8* seq; u64 seq_total; const u64* beg; const u32* len; const double* depth; u64 U; VerifyErr e;
    AC_D void operator()(u64 i) const {
        const u64 a = len[i];
        if (a == 0 || beg[i] + a > seq_total) { e.fail(VF_UNITIG, 0, i); return; }
        if (i + 1 >= U) return;
        const u64 b = len[i + 1];
        if (b > a) { e.fail(VF_ORDER, 0, i); return; }
        if (b < a || beg[i + 1] + b > seq_total) return;
        const u8* x = seq + beg[i]; const u8* y = seq + beg[i + 1];
        for (u64 j = 0; j < a; j++) {
            if (x[j] < y[j]) return;
            if (x[j] > y[j]) { e.fail(VF_ORDER, 0, i); return; }
        }
        if (depth[i] < depth[i + 1]) e.fail(VF_ORDER, 0, i);      // equal length, equal sequence: the deeper one first
    }
};
// A link as one sortable word: (signed a + 2^31) << 32 | (signed b + 2^31), signed = +number on the forward strand, -number on the reverse.
AC_HD u64 link_code(int64_t a, int64_t b) { return ((u64)(a + ((int64_t)1 << 31)) << 32) | (u64)(b + ((int64_t)1 << 31)); }
// A unitig strand as a node index in the order the sorted link codes have them: -U .. -1, then +1 .. +U.
AC_HD u64 verify_node(int64_t s, u64 U) { return s < 0 ? (u64)((int64_t)U + s) : U + (u64)s - 1; }
struct VerifyLinkCodeFunctor {
    const Link* links; u64 U; u64* code; u32* vals; u32* self_mirror; VerifyErr e; u32* outdeg;
    AC_D void operator()(u64 i) const {
        const Link l = links[i];
        vals[i] = (u32)i;
        if (l.na() < 1 || l.na() > U || l.nb() < 1 || l.nb() > U) { e.fail(VF_LINK_RANGE, 1, i); code[i] = ~0ULL; return; }
        const int64_t a = l.a, b = l.b;
        code[i] = link_code(a, b);
        atomic_add32(&outdeg[verify_node(a, U)], 1u);
        if (a == -b) atomic_add32(self_mirror, 1u);      // a+ -> a- / a- -> a+: its own mirror
    }
};
AC_D bool link_set_has(const u64* sorted, u64 n, u64 c) {
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (sorted[mid] < c) lo = mid + 1; else hi = mid; }
    return lo < n && sorted[lo] == c;
}
struct VerifyLinkSetFunctor {      // over the sorted codes: no duplicates, every link's mirror (b- -> a-) is a link
    const u64* sorted; const u32* at; u64 n; VerifyErr e;
    AC_D void operator()(u64 i) const {
        const u64 c = sorted[i];
        if (c == ~0ULL) return;
        if (i + 1 < n && sorted[i + 1] == c) e.fail(VF_LINK_DUP, 1, at[i]);
        const int64_t a = (int64_t)(c >> 32) - ((int64_t)1 << 31), b = (int64_t)(c & 0xFFFFFFFFULL) - ((int64_t)1 << 31);
        if (!link_set_has(sorted, n, link_code(-b, -a))) e.fail(VF_LINK_MIRROR, 1, at[i]);
    }
};
struct VerifyPathLenFunctor {      // entry -> its unitig's length; occurrences per unitig
    const int32_t* path; u64 n_ent; u64 U; const u32* len; u64* elen; u32* occ; VerifyErr e;
    AC_D void operator()(u64 j) const {
        if (j == n_ent) { elen[j] = 0; return; }      // sentinel: the exclusive scan then ends with the total
        const int32_t p = path[j];
        const u64 idx = (u64)(p < 0 ? -(int64_t)p : (int64_t)p) - 1;
        if (p == 0 || idx >= U) { e.fail(VF_PATH_RANGE, 2, j); elen[j] = 0; return; }
        elen[j] = len[idx];
        atomic_add32(&occ[idx], 1u);
    }
};
AC_D u64 upper_bound_u64(const u64* a, u64 n, u64 v) {      // number of entries <= v
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (a[mid] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}
struct VerifyPathStepFunctor {      // consecutive entries of one sequence's path must be a link
    const int32_t* path; u64 n_ent; const u64* off; u32 n_seqs; const u64* sorted; u64 n_links; VerifyErr e;
    AC_D void operator()(u64 j) const {
        if (j + 1 >= n_ent) return;
        const u64 s = upper_bound_u64(off, (u64)n_seqs + 1, j) - 1;      // the sequence entry j belongs to
        if (j + 1 >= off[s + 1]) return;                                  // the last entry of its path
        const int32_t a = path[j], b = path[j + 1];
        if (a == 0 || b == 0) return;                                     // (reported by the range check)
        if (!link_set_has(sorted, n_links, link_code((int64_t)a, (int64_t)b))) e.fail(VF_PATH_STEP, 2, j);
    }
};
struct VerifyPathSumFunctor {      // a path adds up to its sequence's length (the P line's LN tag, unitig_graph.rs:352-360)
    const u64* csum; const u64* off; const u32* seq_len; VerifyErr e;
    AC_D void operator()(u64 s) const { if (csum[off[s + 1]] - csum[off[s]] != (u64)seq_len[s]) e.fail(VF_PATH_LEN, 3, s); }
};
// Decompress identity, VERIFY_SPAN bases per thread.  With every path adding up to its sequence (checked before this runs) base g of
// the job — sequences one behind the other — lies in path entry upper_bound(csum, g) - 1, and in sequence upper_bound(sbase, g) - 1.
static const u32 VERIFY_SPAN = 32;
AC_HD u8 verify_comp(u8 c) { return c == 'A' ? 'T' : (c == 'C' ? 'G' : (c == 'G' ? 'C' : (c == 'T' ? 'A' : 'N'))); }      // (misc.rs:358-367)
struct VerifySpellFunctor {
    const u8* text; const u64* seq_off; const u64* sbase; u32 n_seqs; int half_k; u64 n_bases;
    const int32_t* path; const u64* csum; u64 n_ent; const u8* useq; const u64* beg; const u32* len; VerifyErr e;
    AC_D void operator()(u64 t) const {
        u64 g = t * VERIFY_SPAN;
        const u64 g_end = g + VERIFY_SPAN < n_bases ? g + VERIFY_SPAN : n_bases;
        if (g >= g_end) return;
        u64 j = upper_bound_u64(csum, n_ent + 1, g) - 1;
        u64 s = upper_bound_u64(sbase, (u64)n_seqs + 1, g) - 1;
        while (g < g_end) {
            while (csum[j + 1] <= g) j++;          // (entries of length zero do not exist: checked)
            while (sbase[s + 1] <= g) s++;
            const int32_t p = path[j];
            const u64 idx = (u64)(p < 0 ? -(int64_t)p : (int64_t)p) - 1;
            const u64 L = len[idx], within = g - csum[j];
            const u8 got = p > 0 ? useq[beg[idx] + within] : verify_comp(useq[beg[idx] + (L - 1 - within)]);
            const u8 want = text[seq_off[s] + (u64)half_k + (g - sbase[s])];
            if (got != want) { e.fail(VF_SPELL, 4, g); return; }
            g++;
        }
    }
};
struct VerifyDepthFunctor {
    const double* depth; const u32* occ; VerifyErr e;
    AC_D void operator()(u64 i) const { if (depth[i] != (double)occ[i]) e.fail(VF_DEPTH, 0, i); }
};

// ---- round 6: maximality, expand_repeats' fixed point, L-line order ---------------------------------------------------------------------
// The successors of a unitig strand: a stretch of the sorted link codes (noff = exclusive scan of the out-degrees in node order; links
// out of range sort behind everything).  With every link's mirror present (checked above) the predecessors of s are the flipped
// successors of -s.
struct VerifyAdj {
    const u64* sorted; const u32* noff; u64 U;
    AC_HD u32 deg(int64_t s) const { const u64 n = verify_node(s, U); return noff[n + 1] - noff[n]; }
    AC_HD u32 first(int64_t s) const { return noff[verify_node(s, U)]; }
    AC_HD int64_t target(u32 i) const { return (int64_t)(sorted[i] & 0xFFFFFFFFULL) - ((int64_t)1 << 31); }
};
struct VerifyPathEndsFunctor {      // fs0 / fe0: the unitig's forward start / end lies on the end of a sequence strand (graph_simplification.rs:197-206)
    const int32_t* path; const u64* off; u64 U; u8* fs0; u8* fe0;
    AC_HD void operator()(u64 s) const {
        const u64 b = off[s], e = off[s + 1];
        if (b >= e) return;
        const int32_t first = path[b], last = path[e - 1];
        const u64 fi = (u64)(first < 0 ? -(int64_t)first : (int64_t)first) - 1, li = (u64)(last < 0 ? -(int64_t)last : (int64_t)last) - 1;
        if (first != 0 && fi < U) { if (first > 0) fs0[fi] = 1; else fe0[fi] = 1; }
        if (last != 0 && li < U) { if (last > 0) fe0[li] = 1; else fs0[li] = 1; }
    }
};
struct VerifyFixedFunctor {         // ... and their one-step neighbours (:211-227)
    VerifyAdj A; const u8* fs0; const u8* fe0; u8* fixed_start; u8* fixed_end;
    AC_HD void operator()(u64 u) const {
        const int64_t num = (int64_t)u + 1;
        if (fs0[u]) {      // upstream of a fixed start: forward_prev(u) = the flipped successors of u-
            fixed_start[u] = 1;
            const u32 b = A.first(-num), n = A.deg(-num);
            for (u32 i = 0; i < n; i++) { const int64_t up = -A.target(b + i); if (up > 0) fixed_end[up - 1] = 1; else fixed_start[-up - 1] = 1; }
        }
        if (fe0[u]) {      // downstream of a fixed end
            fixed_end[u] = 1;
            const u32 b = A.first(num), n = A.deg(num);
            for (u32 i = 0; i < n; i++) { const int64_t dn = A.target(b + i); if (dn > 0) fixed_start[dn - 1] = 1; else fixed_end[-dn - 1] = 1; }
        }
    }
};
struct VerifyMaximalFunctor {       // over the sorted links
    VerifyAdj A; const u32* at; u64 n_links; const u8* fs0; const u8* fe0; VerifyErr e;
    AC_HD void operator()(u64 i) const {
        const u64 c = A.sorted[i];
        if (c == ~0ULL) return;
        const int64_t a = (int64_t)(c >> 32) - ((int64_t)1 << 31), b = (int64_t)(c & 0xFFFFFFFFULL) - ((int64_t)1 << 31);
        if (A.deg(a) != 1 || A.deg(-b) != 1) return;                     // a branches, or b has another way in
        if (a == b || a == -b) return;                                   // the `seen` test: the walk met its own seed / Y = rc X
        const bool a_ends_strand = a > 0 ? fe0[a - 1] : fs0[-a - 1];      // first_position(rc X)
        const bool b_starts_strand = b > 0 ? fs0[b - 1] : fe0[-b - 1];    // first_position(Y)
        if (!a_ends_strand && !b_starts_strand) e.fail(VF_MAXIMAL, 6, at[i]);      // (a slot of its own: only reported when the link set holds)
    }
};
struct VerifyPathPosFunctor {       // smallest position of each unitig strand, as add_positions_from_path would give them (unitig_graph.rs:151-174)
    const int32_t* path; u64 n_ent; const u64* off; u32 n_seqs; const u64* csum; const u32* seq_len; const u32* ulen; u32* minf; u32* minr;
    AC_D void operator()(u64 j) const {
        const u64 s = upper_bound_u64(off, (u64)n_seqs + 1, j) - 1;
        const int32_t p = path[j];
        const u64 idx = (u64)(p < 0 ? -(int64_t)p : (int64_t)p) - 1;
        const u64 o = csum[j] - csum[off[s]], L = seq_len[s], back = L - o - (u64)ulen[idx];      // forward path / reverse path offset
        if (p > 0) { atomic_min32(&minf[idx], (u32)o); atomic_min32(&minr[idx], (u32)back); }
        else { atomic_min32(&minr[idx], (u32)o); atomic_min32(&minf[idx], (u32)back); }
    }
};
struct VerifyExpandFunctor {        // junction (u, side): side 0 = the exclusive inputs of u, 1 = its exclusive outputs
    VerifyAdj A; const u8* fixed_start; const u8* fixed_end; const u8* useq; const u64* beg; const u32* len; const u32* minf; const u32* minr; VerifyErr e;
    AC_HD void operator()(u64 idx) const {
        const u64 u = idx >> 1;
        const bool inputs = (idx & 1) == 0;
        const int64_t num = (int64_t)u + 1;
        const int64_t from = inputs ? -num : num;
        const u32 n = A.deg(from), b0 = A.first(from);
        if (n < 2 || n > 5 || (inputs ? fixed_start[u] : fixed_end[u])) return;
        int64_t nums[5]; u32 min_len = 0xFFFFFFFFu; bool dup = false, same = true; u8 c0 = 0;
        for (u32 i = 0; i < n; i++) {
            // inputs: the source strand p = the flipped successor of u-; it must lead to u+ only.  outputs: the source strand s = a successor
            // of u+; u+ must be its only way in, i.e. -s leads to u- only.
            const int64_t t = A.target(b0 + i), src = inputs ? -t : t;
            if (A.deg(inputs ? src : -src) != 1) return;
            const u64 w = (u64)(src < 0 ? -src : src) - 1;
            if (w == u) return;
            if (inputs ? ((src > 0 && fixed_end[w]) || (src < 0 && fixed_start[w])) : ((src > 0 && fixed_start[w]) || (src < 0 && fixed_end[w]))) return;
            for (u32 q = 0; q < i; q++) if (nums[q] == (int64_t)w) dup = true;
            nums[i] = (int64_t)w;
            const u32 l = len[w];
            if (l < min_len) min_len = l;
            // the base of the source that faces u: inputs = the last base of p, outputs = the first base of s (strand sequences)
            const bool at_end = inputs == (src > 0);
            const u8 raw = useq[beg[w] + (at_end ? (u64)l - 1 : 0)];
            const u8 c = src > 0 ? raw : verify_comp(raw);
            if (i == 0) c0 = c; else if (c != c0) same = false;
        }
        if (!same) return;                                            // get_common_end_seq / _start_seq: empty
        if ((min_len - 1) / (dup ? 2u : 1u) < 1) return;              // avoid_zero_len_unitigs leaves nothing
        if ((inputs ? minf[u] : minr[u]) < 2) return;                 // avoid_start_of_path leaves nothing
        e.fail(VF_EXPAND, 5, idx);
    }
};
// L-line order, one thread per link that opens a group (the links of one unitig strand): groups ascending, and inside a group
// create_links' push order.  seed: optional (FinalGraph::seed_index).
struct VerifyLinkOrderFunctor {
    const Link* links; u64 n_links; u64 U; const u32* seed; VerifyErr e;
    AC_HD static u64 grp(const Link& l) { return 2 * (u64)l.na() + (l.a_fwd() ? 0 : 1); }
    AC_HD void operator()(u64 i) const {
        const Link l0 = links[i];
        if (l0.na() < 1 || l0.na() > U || l0.nb() < 1 || l0.nb() > U) return;
        const u64 g = grp(l0);
        if (i > 0) {
            const Link lp = links[i - 1];
            if (lp.na() >= 1 && lp.na() <= U) {
                const u64 gp = grp(lp);
                if (gp == g) return;                                  // not the first of its group
                if (gp > g) { e.fail(VF_LINK_ORDER, 1, i); return; }   // groups out of order (a group cut in two shows up as this as well)
            }
        }
        // class of a target: forward_next: b+ = 0, b- = 1; reverse_next: a'- with seed a' <= a = 0, b+ = 1, a'- with seed a' > a = 2
        u32 prev_cls = 0, prev_seed = 0; bool have_prev = false, seen_plus = false, minus_after_plus = false;
        for (u64 j = i; j < n_links && j < i + 6; j++) {
            const Link l = links[j];
            if (l.na() < 1 || l.na() > U || l.nb() < 1 || l.nb() > U || grp(l) != g) break;
            if (j == i + 5) { e.fail(VF_LINK_ORDER, 1, j); return; }      // a k-mer has at most five successors (kmer_graph.rs:136-150)
            u32 cls;
            if (l0.a_fwd()) cls = l.b_fwd() ? 0u : 1u;
            else if (l.b_fwd()) { cls = 1u; if (minus_after_plus) { e.fail(VF_LINK_ORDER, 1, j); return; } seen_plus = true; }
            else if (seed) cls = seed[l.nb() - 1] <= seed[l.na() - 1] ? 0u : 2u;
            else { cls = seen_plus ? 2u : 0u; if (seen_plus) minus_after_plus = true; }
            if (have_prev && cls < prev_cls) { e.fail(VF_LINK_ORDER, 1, j); return; }
            if (seed) {
                const u32 sd = seed[l.nb() - 1];
                if (have_prev && cls == prev_cls && sd <= prev_seed) { e.fail(VF_LINK_ORDER, 1, j); return; }
                prev_seed = sd;
            }
            prev_cls = cls; have_prev = true;
        }
    }
};

// d_text: the job's text on the device in the layout of include/autocycler_hip.h ('$' + padded sequences each followed by '$'); the
// bases of sequence s are text[off[s] + k/2 .. off[s] + k/2 + len[s]) whatever end repair made of the padding around them.
void verify_graph_device(const FinalGraph& g, const uint8_t* d_text, uint64_t n_text, const std::vector<uint64_t>& off,
                         const std::vector<uint32_t>& len, VerifyReport* rep) {
    const double t0 = now_s();
    const u32 n_seqs = (u32)off.size();
    *rep = VerifyReport();
    if (n_seqs == 0 || g.path_off.size() != (size_t)n_seqs + 1) throw DeviceError("verify: the graph holds no paths for these sequences");
    if (!g.seq_begin || !g.seq_len || !g.depth || (g.n_links && !g.links) || (g.n_path && !g.path)) throw DeviceError("verify: the graph keeps no host arrays");
    if (g.k == 0 || (g.k & 1) == 0) throw DeviceError("verify: the graph has no k-mer size");
    const u64 U = g.n_unitigs, n_links = g.n_links, n_ent = g.n_path;
    if (U == 0) throw DeviceError("verify: the graph has no unitigs");
    const int h = (int)(g.k / 2);
    u64 n_bases = 0;
    std::vector<u64> sbase((size_t)n_seqs + 1);
    for (u32 s = 0; s < n_seqs; s++) {
        if (off[s] + (u64)len[s] + 2 * (u64)h + 1 > n_text) throw DeviceError("verify: sequence table beyond the text");
        sbase[s] = n_bases; n_bases += len[s];
    }
    sbase[n_seqs] = n_bases;
    u64 seq_total = 0, total_len = 0;
    for (u64 i = 0; i < U; i++) { seq_total = std::max<u64>(seq_total, g.seq_begin[i] + g.seq_len[i]); total_len += g.seq_len[i]; }
    if (seq_total > g.seq_block.bytes && g.seq_block.bytes) seq_total = g.seq_block.bytes;      // (a range beyond the block is reported per unitig)
    // offsets that do not ascend from 0 to the number of entries: every kernel below indexes the entries through them, so the run ends here
    // with the first sequence whose range is no range (the last one when the offsets end beside the entries)
    u32 host_flags = 0;
    u64 bad_seq = ~0ULL;
    if (g.path_off[n_seqs] != n_ent) bad_seq = n_seqs - 1;
    for (u32 s = n_seqs; s-- > 0;) if (g.path_off[s + 1] < g.path_off[s]) bad_seq = s;
    if (g.path_off[0] != 0) bad_seq = 0;
    if (bad_seq != ~0ULL) host_flags |= VF_PATH_LEN;
    if (host_flags & VF_PATH_LEN) { rep->failed = host_flags; rep->first_bad_sequence = bad_seq; rep->seconds = now_s() - t0; return; }

    Arena::device().reset();
    DBuf<u64> err(8);
    { const u64 init[8] = {0, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL}; copy_h2d(err.ptr(), init, sizeof init); }
    VerifyErr e{err.ptr()};
    // the graph's arrays, as the caller holds them
    DBuf<u8> useq(seq_total + 1); DBuf<u64> beg(U); DBuf<u32> ulen(U); DBuf<double> depth(U);
    copy_h2d(useq.ptr(), g.seq_block.p, seq_total);
    copy_h2d(beg.ptr(), g.seq_begin, U * 8); copy_h2d(ulen.ptr(), g.seq_len, U * 4); copy_h2d(depth.ptr(), g.depth, U * 8);
    launch(U, VerifyUnitigFunctor{useq.ptr(), seq_total, beg.ptr(), ulen.ptr(), depth.ptr(), U, e});
    // links
    DBuf<u64> code(n_links + 1); DBuf<u32> at(n_links + 1), self_mirror(1, true);
    DBuf<u32> outdeg(2 * U + 1, true), noff(2 * U + 1), d_seed(g.seed_index ? U : 0);
    if (g.seed_index) copy_h2d(d_seed.ptr(), g.seed_index, U * 4);
    if (n_links) {
        DBuf<Link> dl(n_links);
        copy_h2d(dl.ptr(), g.links, n_links * sizeof(Link));
        launch(n_links, VerifyLinkCodeFunctor{dl.ptr(), U, code.ptr(), at.ptr(), self_mirror.ptr(), e, outdeg.ptr()});
        sort_pairs_u64_u32(code, at, n_links, 64);
        launch(n_links, VerifyLinkSetFunctor{code.ptr(), at.ptr(), n_links, e});
        launch(n_links, VerifyLinkOrderFunctor{dl.ptr(), n_links, U, g.seed_index ? d_seed.ptr() : nullptr, e});      // (the links as the caller holds them: the L lines)
    }
    exclusive_scan_u32(outdeg.ptr(), noff.ptr(), 2 * U + 1);      // ([2U] = 0: ends with the number of links in range)
    const VerifyAdj adj{code.ptr(), noff.ptr(), U};
    // paths
    DBuf<int32_t> path(n_ent + 1); DBuf<u64> poff((size_t)n_seqs + 1), elen(n_ent + 1), csum(n_ent + 1); DBuf<u32> occ(U, true), slen(n_seqs);
    copy_h2d(path.ptr(), g.path, n_ent * 4);
    copy_h2d(poff.ptr(), g.path_off.data(), ((size_t)n_seqs + 1) * 8);
    copy_h2d(slen.ptr(), len.data(), (size_t)n_seqs * 4);
    launch(n_ent + 1, VerifyPathLenFunctor{path.ptr(), n_ent, U, ulen.ptr(), elen.ptr(), occ.ptr(), e});
    exclusive_scan_u64(elen.ptr(), csum.ptr(), n_ent + 1);
    launch(n_ent, VerifyPathStepFunctor{path.ptr(), n_ent, poff.ptr(), n_seqs, code.ptr(), n_links, e});
    launch(n_seqs, VerifyPathSumFunctor{csum.ptr(), poff.ptr(), slen.ptr(), e});
    launch(U, VerifyDepthFunctor{depth.ptr(), occ.ptr(), e});
    // maximality: path ends -> strand-end flags; every sole link between two unitigs must be one of the walk's break cases
    DBuf<u8> fs0(U, true), fe0(U, true), fixed_start(U, true), fixed_end(U, true);
    launch(n_seqs, VerifyPathEndsFunctor{path.ptr(), poff.ptr(), U, fs0.ptr(), fe0.ptr()});
    if (n_links) launch(n_links, VerifyMaximalFunctor{adj, at.ptr(), n_links, fs0.ptr(), fe0.ptr(), e});
    std::vector<u64> h_err = to_host(err, 8);
    const u32 sm = read_scalar(self_mirror.ptr());
    // the decompress identity needs every path to add up to its sequence and every entry to name a unitig with a valid range
    u64 bases_checked = 0;
    u32 checks = VC_LINK_ORDER | (g.seed_index ? VC_LINK_ORDER_SEEDS : 0);
    const bool link_set_ok = !(h_err[0] & (VF_LINK_RANGE | VF_LINK_DUP | VF_LINK_MIRROR));      // (predecessors are read as flipped successors)
    if (link_set_ok) checks |= VC_MAXIMAL;
    if (!(h_err[0] & (VF_PATH_LEN | VF_PATH_RANGE | VF_UNITIG))) {
        if (link_set_ok) {      // expand_repeats' fixed point: no junction would shift anything
            DBuf<u32> minf(U), minr(U);
            minf.fill_bytes(0xFF); minr.fill_bytes(0xFF);
            if (n_ent) launch(n_ent, VerifyPathPosFunctor{path.ptr(), n_ent, poff.ptr(), n_seqs, csum.ptr(), slen.ptr(), ulen.ptr(), minf.ptr(), minr.ptr()});
            launch(U, VerifyFixedFunctor{adj, fs0.ptr(), fe0.ptr(), fixed_start.ptr(), fixed_end.ptr()});
            launch(2 * U, VerifyExpandFunctor{adj, fixed_start.ptr(), fixed_end.ptr(), useq.ptr(), beg.ptr(), ulen.ptr(), minf.ptr(), minr.ptr(), e});
            checks |= VC_EXPAND;
        }
        DBuf<u64> d_off(n_seqs), d_sbase((size_t)n_seqs + 1);
        copy_h2d(d_off.ptr(), off.data(), (size_t)n_seqs * 8);
        copy_h2d(d_sbase.ptr(), sbase.data(), ((size_t)n_seqs + 1) * 8);
        launch((n_bases + VERIFY_SPAN - 1) / VERIFY_SPAN, VerifySpellFunctor{d_text, d_off.ptr(), d_sbase.ptr(), n_seqs, h, n_bases, path.ptr(), csum.ptr(), n_ent,
                                                                             useq.ptr(), beg.ptr(), ulen.ptr(), e});
        h_err = to_host(err, 8);
        bases_checked = n_bases;
    }
    u32 flags = (u32)h_err[0] | host_flags;
    if (!link_set_ok) { flags &= ~(u32)(VF_MAXIMAL | VF_EXPAND); h_err[6] = ~0ULL; }      // (not checked: the link set itself is broken, and reported as that)
    else h_err[2] = std::min(h_err[2], h_err[7]);
    // the printed statistics (unitig_graph.rs:474-516; compress.rs:152: kmers.len() is twice the pre-simplification total length)
    if (g.post.total_length != total_len || g.post.unitigs != U || g.pre.unitigs != U || g.post.links_one_way != (n_links + sm) / 2 ||
        (g.n_kmers && g.n_kmers != 2 * g.pre.total_length))
        flags |= VF_STATS;
    rep->failed = flags;
    rep->first_bad_unitig = h_err[1]; rep->first_bad_link = h_err[2]; rep->first_bad_path_entry = h_err[3];
    rep->first_bad_sequence = h_err[4]; rep->first_bad_base = h_err[5]; rep->first_bad_junction = h_err[6]; rep->checks = checks;
    rep->unitigs = U; rep->links = n_links; rep->path_entries = n_ent; rep->bases_checked = bases_checked; rep->self_mirror_links = sm;
    stream_sync();
    rep->seconds = now_s() - t0;
}

// reconstruct_original_sequences (unitig_graph.rs:362-400; decompress.rs:83-105) on the device: all sequences of the graph spelled from
// their paths into one buffer, sequence s at out[sbase[s] .. sbase[s + 1]) — the writing twin of VerifySpellFunctor (f-4: what `autocycler
// decompress` does one sequence after the other on the host).  out: host memory of sum(lengths) bytes.
struct DecompressFunctor {
    const u64* sbase; u32 n_seqs; u64 n_bases; const int32_t* path; const u64* csum; u64 n_ent; const u8* useq; const u64* beg; const u32* len; u8* out;
    AC_D void operator()(u64 t) const {
        u64 g = t * VERIFY_SPAN;
        const u64 g_end = g + VERIFY_SPAN < n_bases ? g + VERIFY_SPAN : n_bases;
        if (g >= g_end) return;
        u64 j = upper_bound_u64(csum, n_ent + 1, g) - 1;
        while (g < g_end) {
            while (csum[j + 1] <= g) j++;
            const int32_t p = path[j];
            const u64 idx = (u64)(p < 0 ? -(int64_t)p : (int64_t)p) - 1;
            const u64 L = len[idx], within = g - csum[j];
            out[g] = p > 0 ? useq[beg[idx] + within] : verify_comp(useq[beg[idx] + (L - 1 - within)]);
            g++;
        }
    }
};
void decompress_device(const FinalGraph& g, const std::vector<uint32_t>& seq_len, uint8_t* out_host) {
    const u32 n_seqs = (u32)seq_len.size();
    if (n_seqs == 0 || g.path_off.size() != (size_t)n_seqs + 1) throw DeviceError("decompress: the graph holds no paths");
    if (!g.seq_begin || !g.seq_len || (g.n_path && !g.path)) throw DeviceError("decompress: the graph keeps no host arrays");
    const u64 U = g.n_unitigs, n_ent = g.n_path;
    u64 n_bases = 0, seq_total = 0;
    std::vector<u64> sbase((size_t)n_seqs + 1);
    for (u32 s = 0; s < n_seqs; s++) { sbase[s] = n_bases; n_bases += seq_len[s]; }
    sbase[n_seqs] = n_bases;
    for (u64 i = 0; i < U; i++) seq_total = std::max<u64>(seq_total, g.seq_begin[i] + g.seq_len[i]);
    Arena::device().reset();
    DBuf<u64> err(8);
    { const u64 init[8] = {0, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL, ~0ULL}; copy_h2d(err.ptr(), init, sizeof init); }
    VerifyErr e{err.ptr()};
    DBuf<u8> useq(seq_total + 1), out(n_bases + 1); DBuf<u64> beg(U), poff((size_t)n_seqs + 1), elen(n_ent + 1), csum(n_ent + 1), d_sbase((size_t)n_seqs + 1);
    DBuf<u32> ulen(U), occ(U, true), slen(n_seqs); DBuf<int32_t> path(n_ent + 1);
    copy_h2d(useq.ptr(), g.seq_block.p, seq_total); copy_h2d(beg.ptr(), g.seq_begin, U * 8); copy_h2d(ulen.ptr(), g.seq_len, U * 4);
    copy_h2d(path.ptr(), g.path, n_ent * 4); copy_h2d(poff.ptr(), g.path_off.data(), ((size_t)n_seqs + 1) * 8);
    copy_h2d(slen.ptr(), seq_len.data(), (size_t)n_seqs * 4); copy_h2d(d_sbase.ptr(), sbase.data(), ((size_t)n_seqs + 1) * 8);
    launch(n_ent + 1, VerifyPathLenFunctor{path.ptr(), n_ent, U, ulen.ptr(), elen.ptr(), occ.ptr(), e});
    exclusive_scan_u64(elen.ptr(), csum.ptr(), n_ent + 1);
    launch(n_seqs, VerifyPathSumFunctor{csum.ptr(), poff.ptr(), slen.ptr(), e});
    const std::vector<u64> h_err = to_host(err, 8);
    if (h_err[0]) throw DeviceError("decompress: the paths of the graph do not add up to its sequences (sequence " + std::to_string(h_err[4] == ~0ULL ? 0 : h_err[4] + 1) + ")");
    launch((n_bases + VERIFY_SPAN - 1) / VERIFY_SPAN, DecompressFunctor{d_sbase.ptr(), n_seqs, n_bases, path.ptr(), csum.ptr(), n_ent, useq.ptr(), beg.ptr(), ulen.ptr(), out.ptr()});
    copy_d2h(out_host, out.ptr(), n_bases);
    stream_sync();
}

