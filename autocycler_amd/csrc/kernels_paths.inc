// K10 path walk — part of graph_build.hip (included inside namespace ac; not a translation unit of its own).
// ---- K10: paths, depth and min positions (find_starting_unitig / get_next_unitig, unitig_graph.rs:407-465;
// simplify_seqs positions, unitig.rs:136-147) ------------------------------------------------------------------
// Every occurrence of a unitig's first k-mer is followed by the whole unitig (SURVEY App. A.3), so a sequence
// path is walked unitig by unitig: ONE table lookup locates the walker inside its first unitig, after that the
// next unitig (and its length) is wlinks[(current strand end)][next text symbol] — one gather, no hashing.  Thread tid
// owns the unitig heads that fall into text positions [tid*PC, (tid+1)*PC) and writes them to its own staging slots;
// an exclusive scan of the counts and a compaction put them in text order without a sort or a second walk.
// `t` is the text being walked (this rank's sequences), `g` the text the graph was built from (the same text for a
// single-device build, the union of all ranks' novel fragments for a sharded one): table slots point into `g`.
// Layouts that were measured and dropped (profiles/r03i..k_ab_knobs_configC.jsonl): one 128-byte record per unitig holding the
// successor words, the length AND the updated words (1.70 ms against 1.34 ms for the whole stage), the updated words alone in
// one 16-byte struct (1.95 ms), the read-only part alone in a record (1.39 ms).  The atomics keep invalidating whatever shares
// their line, so the three updated arrays stay apart from each other and from what is only read.  With the depth atomics
// switched off the stage takes 1.19 ms, without the position reads / updates 1.07 ms, without both 0.81 ms (AC_PATH_DIAG).
// Which (unitig, side) can ever be the DESTINATION of an expand_repeats shift?  The smallest positions the walk collects are
// only consulted for those (avoid_start_of_path, graph_simplification.rs:164-181, reads the destination's positions; the
// sources' words are only ever added to).  A superset from the links alone — the exclusive-input / exclusive-output test of
// graph_simplification.rs:233-280 without the fixed-start / fixed-end guards, which need the paths this walk is about to
// produce: side 0 = inputs (forward positions), side 1 = outputs (reverse positions).
AC_HD u32 idx_of(int32_t v) { return (u32)(v < 0 ? -v : v) - 1; }      // signed unitig number -> index
struct MaybeDestFunctor {
    const int32_t* links; u8* maybe;
    AC_HD static u64 row(int32_t v) { return ((u64)((u32)(v < 0 ? -v : v) - 1) * 2 + (v > 0 ? 0 : 1)) * 5; }
    AC_HD void operator()(u64 idx) const {
        const u32 x = (u32)(idx >> 1);
        const bool inputs = (idx & 1) == 0;
        const int32_t xnum = (int32_t)x + 1;
        const u64 mine = row(inputs ? -xnum : xnum);
        u32 n = 0;
        bool ok = true;
        for (int c = 0; c < 5; c++) {
            int32_t p = links[mine + (u64)c];
            if (p == 0) continue;
            n++;
            int32_t other = inputs ? -p : p;
            const u64 theirs = row(inputs ? other : -other);
            u32 m = 0; int32_t only = 0;
            for (int d = 0; d < 5; d++) { int32_t q = links[theirs + (u64)d]; if (q != 0) { m++; only = q; } }
            if (!(m == 1 && only == (inputs ? xnum : -xnum))) ok = false;
            if ((u32)(other < 0 ? -other : other) - 1 == x) ok = false;
        }
        maybe[idx] = (ok && n >= 2) ? 1 : 0;
    }
};
// The walk's successor table carries, next to the target and its length, whether the TARGET unitig may become an expand_repeats
// destination on its inputs side (bit 30 of the length word) / outputs side (bit 31): the walker then knows from the one load it
// does anyway whether the smallest positions of the unitig it steps into are wanted (it used to read a flag array per entry).
static const u32 WL_LEN_MASK = (1u << 30) - 1;
struct WlinkFlagFunctor {
    const u8* maybe; u64* wlinks; u32* err;      // maybe == nullptr: positions of every unitig are wanted
    AC_HD void operator()(u64 i) const {
        u64 wl = wlinks[i];
        int32_t val = (int32_t)(u32)wl;
        if (val == 0) return;
        u32 len = (u32)(wl >> 32);
        if (len > WL_LEN_MASK) { atomic_or32(err, 32u); return; }
        u64 rr = (u64)((u32)(val < 0 ? -val : val) - 1);
        u32 flags = maybe ? ((maybe[rr * 2] ? 1u : 0u) | (maybe[rr * 2 + 1] ? 2u : 0u)) : 3u;
        wlinks[i] = ((u64)(len | (flags << 30)) << 32) | (u64)(u32)val;
    }
};
// Round 6: the walk numbers the unitigs in TEXT order — u = the unitig's index in the novel list, i.e. the order in which the unitigs first
// appear in the text — and not in seed order.  A walker moves along the text, so the unitigs it steps through are mostly u, u + 1, u + 2, ...
// (the first occurrence created them in that order; later strains follow it between their variants): the rows of the successor table it
// reads lie next to each other instead of at random places of a table ordered by the rank of a unitig's smallest k-mer, and a stretch of
// consecutive numbers costs the depth counters two atomics instead of one per entry (PathWalkFunctor::WalkRun).  wl_text[(u * 2 + strand)
// * 5 + c] = [flags:2][length:30][signed (target's u + 1):32]: wlinks (seed order, LinksFunctor / WlinkFlagFunctor) permuted, targets renamed.
// "strand" and the SIGN of an entry are relative to the TEXT too: + = the unitig in the direction of its first occurrence, - = against it
// (the canonical strand — the one holding the smallest k-mer — is random along the text and would cut every stretch after a step or two).
// Everything the walk produces is in these numbers — path entries, depth, smallest positions — until walk_to_seed_order / the final
// numbering (FinalMetaFunctor's number table by u) turn them into what the tail works with.
struct WlinkTextOrderFunctor {
    const u64* wlinks; const u32* rank; const u32* order; const u8* uorient; u64* wl_text;
    u32* mf; u32* mr; u32 pos_init;      // ... and the value the smallest positions start from (exact: all ones; bounded: the bound, POS_BOUND set)
    AC_HD void operator()(u64 i) const {
        // row (u, rel): rel 0 = the unitig walked the way its FIRST OCCURRENCE lies in the text, 1 = against it — the walker's notion of strand
        // (uorient[r]: the unitig's own forward strand is that text orientation).  Signs of the targets likewise: a strain that follows the
        // first occurrence walks +u, +(u + 1), ... whatever strands the seed k-mers happen to make "forward".
        const u64 u = i / 10, rel = (i % 10) / 5, c = i % 5;
        if (i % 10 == 0) { mf[u] = pos_init; mr[u] = pos_init; }
        const u32 r = rank[u];
        const u64 canon = (rel == 0) == (uorient[r] != 0) ? 0 : 1;      // the canonical strand row (0 forward, 1 reverse) this text-relative row is
        const u64 wl = wlinks[((u64)r * 2 + canon) * 5 + c];
        const int32_t val = (int32_t)(u32)wl;
        if (val == 0) { wl_text[i] = 0; return; }
        const u32 tr = idx_of(val);
        const int32_t tu = (int32_t)order[tr] + 1;
        const bool t_rel_same = (val > 0) == (uorient[tr] != 0);      // the target, walked on: with or against ITS first occurrence
        wl_text[i] = (wl & 0xFFFFFFFF00000000ULL) | (u64)(u32)(t_rel_same ? tu : -tu);
    }
};
// depth / smallest positions of the walk (by u) -> the arrays the tail reads (by seed-order index r): depth = the single-entry counts + the
// stretches covering u (cover = starts at or before u - ends before u: the two scans of WalkRun's counters; nullptr: the copying walk, whose
// depth GapOutFunctor adds up directly)
struct WalkToSeedOrderFunctor {
    const u32* order; const u32* depth_u; const u32* started; const u32* ended; const u32* mf_u; const u32* mr_u; u32* depth; u32* mf; u32* mr;
    AC_HD void operator()(u64 r) const {
        const u32 u = order[r];
        depth[r] = depth_u[u] + (started ? started[u] - ended[u] : 0u);
        mf[r] = mf_u[u]; mr[r] = mr_u[u];
    }
};
// What a walker needs to know about the unitig it lands in, in ONE 16-byte load instead of a chain of five (first / one-past-last
// index in the novel list, final-order number, orientation, destination flags): indexed by the unitig's seed-order index u.
struct WalkInfoFunctor {
    UnitigCtx uc; const u8* maybe; V16* info;
    AC_HD void operator()(u64 u) const {
        const u32 a = uc.ustart[u], b = (u + 1 < (u64)uc.n_unitigs) ? uc.ustart[u + 1] : (u32)uc.n_novel, r = uc.rank[u];
        const u32 want = maybe ? ((maybe[(u64)r * 2] ? 1u : 0u) | (maybe[(u64)r * 2 + 1] ? 2u : 0u)) : 3u;
        info[u] = V16{a, b, r, (uc.uorient[r] ? 1u : 0u) | (want << 1)};
    }
};
// The extended k-mer at position p of sequence s (p is known to be one of its k-mer starts): xkmer_at without the search.
template <int W> AC_HD void xkmer_in_seq(const TextCtx& t, u32 s, u64 p, XKmer<W>* x) {
    const int k = t.k;
    const int f = (int)(p - t.seq_off[s]);
    const int plen = (int)t.seq_len[s] + k - 1;
    const int ld = (int)t.seq_d1[s] - f;
    const int td = f + k - (plen - (int)t.seq_d2[s]);
    x->ld = ld > 0 ? ld : 0;
    x->td = td > 0 ? td : 0;
    x->fwd = text_extract<W>(t.bits, p, k);
}
template <int W> struct PathWalkFunctor {
    TextCtx t; TextCtx g; Table tb; Novel nv; UnitigCtx uc; const V16* uinfo; const u64* wlinks; u32 pc;
    // stage: the j-th entry of walker tid goes to stage[((tid / 64) * pc + j) * 64 + tid % 64] — the 64 walkers of a wavefront
    // interleave, so the lanes of one store instruction (which have emitted about the same number of entries so far) hit a few
    // 256-byte rows instead of 64 different lines pc * 4 bytes apart; cnt[tid]: how many
    int32_t* stage; u64* cnt;
    u32* seq_tid; u32* seq_j;         // where each sequence's path starts: (walker, index in its staging slots)
    u32* depth; u32* minpos_fwd; u32* minpos_rev; u32* err; const u8* maybe;   // all by TEXT-order index u; maybe == nullptr: positions of every unitig
    u32 cap;                          // positions beyond it (from either end of the sequence) are not noted: kernels_tail.inc exp_avoid_start_of_path
    int diag;                         // measurement only (AC_PATH_DIAG, wrong results): bit 0 skips the depth atomics, bit 1 the position updates
    // Sharded builds (§7): this rank's table only holds the k-mers it owns, so the one lookup a walker needs per sequence segment has
    // been answered by the owning rank beforehand — ans[tid] for a segment that starts at the walker's first position inside a
    // sequence, ans[n_walkers + s] for one that starts with sequence s (WalkQueryFunctor / AnswerFunctor).  nullptr: look it up here.
    const u64* ans; u64 n_walkers;
    // The copying walk (K10c): walker tid covers [w_begin[tid], w_end[tid]) instead of [tid * pc, (tid + 1) * pc) (a gap between two
    // copied runs, cut into pieces of at most pc positions), notes where in its range every entry's unitig begins (stage_off, same slots
    // as stage) and leaves the depth to the pass that knows how often each of its entries is copied.  nullptr: the plain walk.
    const u64* w_begin; const u64* w_end; u16* stage_off;
    // The plain walk's depth counters: a walker keeps the stretch [lo, hi] of consecutive text-order numbers its last entries formed and
    // books it when an entry does not extend it — ONE atomic for a single entry (depth[u]), TWO for a stretch of any length (run_start[lo],
    // run_end[hi]; WalkToSeedOrderFunctor adds the cover from their scans) instead of one per entry: on mixed-species inputs the stage ran
    // at the device's atomic rate (mini-E: 111 M entries at 18 G/s, r13p).  nullptr (the copying walk): depth comes from GapOutFunctor.
    u32* run_start; u32* run_end;
    struct WalkRun { u32 lo, hi; bool live; };
    AC_D void run_flush(WalkRun& w) const {
        if (!w.live) return;
        if (w.lo == w.hi) atomic_add32(&depth[w.lo], 1u);
        else { atomic_add32(&run_start[w.lo], 1u); atomic_add32(&run_end[w.hi], 1u); }
        w.live = false;
    }
    // f = the occurrence's offset in its sequence, s_len = that sequence's length, n = the unitig's length (the walker has all
    // three at hand: no loads here but the two words that may have to be lowered)
    AC_D void emit(u64 tid, u32& j, u32 f, u32 s_len, u32 r, u32 n, bool strand, u32 want, u64 p, u64 p0, WalkRun& run) const {      // r: text-order index; want: bit 0 inputs side, bit 1 outputs side
        const u64 slot = ((tid >> 6) * (u64)pc + j) * 64 + (tid & 63);
        stage[slot] = strand ? (int32_t)(r + 1) : -(int32_t)(r + 1);
        if (stage_off) stage_off[slot] = (u16)(p - p0);
        j++;
        if ((diag & 3) == 3) return;
        // the words only ever decrease, so a plain (possibly stale) read that is already <= ours makes the atomic
        // redundant: a unitig of depth d settles after a few of its d occurrences
        if (!(diag & 1) && !stage_off) {
            if (run.live && r == run.hi + 1) run.hi = r;
            else if (run.live && r + 1 == run.lo) run.lo = r;
            else { run_flush(run); run.lo = run.hi = r; run.live = true; }
        }
        if ((diag & 2) || !want) return;
        u32 other = s_len - n - f;   // position of the same occurrence on the opposite strand
        if (f > cap && other > cap) return;      // (neither strand's position can matter: nearly every entry — and no load for it)
        const bool canon = strand == ((uinfo[r].d & 1u) != 0);      // (forward / reverse positions are the unitig's OWN strands': only near a sequence end)
        u32 vf = canon ? f : other, vr = canon ? other : f;
        if ((want & 1u) && vf <= cap && vf < minpos_fwd[r]) atomic_min32(&minpos_fwd[r], vf);
        if ((want & 2u) && vr <= cap && vr < minpos_rev[r]) atomic_min32(&minpos_rev[r], vr);
    }
    AC_D void operator()(u64 tid) const {
        const int k = t.k;
        u64 p0 = w_begin ? w_begin[tid] : tid * (u64)pc;
        u32 j = 0;
        WalkRun run{0, 0, false};
        if (p0 >= t.n_text) { cnt[tid] = 0; return; }
        u64 p1 = w_begin ? w_end[tid] : p0 + (u64)pc;
        if (p1 > t.n_text) p1 = t.n_text;
        // first sequence whose k-mer starts are not all below p0
        u32 lo = 0, hi = t.n_seqs;
        while (lo < hi) { u32 mid = lo + ((hi - lo) >> 1); if (t.seq_off[mid] + (u64)t.seq_len[mid] <= p0) lo = mid + 1; else hi = mid; }
        u32 s = lo;
        u64 p = p0;
        while (s < t.n_seqs) {
            u64 s_begin = t.seq_off[s], s_end = s_begin + (u64)t.seq_len[s];
            if (p < s_begin) p = s_begin;
            if (p >= p1) break;
            if (p == s_begin) { seq_tid[s] = (u32)tid; seq_j[s] = j; }
            // locate the walker: which unitig strand covers the k-mer at p, and where does that unitig end here?
            XKmer<W> x;
            u64 pos; bool rel_same;
            xkmer_in_seq<W>(t, s, p, &x);
            if (ans) {
                const u64 a = ans[p == s_begin ? n_walkers + (u64)s : tid];
                if (!(a >> 63)) { atomic_or32(err, 8u); break; }
                bool flipped;
                (void)xk_canonical<W>(x, k, &flipped);
                pos = a & POS_MASK;
                rel_same = (((a >> 62) & 1) != 0) == flipped;
            } else if (!find_xk<W>(g, tb, x, &pos, &rel_same)) { atomic_or32(err, 8u); break; }
            u32 jn = novel_rank(nv, pos);
            u32 r = uc.scan[jn] - 1;      // (text order: the index of the unitig in the novel list)
            const V16 ui = uinfo[r];
            const u32 a = ui.a, b = ui.b;
            bool strand = rel_same;      // (text-relative: with / against the unitig's first occurrence)
            const bool at_head = rel_same ? (jn == a) : (jn == b - 1);
            if (at_head) emit(tid, j, (u32)(p - s_begin), (u32)(s_end - s_begin), r, b - a, strand, ui.d >> 1, p, p0, run);
            p += rel_same ? (u64)(b - jn) : (u64)(jn - a + 1);
            // walk the links.  A step is a chain of dependent loads — the next symbol's mask bit and code, then the successor word — and a
            // lane's time is its steps x that chain (round 6: on mixed-species inputs a step moves a few positions, so the symbol's words are
            // those of the step before seven times in eight: they stay in registers, and the chain is the successor word alone)
            bool bad = false;
            u64 cw = ~0ULL, cbits = 0, mw = ~0ULL, mbits = 0;
            while (p < s_end && p < p1) {
                u64 e = p + (u64)k - 1;
                if ((e >> 6) != mw) { mw = e >> 6; mbits = t.mask[mw]; }
                if ((e >> 5) != cw) { cw = e >> 5; cbits = t.bits[cw]; }
                u32 c = ((mbits >> (e & 63)) & 1ULL) ? 4u : (u32)(cbits >> (62 - 2 * (int)(e & 31))) & 3u;
                u64 wl = wlinks[((u64)r * 2 + (strand ? 0 : 1)) * 5 + c];
                int32_t val = (int32_t)(u32)wl;
                if (val == 0) { atomic_or32(err, 16u); bad = true; break; }
                strand = val > 0;
                r = (u32)(strand ? val : -val) - 1;
                const u32 hi = (u32)(wl >> 32);
                emit(tid, j, (u32)(p - s_begin), (u32)(s_end - s_begin), r, hi & WL_LEN_MASK, strand, hi >> 30, p, p0, run);
                p += (u64)(hi & WL_LEN_MASK);
            }
            if (bad) break;
            if (p >= s_end) s++; else break;   // p >= p1
        }
        run_flush(run);
        cnt[tid] = j;
    }
};
// Staging slots -> the path entries in text order.  A wavefront owns the 64 walkers whose entries interleave in the staging
// area; their outputs are one contiguous stretch of ent_val (woff is the exclusive scan of the counts in walker order), so the
// lanes write consecutive output slots (coalesced) and find, for each slot, which walker it belongs to by a binary search over
// the 64 running offsets (six shuffles); the gathers stay inside the wavefront's own staging rows.
struct PathCompactFunctor {
    const int32_t* stage; const u64* cnt; const u64* woff; u32 pc; u64 n_walkers; int32_t* ent_val;
    AC_D void operator()(u64 tid, bool valid) const {
        (void)valid;
        const int lane = wv::lane();
        const u64 w0 = tid - (u64)lane;                         // first walker of this wavefront
        if (w0 >= n_walkers) return;                            // wave-uniform
        const bool live = tid < n_walkers;
        const u64 base = woff[w0];
        const u32 rel = live ? (u32)(woff[tid] - base) : 0xFFFFFFFFu;       // where this lane's walker starts inside the stretch
        const u64 last = (w0 + 63 < n_walkers) ? w0 + 63 : n_walkers - 1;
        const u32 total = (u32)(woff[last] + cnt[last] - base);
        const int32_t* rows = stage + (tid >> 6) * (u64)pc * 64;
        for (u32 o0 = 0; o0 < total; o0 += 64) {                // wave-uniform trip count: every lane takes part in the shuffles
            const u32 o = o0 + (u32)lane;
            int lo = 0;                                          // largest lane whose start is <= o
#pragma unroll
            for (int step = 32; step; step >>= 1) {
                const int cand = lo + step;
                const u32 v = (u32)wv::shfl((int)rel, cand & 63);
                if (cand < 64 && v <= o) lo = cand;
            }
            const u32 start = (u32)wv::shfl((int)rel, lo);
            if (o < total) ent_val[base + o] = rows[(u64)(o - start) * 64 + (u64)lo];
        }
    }
};
// ---- K10c: the copying walk ------------------------------------------------------------------------------------------------
// The insert knows, for every run it followed, that text positions [p, p + n) repeat [q, q + n) (or, reverse-complemented, q, q - 1, ...):
// Table::runs.  Whether a unitig strand BEGINS at a text position depends on the k-mer there alone, so the path entries of a run's
// positions are those of the stretch it repeats: the same entries at the same offsets for a run in the same orientation; for a
// reverse-complement run the unitigs that END in the repeated stretch, last one first, on the other strand.  The stretches that are
// repeated are first occurrences — novel positions, which no run contains — so walking only the text BETWEEN the runs yields every entry a
// copy needs, and nothing is copied from a copy.  On 96 similar assemblies 97 % of the text lies in runs: the walk shrinks to the first
// assembly's worth of text, 1.9 M walker start-ups (a table lookup each) become ~0.3 M, 10.6 M successor-table gathers, depth atomics
// and position probes become streaming copies of 4-byte entries, and a unitig's depth is the number of its walked entries plus, per
// entry, the number of runs whose repeated stretch contains it.
struct RunRec { u64 p; u64 n; u64 q; };      // q: bit 63 = same orientation
struct RunGatherFunctor {      // slot `tid % RUN_ROW` of row `tid / RUN_ROW` -> its place in the list (rfirst = the exclusive scan of the rows' counts)
    const u64* runs; const u32* count; const u32* rfirst; RunRec* out;
    AC_HD void operator()(u64 tid) const {
        const u64 row = tid / RUN_ROW; const u32 i = (u32)(tid % RUN_ROW);
        if (i >= count[row]) return;
        const u64* rec = runs + 3 * tid;
        out[(u64)rfirst[row] + i] = RunRec{rec[0], rec[1], rec[2]};
    }
};
// Run r of the list sorted by p is copied in pieces of at most `piece` positions (which entries a run holds depends on the positions
// alone, so a run may be cut anywhere; the piece bounds the entries one group of lanes copies: a run can be a whole replicon long).  A
// piece is usable if every position of the stretch it repeats is novel; ok[r] = the number of usable pieces (the others are left to the
// walkers, like the text between the runs).  Piece by piece since round 5: the insert takes the bits of the launch it is running in on
// trust (wave_match), so a run may hold a stretch whose source is itself a repeat — a within-genome repeat of a species whose first
// assembly went in with the same launch — and that costs the pieces it touches, not the run.  Runs that overlap — the insert's waves
// never produce them — set *overlap, and the build walks the whole text instead.
AC_HD bool run_piece_good(const Novel& nv, u64 n_text, const RunRec& x, u64 d, u64 n) {      // positions [x.p + d, x.p + d + n) of run x
    const bool same = (x.q >> 63) != 0;
    const u64 q = x.q & ~(1ULL << 63);
    if (!same && q < d + n - 1) return false;
    const u64 qlo = same ? q + d : q - d + 1 - n, qhi = qlo + n;      // the stretch the piece repeats: [qlo, qhi)
    if (qhi > n_text) return false;
    return (u64)(novel_rank(nv, qhi) - novel_rank(nv, qlo)) == n;
}
struct RunFilterFunctor {
    const RunRec* runs; RunRec* fixed; u64 n_runs; Novel nv; u64 n_text; u32* ok; u64* covered; TextCtx t; u32* overlap; u64 piece; u32* fseq;      // fseq[r] = the sequence the run lies in; fixed[r] = run r as it is used (its end never moves)
    AC_D void operator()(u64 r) const {
        RunRec x = runs[r];
        const bool same = (x.q >> 63) != 0;
        u64 q = x.q & ~(1ULL << 63);
        u32 lo = 0;
        {   // a run that begins with the very first position of a sequence (an anchor there, no leading dot left) gives that position up: the
            // walker that meets a sequence's first position is the one that notes where its path begins
            u32 hi = t.n_seqs;
            while (hi - lo > 1) { u32 mid = lo + ((hi - lo) >> 1); if (t.seq_off[mid] <= x.p) lo = mid; else hi = mid; }
            if (t.n_seqs && t.seq_off[lo] == x.p && x.n > 0) {
                x.p += 1; x.n -= 1; q = same ? q + 1 : q - 1;
                x.q = q | ((u64)(same ? 1 : 0) << 63);
            }
        }
        fixed[r] = x; fseq[r] = lo;
        if (r > 0 && runs[r - 1].p + runs[r - 1].n > runs[r].p) atomic_or32(overlap, 1u);
        u32 good = 0; u64 cov = 0;
        if (x.n > 0 && x.p + x.n <= n_text)
            for (u64 d = 0; d < x.n; d += piece) {
                const u64 n = x.n - d < piece ? x.n - d : piece;
                if (run_piece_good(nv, n_text, x, d, n)) { good++; cov += n; }
            }
        ok[r] = good;
        if (cov) atomic_add64(covered, cov);
    }
};
struct RunCompactFunctor {
    const RunRec* runs; const u32* ok; const u32* at; RunRec* out; u64 piece; const u32* fseq; u32* rseq; Novel nv; u64 n_text;
    AC_HD void operator()(u64 r) const {
        if (!ok[r]) return;
        const RunRec x = runs[r];
        const bool same = (x.q >> 63) != 0;
        const u64 q = x.q & ~(1ULL << 63);
        u32 j = 0;
        for (u64 d = 0; d < x.n; d += piece) {
            const u64 n = x.n - d < piece ? x.n - d : piece;
            if (!run_piece_good(nv, n_text, x, d, n)) continue;
            out[at[r] + j] = RunRec{x.p + d, n, (same ? q + d : q - d) | ((u64)(same ? 1 : 0) << 63)};
            rseq[at[r] + j] = fseq[r];
            j++;
        }
    }
};
// Gap g = the text between run g - 1 and run g (gap 0 starts at position 0, the last one ends at n_text): how many walkers of pc positions it takes.
struct GapWalkersFunctor {      // (launched over a bound on the number of pieces: how many there are is still on its way to the host)
    const RunRec* runs; const u32* n_runs_at; u64 n_text; u32 pc; u64* n_walkers;
    AC_HD void operator()(u64 g) const {
        const u64 n_runs = *n_runs_at;
        if (g > n_runs) { n_walkers[g] = 0; return; }      // beyond the last gap: nothing (and the scan's last word is the total)
        const u64 b = g == 0 ? 0 : runs[g - 1].p + runs[g - 1].n, e = g == n_runs ? n_text : runs[g].p;
        n_walkers[g] = e > b ? (e - b + pc - 1) / pc : 0;
    }
};
struct WalkerRangeFunctor {
    const RunRec* runs; u64 n_runs; u64 n_text; u32 pc; const u64* wfirst; u64* w_begin; u64* w_end; u32* w_gap;
    AC_HD void operator()(u64 w) const {
        u64 lo = 0, hi = n_runs + 1;      // largest gap g with wfirst[g] <= w
        while (hi - lo > 1) { u64 mid = lo + ((hi - lo) >> 1); if (wfirst[mid] <= w) lo = mid; else hi = mid; }
        const u64 g = lo;
        const u64 b = g == 0 ? 0 : runs[g - 1].p + runs[g - 1].n, e = g == n_runs ? n_text : runs[g].p;
        const u64 wb = b + (w - wfirst[g]) * (u64)pc;
        w_begin[w] = wb; w_end[w] = wb + pc < e ? wb + pc : e; w_gap[w] = (u32)g;
    }
};
// Staging slots of the gap walkers -> their entries in text order, with the text position at which each entry's unitig begins and ends,
// the gap it lies in and whether its positions are wanted.  Wavefront-cooperative like PathCompactFunctor: the 64 walkers of a wavefront
// fill one contiguous stretch of the list, consecutive lanes take consecutive entries of it and find their walker by six shuffles (a thread
// per walker looping over its own entries took as long as the slowest walker of the launch: 51 us for 0.6 M entries on config C).
struct WalkCompactFunctor {
    const int32_t* stage; const u16* stage_off; const u64* cnt; const u64* woff; const u64* w_begin; const u32* w_gap; u32 pc; u64 n_walkers; const V16* uinfo;      // uinfo: by text-order index (WalkInfoFunctor)
    int32_t* ent; u64* ent_pos; u64* ent_end; u8* ent_want; u32* ent_gap;      // ent_want: may the unitig become an expand_repeats destination (bit 0 inputs, bit 1 outputs side)?
    AC_D void put(u64 at, int32_t v, u64 pos, u32 gap) const {
        const V16 ui = uinfo[idx_of(v)];
        ent[at] = v; ent_pos[at] = pos; ent_end[at] = pos + (u64)(ui.b - ui.a) - 1; ent_gap[at] = gap;
        ent_want[at] = (u8)(ui.d >> 1);
    }
    AC_D void operator()(u64 tid, bool valid) const {
        (void)valid;
        const int lane = wv::lane();
        const u64 w0 = tid - (u64)lane;                         // first walker of this wavefront
        if (w0 >= n_walkers) return;                            // wave-uniform
        const bool live = tid < n_walkers;
        const u64 base = woff[w0];
        const u32 rel = live ? (u32)(woff[tid] - base) : 0xFFFFFFFFu;       // where this lane's walker starts inside the stretch
        const u64 last = (w0 + 63 < n_walkers) ? w0 + 63 : n_walkers - 1;
        const u32 total = (u32)(woff[last] + cnt[last] - base);
        const u64 my_begin = live ? w_begin[tid] : 0;
        const u32 my_gap = live ? w_gap[tid] : 0;
        const u64 row0 = (tid >> 6) * (u64)pc * 64;
        for (u32 o0 = 0; o0 < total; o0 += 64) {                // wave-uniform trip count: every lane takes part in the shuffles
            const u32 o = o0 + (u32)lane;
            int lo = 0;                                          // largest lane whose start is <= o
#pragma unroll
            for (int step = 32; step; step >>= 1) {
                const int cand = lo + step;
                const u32 v = (u32)wv::shfl((int)rel, cand & 63);
                if (cand < 64 && v <= o) lo = cand;
            }
            const u32 start = (u32)wv::shfl((int)rel, lo);
            const u64 wb = (u64)wv::shfl64((unsigned long long)my_begin, lo);
            const u32 gap = (u32)wv::shfl((int)my_gap, lo);
            if (o < total) {
                const u64 slot = row0 + (u64)(o - start) * 64 + (u64)lo;
                put(base + o, stage[slot], wb + (u64)stage_off[slot], gap);
            }
        }
    }
};
AC_HD u64 lower_bound_u64(const u64* a, u64 n, u64 key) {      // first index whose value is >= key
    u64 lo = 0, hi = n;
    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// The walked entries run r copies: [a, b) of the entry list (those whose unitig begins — ends, for a reverse-complement run — inside the
// stretch the run repeats); every one of them gains a copy (cov: +1 at a, -1 at b; its prefix sum is the number of copies per entry).
struct RunRangeFunctor {
    const RunRec* runs; const u64* ent_pos; const u64* ent_end; u64 n_ent; u64* ra; u64* cnt; u32* cov;
    AC_D void operator()(u64 r) const {
        const RunRec x = runs[r];
        const bool same = (x.q >> 63) != 0;
        const u64 q = x.q & ~(1ULL << 63);
        u64 a, b;
        // (positions strictly increase along the list: at most x.n entries lie between the two bounds, so the second search is a short one)
        if (same) { a = lower_bound_u64(ent_pos, n_ent, q); const u64 m = n_ent - a < x.n ? n_ent - a : x.n; b = a + lower_bound_u64(ent_pos + a, m, q + x.n); }
        else { a = lower_bound_u64(ent_end, n_ent, q + 1 - x.n); const u64 m = n_ent - a < x.n ? n_ent - a : x.n; b = a + lower_bound_u64(ent_end + a, m, q + 1); }
        ra[r] = a; cnt[r] = b - a;
        if (b > a) { atomic_add32(&cov[a], 1u); atomic_add32(&cov[b], 0xFFFFFFFFu); }
    }
};
// Entries per segment of the text, in text order: gap 0, run 0, gap 1, run 1, ..., gap R (2 R + 1 segments; [2 R + 1] = 0 for the scan).
struct SegCountFunctor {
    const u64* wfirst; const u64* woff; const u64* run_cnt; u64 n_runs; u64* seg;
    AC_HD void operator()(u64 i) const {
        if (i > 2 * n_runs) { seg[i] = 0; return; }
        if (i & 1) { seg[i] = run_cnt[i >> 1]; return; }
        const u64 g = i >> 1;
        seg[i] = woff[wfirst[g + 1]] - woff[wfirst[g]];
    }
};
// The walked entries to their final places (a thread per entry: those of a gap stay together, segoff[2 g] = where gap g's begin); a unitig's
// depth = its walked entries + their copies.
struct GapOutFunctor {
    const int32_t* ent; const u32* ent_gap; const u64* woff; const u64* wfirst; const u64* segoff; const u32* copies; int32_t* out; u32* depth;
    AC_D void operator()(u64 e) const {
        const u64 g = ent_gap[e];
        const int32_t v = ent[e];
        out[segoff[2 * g] + (e - woff[wfirst[g]])] = v;
        atomic_add32(&depth[idx_of(v)], 1u + copies[e]);
    }
};
// Run r's entries: LANES lanes copy them (reversed and on the other strand for a reverse-complement run; a run holds ~45 entries) and lower
// the smallest positions of the unitigs that may become expand_repeats destinations, exactly as a walker that met the occurrence would.
// Measured on config C (profiles/r08t_runout_shapes.txt): the copy itself takes 38 us (32 lanes, one entry in flight per lane; 8 x 4: 32 us),
// the positions 160 us more — ~4 M check-then-atomic updates on addresses that the ~96 copies of a unitig share; with the position bound
// (`cap`, checked once per piece against the piece's distance from both ends of its sequence) nearly all of them are skipped: 69 us in all.
template <u32 LANES, u32 FLIGHT> struct RunOutFunctor {
    const RunRec* runs; u64 n_runs; const u64* ra; const u64* rcnt; const u64* segoff; const int32_t* ent; const u64* ent_pos; const u64* ent_end;
    const V16* uinfo; const u8* ent_want; TextCtx t; const u32* rseq; u32* minpos_fwd; u32* minpos_rev; int32_t* out; u32 cap;      // (unitigs by text-order index)
    AC_D void position(const RunRec& x, bool same, u64 q, u64 s_begin, u32 s_len, u64 e, int32_t w, u32 want) const {
        const u32 ri = idx_of(w);
        const u64 p = same ? x.p + (ent_pos[e] - q) : x.p + (q - ent_end[e]);      // where this occurrence's unitig strand begins
        const V16 ui = uinfo[ri];
        const u32 f = (u32)(p - s_begin), len = ui.b - ui.a;
        const u32 other = s_len - len - f;
        const bool strand = (w > 0) == ((ui.d & 1u) != 0);      // (the entry's sign is text-relative; the positions belong to the unitig's own strands)
        const u32 vf = strand ? f : other, vr = strand ? other : f;
        if ((want & 1u) && vf <= cap && vf < minpos_fwd[ri]) atomic_min32(&minpos_fwd[ri], vf);
        if ((want & 2u) && vr <= cap && vr < minpos_rev[ri]) atomic_min32(&minpos_rev[ri], vr);
    }
    AC_D void operator()(u64 tid, bool valid) const {
        const u64 r = tid / LANES;
        if (!valid || r >= n_runs) return;
        const u32 lane = (u32)(tid % LANES);
        const u64 n = rcnt[r];
        if (n == 0) return;
        const RunRec x = runs[r];
        const bool same = (x.q >> 63) != 0;
        const u64 q = x.q & ~(1ULL << 63);
        const u64 a = ra[r], o = segoff[2 * r + 1];
        // is any of the run's occurrences within `cap` of an end of its sequence (a run never crosses a separator)?  The first one begins
        // at or behind x.p; the one that reaches furthest is the last entry's (the first's, for a reverse-complement run)
        const u32 sq = rseq[r];
        const u64 s_begin = t.seq_off[sq]; const u32 s_len = t.seq_len[sq];
        const u64 reach = same ? x.p + (ent_end[a + n - 1] - q) : x.p + (q - ent_pos[a]);      // last position of that occurrence
        const u64 from_end = s_begin + (u64)s_len - 1 - reach;
        const bool near = x.p - s_begin <= (u64)cap || from_end <= (u64)cap;
        for (u64 j0 = lane; j0 < n; j0 += LANES * FLIGHT) {
            int32_t v[FLIGHT]; u32 want[FLIGHT];
AC_UNROLL_FULL
            for (u32 u = 0; u < FLIGHT; u++) {
                const u64 j = j0 + (u64)u * LANES;
                const bool in = j < n;
                const u64 e = in ? (same ? a + j : a + n - 1 - j) : a;
                v[u] = ent[e]; want[u] = in && near ? (u32)ent_want[e] : 0u;      // (a property of the unitig: the same on either strand)
            }
AC_UNROLL_FULL
            for (u32 u = 0; u < FLIGHT; u++) {
                const u64 j = j0 + (u64)u * LANES;
                if (j < n) out[o + j] = same ? v[u] : -v[u];
            }
AC_UNROLL_FULL
            for (u32 u = 0; u < FLIGHT; u++) {
                const u64 j = j0 + (u64)u * LANES;
                if (want[u]) position(x, same, q, s_begin, s_len, same ? a + j : a + n - 1 - j, same ? v[u] : -v[u], want[u]);
            }
        }
    }
};
struct PathOffCopyFunctor {      // where each sequence's path starts: the j-th entry of the walker that met the sequence's first position
    const u32* seq_tid; const u32* seq_j; const u64* woff; const u64* wfirst; const u32* w_gap; const u64* segoff; u64* path_off;
    AC_HD void operator()(u64 s) const {
        const u64 w = seq_tid[s], g = w_gap[w];
        path_off[s] = segoff[2 * g] + (woff[w] - woff[wfirst[g]]) + (u64)seq_j[s];
    }
};
// Sharded builds: the canonical keys a rank's walkers start from — query tid < n_walkers = the k-mer at the walker's first
// position if that lies strictly inside a sequence, query n_walkers + s = the first k-mer of sequence s; W words each, all-ones =
// no such k-mer.  AnswerFunctor (on every rank, over the queries of all ranks) looks up the ones its table owns:
// [found:1][claimant flipped:1][smallest position:40], 0 otherwise — the ranks' answers are disjoint and add up.
template <int W> struct WalkQueryFunctor {
    TextCtx t; u32 pc; u64 n_walkers; u64* keys; const u64* w_begin;      // w_begin: the walkers of a copying walk (their first positions), nullptr = walker q starts at q * pc
    AC_D void operator()(u64 q) const {
        u64 p; bool valid = false;
        if (q < n_walkers) {
            p = w_begin ? w_begin[q] : q * (u64)pc;
            if (p < t.n_text) {
                u32 lo = 0, hi = t.n_seqs;      // first sequence whose k-mer starts are not all below p
                while (lo < hi) { u32 mid = lo + ((hi - lo) >> 1); if (t.seq_off[mid] + (u64)t.seq_len[mid] <= p) lo = mid + 1; else hi = mid; }
                valid = lo < t.n_seqs && t.seq_off[lo] < p;      // strictly inside (a segment that starts WITH the sequence uses the other query)
            }
        } else {
            p = t.seq_off[q - n_walkers];
            valid = true;
        }
        Key<W> uk;
AC_UNROLL_W
        for (int i = 0; i < W; i++) uk.w[i] = ~0ULL;
        XKmer<W> x;
        if (valid && xkmer_at<W>(t, p, &x)) { bool flipped; uk = xk_canonical<W>(x, t.k, &flipped); }
AC_UNROLL_W
        for (int i = 0; i < W; i++) keys[q * W + (u64)i] = uk.w[i];
    }
};
template <int W> struct AnswerFunctor {
    TextCtx g; Table tb; const u64* keys; u64* out;
    AC_D void operator()(u64 q) const {
        Key<W> uk;
AC_UNROLL_W
        for (int i = 0; i < W; i++) uk.w[i] = keys[q * W + (u64)i];
        u64 a = 0;
        if (uk.w[0] != ~0ULL) {
            FindResult r = table_find<W>(g, tb, uk, key_ld<W>(uk) > 0);
            if (r.found) a = (1ULL << 63) | ((u64)(r.claimant_flipped ? 1 : 0) << 62) | r.pos;
        }
        out[q] = a;
    }
};
// ---- the paths as STRETCHES, for the way to the host (round 6) ---------------------------------------------------------------------------
// In text-order numbers a strain walks u, u + 1, u + 2, ... between its own variants (and -u, -(u - 1), ... on the other strand): entry i
// continues a stretch iff ent[i] == ent[i - 1] + 1 — in either direction, the numbers being signed.  A stretch crosses the link as ONE
// record (its first value, its place in the entry list) instead of 4 bytes per entry; the host writes the final numbers of its entries from
// a table that it reads front to back (PathRemapJob).  configs[4]: 1.21 G entries, 4.8 GB = 84 ms of the link (57 GB/s device -> host) as entries, 0.94 GB as stretches.
// Two passes of whole wavefronts over the entries, 64 per wavefront: count the stretch starts of the group (a ballot), scan the counts, then
// write the group's records behind its offset (the ballot again, a lane's rank among the set bits).  (First form: a flag word per entry, a
// scan over the entries, a gather — 35 GB of traffic for configs[4]'s 1.21 G entries, 11 ms; this one 11 GB.)
AC_D bool stretch_starts(const int32_t* ent, u64 n, u64 i) { return i < n && (i == 0 || ent[i] != ent[i - 1] + 1); }
struct StretchCountFunctor {
    const int32_t* ent; u64 n; u32* count;      // count[g] for group g = entries [64 g, 64 g + 64); one more group than needed holds 0
    AC_D void operator()(u64 i, bool valid) const {
        const u64 b = wv::ballot(valid && stretch_starts(ent, n, i));
        if (valid && wv::lane() == 0) count[i >> 6] = (u32)popc64(b);      // (the launch is whole workgroups: up to three wavefronts lie behind the last group, none of their lanes valid)
    }
};
struct StretchRecordFunctor {
    const int32_t* ent; u64 n; const u32* at; int32_t* rec_val; u32* rec_pos;      // at[g]: records before group g
    AC_D void operator()(u64 i, bool valid) const {
        const bool st = valid && stretch_starts(ent, n, i);
        const u64 b = wv::ballot(st);
        if (!st) return;
        const u32 slot = at[i >> 6] + (u32)popc64(b & ((1ULL << wv::lane()) - 1));
        rec_val[slot] = ent[i]; rec_pos[slot] = (u32)i;
    }
};
struct PathOffFunctor {
    const u32* seq_tid; const u32* seq_j; const u64* woff; u64* path_off;
    AC_HD void operator()(u64 s) const { path_off[s] = woff[seq_tid[s]] + (u64)seq_j[s]; }
};

