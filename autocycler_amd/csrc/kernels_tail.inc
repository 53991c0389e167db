// K13 link order, K14 analysis, K15 renumbering, K17 expand_repeats, K16 finalisation, K12 sequences — part of graph_build.hip (included inside namespace ac; not a translation unit of its own).
// ---- K13: create_links' push order (unitig_graph.rs:248-286; SURVEY App. A.4), a function of seed numbers only:
//   forward_next(a): all b+ (seed order ascending) then all b- (ascending);
//   reverse_next(a): a'- for a' <= a (ascending; a' == a is the a+ -> a+ self loop pushed in case 1 of iteration a),
//                    then b+ (case 3 of iteration a, ascending), then a'- for a' > a (ascending).
struct LinkOrderFunctor {      // (whole wavefronts: launch_full)
    const int32_t* sym; int32_t* ord; u8* cnt; u32* n_self_mirror;
    u64* n_links;      // n_links[256]: partial sums of the counts (round 6: read with the candidate count instead of by a round trip of its own) — one atomic per
                       // WAVEFRONT (an atomic per strand, even over 256 words, cost the analysis stage 15-40 %: r14i)
    AC_D void operator()(u64 idx, bool valid) const {
        int n = 0;
        if (valid) {
            int side = (int)(idx & 1);
            int32_t num = (int32_t)(idx >> 1) + 1;
            int32_t tmp[5]; u64 key[5];
            for (int c = 0; c < 5; c++) {
                int32_t v = sym[idx * 5 + (u64)c];
                if (v == 0) continue;
                u32 cls = (side == 0) ? (v > 0 ? 0u : 1u) : (v > 0 ? 1u : ((-v <= num) ? 0u : 2u));
                u64 kv = ((u64)cls << 32) | (u64)(v < 0 ? -v : v);
                int j = n++;
                while (j > 0 && key[j - 1] > kv) { key[j] = key[j - 1]; tmp[j] = tmp[j - 1]; j--; }
                key[j] = kv; tmp[j] = v;
            }
            u32 self = 0;
            for (int i = 0; i < 5; i++) {
                ord[idx * 5 + (u64)i] = i < n ? tmp[i] : 0;
                if (i < n && tmp[i] == (side == 0 ? -num : num)) self++;
            }
            cnt[idx] = (u8)n;
            if (self) atomic_add32(n_self_mirror, self);
        }
        int t = n;
#pragma unroll
        for (int o = 32; o; o >>= 1) t += wv::shfl_xor(t, o);
        if (wv::lane() == 0 && t) atomic_add64(&n_links[(idx >> 6) & 255], (u64)t);
    }
};
struct OrderedLinks {
    const int32_t* ord; const u8* cnt;
    AC_HD const int32_t* next_of(int32_t x, u32* n) const {   // next links of a unitig strand
        u64 i = (u64)idx_of(x) * 2 + (x > 0 ? 0 : 1);
        *n = cnt[i];
        return ord + i * 5;
    }
};

// ---- K14: static analysis for expand_repeats -------------------------------------------------------------------
// Fixed starts/ends (graph_simplification.rs:190-230): first/last unitig of every sequence path plus their one-step
// neighbours; invariant across passes because paths and links never change.
struct PathEndsFunctor {
    const int32_t* path; const u64* path_off; u8* fs0; u8* fe0; const u32* rank; const u8* uorient;      // path: text-order numbers, text-relative signs (kernels_paths.inc); rank: -> seed-order index
    AC_HD void operator()(u64 s) const {
        u64 b = path_off[s], e = path_off[s + 1];
        if (b == e) return;
        int32_t first = path[b], last = path[e - 1];
        const u32 fi = rank[idx_of(first)], li = rank[idx_of(last)];
        const bool first_fwd = (first > 0) == (uorient[fi] != 0), last_fwd = (last > 0) == (uorient[li] != 0);      // on the unitig's own forward strand?
        if (first_fwd) fs0[fi] = 1; else fe0[fi] = 1;
        if (last_fwd) fe0[li] = 1; else fs0[li] = 1;
    }
};
struct FixedSpreadFunctor {
    const u8* fs0; const u8* fe0; OrderedLinks L; u8* fixed_start; u8* fixed_end;
    AC_HD void operator()(u64 u) const {
        int32_t num = (int32_t)u + 1;
        if (fs0[u]) {   // upstream of a fixed start: forward_prev(u) = { -e : e in reverse_next(u) }
            fixed_start[u] = 1;
            u32 n; const int32_t* p = L.next_of(-num, &n);
            for (u32 i = 0; i < n; i++) { int32_t up = -p[i]; if (up > 0) fixed_end[idx_of(up)] = 1; else fixed_start[idx_of(up)] = 1; }
        }
        if (fe0[u]) {   // downstream of a fixed end
            fixed_end[u] = 1;
            u32 n; const int32_t* p = L.next_of(num, &n);
            for (u32 i = 0; i < n; i++) { int32_t down = p[i]; if (down > 0) fixed_start[idx_of(down)] = 1; else fixed_end[idx_of(down)] = 1; }
        }
    }
};
// get_exclusive_inputs / get_exclusive_outputs (:233-280) and the fixed-end guards of expand_repeats (:66-83).
struct CandFunctor {
    OrderedLinks L; const u8* fixed_start; const u8* fixed_end; u8* cand;
    AC_HD void operator()(u64 idx) const {
        u32 x = (u32)(idx >> 1);
        bool inputs = (idx & 1) == 0;
        int32_t xnum = (int32_t)x + 1;
        u32 n; const int32_t* p = L.next_of(inputs ? -xnum : xnum, &n);
        bool ok = n >= 2 && !(inputs ? fixed_start[x] : fixed_end[x]);
        for (u32 i = 0; ok && i < n; i++) {
            int32_t other = inputs ? -p[i] : p[i];
            // inputs: other's next list must be exactly [x+].  outputs: other's prev list must be exactly [x+],
            // i.e. the next list of other's opposite strand must be exactly [x-].
            u32 m; const int32_t* q = L.next_of(inputs ? other : -other, &m);
            if (!(m == 1 && q[0] == (inputs ? xnum : -xnum))) ok = false;
            u32 u = idx_of(other);
            if (u == x) ok = false;
            if (inputs) { if ((other > 0 && fixed_end[u]) || (other < 0 && fixed_start[u])) ok = false; }
            else { if ((other > 0 && fixed_start[u]) || (other < 0 && fixed_end[u])) ok = false; }
        }
        cand[idx] = ok ? 1 : 0;
    }
};

struct CandCoveredFunctor {      // error bit 32 of the path error word if a candidate junction was not in the walk's position filter
    const u8* cand; const u8* maybe; u32* err;
    AC_D void operator()(u64 idx) const { if (cand[idx] && !maybe[idx]) atomic_or32(err, 32u); }
};

// ---- K15: renumber_unitigs (unitig_graph.rs:295-315): length descending, forward sequence ascending, depth
// descending; the sort is stable on the incoming order -------------------------------------------------------------
struct UnitigLess {
    const u32* len; const u64* off; const u8* seq; const u32* depth;
    AC_HD bool operator()(const u32& a, const u32& b) const {
        u32 la = len[a], lb = len[b];
        if (la != lb) return la > lb;
        const u8* pa = seq + off[a]; const u8* pb = seq + off[b];
        for (u32 i = 0; i < la; i++) { u8 ca = pa[i], cb = pb[i]; if (ca != cb) return ca < cb; }
        return depth[a] > depth[b];
    }
};

// The same order without a comparator sort.  ONE stable sort on (length desc | first 16 bases asc), then a stable insertion sort
// with the full comparator inside each group of unitigs that agree on both (the two alleles of a SNP, typically: same length,
// same first 25 bases) — exact, since the comparator orders by length and sequence first and both sorts are stable.  Only when a
// group is larger than RENUM_MAX_GROUP (many identical very short unitigs) does the caller fall back to TWO stable passes on
// (length desc | first 32 bases asc | depth desc) — exact whenever the sequence is at most 32 long or differs from its neighbours
// within the first 32 bases — and the same insertion sort inside the groups of longer unitigs that still agree.
struct RenumKeyFunctor {
    const u32* len; const u64* off; const u8* seq; u64* prefix;
    AC_HD void operator()(u64 u) const {
        u32 l = len[u];
        const u8* p = seq + off[u];
        u64 w = 0;
        u32 m = l < 32 ? l : 32;
        for (u32 i = 0; i < m; i++) { u32 ch = p[i]; w |= (u64)(((ch >> 1) ^ (ch >> 2)) & 3u) << (62 - 2 * i); }
        prefix[u] = w;
    }
};
// Key of the element currently at position i.  Two-pass form: pass 0 = (prefix low | ~depth), pass 1 = (~len | prefix high).
// One-pass form (pass 2): (~len | what orders this length class) — up to 4 bases: the whole sequence (8 bits) and the depth (24
// bits); up to 8 bases: the whole sequence (16 bits) and the depth (16 bits, saturated); longer: the first 16 bases.  The layout
// only depends on the length, the leading field, so keys of different layouts never meet.  renum_key_exact: the key IS the
// comparator (expand_repeats leaves many identical one- or two-base unitigs; they need no tie-break and no group limit).
AC_HD bool renum_key_exact(u32 len, u32 depth) { return len <= 4 ? depth < (1u << 24) : (len <= 8 && depth < 0xFFFFu); }
struct RenumPassFunctor {
    const u32* order; const u32* len; const u32* depth; const u64* prefix; int pass; u64* key;
    AC_HD void operator()(u64 i) const {
        u32 u = order[i];
        if (pass == 2) {
            const u32 l = len[u], d = depth[u];
            u32 low;
            if (l <= 4) low = ((u32)(prefix[u] >> 56) << 24) | (~(d < (1u << 24) ? d : (1u << 24) - 1) & 0xFFFFFFu);
            else if (l <= 8) low = ((u32)(prefix[u] >> 48) << 16) | (~(d < 0xFFFFu ? d : 0xFFFFu) & 0xFFFFu);
            else low = (u32)(prefix[u] >> 32);
            key[i] = ((u64)(~l) << 32) | low;
            return;
        }
        key[i] = pass == 0 ? ((prefix[u] << 32) | (u64)(~depth[u])) : (((u64)(~len[u]) << 32) | (prefix[u] >> 32));
    }
};
// RenumKeyFunctor + the one-pass RenumPassFunctor in one kernel (round 6): the element at position i computes its unitig's prefix word,
// stores it for the tie-break and builds its key from it.
struct RenumKeyPassFunctor {
    RenumKeyFunctor kf; RenumPassFunctor pf;      // pf.pass == 2, pf.prefix == kf.prefix
    AC_HD void operator()(u64 i) const { kf((u64)pf.order[i]); pf(i); }
};
static const u32 RENUM_MAX_GROUP = 64;
struct RenumTieFunctor {
    u32* order; u64 n; const u32* len; const u32* depth; const u64* prefix; UnitigLess less; u32* too_big;
    int two_pass;      // 1: the order came from both passes (groups agree on 32 bases, and a sequence of at most 32 is settled)
    u32 max_group;
    AC_HD bool same(u32 a, u32 b) const { return len[a] == len[b] && (two_pass ? prefix[a] == prefix[b] : (prefix[a] >> 32) == (prefix[b] >> 32)); }
    AC_D void operator()(u64 i) const {
        u32 u = order[i];
        if (two_pass ? len[u] <= 32 : renum_key_exact(len[u], depth[u])) return;      // the radix key was the whole comparator
        if (i > 0 && same(order[i - 1], u)) return;               // not the first of its group
        u64 e = i + 1;
        while (e < n && e - i <= max_group && same(order[e], u)) e++;
        if (e - i > max_group) { atomic_or32(too_big, 1u); return; }
        for (u64 a = i + 1; a < e; a++) {                         // stable insertion sort of order[i, e)
            u32 v = order[a];
            u64 b = a;
            while (b > i && less(v, order[b - 1])) { order[b] = order[b - 1]; b--; }
            order[b] = v;
        }
    }
};

// ---- K17: expand_repeats on the device (graph_simplification.rs:26-142, shift primitives unitig.rs:217-249) ---------
// The reference visits junctions sequentially (unitigs in first-renumber order, inputs side then outputs side) and
// the result depends on that order only where two junctions touch a common unitig.  A junction (x, side) reads and
// writes x (as the destination that gains sequence) and its exclusive sources (which lose it); everything that
// decides WHICH junctions qualify is static (K14).  So: number the candidate junctions in visiting order, give
// every candidate the level 1 + max(level of earlier candidates sharing a unitig with it), and run each pass level
// by level — candidates of one level never share a unitig, every conflicting pair keeps the reference's order.
// The two sides of the same destination touch disjoint fields of it (prefix + min forward position vs. suffix + min
// reverse position) and are not a conflict.
// A unitig's sequence during a pass is [bytes gained at its start this pass][core view][bytes gained at its end this
// pass]; after every pass that moved something the sequences are rewritten contiguously.
// One unitig's view, 32 bytes = half a line (round 5; rounds 1-4 kept six arrays): a junction visit is a string of random accesses — its
// level's kernels ran at the device's random-transaction rate (config C, level 1 of pass 1: ~60 K junctions x ~40 transactions in 47 us) —
// and reading a source's view was six of them.  The prefix pair and the suffix pair are 8-byte aligned: the two junctions of one
// destination may run side by side, each writing its own pair.
struct alignas(32) ExpU {
    u64 coff; u32 clen, pad;                                   // core: view into the current sequence buffer
    u32 pre_off, pre_len, post_off, post_len;                  // gained this pass: offsets into `pool`
};
struct ExpState {
    const u8* cur; ExpU* v;
    u8* pool; u32* pool_used;
    u32* minf; u32* minr;                                      // min forward / reverse position (graph_simplification.rs:164-181)
    u8* dirty; const u8* cand;
    OrderedLinks L;
    u64* shifted;
    const V16* touch;                                          // the (at most four) candidate junctions that read or write each unitig (TouchFunctor): static
};
AC_HD u8 comp_base(u8 c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
AC_HD u32 exp_len(const ExpState& e, u32 u) { const ExpU x = e.v[u]; return x.pre_len + x.clen + x.post_len; }
AC_HD u8 exp_at(const ExpState& e, u32 u, u32 i) {
    const ExpU x = e.v[u];
    if (i < x.pre_len) return e.pool[x.pre_off + i];
    i -= x.pre_len;
    if (i < x.clen) return e.cur[x.coff + i];
    return e.pool[x.post_off + (i - x.clen)];
}
AC_HD u8 exp_from_start(const ExpState& e, int32_t s, u32 i) { u32 u = idx_of(s); return s > 0 ? exp_at(e, u, i) : comp_base(exp_at(e, u, exp_len(e, u) - 1 - i)); }
AC_HD u8 exp_from_end(const ExpState& e, int32_t s, u32 i) { u32 u = idx_of(s); return s > 0 ? exp_at(e, u, exp_len(e, u) - 1 - i) : comp_base(exp_at(e, u, i)); }
// (a source belongs to one junction of a level: its whole view is read, changed and written back)
AC_HD void exp_remove_start(const ExpState& e, u32 u, u32 n) {
    ExpU x = e.v[u];
    u32 d = n < x.pre_len ? n : x.pre_len; x.pre_off += d; x.pre_len -= d; n -= d;
    d = n < x.clen ? n : x.clen; x.coff += d; x.clen -= d; n -= d;
    x.post_off += n; x.post_len -= n;
    e.v[u] = x;
}
AC_HD void exp_remove_end(const ExpState& e, u32 u, u32 n) {
    ExpU x = e.v[u];
    u32 d = n < x.post_len ? n : x.post_len; x.post_len -= d; n -= d;
    d = n < x.clen ? n : x.clen; x.clen -= d; n -= d;
    x.pre_len -= n;
    e.v[u] = x;
}
// The (at most four) candidate junctions that read or write unitig u: u as destination (2u, 2u+1) and u as an
// exclusive source of the junction its only forward / reverse link leads to.  0xFFFFFFFF = none.
AC_HD void touchers(const OrderedLinks& L, const u8* cand, u32 u, u32 out[4]) {
    out[0] = cand[2 * (u64)u] ? 2 * u : 0xFFFFFFFFu;
    out[1] = cand[2 * (u64)u + 1] ? 2 * u + 1 : 0xFFFFFFFFu;
    for (int side = 0; side < 2; side++) {
        u32 c = 0xFFFFFFFFu;
        if (L.cnt[2 * (u64)u + side] == 1) {
            int32_t p0 = L.ord[(2 * (u64)u + side) * 5];
            u32 cc = 2 * idx_of(p0) + (p0 > 0 ? 0u : 1u);
            if (cand[cc]) c = cc;
        }
        out[2 + side] = c;
    }
}
struct CandFlagFunctor {    // j = 2*oi + side over the visiting order: is (order1[oi], side) a candidate?
    const u32* order1; const u8* cand; u32* flag;
    AC_HD void operator()(u64 j) const { flag[j] = cand[2 * (u64)order1[j >> 1] + (j & 1)] ? 1u : 0u; }
};
struct CandListFunctor {
    const u32* order1; const u32* flag; const u32* pos; u32* clist; u32* prio;
    AC_HD void operator()(u64 j) const {
        if (!flag[j]) return;
        u32 c = 2 * order1[j >> 1] + (u32)(j & 1);
        clist[pos[j]] = c;
        prio[c] = pos[j];
    }
};
// The earlier candidates a candidate conflicts with (they share a unitig), found ONCE: the relaxation sweeps below then only
// read levels.  At most 24 per candidate (the destination and its <= 5 sources, <= 4 junctions touching each); stored
// transposed (preds[j * C + ci]) so that a sweep reads them coalesced.
static const u32 MAX_PREDS = 24;
struct LevelPredsFunctor {
    OrderedLinks L; const u8* cand; const u32* clist; const u32* prio; u64 C; u32* preds; u8* npred; const V16* touch;      // touch: TouchFunctor's records (one read per unitig instead of touchers()' eight)
    AC_D void operator()(u64 ci) const {
        u32 c = clist[ci];
        u32 x = c >> 1;
        bool inputs = (c & 1) == 0;
        u32 n; const int32_t* p = L.next_of(inputs ? -((int32_t)x + 1) : (int32_t)x + 1, &n);
        u32 np = 0;
        for (u32 i = 0; i <= n; i++) {
            u32 u = (i == n) ? x : idx_of(p[i]);
            const V16 tt = touch[u];
            const u32 t[4] = {tt.a, tt.b, tt.c, tt.d};
            for (int j = 0; j < 4; j++) {
                u32 c2 = t[j];
                if (c2 == 0xFFFFFFFFu || c2 == c) continue;
                if (u == x && (c2 >> 1) == x) continue;     // the other side of the same destination: disjoint fields
                u32 pr = prio[c2];
                if (pr < (u32)ci && np < MAX_PREDS) preds[(u64)np++ * C + ci] = pr;
            }
        }
        npred[ci] = (u8)np;
    }
};
// Level of a candidate = 1 + the highest level among the earlier candidates it conflicts with, settled front to back: a candidate is
// FINAL once all of its predecessors are (they have smaller indices: no cycles), and a final one costs a sweep one coalesced word.  Until
// round 5 every sweep recomputed every candidate from its predecessors' current levels (monotone relaxation): E' paid 16 sweeps of 1.05 M
// candidates x ~6 random reads = 1.4 ms of its 4.1 ms expand stage; now the work of all sweeps together is about one such sweep.
// open: "some candidate is still open after this sweep"; prev: that flag of the previous sweep of the batch (nullptr for the first) —
// once a sweep leaves nothing open the rest of the batch returns at once.  maxlv: the highest level (sizes the radix sort by level).
static const u32 LEVEL_FINAL = 0x80000000u;
struct LevelRelaxFunctor {
    const u32* preds; const u8* npred; u64 C; u32* level; u32* open; const u32* prev; u32* maxlv;
    AC_D void operator()(u64 ci) const {
        if (prev && *prev == 0) return;
        if (level[ci] & LEVEL_FINAL) return;
        u32 lv = 1;
        const u32 np = npred[ci];
        for (u32 j = 0; j < np; j++) {
            const u32 l2 = level[preds[(u64)j * C + ci]];
            if (!(l2 & LEVEL_FINAL)) { if (*open == 0) atomic_or32(open, 1u); return; }      // (a stale read only delays; the flag is read first: a million atomics on one word would serialise)
            const u32 v = (l2 & ~LEVEL_FINAL) + 1;
            if (v > lv) lv = v;
        }
        level[ci] = lv | LEVEL_FINAL;
        if (maxlv && lv > 1 && lv > *maxlv) atomic_max32(maxlv, lv);      // (level 1 is where the host's maximum starts)
    }
};
struct LevelKeyFunctor {
    const u32* level; u64* key;
    AC_HD void operator()(u64 ci) const { key[ci] = (u64)(level[ci] & ~LEVEL_FINAL); }      // (the sort is stable and the candidates are in visiting order already)
};
struct LevelBoundsFunctor {   // keys sorted by (level >= 1, visiting position): bstart[lv] = first index of level lv (lv <= cap),
    const u64* key; u64 n; u32* bstart; u32 cap;      // bstart[0] = number of levels
    AC_HD void operator()(u64 i) const {
        u32 lv = (u32)key[i];
        if ((i == 0 || (u32)key[i - 1] != lv) && lv <= cap) bstart[lv] = (u32)i;
        if (i + 1 == n) bstart[0] = lv;
    }
};
// A unitig strand's current sequence as seen by one junction: the descriptor is read once, after that every character
// is one independent byte load (the per-character exp_at chain of five dependent loads made every level of a pass
// latency-bound at ~25 characters x sources).
struct ExpView { u64 coff; u32 pre_len, clen, pre_off, post_off, len; bool fwd; };
AC_HD ExpView exp_view(const ExpState& e, int32_t s) {
    u32 u = idx_of(s);
    ExpView v;
    const ExpU x = e.v[u];
    v.coff = x.coff; v.pre_len = x.pre_len; v.clen = x.clen; v.pre_off = x.pre_off; v.post_off = x.post_off;
    v.len = x.pre_len + x.clen + x.post_len;
    v.fwd = s > 0;
    return v;
}
// Branch-free addressing (selects, no control flow), so that a group of character loads can be issued back to back:
// with branches every load waited for the previous one and a level's kernel became one long latency chain.
AC_HD const u8* view_ptr(const ExpState& e, const ExpView& v, u32 i) {
    u32 i2 = i - v.pre_len;
    const u8* p_pre = e.pool + v.pre_off + i;
    const u8* p_core = e.cur + v.coff + i2;
    const u8* p_post = e.pool + v.post_off + (i2 - v.clen);
    return i < v.pre_len ? p_pre : (i2 < v.clen ? p_core : p_post);
}
AC_HD u8 comp_sel(u8 c) { u8 r = 'N'; r = c == 'A' ? (u8)'T' : r; r = c == 'C' ? (u8)'G' : r; r = c == 'G' ? (u8)'C' : r; r = c == 'T' ? (u8)'A' : r; return r; }
// Characters start .. start+7 counted from the strand's start (from_end = false) or backwards from its end (true);
// indices beyond the sequence are clamped (callers ignore those slots).
AC_HD void view_load8(const ExpState& e, const ExpView& v, bool from_end, u32 start, u8 out[8]) {
    const u32 last = v.len - 1;
#pragma unroll
    for (u32 b = 0; b < 8; b++) {
        u32 i = start + b;
        i = i > last ? last : i;
        u32 pos = (from_end == v.fwd) ? last - i : i;      // forward strand read from its end, or reverse strand read from its start
        out[b] = *view_ptr(e, v, pos);
    }
    if (!v.fwd) {
#pragma unroll
        for (u32 b = 0; b < 8; b++) out[b] = comp_sel(out[b]);
    }
}
// Pool allocation.  One counter for all junctions serialises on its cache line (same-address atomics: ~90 per microsecond, and a
// level has thousands of junctions), so the first half of the pool is split into EXP_SUBPOOLS regions with a counter each
// (a junction uses the region its position in the visiting order selects); a region that is full overflows into the second
// half, which has the one shared counter.  pool_used[0 .. EXP_SUBPOOLS) = bytes used per region, [EXP_SUBPOOLS] = of the overflow
// half.  Returns 0xFFFFFFFF (and raises the error bit) when both are exhausted.
static const u32 EXP_SUBPOOLS = 256;
AC_D u32 exp_pool_alloc(const ExpState& e, u64 key, u32 need, u32 pool_cap, u32* err) {
    const u32 sub_cap = (pool_cap / 2) / EXP_SUBPOOLS;
    const u32 sub = (u32)(key % EXP_SUBPOOLS);
    if (need <= sub_cap) {
        u32 o = atomic_add32(&e.pool_used[sub], need);
        if ((u64)o + need <= (u64)sub_cap) return sub * sub_cap + o;
    }
    const u32 ov_base = sub_cap * EXP_SUBPOOLS, ov_cap = pool_cap - ov_base;
    u32 o = atomic_add32(&e.pool_used[EXP_SUBPOOLS], need);
    if ((u64)o + need <= (u64)ov_cap) return ov_base + o;
    atomic_or32(err, 64u);
    return 0xFFFFFFFFu;
}
// avoid_start_of_path (graph_simplification.rs:164-181): trim while any forward / reverse position of the destination is <= the length.
// m = the destination's smallest position — exact, or (top bit set) only a LOWER BOUND: the walk skips occurrences further than
// POS_CAP from both ends of their sequence (graph_build.hip pos_cap(): nearly all of them, and each costs a read and often an atomic on
// a word that every copy of the unitig shares), and a word no near occurrence lowered still says "> POS_CAP" with the bit set.  Shifts
// add to / subtract from bound and exact value alike.  A bound at or above the length decides like the exact value would (no trim); one
// below it cannot: error bit 128, the build is repeated with exact positions (GraphBuilder::build).
static const u32 POS_BOUND = 0x80000000u;
AC_D u32 exp_avoid_start_of_path(u32 m, u32 amount, u32* err) {
    if (m & POS_BOUND) {
        const u32 lb = m & ~POS_BOUND;
        if (amount + 1 > lb) { atomic_or32(err, 128u); amount = lb > 0 ? lb - 1 : 0; }
        return amount;
    }
    const u32 lim = m > 0 ? m - 1 : 0;
    return amount > lim ? lim : amount;
}
// Gained sequence accumulates in the pool across passes (a side that gains again gets a new piece = new characters +
// old piece); the host rewrites the sequences contiguously after the last pass (and earlier when the pool fills up).
// One character of a strand's current sequence: index i counted from its start (from_end = false) or backwards from its end.
AC_D u8 view_char(const ExpState& e, const ExpView& v, bool from_end, u32 i) {
    const u32 last = v.len - 1;
    i = i > last ? last : i;
    const u32 pos = (from_end == v.fwd) ? last - i : i;
    const u8 c = *view_ptr(e, v, pos);
    return v.fwd ? c : comp_sel(c);
}
// The junction logic with a lane GROUP per junction.  As one thread a junction is a chain of ~25 dependent memory operations
// (links, five views, 8 characters per comparison step, copies byte by byte): every level of a pass took 20-60 us whatever its
// size.  Here the 64 lanes compare 64 characters per step, copy the gained piece and the old one in parallel, update the sources
// and mark the dirty junctions side by side: about six dependent steps.
// The sparse tail of the pass loop (round 6, expand_mopup_kernel below): what a junction visit needs beyond ExpState when ONE workgroup runs
// the remaining passes from a LIST of the dirty junctions.  dirty[c] then carries two bits: 1 = dirty, 2 = on the list.
struct MopCtx { u64* list; u32* n; const u32* prio; const u32* level; u32* next_lv; u32* moved; u32 cur_lv; };
AC_D void mop_mark(const ExpState& e, const MopCtx& m, u32 c2) {      // c2 must be looked at again: flag it, list it once, and tell the sweep if its level is still ahead
    const u32 sh = (c2 & 3u) * 8u;
    const u32 old = atomic_fetch_or32((u32*)e.dirty + (c2 >> 2), 3u << sh);
    const u32 lv = m.level[m.prio[c2]] & ~LEVEL_FINAL;
    if (!((old >> sh) & 2u)) m.list[atomic_add32(m.n, 1u)] = ((u64)lv << 32) | c2;
    if (lv > m.cur_lv) atomic_min32(m.next_lv, lv);
}
// One visit of junction c by a group of G lanes (`lane` within the group, `gshift` = the group's first lane in its wavefront); the caller
// has found it dirty and cleared the flag.  SPARSE: called from the one-workgroup tail (marks go through mop_mark, "moved" is a workgroup flag).
template <int G, bool SPARSE> AC_D void expand_junction(const ExpState& e, const u32 c, const u64 alloc_key, const int lane, const int gshift, u32 pool_cap, u32* err, const MopCtx* mop) {
    const u32 x = c >> 1;
    const bool inputs = (c & 1) == 0;
    u32 n = 0;
    const int32_t* p = e.L.next_of(inputs ? -((int32_t)x + 1) : (int32_t)x + 1, &n);
    // inputs:  forward_prev(x) = { -l : l in reverse_next(x) }   (graph_simplification.rs:233-255); outputs: forward_next(x) (:258-280)
    int32_t srcs[5];
    ExpView sv[5];
    u32 min_len = 0xFFFFFFFFu;
    bool dup = false;
#pragma unroll
    for (u32 j = 0; j < 5; j++) {
        srcs[j] = 0;
        if (j >= n) continue;
        srcs[j] = inputs ? -p[j] : p[j];
        sv[j] = exp_view(e, srcs[j]);
        if (sv[j].len < min_len) min_len = sv[j].len;
#pragma unroll
        for (u32 q = 0; q < 5; q++) if (q < j && idx_of(srcs[q]) == idx_of(srcs[j])) dup = true;
    }
    // get_common_end_seq (:298-312) / get_common_start_seq (:283-295) of the source strand sequences, G characters per step
    u32 amount = 0;
    while (amount < min_len) {
        const u32 i = amount + (u32)lane;
        const bool in = i < min_len;
        bool mism = false;
        if (in) {
            const u8 c0 = view_char(e, sv[0], inputs, i);
#pragma unroll
            for (u32 j = 1; j < 5; j++) if (j < n && view_char(e, sv[j], inputs, i) != c0) mism = true;
        }
        const u64 bal = wv::grp_ballot<G>(in && mism, gshift);
        if (bal) { amount += (u32)ctz64(bal); break; }
        amount += (min_len - amount < (u32)G) ? min_len - amount : (u32)G;
    }
    if (amount > 0) {   // avoid_zero_len_unitigs (:145-161): trim while min_source_len <= len * dup
        const u32 lim = (min_len - 1) / (dup ? 2u : 1u);
        if (amount > lim) amount = lim;
    }
    if (amount > 0) amount = exp_avoid_start_of_path(inputs ? e.minf[x] : e.minr[x], amount, err);
    if (amount == 0) return;
    const u32 old_len = inputs ? e.v[x].pre_len : e.v[x].post_len;
    const u32 old_off = inputs ? e.v[x].pre_off : e.v[x].post_off;
    u32 off = 0;
    if (lane == 0) { if (SPARSE) *mop->moved = 1; else *e.shifted = 1; off = exp_pool_alloc(e, alloc_key, amount + old_len, pool_cap, err); }
    off = (u32)wv::grp_shfl<G>((int)off, 0, gshift);
    if (off == 0xFFFFFFFFu) return;
    if (inputs) {   // shift_sequence_1 (:89-119): the LAST `amount` characters of the common suffix move onto x's start
        for (u32 j = (u32)lane; j < amount; j += G) e.pool[off + (amount - 1 - j)] = view_char(e, sv[0], true, j);
        for (u32 j = (u32)lane; j < old_len; j += G) e.pool[off + amount + j] = e.pool[old_off + j];
    } else {        // shift_sequence_2 (:122-142): the FIRST `amount` characters of the common prefix move onto x's end
        for (u32 j = (u32)lane; j < old_len; j += G) e.pool[off + j] = e.pool[old_off + j];
        for (u32 j = (u32)lane; j < amount; j += G) e.pool[off + old_len + j] = view_char(e, sv[0], false, j);
    }
    // the sources lose what the destination gained (unitig.rs:217-233).  One lane per source — unless a unitig is a source on both
    // strands: its two updates touch the same fields and keep the reference's order.
    int32_t sj = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) sj = (lane == j) ? srcs[j] : sj;
    if (!dup) {
        if ((u32)lane < n) {
            const u32 u = idx_of(sj);
            if (inputs) { if (sj > 0) { exp_remove_end(e, u, amount); e.minr[u] += amount; } else { exp_remove_start(e, u, amount); e.minf[u] += amount; } }
            else { if (sj > 0) { exp_remove_start(e, u, amount); e.minf[u] += amount; } else { exp_remove_end(e, u, amount); e.minr[u] += amount; } }
        }
    } else if (lane == 0) {
#pragma unroll
        for (u32 j = 0; j < 5; j++) {
            if (j >= n) continue;
            const u32 u = idx_of(srcs[j]);
            if (inputs) { if (srcs[j] > 0) { exp_remove_end(e, u, amount); e.minr[u] += amount; } else { exp_remove_start(e, u, amount); e.minf[u] += amount; } }
            else { if (srcs[j] > 0) { exp_remove_start(e, u, amount); e.minf[u] += amount; } else { exp_remove_end(e, u, amount); e.minr[u] += amount; } }
        }
    }
    if (lane == 0) {
        if (inputs) { e.v[x].pre_off = off; e.v[x].pre_len = amount + old_len; e.minf[x] -= amount; }       // unitig.rs:235-241
        else { e.v[x].post_off = off; e.v[x].post_len = amount + old_len; e.minr[x] -= amount; }             // unitig.rs:243-249
    }
    // Which junctions must be looked at again?  Only one that this shift may have given MORE room (round 6; rounds 2-5 marked every junction
    // touching any changed unitig: this one, the sources' other junctions, the destination's — three to five, most of which could only have
    // lost room).  What a junction (d, side) shifts is min(common facing sequence of its sources, (shortest source - 1) / dup, smallest
    // position of d on that strand - 1):
    //   * the sources' facing ends are only ever shortened, by the junction itself;
    //   * a source's LENGTH grows only when it gains at its far end, i.e. when it is the destination of a shift there;
    //   * the destination's smallest position only falls (its own gains): it could rise only if d lost sequence at that end as a source, and a
    //     unitig with two or more links there is nobody's exclusive source.
    // So after this shift the one junction with more room than before is the junction — if any — whose source x is through its OTHER end
    // (x just grew); the sources only shrank, and this junction took all it could (but see below).  (A missed visit would leave a junction that still shifts:
    // exactly what ac_verify_graph's fixed-point check reports, and what the parity tests would see as a different graph.)
    // ... with ONE exception, found by the fuzz sweep and named by the verifier's fixed-point check: with a unitig on both strands among the
    // sources (dup) the clamp is (shortest source - 1) / 2, and a shortest source that is NOT that unitig only lost `amount`, not twice
    // it — (5 - 1) / 2 = 2 moved, 3 left, (3 - 1) / 2 = 1 more in the reference's next pass.  Such a junction looks at itself again.
    if (lane == 0) {
        const V16 tt = e.touch[x];
        if (SPARSE) {
            if (tt.c != 0xFFFFFFFFu && tt.c != c) mop_mark(e, *mop, tt.c);
            if (tt.d != 0xFFFFFFFFu && tt.d != c) mop_mark(e, *mop, tt.d);
            if (dup) mop_mark(e, *mop, c);
        } else {
            if (tt.c != 0xFFFFFFFFu && tt.c != c) e.dirty[tt.c] = 1;      // x an exclusive source through its forward end
            if (tt.d != 0xFFFFFFFFu && tt.d != c) e.dirty[tt.d] = 1;      // ... through its reverse end
            if (dup) e.dirty[c] = 1;
        }
    }
}
template <int G> AC_KERNEL void __launch_bounds__(256) expand_wave_kernel(ExpState e, const u32* clist, u64 begin, u64 count, u32 pool_cap, u32* err) {
    // G lanes per junction (64, or 16: four junctions per wavefront — most shifts are a few dozen characters, and a level's time is
    // its number of wavefronts / the resident ones x one junction's dependency chain).  `lane` = lane within the group; ballots are
    // cut down to the group's bits, shuffles read the group's first lane; everything that branches does so per group.
    const int lane = (int)(wv::tid() & (G - 1));
    const int gshift = (int)(wv::tid() & 63 & ~(G - 1));     // position of the group's bits in a ballot = its first lane
    const u64 w = ((u64)wv::bid() * 256 + wv::tid()) / G;
    if (w >= count) return;                                    // group-uniform
    const u32 c = clist[begin + w];
    // unchanged since it last shifted nothing: shifts nothing again.  (The group agrees on the flag BEFORE its first lane clears it: the
    // lanes of a wavefront only run instruction by instruction on the device; the lockstep emulation orders them at cross-lane operations.)
    if (!wv::grp_ballot<G>(e.dirty[c] != 0, gshift)) return;
    if (lane == 0) e.dirty[c] = 0;
    expand_junction<G, false>(e, c, begin + w, lane, gshift, pool_cap, err, nullptr);
}
// ---- the sparse tail of the pass loop (round 6) -----------------------------------------------------------------------------------------
// With the precise dirty rule above the later passes ARE sparse: after the first two passes a one-species input has a few dozen dirty
// junctions left (of 10^5 candidates), a mixed-species one 2-3 %, after four passes 0.02 % — and yet every further pass was a launch per
// level over ALL the level's candidates (config C: passes 3-6 = 28 launches and two host checks for a handful of visits).  So behind the two
// passes of every host check MopCompactFunctor lists the dirty junctions (in level order, one atomic per wavefront) and expand_mopup_kernel —
// ONE workgroup, launched unconditionally, deciding on the device — runs ALL remaining passes if the list is short enough and the second
// pass moved something: a sweep goes through the levels that have dirty junctions in ascending order (a scan of the list per level: the
// junctions of that level into LDS, the lowest level still ahead), 32 groups of 16 lanes visit them with the kernel's own junction routine,
// a workgroup barrier where the host loop has a kernel boundary (one CU: its waves share the L1, no agent-scope fence as the retired grid-wide
// forms needed); a junction marked during the sweep joins the list (once: the "listed" bit) and the sweep, if its level is still ahead — the
// semantics of the level launches, pass for pass.  The dirty flags stay the truth and the list an index into them: the kernel stops at a
// sweep boundary when a pool region fills up or the list outgrows it, and the host loop goes on from the flags.
static const u32 MOP_THREADS = 512, MOP_BATCH = 4096;
struct MopCompactFunctor {      // launch_full over the candidates (in level order): the dirty ones onto the list, their "listed" bits set, everybody else's cleared
    const u32* clist; const u64* lkey; u8* dirty; u64* list; u32* n; u64 C;
    AC_D void operator()(u64 idx, bool valid) const {
        valid = valid && idx < C;
        const u32 c = valid ? clist[idx] : 0u;
        const u8 b = valid ? dirty[c] : (u8)0;
        const bool is = (b & 1u) != 0;
        const u64 bal = wv::ballot(is);
        if (valid && !is && b) dirty[c] = 0;
        if (!bal) return;
        const int lane = wv::lane();
        u32 base = 0;
        if (lane == (int)ctz64(bal)) base = atomic_add32(n, (u32)popc64(bal));
        base = (u32)wv::shfl((int)base, (int)ctz64(bal));
        if (is) {
            list[base + (u32)popc64(bal & ((1ULL << lane) - 1))] = (lkey[idx] << 32) | c;
            dirty[c] = 3;
        }
    }
};
struct MopState { u64* list; u32* n; const u32* prio; const u32* level; const u64* sh_words; u32* out; u32 max_start, max_list, sub_limit, batch; };      // batch <= MOP_BATCH (smaller in tests: the straight-from-the-list branch)
// out[0]: 0 = did not run (list too long, or the passes before it had already finished), 1 = ran to the fixed point, 2 = stopped at a sweep
// boundary (the host loop goes on); out[1]: sweeps = passes of the reference (the last one of status 1 moved nothing); out[2]: the list at its start
template <int UNUSED> AC_KERNEL void __launch_bounds__(512) expand_mopup_kernel(ExpState e, MopState m, u32 pool_cap, u32* err) {      // (a template only so that every translation unit may hold a copy)
    AC_SHARED u32 s_batch[MOP_BATCH];
    AC_SHARED u32 s_cnt, s_next, s_moved, s_stop, s_run;
    const u32 tid = wv::tid();
    const int lane = (int)(tid & 15u);
    const int gshift = (int)(tid & 63u & ~15u);
    const u32 grp = tid >> 4, n_grp = MOP_THREADS / 16;
    if (tid == 0) {
        const u32 n0 = atomic_load32(m.n);
        s_run = (m.sh_words[0] != 0 && m.sh_words[1] != 0 && n0 <= m.max_start) ? 1u : 0u;
        m.out[2] = n0;
    }
    wv::block_sync();
    if (!s_run) { if (tid == 0) { m.out[0] = 0; m.out[1] = 0; *m.n = 0; } return; }
    MopCtx mc{m.list, m.n, m.prio, m.level, &s_next, &s_moved, 0};
    u32 sweeps = 0, status = 0;
    for (;;) {
        if (tid == 0) s_moved = 0;
        u32 lv = 0;      // (levels start at 1: the first scan of a sweep only finds the lowest level with a dirty junction)
        for (;;) {
            if (tid == 0) { s_cnt = 0; s_next = 0xFFFFFFFFu; }
            wv::block_sync();
            const u32 n = atomic_load32(m.n);
            for (u32 i = tid; i < n; i += MOP_THREADS) {
                const u64 ent = m.list[i];
                const u32 c = (u32)ent, l = (u32)(ent >> 32);
                if (!((atomic_load32((const u32*)e.dirty + (c >> 2)) >> ((c & 3u) * 8u)) & 1u)) continue;
                if (l == lv) { const u32 slot = atomic_add32(&s_cnt, 1u); if (slot < m.batch) s_batch[slot] = c; }
                else if (l > lv) atomic_min32(&s_next, l);
            }
            wv::block_sync();
            const u32 cnt = s_cnt;
            mc.cur_lv = lv;
            // a visit claims its junction (the dirty bit off, atomically: whoever finds it set runs it) — the list holds every junction once,
            // and one that marks ITSELF again (dup) is dirty for the next sweep, not for this level a second time
            if (cnt <= m.batch) {
                for (u32 b = grp; b < cnt; b += n_grp) {
                    const u32 c = s_batch[b];
                    u32 ok = 0;
                    if (lane == 0) { const u32 sh = (c & 3u) * 8u; ok = (atomic_fetch_and32((u32*)e.dirty + (c >> 2), ~(1u << sh)) >> sh) & 1u; }
                    ok = (u32)wv::grp_shfl<16>((int)ok, 0, gshift);
                    if (ok) expand_junction<16, true>(e, c, c, lane, gshift, pool_cap, err, &mc);
                }
            } else {      // more junctions of one level than the LDS batch holds: straight from the list (each index once per level)
                for (u32 i = grp; i < n; i += n_grp) {
                    const u64 ent = m.list[i];
                    const u32 c = (u32)ent;
                    u32 ok = 0;
                    if (lane == 0 && (u32)(ent >> 32) == lv) { const u32 sh = (c & 3u) * 8u; if ((atomic_load32((const u32*)e.dirty + (c >> 2)) >> sh) & 1u) ok = (atomic_fetch_and32((u32*)e.dirty + (c >> 2), ~(1u << sh)) >> sh) & 1u; }
                    ok = (u32)wv::grp_shfl<16>((int)ok, 0, gshift);
                    if (ok) expand_junction<16, true>(e, c, c, lane, gshift, pool_cap, err, &mc);
                }
            }
            wv::block_sync();
            const u32 nx = s_next;
            wv::block_sync();      // (everybody has read it before the next step resets it)
            if (nx == 0xFFFFFFFFu) break;
            lv = nx;
        }
        sweeps++;
        if (!s_moved) { status = 1; break; }
        if (tid == 0) s_stop = 0;
        wv::block_sync();
        if (tid <= EXP_SUBPOOLS) { const u32 used = atomic_load32(e.pool_used + tid); if (tid < EXP_SUBPOOLS ? used > m.sub_limit : used != 0) s_stop = 1; }
        if (tid == 0 && atomic_load32(m.n) > m.max_list) s_stop = 1;
        wv::block_sync();
        if (s_stop) { status = 2; break; }
    }
    if (tid == 0) { m.out[0] = status; m.out[1] = sweeps; *m.n = 0; }
}
// ---- grid-wide barriers instead of launches: measured and retired (round 5) -----------------------------------------------------------
// The level loop above is a kernel per level and pass (config C: 42 launches, 0.74 ms for ~0.3 ms of junction work), the relaxation a
// kernel per sweep.  Both were rebuilt as ONE launch of resident workgroups that meet at a counter where the host has a kernel boundary,
// and both lost.  What such a barrier costs on the eight XCDs of gfx950 (tools/microbench/grid_barrier_bench.hip,
// profiles/r12o_grid_barrier_bench.jsonl):
//     workgroups                                   8      64     128     256     1024
//     with agent-scope release / acquire fences   1.7    4.7    9.1    17.7     96 us     (the cooperative-groups barrier: every
//     the counter alone                           1.0    1.6    2.3     4.1     17 us      workgroup writes back and invalidates its L2)
// expand_repeats needs the fences (its junctions share unitig views, pool bytes and dirty flags through plain loads and stores): at the
// width of the device config C's expand stage took 6.1 ms instead of 0.74 (r12n); a 64-workgroup grid that picks the dirty junctions of
// its level, behind a first pass launched level by level, 1.83 ms (E' 13.6 instead of 4.7, mini-E 43.5 instead of 14.3: r12p) — a pass
// of config C still has thousands of dirty junctions per level, and their dependent loads want the device's width, which a launch gives
// for ~12 us.  The relaxation can run fence-free (its levels are the only shared data, read and written with agent-scope atomics): seven
// launches fewer, the same time (C 0.80 vs 0.74 ms, E' 4.55 vs 4.68, D 2.30 vs 2.20: r12q).
// Nor are the later passes sparse enough for a lane per junction to pay (the wavefront reads 64 dirty flags, its four lane groups then run
// the dirty ones four at a time: sixteen times fewer wavefronts per level): config C 1.15 instead of 0.74 ms, E' 5.58 instead of 4.66,
// D 2.48 / 2.20, the 8-species job 3.54 / 3.14 (r12x) — most junctions of a level ARE dirty again in the next pass, and sixteen deep
// is slower than sixteen wide.  The stage is bound by its junction visits (E': ~9.4 M of them in 4.7 ms), not by its launches.
// ---- expand_repeats of ONE job over several devices: the junctions partitioned by conflict component (round 4, DESIGN.md §7) ----------
// Two candidate junctions depend on each other only if they share a unitig (the conflict edges LevelPredsFunctor lists: what the level
// schedule rests on), so the connected components of that relation can run on different ranks.  A component's label is its smallest
// candidate (union-find, the larger root hooked under the smaller: the same forest whatever order the atomics land in), its rank a hash
// of the label.  A rank only ever marks its own junctions dirty, so every kernel of the pass loop skips the rest.  What a rank's
// junctions did to the unitigs is then merged FIELD by field: a unitig that is a source of some junction has all its junctions in one
// component (they all touch it) and one owner; one that never is a source keeps its core as it was and may have gained a prefix from one
// rank (its start junction) and a suffix from another (its end junction) — [gained prefix | core | gained suffix], each field written
// by its owner, the lengths and then the bytes summed over the ranks (disjoint contributions, like every other exchange of the build).
struct UfInitFunctor { u32* parent; AC_HD void operator()(u64 i) const { parent[i] = (u32)i; } };
AC_D u32 uf_find(u32* parent, u32 x) {
    for (;;) {
        const u32 p = atomic_load32(parent + x);
        if (p == x) return x;
        const u32 g = atomic_load32(parent + p);
        if (g != p) parent[x] = g;      // path halving: p is an ancestor of x, so is g (a plain store: any ancestor is a valid value)
        x = p;
    }
}
struct UfUnionFunctor {      // candidate ci with each of the earlier candidates it conflicts with
    const u32* preds; const u8* npred; u64 C; u32* parent;
    AC_D void operator()(u64 ci) const {
        const u32 np = npred[ci];
        for (u32 j = 0; j < np; j++) {
            u32 a = (u32)ci, b = preds[(u64)j * C + ci];
            for (;;) {
                a = uf_find(parent, a); b = uf_find(parent, b);
                if (a == b) break;
                if (a < b) { const u32 t = a; a = b; b = t; }      // a > b: the larger root goes under the smaller
                if (atomic_cas32(parent + a, a, b) == a) break;
            }
        }
    }
};
AC_HD u32 comp_owner(u32 label, u32 n_owners) { return (u32)(((u64)label * 0x9E3779B1ULL) >> 12) % n_owners; }
struct UfOwnerFunctor { u32* parent; u32 n_owners; u8* jowner; AC_D void operator()(u64 ci) const { jowner[ci] = (u8)comp_owner(uf_find(parent, (u32)ci), n_owners); } };
// dirty[c] = c is a candidate of a component this rank owns; count = how many
struct OwnedDirtyFunctor {
    const u8* cand; const u32* prio; const u8* jowner; u32 me; u8* dirty; u32* count; u64 J;
    AC_D void operator()(u64 c, bool valid) const {
        const bool mine = valid && c < J && cand[c] && jowner[prio[c]] == me;
        if (valid && c < J) dirty[c] = mine ? 1 : 0;
        const u32 o = wave_alloc32(count, mine ? 1u : 0u);
        (void)o;
    }
};
// fown[3u .. 3u+2] = the ranks that write unitig u's gained prefix, core and gained suffix (a single-owner unitig: all three the same)
struct FieldOwnerFunctor {
    OrderedLinks L; const u8* cand; const u32* prio; const u8* jowner; u32 n_owners; u8* fown;
    AC_HD void operator()(u64 u) const {
        u32 t[4];
        touchers(L, cand, (u32)u, t);
        const u8 dflt = (u8)(u % n_owners);
        u8 pre, core, post;
        if (t[2] != 0xFFFFFFFFu || t[3] != 0xFFFFFFFFu) pre = core = post = jowner[prio[t[2] != 0xFFFFFFFFu ? t[2] : t[3]]];      // a source: one component
        else {
            core = dflt;
            pre = t[0] != 0xFFFFFFFFu ? jowner[prio[t[0]]] : dflt;
            post = t[1] != 0xFFFFFFFFu ? jowner[prio[t[1]]] : dflt;
        }
        fown[3 * u] = pre; fown[3 * u + 1] = core; fown[3 * u + 2] = post;
    }
};
// A rank-local rewrite folds the gained pieces into the core view: gpre / gpost remember how much of it is gained prefix / suffix
// (only read for unitigs that are never a source: their core is never trimmed).
struct ExpFoldFunctor { ExpState e; u32* gpre; u32* gpost; AC_HD void operator()(u64 u) const { gpre[u] += e.v[u].pre_len; gpost[u] += e.v[u].post_len; } };
// This rank's view of unitig u as [prefix | core | suffix]: lengths of the three fields
AC_HD void field_lens(const ExpState& e, const u8* fown, const u32* gpre, const u32* gpost, u32 u, u32 f[3]) {
    const u32 whole = exp_len(e, u);
    if (fown[3 * (u64)u] == fown[3 * (u64)u + 1] && fown[3 * (u64)u + 1] == fown[3 * (u64)u + 2]) { f[0] = whole; f[1] = 0; f[2] = 0; return; }
    f[0] = gpre[u] + e.v[u].pre_len; f[2] = gpost[u] + e.v[u].post_len; f[1] = whole - f[0] - f[2];
}
struct OwnedLensFunctor {      // lens3[3u + f] = the length of field f if this rank writes it, else 0
    ExpState e; const u8* fown; const u32* gpre; const u32* gpost; u32 me; int32_t* lens3;
    AC_HD void operator()(u64 u) const {
        u32 f[3];
        field_lens(e, fown, gpre, gpost, (u32)u, f);
        for (int q = 0; q < 3; q++) lens3[3 * u + q] = fown[3 * u + q] == me ? (int32_t)f[q] : 0;
    }
};
struct Lens3SumFunctor { const int32_t* lens3; u64* len64; u32 n_unitigs; AC_HD void operator()(u64 u) const { len64[u] = u < n_unitigs ? (u64)lens3[3 * u] + (u64)lens3[3 * u + 1] + (u64)lens3[3 * u + 2] : 0; } };
// The merged sequences: byte g of the final layout (noff from the SUMMED field lengths) if this rank writes its field, else 0
struct MergeSeqFunctor {
    ExpState e; const u8* fown; const u32* gpre; const u32* gpost; u32 me; const int32_t* lens3 /* summed */; const u64* noff; u32 n_unitigs; u64 total; u8* out; u32 per;
    AC_HD void operator()(u64 tid) const {
        const u64 g0 = tid * per;
        if (g0 >= total) return;
        u32 lo = 0, hi = n_unitigs;   // largest r with noff[r] <= g0
        while (hi - lo > 1) { u32 mid = lo + ((hi - lo) >> 1); if (noff[mid] <= g0) lo = mid; else hi = mid; }
        u32 r = lo;
        for (u32 j = 0; j < per; j++) {
            const u64 g = g0 + (u64)j;
            if (g >= total) break;
            while (g >= noff[r + 1]) r++;
            u32 i = (u32)(g - noff[r]);
            const u32 P = (u32)lens3[3 * (u64)r], Cn = (u32)lens3[3 * (u64)r + 1];
            const int fld = i < P ? 0 : (i < P + Cn ? 1 : 2);
            u8 v = 0;
            if (fown[3 * (u64)r + fld] == me) {
                u32 f[3];
                field_lens(e, fown, gpre, gpost, r, f);      // this rank's own boundaries: it may hold fields it does not write
                const u32 in_field = i - (fld == 0 ? 0 : (fld == 1 ? P : P + Cn));
                v = exp_at(e, r, in_field + (fld == 0 ? 0 : (fld == 1 ? f[0] : f[0] + f[1])));
            }
            out[g] = v;
        }
    }
};
struct FillU32Functor { u32* a; u32 v; AC_HD void operator()(u64 i) const { a[i] = v; } };
struct ExpInitFunctor {      // expand_repeats starts from the unitigs as they are: core offsets / lengths, and every candidate junction dirty
    const u64* off; const u32* len; const u8* cand; ExpU* v; u64* coff; u32* clen; u8* dirty;      // coff / clen: the same two as plain arrays (what the stages behind expand_repeats read)
    AC_HD void operator()(u64 u) const {
        v[u] = ExpU{off[u], len[u], 0, 0, 0, 0, 0};
        coff[u] = off[u]; clen[u] = len[u]; dirty[2 * u] = cand[2 * u]; dirty[2 * u + 1] = cand[2 * u + 1];
    }
};
// The candidate junctions that read or write each unitig (touchers): static, so looked up once instead of ~8 random reads per changed
// unitig of every junction that moves something.
struct TouchFunctor {
    OrderedLinks L; const u8* cand; V16* touch;
    AC_HD void operator()(u64 u) const { u32 t[4]; touchers(L, cand, (u32)u, t); touch[u] = V16{t[0], t[1], t[2], t[3]}; }
};
struct ExpLenFunctor {
    ExpState e; u64* len64; u32 n_unitigs;
    AC_HD void operator()(u64 u) const { len64[u] = u < n_unitigs ? (u64)exp_len(e, (u32)u) : 0; }
};
struct MaterializeFunctor {   // `per` output bytes per thread: the emulation's form, and the device's for small outputs (else seq_write_kernel<1>)
    ExpState e; const u64* noff; u32 n_unitigs; u64 total_in; u8* out; u32 per;
    bool total_on_device;      // total_in is only a bound (the launch's size): the sum is noff[n_unitigs], still on its way to the host
    AC_HD void operator()(u64 tid) const {
        const u64 total = total_on_device ? noff[n_unitigs] : total_in;
        const u64 g0 = tid * per;
        if (g0 >= total) return;
        u32 lo = 0, hi = n_unitigs;   // largest r with noff[r] <= g0
        while (hi - lo > 1) { u32 mid = lo + ((hi - lo) >> 1); if (noff[mid] <= g0) lo = mid; else hi = mid; }
        u32 r = lo;
        for (u32 j = 0; j < per; j++) {
            const u64 g = g0 + (u64)j;
            if (g >= total) break;
            while (g >= noff[r + 1]) r++;
            out[g] = exp_at(e, r, (u32)(g - noff[r]));
        }
    }
};
struct ExpResetFunctor {
    ExpState e; const u64* noff; u64* coff; u32* clen;
    AC_HD void operator()(u64 u) const {
        const u32 len = (u32)(noff[u + 1] - noff[u]);
        e.v[u] = ExpU{noff[u], len, 0, 0, 0, 0, 0};
        coff[u] = noff[u]; clen[u] = len;
    }
};

// ---- K16: finalisation in the final numbering -----------------------------------------------------------------
struct FinalMetaFunctor {   // per final index i
    const u32* order2; const u64* foff; const u32* flen; const u32* depth; const u8* lcnt;
    u64* number_len; u64* seq_begin; double* depth_out; u32* seq_len; u64* lcount;
    u32* number_only;      // optional: the final number alone, by TEXT-order index (what the host's path renumbering gathers from)
    u32* seed_index;       // optional: the seed-order index of final unitig i (FinalGraph::seed_index)
    const u32* text_of_seed; u64* number_len_text;      // the path entries are in text-order numbers (kernels_paths.inc): their table
    const u8* uorient;      // ... with text-relative signs: the table's numbers are SIGNED — negative where the unitig's forward strand lies against its first occurrence
    AC_HD void operator()(u64 i) const {
        u32 r = order2[i];
        if (seed_index) seed_index[i] = r;
        const u64 nl = ((u64)flen[r] << 32) | (u64)(i + 1);
        number_len[r] = nl;
        const u32 u = text_of_seed[r];
        const int32_t signed_number = uorient[r] ? (int32_t)(i + 1) : -(int32_t)(i + 1);
        number_len_text[u] = ((u64)flen[r] << 32) | (u64)(u32)signed_number;
        if (number_only) number_only[u] = (u32)signed_number;
        seq_begin[i] = foff[r];
        depth_out[i] = (double)depth[r];
        seq_len[i] = flen[r];
        lcount[i] = (u64)lcnt[2 * (u64)r] + (u64)lcnt[2 * (u64)r + 1];
    }
};
struct LinkOutFunctor {     // get_links_for_gfa (unitig_graph.rs:333-350): per final unitig, forward_next then reverse_next
    const u32* order2; OrderedLinks L; const u64* number_len; const u64* loff; Link* out;
    AC_HD void operator()(u64 i) const {
        u32 r = order2[i];
        u64 w = loff[i];
        for (int side = 0; side < 2; side++) {
            u32 n; const int32_t* p = L.next_of(side == 0 ? (int32_t)r + 1 : -((int32_t)r + 1), &n);
            for (u32 j = 0; j < n; j++) {
                Link l; l.a = side == 0 ? (int32_t)(i + 1) : -(int32_t)(i + 1);
                const int32_t nb = (int32_t)(number_len[idx_of(p[j])] & 0xFFFFFFFFu); l.b = p[j] > 0 ? nb : -nb;
                out[w++] = l;
            }
        }
    }
};
// The final sequences as 2-bit codes for the way to the host (SeqExpandJob): a thread packs 32 bytes into one word, base i in bits 2i, 2i + 1.
// Trimmed unitig sequences hold A, C, G, T only; any other byte is counted (the build then sends the bytes themselves).
struct SeqPack2Functor {
    const u8* seq; u64 total; u64* words; u32* bad;
    AC_D void operator()(u64 w) const {
        const u64 b = w * 32;
        u64 x = 0; u32 wrong = 0;
        for (u32 i = 0; i < 32 && b + i < total; i++) {
            const u32 ch = seq[b + i];
            wrong += (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') ? 1u : 0u;
            x |= (u64)(((ch >> 1) ^ (ch >> 2)) & 3u) << (2 * i);
        }
        words[w] = x;
        if (wrong) atomic_add32(bad, wrong);
    }
};
struct RemapFunctor {       // seed numbers -> final numbers, per-sequence length sums.  A wavefront owns `block` consecutive
    int32_t* path; const u64* number_len; const u64* path_off; u32 n_seqs; u64 n_ent; u64* sums; u64 first_wave; u32 block;   // entries; lane l takes l, l+64, ...
    int32_t* host_out;      // optional: the caller's pinned result block, written straight from here (64 lanes x 4 B = one 256-byte PCIe write per step)
    bool store;             // false: only the sums (the entries get their final numbers on the host, PathRemapJob)
    AC_D void operator()(u64 tid, bool valid) const {
        if (!valid) return;   // the launch is a whole number of wavefronts, so this is wavefront-uniform
        const u64 wave = first_wave + (tid >> 6);
        const u32 lane = (u32)(tid & 63);
        const u64 w0 = wave * (u64)block;
        u64 w1 = w0 + (u64)block;
        if (w1 > n_ent) w1 = n_ent;
        u32 s = 0;
        u64 acc = 0;
        u64 i = w0 + lane;
        if (i < w1) {
            u32 lo = 0, hi = n_seqs;   // largest s with path_off[s] <= i
            while (hi - lo > 1) { u32 mid = lo + ((hi - lo) >> 1); if (path_off[mid] <= i) lo = mid; else hi = mid; }
            s = lo;
        }
        for (; i < w1; i += 64) {
            while (s + 1 < n_seqs && i >= path_off[s + 1]) { if (acc) atomic_add64(&sums[s], acc); acc = 0; s++; }
            int32_t v = path[i];
            u64 nl = number_len[idx_of(v)];
            int32_t f = (int32_t)(nl & 0xFFFFFFFFu);
            const int32_t o = v > 0 ? f : -f;
            if (store) path[i] = o;
            if (host_out) host_out[i] = o;
            acc += nl >> 32;
        }
        // usually the whole wavefront ends inside one sequence: one atomic instead of 64 to the same address
        const u32 s0 = (u32)wv::shfl((int)s, 0);
        if (wv::all(s == s0 || acc == 0)) {
            u64 t = acc;
#pragma unroll
            for (int o = 32; o; o >>= 1) t += (u64)wv::shfl_xor64((unsigned long long)t, o);
            if (lane == 0 && t) atomic_add64(&sums[s0], t);
            return;
        }
        if (acc) atomic_add64(&sums[s], acc);
    }
};

// ---- K12: trimmed unitig sequences (unitig.rs:113-166) -----------------------------------------------------
// SeqFunctor / MaterializeFunctor: a thread writes `per` consecutive output bytes after a binary search for the unitig its first
// byte belongs to — the emulation's form and the definition of the result; the device uses it for small outputs with 16 bytes per
// thread (the search and the byte loop are one dependent chain per thread, and 64 bytes per thread leave most of the chip idle:
// config C 7.8 MB, 0.14 ms at 64, see DESIGN.md §4 K12).  The device runs seq_write_kernel (below): the
// search (17-21 dependent loads per thread, for 64 bytes of output) is replaced by one load from an index of "which unitig holds
// byte 64 b" (one atomicMax per unitig + a max-scan), bases come 32 at a time from the packed text, and a workgroup's 16 KB go
// through LDS so that the global stores are 16 bytes per lane and coalesced (byte stores 64 bytes apart per lane before).
struct SeqFunctor {
    const u64* bits; const u64* useq_off; const u64* ustartpos; const u32* ulen; const u8* uorient;
    u32 n_unitigs; u64 total; int h; u8* out; u32 per;      // per: output bytes per thread
    AC_HD void operator()(u64 tid) const {
        const u64 g0 = tid * per;
        if (g0 >= total) return;
        u32 lo = 0, hi = n_unitigs;   // largest r with useq_off[r] <= g0
        while (hi - lo > 1) { u32 mid = lo + ((hi - lo) >> 1); if (useq_off[mid] <= g0) lo = mid; else hi = mid; }
        u32 r = lo;
        for (u32 j = 0; j < per; j++) {
            const u64 g = g0 + (u64)j;
            if (g >= total) break;
            while (g >= useq_off[r] + (u64)ulen[r]) r++;
            u64 i = g - useq_off[r];
            u32 n = ulen[r];
            u32 c;
            if (uorient[r]) c = text_code(bits, ustartpos[r] + (u64)h + i);
            else c = 3u - text_code(bits, ustartpos[r] + (u64)h + ((u64)n - 1 - i));
            out[g] = (u8)("ACGT"[c]);
        }
    }
};
// Index for the device writers: first[b] = the unitig that holds output byte 64 b = the largest r with off[r] <= 64 b, i.e. the
// running maximum over blocks of max{ r : ceil(off[r] / 64) == b }.
struct BlockMaxFunctor {
    const u64* off; u32 n_unitigs; u64 n_blocks; u32* m;
    AC_D void operator()(u64 r) const {
        const u64 b = (off[r] + 63) / 64;
        if (b < n_blocks) atomic_max32(&m[b], (u32)r);
    }
};
AC_D u8 base_char(u32 c) { return (u8)((0x54474341u >> (8 * c)) & 0xFFu); }      // "ACGT"[c]
// MODE 0: K12 (bases of unitig r from the packed text, reverse-complemented when the unitig's forward strand is the text's
// reverse); MODE 1: the rewrite after expand_repeats (bytes of [gained prefix][core][gained suffix]).
struct SeqSrc { const u64* bits; const u64* ustartpos; const u32* ulen; const u8* uorient; int h; };
template <int MODE>
AC_KERNEL void __launch_bounds__(256) seq_write_kernel(SeqSrc q, ExpState e, const u64* off, const u32* first, u32 n_unitigs, u64 total, u8* out) {
    AC_SHARED u32 tile[16 * 257];      // word w of thread t at [w * 257 + t]: conflict-free on the way in, two-way on the way out
    const u32 t = wv::tid();
    const u64 tid = (u64)wv::bid() * 256 + t;
    const u64 g0 = tid * 64;
    if (g0 < total) {
        u32 r = first[tid];
        u64 g = g0;
        const u64 g_end = (g0 + 64 < total) ? g0 + 64 : total;
        u32 acc = 0; int j = 0;
        while (g < g_end) {
            u64 o = off[r]; u64 o_next = (r + 1 < n_unitigs) ? off[r + 1] : total;
            while (g >= o_next) { r++; o = o_next; o_next = (r + 1 < n_unitigs) ? off[r + 1] : total; }
            const u32 i0 = (u32)(g - o);
            const u32 cnt = (u32)(((o_next < g_end) ? o_next : g_end) - g);
            if (MODE == 0) {
                const u32 n = q.ulen[r];
                const bool fwd = q.uorient[r] != 0;
                const u64 base = q.ustartpos[r] + (u64)q.h;
                for (u32 d = 0; d < cnt; d += 32) {
                    // 32 bases from offset i0 + d of the unitig: forward = text positions base + i .., reverse = complement of base + n-1-i downwards
                    const u64 w = fwd ? text_word(q.bits, base + i0 + d) : text_word_rc(q.bits, base + (u64)n - 1 - (i0 + d));
                    const u32 m = cnt - d < 32 ? cnt - d : 32;
                    for (u32 x = 0; x < m; x++) {
                        acc |= (u32)base_char((u32)(w >> (62 - 2 * x)) & 3u) << (8 * (j & 3));
                        if ((j & 3) == 3) { tile[(j >> 2) * 257 + t] = acc; acc = 0; }
                        j++;
                    }
                }
            } else {
                const ExpView v = exp_view(e, (int32_t)r + 1);
                for (u32 x = 0; x < cnt; x++) {
                    acc |= (u32)(*view_ptr(e, v, i0 + x)) << (8 * (j & 3));
                    if ((j & 3) == 3) { tile[(j >> 2) * 257 + t] = acc; acc = 0; }
                    j++;
                }
            }
            g += cnt;
        }
        if (j & 3) tile[(j >> 2) * 257 + t] = acc;      // the text's last, partial word
    }
    wv::block_sync();
    // the workgroup's 16 KB, coalesced: lane-consecutive 16-byte pieces
    const u64 block_base = (u64)wv::bid() * 256 * 64;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const u32 piece = (u32)pass * 256 + t;                 // 16-byte piece of the tile
        const u64 gb = block_base + (u64)piece * 16;
        if (gb >= total) continue;
        const u32 owner = piece >> 2, w0 = (piece & 3) * 4;   // thread whose 64 bytes hold it, first word inside them
        V16 v;
        v.a = tile[(w0 + 0) * 257 + owner]; v.b = tile[(w0 + 1) * 257 + owner]; v.c = tile[(w0 + 2) * 257 + owner]; v.d = tile[(w0 + 3) * 257 + owner];
        if (gb + 16 <= total) *(V16*)(out + gb) = v;
        else { const u8* pb = (const u8*)&v; for (u64 x = 0; gb + x < total; x++) out[gb + x] = pb[x]; }
    }
}

