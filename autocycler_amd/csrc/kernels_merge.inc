// The linear-path merge plan — merge_linear_paths, merge_path, delete_dangling_links (graph_simplification.rs:315-371, 410-485) as a
// read-only analysis ON THE DEVICE — part of graph_extras.hip (included inside namespace ac; not a translation unit of its own).  The host
// side (merge_host.cpp) seeds the fixed sets from the path ends and applies the depth and type rules to what comes back.
//
// The reference's loop is sequential (already_used, graph order, + before -).  Where the link entries among alive unitigs are a set that
// is closed under reverse complement it has an order-free form, and that is what runs here:
//   an oriented unitig x = (u, strand) is node 2 (u - 1) + (strand is reverse); its reverse complement is x ^ 1
//   out(x)            get_exclusive_outputs(u) for +, get_exclusive_inputs(u) with the strands flipped for - (:233-280, :346-349), where it
//                     has exactly one entry
//   valid join x->y   !cannot_merge_end(x) && out(x) == [y] && !cannot_merge_start(y); a node has at most one join in and one out, and the
//                     reverse complement of a join is a join: the joins form paths and cycles that come in mirrored pairs
//   literal head x    !(has_single_exclusive_input(x) && can_merge_start(x)) (:338).  A literal head has no join coming in, so it starts a
//                     maximal join path; the start of a maximal join path need not be a literal head (its predecessor's END may be fixed)
//   chain             a maximal join path of two or more members, in the orientation whose start is a literal head; where both starts
//                     are, the one whose unitig has the lower number (the reference meets it first).  Cycles have no head: nothing merges
// Duplicated entries or a missing reverse complement are an error, found here by a radix sort of the entries' keys.
//
// Stages, all on stream 0, nothing read by the host in between (the components and loop flags come from components_device, before):
//   histogram   (handles with paths) the signed path entries per unitig and strand: the position counts
//   init        fixed[u] = seed[u] (path ends; the lowest member of every circular loop)
//   census      one pass over the entries: alive filter, the four list lengths per unitig with one target each (read only where the list
//               has one entry), the one-level propagation of the fixed seeds (:213-227), the entry's key
//   radix sort  the keys; check: equal neighbours are duplicates, a binary search for every key's mirror image
//   succ        per node: out, the literal-head flag, and the valid join to its successor (succ / pred)
//   rank        list ranking by pointer jumping over pred, ceil(log2 n) + 1 rounds on two buffers: (start, hops, bases before)
//   select      per path end: which orientation is emitted; scan of the flags over the unitigs: the chain index
//   compact     per-chain members and length by chain index; two scans: member_off and seq_off
//   members     per node of an emitted chain: members[member_off + hops], chain_of_unitig, the member's offset in the merged bytes
//   records     per chain: the record; the loop flag by a binary search for the link last -> first among the sorted keys
//   relabel     per entry: dropped (dead, or a join inside a chain) or its endpoints mapped to the merged numbers; radix sort; decode
//   (header read-back: errors, chains, members, bases, links)
//   copy        the merged sequences, partitioned by OUTPUT: a wavefront owns 4 KB of merged bytes and finds their members by a 64-way search
//               of the member offsets, a lane owns four 16-byte pieces 1 KB apart and finds each by a binary search inside that range
// No loop bound and no launch count grows with the length of a chain.
static const u32 MERGE_NONE = 0xFFFFFFFFu;
static const u32 MERGE_ERR_INTERNAL = 1;
struct MergeCounts { u64 n_chains, n_members, n_bases, n_links_after, reserved[2]; };      // zeroed; with the two error words: the 64-byte header

AC_D u32 merge_node(int32_t e) { return e > 0 ? 2u * ((u32)e - 1u) : 2u * ((u32)(-(int64_t)e) - 1u) + 1u; }
AC_D int32_t merge_signed(u32 x) { return (x & 1u) ? -(int32_t)((x >> 1) + 1u) : (int32_t)((x >> 1) + 1u); }
AC_D u64 merge_key(int64_t a, int64_t b, u64 offset, int key_bits) { return ((u64)(a + (int64_t)offset) << key_bits) | (u64)(b + (int64_t)offset); }
// is `k` among key[0, n) (ascending)?
AC_D bool merge_has_key(const u64* key, u64 n, u64 k) {
    u64 lo = 0, hi = n;
    for (int it = 0; it < 64 && lo < hi; it++) {
        const u64 mid = lo + (hi - lo) / 2;
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < n && key[lo] == k;
}

struct MergeHistogramFunctor {
    const int32_t* path; u32 n; u32* fwd; u32* rev;
    AC_D void operator()(u64 i) const {
        const int64_t e = path[i];
        const int64_t u = e < 0 ? -e : e;
        if (u == 0 || u > (int64_t)n) return;
        atomic_add32(e > 0 ? &fwd[u - 1] : &rev[u - 1], 1u);
    }
};

// seed[u]: MERGE_FIXED_START / MERGE_FIXED_END from the path ends — what the census propagates one level — and MERGE_SEED_LOOP for the lowest
// member of a circular loop, which fix_circular_loops adds to the fixed starts after the propagation
static const u8 MERGE_SEED_LOOP = 0x80;
struct MergeInitFunctor {
    const u8* seed; u32* fixed;
    AC_D void operator()(u64 u) const { fixed[u] = (u32)(seed[u] & 3u) | ((seed[u] & MERGE_SEED_LOOP) ? (u32)MERGE_FIXED_START : 0u); }
};

struct MergeCensusFunctor {
    const Link* links; u32 n; const u8* alive; const u8* seed; int key_bits;
    u32* deg; int32_t* target; u32* fixed; u64* key; u32* key_index;
    AC_D void operator()(u64 i) const {
        const int64_t a = links[i].a, b = links[i].b;
        key[i] = link_key_dropped(key_bits); key_index[i] = (u32)i;
        LinkEnds e;
        if (link_ends(links[i], n, alive, &e) != LINK_OK) return;      // (components_device has refused the entries that name no unitig already)
        const u32 ua = e.ua, ub = e.ub;
        link_into_lists(links[i], e, n, deg, target);
        {
            // a is in b's forward_prev: upstream of a fixed start (:214-219); b is in a's forward_next: downstream of a fixed end (:222-227)
            if (b > 0 && (seed[ub] & MERGE_FIXED_START)) atomic_or32(&fixed[ua], a > 0 ? MERGE_FIXED_END : MERGE_FIXED_START);
            if (a > 0 && (seed[ua] & MERGE_FIXED_END)) atomic_or32(&fixed[ub], b > 0 ? MERGE_FIXED_START : MERGE_FIXED_END);
        }
        key[i] = merge_key(a, b, n, key_bits);
    }
};

// key[j] ascending (dropped entries last), key_index[j] = the entry's index; the sort is stable: equal keys keep their entries' order
struct MergeLinkCheckFunctor {
    const u64* key; const u32* key_index; u64 n_links; u32 n; int key_bits; u64* first_bad;      // [0]: duplicate, [1]: no reverse complement
    AC_D void operator()(u64 j) const {
        const u64 k = key[j];
        if (k == link_key_dropped(key_bits)) return;
        if (j > 0 && key[j - 1] == k) atomic_min64(&first_bad[0], (u64)key_index[j]);
        const int64_t a = (int64_t)(k >> key_bits) - (int64_t)n, b = (int64_t)(k & ((1ULL << key_bits) - 1ULL)) - (int64_t)n;
        if (!merge_has_key(key, n_links, merge_key(-b, -a, n, key_bits))) atomic_min64(&first_bad[1], (u64)key_index[j]);
    }
};

struct MergeGraphView { u32 n; const u32* deg; const int32_t* target; const u32* fixed; };
// out(x): the node the one exclusive output of x leads to, or MERGE_NONE
AC_D u32 merge_out(const MergeGraphView& g, u32 x) {
    const u32 u = x >> 1;
    const int32_t self = (int32_t)(u + 1);
    if (!(x & 1u)) {      // get_exclusive_outputs(u) has one entry
        if (g.deg[(u64)COMP_FN * g.n + u] != 1) return MERGE_NONE;
        const int32_t y = g.target[(u64)COMP_FN * g.n + u];
        const u32 v = (u32)(y < 0 ? -(int64_t)y : y) - 1;
        if (v == u) return MERGE_NONE;
        const u32 plane = y > 0 ? COMP_FP : COMP_RP;
        if (g.deg[(u64)plane * g.n + v] != 1 || g.target[(u64)plane * g.n + v] != self) return MERGE_NONE;
        return merge_node(y);
    }
    // get_exclusive_inputs(u) has one entry; the output is that entry on the other strand
    if (g.deg[(u64)COMP_FP * g.n + u] != 1) return MERGE_NONE;
    const int32_t p = g.target[(u64)COMP_FP * g.n + u];
    const u32 w = (u32)(p < 0 ? -(int64_t)p : p) - 1;
    if (w == u) return MERGE_NONE;
    const u32 plane = p > 0 ? COMP_FN : COMP_RN;
    if (g.deg[(u64)plane * g.n + w] != 1 || g.target[(u64)plane * g.n + w] != self) return MERGE_NONE;
    return merge_node(-p);
}
AC_D bool merge_cannot_start(const MergeGraphView& g, u32 x) { return (g.fixed[x >> 1] & ((x & 1u) ? MERGE_FIXED_END : MERGE_FIXED_START)) != 0; }
AC_D bool merge_cannot_end(const MergeGraphView& g, u32 x) { return (g.fixed[x >> 1] & ((x & 1u) ? MERGE_FIXED_START : MERGE_FIXED_END)) != 0; }

// per node x: succ[x] and pred[succ[x]] (both MERGE_NONE-filled before), literal_head[x], and fixed_out[u] once per unitig
struct MergeSuccFunctor {
    MergeGraphView g; const u8* alive; u32* succ; u32* pred; u8* literal_head; u8* fixed_out;
    AC_D void operator()(u64 xi) const {
        const u32 x = (u32)xi, u = x >> 1;
        if (!(x & 1u)) fixed_out[u] = (u8)g.fixed[u];
        literal_head[x] = 0;
        if (alive && !alive[u]) return;
        // has_single_exclusive_input(x): the one exclusive output of the other strand (:404-407)
        literal_head[x] = !(merge_out(g, x ^ 1u) != MERGE_NONE && !merge_cannot_start(g, x)) ? 1 : 0;
        const u32 y = merge_out(g, x);
        if (y == MERGE_NONE || merge_cannot_end(g, x) || merge_cannot_start(g, y)) return;
        succ[x] = y; pred[y] = x;      // (out(x) = [y] says y's list of inputs has one entry: one writer per pred word)
    }
};

struct MergeRank { u32* start; u32* hops; u64* bases; };
struct MergeRankInitFunctor {
    const u32* pred; const u32* unitig_len; MergeRank r;
    AC_D void operator()(u64 x) const {
        const u32 p = pred[x];
        r.start[x] = p == MERGE_NONE ? (u32)x : p;
        r.hops[x] = p == MERGE_NONE ? 0u : 1u;
        r.bases[x] = p == MERGE_NONE ? 0ULL : (u64)unitig_len[p >> 1];
    }
};
// one round of pointer jumping from buffer `a` into buffer `b`: a start of a path is its own start with 0 hops, so it adds nothing; the
// nodes of a cycle go round (their sums may wrap: they are never read — a cycle's "start" has a predecessor, which is how it is told)
struct MergeRankJumpFunctor {
    MergeRank a, b;
    AC_D void operator()(u64 x) const {
        const u32 s = a.start[x];
        b.start[x] = a.start[s]; b.hops[x] = a.hops[x] + a.hops[s]; b.bases[x] = a.bases[x] + a.bases[s];
    }
};

// per node t that ends a maximal join path of two or more members: is this orientation the emitted one?  Written at the head's unitig.
struct MergeSelectFunctor {
    const u32* succ; const u32* pred; const u8* literal_head; const u8* alive; const u32* unitig_len; MergeRank r;
    u32* c_flag; u32* c_head; u32* c_tail; u32* c_members; u64* c_length;
    AC_D void operator()(u64 ti) const {
        const u32 t = (u32)ti;
        if (alive && !alive[t >> 1]) return;
        if (succ[t] != MERGE_NONE || r.hops[t] == 0) return;
        const u32 h = r.start[t];
        if (pred[h] != MERGE_NONE) return;      // (cannot happen: a node without a successor is on no cycle)
        const u32 uh = h >> 1, ut = t >> 1;
        if (!literal_head[h]) return;
        if (literal_head[t ^ 1u] && ut < uh) return;      // the mirrored path is a chain too, and the reference meets its head first
        c_flag[uh] = 1; c_head[uh] = h; c_tail[uh] = t; c_members[uh] = r.hops[t] + 1; c_length[uh] = r.bases[t] + (u64)unitig_len[ut];
    }
};

struct MergeCompactFunctor {
    u32 n; const u32* c_flag; const u32* c_rank; const u32* c_head; const u32* c_tail; const u32* c_members; const u64* c_length;
    u32* k_head; u32* k_tail; u32* k_members; u64* k_length; u32* chain_of_head; MergeCounts* counts;
    AC_D void operator()(u64 u) const {
        if (u + 1 == n) counts->n_chains = (u64)c_rank[u] + c_flag[u];
        if (!c_flag[u]) return;
        const u32 c = c_rank[u];
        k_head[c] = c_head[u]; k_tail[c] = c_tail[u]; k_members[c] = c_members[u]; k_length[c] = c_length[u];
        chain_of_head[c_head[u]] = c;
    }
};

struct MergeMembersFunctor {
    const u32* pred; const u8* alive; MergeRank r; const u32* chain_of_head; const u32* k_member_off; const u64* k_seq_off;
    int32_t* members; u64* member_seq_off; u32* chain_of; u32* pos_in_chain; u8* strand_in_chain; u32 n; u32* err;
    AC_D void operator()(u64 xi) const {
        const u32 x = (u32)xi, u = x >> 1;
        if (alive && !alive[u]) return;
        const u32 h = r.start[x];
        if (pred[h] != MERGE_NONE) return;      // on a cycle
        const u32 c = chain_of_head[h];
        if (c == MERGE_NONE) return;
        const u64 j = (u64)k_member_off[c] + r.hops[x];
        if (j >= (u64)n) { atomic_or32(err, MERGE_ERR_INTERNAL); return; }      // (only where the links are no closed set: both orientations of a path emitted)
        members[j] = merge_signed(x); member_seq_off[j] = k_seq_off[c] + r.bases[x];
        chain_of[u] = c; pos_in_chain[u] = r.hops[x]; strand_in_chain[u] = (u8)(x & 1u);
    }
};

// chain c: its record; c == n_chains: the totals and the end of the member offsets
struct MergeRecordsFunctor {
    MergeCounts* counts; u32 n; int key_bits; const u64* key; u64 n_links; const u32* k_head; const u32* k_tail; const u32* k_members; const u64* k_length;
    const u32* k_member_off; const u64* k_seq_off; MergeChainRecord* records; u64* member_seq_off;
    AC_D void operator()(u64 c) const {
        const u64 nc = counts->n_chains;
        if (c > nc) return;
        if (c == nc) {
            counts->n_members = k_member_off[c]; counts->n_bases = k_seq_off[c];
            if (k_member_off[c] <= n) member_seq_off[k_member_off[c]] = k_seq_off[c];
            return;
        }
        MergeChainRecord& rec = records[c];      // (the buffer was zeroed: number, depth, type and the padding stay 0 for the host)
        rec.members = k_members[c]; rec.length = k_length[c]; rec.member_off = k_member_off[c]; rec.seq_off = k_seq_off[c];
        // link_exists(last, first) (:418): the merged unitig's own + -> + link
        rec.loop = merge_has_key(key, n_links, merge_key(merge_signed(k_tail[c]), merge_signed(k_head[c]), n, key_bits)) ? 1 : 0;
    }
};

// per entry, in the caller's order: dead or a join inside a chain -> dropped; else both ends under their numbers after the merge
struct MergeRelabelFunctor {
    const Link* links; u32 n; const u8* alive; const u32* succ; const u32* chain_of; const u32* pos_in_chain; const u8* strand_in_chain; const u32* k_members;
    u64 offset; int key_bits; u64* key; u32* val; u32* err;
    AC_D void operator()(u64 i) const {
        key[i] = link_key_dropped(key_bits); val[i] = (u32)i;
        int64_t a = links[i].a, b = links[i].b;
        LinkEnds e;
        if (link_ends(links[i], n, alive, &e) != LINK_OK) return;
        const u32 ua = e.ua, ub = e.ub;
        const u32 ca = chain_of[ua], cb = chain_of[ub];
        if (ca != MERGE_NONE && succ[merge_node((int32_t)a)] == merge_node((int32_t)b)) return;      // a join of the chain, or the mirror image of one
        if (ca != MERGE_NONE) {      // as a source: the last member on its chain strand is +, the first on the other strand is -
            const bool on_strand = (strand_in_chain[ua] != 0) == (a < 0);
            const int64_t num = (int64_t)n + 1 + ca;
            if (on_strand && pos_in_chain[ua] + 1 == k_members[ca]) a = num;
            else if (!on_strand && pos_in_chain[ua] == 0) a = -num;
            else { atomic_or32(err, MERGE_ERR_INTERNAL); return; }
        }
        if (cb != MERGE_NONE) {      // as a target: the first member on its chain strand is +, the last on the other strand is -
            const bool on_strand = (strand_in_chain[ub] != 0) == (b < 0);
            const int64_t num = (int64_t)n + 1 + cb;
            if (on_strand && pos_in_chain[ub] == 0) b = num;
            else if (!on_strand && pos_in_chain[ub] + 1 == k_members[cb]) b = -num;
            else { atomic_or32(err, MERGE_ERR_INTERNAL); return; }
        }
        key[i] = merge_key(a, b, offset, key_bits);
    }
};

struct MergeDecodeFunctor {
    const u64* key; u64 n_links; u64 offset; int key_bits; Link* out; MergeCounts* counts;
    AC_D void operator()(u64 j) const {
        const u64 k = key[j], dropped = link_key_dropped(key_bits);
        if (k == dropped) return;
        out[j].a = (int32_t)((int64_t)(k >> key_bits) - (int64_t)offset);
        out[j].b = (int32_t)((int64_t)(k & ((1ULL << key_bits) - 1ULL)) - (int64_t)offset);
        if (j + 1 == n_links || key[j + 1] == dropped) counts->n_links_after = j + 1;
    }
};

// complement_base (misc.rs:358-367)
AC_D u8 merge_complement(u8 c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'C' ? 'G' : c == '.' ? '.' : 'N'; }

// The merged sequences, partitioned by output.  A wavefront owns 4 KB of merged bytes, a lane four 16-byte pieces of them, 1 KB apart (so
// that the lanes' stores of one piece are one contiguous KB); member_seq_off[j] (ascending, n_members + 1 entries, the last one =
// n_bases) is where member j begins.  The wavefront finds the last member that begins at or before its first byte and the last one that
// begins at or before its last byte, each by a 64-way search (one probe per lane and step: at most 6 steps for 2^32 members); the lane
// then searches between the two, and only when a piece leaves the member of the piece before.  The work per byte does not depend on how
// the bytes are cut into members — what does is the gather: a 1-base member costs three scattered reads (its length, its offset, its byte).  Where the 16 bytes lie inside one member they are fetched as one 16-byte read (the hardware takes it unaligned) and, for a reverse
// strand, reversed and complemented in registers; the store is one aligned 16-byte write.
AC_D u64 merge_wave_search(const u64* off, u64 n, u64 at) {      // the largest j < n with off[j] <= at (off[0] = 0); `at` and the result are wave-uniform
    u64 lo = 0, hi = n;
    const int lane = wv::lane();
    for (int it = 0; it < 12; it++) {
        const u64 span = hi - lo;
        if (span <= 1) break;      // (wave-uniform: every lane leaves together)
        const u64 step = (span + 63) / 64;
        const u64 p = lo + (u64)lane * step;
        const u64 ok = wv::ballot(p < hi && off[p] <= at);      // lane 0 probes lo: always set; the set lanes are a prefix
        const u64 k = (u64)prim_popc64(ok) - 1;
        const u64 new_lo = lo + k * step;
        hi = new_lo + step < hi ? new_lo + step : hi;
        lo = new_lo;
    }
    return lo;
}
static const u64 MERGE_COPY_CHUNKS = 4, MERGE_COPY_WAVE_BYTES = MERGE_COPY_CHUNKS * 64 * 16;      // a wavefront owns 4 KB: four 16-byte pieces per lane, 1 KB apart
struct MergeCopyFunctor {
    const u64* member_seq_off; const int32_t* members; u64 n_members; u64 n_bases; const u8* seq; const u64* seq_begin; const u32* unitig_len; u8* out;
    AC_D void operator()(u64 t, bool valid) const {
        const u64 wave_first = (t >> 6) * MERGE_COPY_WAVE_BYTES;
        if (wave_first >= n_bases) return;      // (wave-uniform)
        const u64 wave_last = wave_first + MERGE_COPY_WAVE_BYTES - 1 < n_bases ? wave_first + MERGE_COPY_WAVE_BYTES - 1 : n_bases - 1;
        const u64 j_first = merge_wave_search(member_seq_off, n_members, wave_first);
        const u64 j_last = merge_wave_search(member_seq_off, n_members, wave_last);
        if (!valid) return;
        // the member the lane is in, kept across its pieces: a long member is looked up once
        u64 j = j_first, m_begin = member_seq_off[j_first], m_end = member_seq_off[j_first + 1], len = 0;
        const u8* src = nullptr;
        int32_t e = 0;
        bool loaded = false;
        for (u64 c = 0; c < MERGE_COPY_CHUNKS; c++) {
            const u64 o = wave_first + (c * 64 + (u64)wv::lane()) * 16;
            if (o >= n_bases) break;
            if (o >= m_end) {      // the largest j in [j, j_last] with member_seq_off[j] <= o
                u64 lo = j, hi = j_last + 1;
                for (int it = 0; it < 64 && hi - lo > 1; it++) {
                    const u64 mid = lo + (hi - lo) / 2;
                    if (member_seq_off[mid] <= o) lo = mid; else hi = mid;
                }
                j = lo; m_begin = member_seq_off[j]; m_end = member_seq_off[j + 1]; loaded = false;
            }
            const u64 end = o + 16 < n_bases ? o + 16 : n_bases;
            alignas(16) u8 buf[16];
            u64 pos = o;
            while (pos < end) {
                if (m_end <= pos) { j++; m_begin = m_end; m_end = member_seq_off[j + 1]; loaded = false; continue; }      // (the next member; one without bases is passed over)
                if (!loaded) {
                    e = members[j];
                    const u32 u = (u32)(e < 0 ? -(int64_t)e : e) - 1;
                    len = unitig_len[u]; src = seq + seq_begin[u]; loaded = true;
                }
                const u64 within = pos - m_begin;
                const u64 take = (m_end < end ? m_end : end) - pos;
                if (take == 16) {
                    if (e > 0) {
                        __builtin_memcpy(buf, src + within, 16);
                    } else {
                        alignas(16) u8 in[16];
                        __builtin_memcpy(in, src + (len - within - 16), 16);
#pragma unroll
                        for (int i = 0; i < 16; i++) buf[i] = merge_complement(in[15 - i]);
                    }
                } else {
                    for (u64 i = 0; i < take; i++) buf[pos - o + i] = e > 0 ? src[within + i] : merge_complement(src[len - 1 - (within + i)]);
                }
                pos += take;
            }
            if (end - o == 16) *(PrimV16*)(out + o) = *(const PrimV16*)buf;
            else for (u64 i = 0; i < end - o; i++) out[o + i] = buf[i];
        }
    }
};

void merge_plan_device(const MergePlanInput& in, MergeResult* out) {
    *out = MergeResult();
    const u32 n = in.n_unitigs;
    const u64 nl = in.n_links;
    out->n_unitigs = n; out->links_in = nl;
    if (n > 0x7FFFFFFEu) throw DeviceError("merge plan: more unitigs than a signed unitig number can name");
    if (nl >= 0xFFFFFFF0ULL) throw DeviceError("merge plan: more than 2^32 links");
    if (n == 0) {
        if (nl) throw DeviceError(components_bad_link_message(0, in.links[0].a, in.links[0].b, 0));
        return;
    }
    // connected components with their circular-loop flags, on the device (kernels_components.inc): it refuses links that name no unitig,
    // and fix_circular_loops (:374-384) is the lowest member of every loop
    std::vector<u8> seed(in.seed_fixed, in.seed_fixed + n);
    {
        ComponentsResult comp;
        components_device(n, in.links, nl, in.unitig_len, in.alive, nullptr, &comp);
        for (const ComponentRecord& rec : comp.records)
            if (rec.circular_loop) seed[rec.first - 1] |= MERGE_SEED_LOOP;
        out->stats = comp.stats;
    }
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    const u64 nodes = 2 * (u64)n, nc_max = (u64)n + 1;      // (a valid input has at most n / 2 chains; one whose links are no closed set, refused below, up to n)
    const u64 offset_after = (u64)n + nc_max;      // no number after the merge is above this
    const int key_bits = bit_width(2 * (u64)n), key_bits_after = bit_width(2 * offset_after);
    if (key_bits_after > 32) throw DeviceError("merge plan: more unitigs than a 64-bit link key after the merge can name");
    const u32 rounds = jump_rounds(n);      // a path has at most n members
    const bool with_paths = in.path != nullptr && in.n_path > 0;
    const bool with_seq = in.seq_bytes != nullptr;

    DBuf<Link> d_links(nl);
    DBuf<u32> d_len(n);
    DBuf<u8> d_alive(in.alive ? n : 0), d_seed(n);
    DBuf<int32_t> d_path(with_paths ? in.n_path : 0);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    copy_h2d(d_len.ptr(), in.unitig_len, (u64)n * 4);
    if (in.alive) copy_h2d(d_alive.ptr(), in.alive, n);
    copy_h2d(d_seed.ptr(), seed.data(), n);
    if (with_paths) copy_h2d(d_path.ptr(), in.path, in.n_path * 4);
    const u8* p_alive = in.alive ? d_alive.ptr() : nullptr;

    DBuf<u32> d_fwd(with_paths ? n : 0), d_rev(with_paths ? n : 0);
    DBuf<u32> d_deg((u64)4 * n), d_fixed(n), d_key_index(nl), d_succ(nodes), d_pred(nodes), d_start_a(nodes), d_start_b(nodes), d_hops_a(nodes), d_hops_b(nodes);
    DBuf<int32_t> d_target((u64)4 * n);
    DBuf<u64> d_key(nl), d_first_bad(2), d_bases_a(nodes), d_bases_b(nodes);
    DBuf<u8> d_literal_head(nodes), d_fixed_out(n), d_strand_in_chain(n);
    DBuf<u32> d_c_flag(n), d_c_rank(n), d_c_head(n), d_c_tail(n), d_c_members(n), d_chain_of_head(nodes), d_chain_of(n), d_pos_in_chain(n);
    DBuf<u64> d_c_length(n);
    DBuf<u32> d_k_head(nc_max), d_k_tail(nc_max), d_k_members(nc_max), d_k_member_off(nc_max), d_err(2);
    DBuf<u64> d_k_length(nc_max), d_k_seq_off(nc_max), d_member_seq_off((u64)n + 1);
    DBuf<int32_t> d_members(n);
    DBuf<MergeChainRecord> d_records(nc_max);
    DBuf<MergeCounts> d_counts(1);
    DBuf<u64> d_key_after(nl);
    DBuf<u32> d_val_after(nl);
    DBuf<Link> d_links_after(nl);
    d_fwd.fill_bytes(0); d_rev.fill_bytes(0); d_deg.fill_bytes(0); d_target.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_succ.fill_bytes(0xFF); d_pred.fill_bytes(0xFF);
    d_c_flag.fill_bytes(0); d_chain_of_head.fill_bytes(0xFF); d_chain_of.fill_bytes(0xFF); d_pos_in_chain.fill_bytes(0); d_strand_in_chain.fill_bytes(0);
    d_k_members.fill_bytes(0); d_k_length.fill_bytes(0); d_k_head.fill_bytes(0); d_k_tail.fill_bytes(0); d_err.fill_bytes(0); d_records.fill_bytes(0); d_counts.fill_bytes(0);
    d_member_seq_off.fill_bytes(0); d_members.fill_bytes(0);
    RadixScratch sort_links, sort_after;
    sort_links.prepare(nl, 2 * key_bits);
    sort_after.prepare(nl, 2 * key_bits_after);

    meter.begin();
    if (with_paths) launch(in.n_path, MergeHistogramFunctor{d_path.ptr(), n, d_fwd.ptr(), d_rev.ptr()});
    launch(n, MergeInitFunctor{d_seed.ptr(), d_fixed.ptr()});
    if (nl) {
        launch(nl, MergeCensusFunctor{d_links.ptr(), n, p_alive, d_seed.ptr(), key_bits, d_deg.ptr(), d_target.ptr(), d_fixed.ptr(), d_key.ptr(), d_key_index.ptr()});
        sort_pairs_u64_u32(d_key, d_key_index, nl, 2 * key_bits, 0, 0, &sort_links);
        launch(nl, MergeLinkCheckFunctor{d_key.ptr(), d_key_index.ptr(), nl, n, key_bits, d_first_bad.ptr()});
    }
    const MergeGraphView view{n, d_deg.ptr(), d_target.ptr(), d_fixed.ptr()};
    launch(nodes, MergeSuccFunctor{view, p_alive, d_succ.ptr(), d_pred.ptr(), d_literal_head.ptr(), d_fixed_out.ptr()});
    MergeRank ra{d_start_a.ptr(), d_hops_a.ptr(), d_bases_a.ptr()}, rb{d_start_b.ptr(), d_hops_b.ptr(), d_bases_b.ptr()};
    launch(nodes, MergeRankInitFunctor{d_pred.ptr(), d_len.ptr(), ra});
    for (u32 r = 0; r < rounds; r++) { launch(nodes, MergeRankJumpFunctor{ra, rb}); std::swap(ra, rb); }
    launch(nodes, MergeSelectFunctor{d_succ.ptr(), d_pred.ptr(), d_literal_head.ptr(), p_alive, d_len.ptr(), ra, d_c_flag.ptr(), d_c_head.ptr(), d_c_tail.ptr(),
                                     d_c_members.ptr(), d_c_length.ptr()});
    exclusive_scan_u32(d_c_flag.ptr(), d_c_rank.ptr(), n);
    launch(n, MergeCompactFunctor{n, d_c_flag.ptr(), d_c_rank.ptr(), d_c_head.ptr(), d_c_tail.ptr(), d_c_members.ptr(), d_c_length.ptr(), d_k_head.ptr(), d_k_tail.ptr(),
                                  d_k_members.ptr(), d_k_length.ptr(), d_chain_of_head.ptr(), d_counts.ptr()});
    exclusive_scan_u32(d_k_members.ptr(), d_k_member_off.ptr(), nc_max);
    exclusive_scan_u64(d_k_length.ptr(), d_k_seq_off.ptr(), nc_max);
    launch(nodes, MergeMembersFunctor{d_pred.ptr(), p_alive, ra, d_chain_of_head.ptr(), d_k_member_off.ptr(), d_k_seq_off.ptr(), d_members.ptr(), d_member_seq_off.ptr(),
                                      d_chain_of.ptr(), d_pos_in_chain.ptr(), d_strand_in_chain.ptr(), n, d_err.ptr()});
    launch(nc_max, MergeRecordsFunctor{d_counts.ptr(), n, key_bits, d_key.ptr(), nl, d_k_head.ptr(), d_k_tail.ptr(), d_k_members.ptr(), d_k_length.ptr(), d_k_member_off.ptr(),
                                       d_k_seq_off.ptr(), d_records.ptr(), d_member_seq_off.ptr()});
    if (nl) {
        launch(nl, MergeRelabelFunctor{d_links.ptr(), n, p_alive, d_succ.ptr(), d_chain_of.ptr(), d_pos_in_chain.ptr(), d_strand_in_chain.ptr(), d_k_members.ptr(), offset_after,
                                       key_bits_after, d_key_after.ptr(), d_val_after.ptr(), d_err.ptr()});
        sort_pairs_u64_u32(d_key_after, d_val_after, nl, 2 * key_bits_after, 0, 0, &sort_after);
        launch(nl, MergeDecodeFunctor{d_key_after.ptr(), nl, offset_after, key_bits_after, d_links_after.ptr(), d_counts.ptr()});
    }
    meter.end();
    // the header: errors and sizes (the arrays are sized by n; what crosses is sized by the chains)
    MergeCounts h; u64 first_bad[2] = {~0ULL, ~0ULL}; u32 err[2] = {0, 0};
    {
        ReadBatch rb_;
        rb_.add(&h, d_counts.ptr(), sizeof h); rb_.add(first_bad, d_first_bad.ptr(), sizeof first_bad); rb_.add(err, d_err.ptr(), sizeof err);
        rb_.run();
    }
    if (first_bad[0] < nl) throw DeviceError(merge_duplicate_link_message(first_bad[0], in.links[first_bad[0]].a, in.links[first_bad[0]].b));
    if (first_bad[1] < nl) throw DeviceError(merge_unclosed_link_message(first_bad[1], in.links[first_bad[1]].a, in.links[first_bad[1]].b));
    if (err[0]) throw DeviceError("merge plan: a link at a chain's inside survived the relabelling (internal error)");
    if (2 * h.n_chains > n || h.n_members > n || h.n_members < 2 * h.n_chains || h.n_links_after > nl)
        throw DeviceError("merge plan: the device returned an impossible header (internal error)");
    const size_t nc = (size_t)h.n_chains, nm = (size_t)h.n_members;
    const u64 n_bases = h.n_bases;
    if (with_seq && n_bases) {
        DBuf<u8> d_seq(in.seq_total), d_out(n_bases);
        copy_h2d(d_seq.ptr(), in.seq_bytes, in.seq_total);
        DBuf<u64> d_seq_begin(n);
        copy_h2d(d_seq_begin.ptr(), in.seq_begin, (u64)n * 8);
        meter.begin();      // the copy kernel alone: seconds_copy
        launch_full((n_bases + MERGE_COPY_WAVE_BYTES - 1) / MERGE_COPY_WAVE_BYTES * 64, MergeCopyFunctor{d_member_seq_off.ptr(), d_members.ptr(), nm, n_bases, d_seq.ptr(), d_seq_begin.ptr(), d_len.ptr(), d_out.ptr()});
        meter.end();
        out->seq.resize(n_bases);
        copy_d2h_async(out->seq.data(), d_out.ptr(), n_bases);
    }
    out->chains.resize(nc); out->members.resize(nm); out->chain_of.resize(n); out->fixed.resize(n); out->links.resize((size_t)h.n_links_after);
    copy_d2h_async(out->chains.data(), d_records.ptr(), nc * sizeof(MergeChainRecord));
    copy_d2h_async(out->members.data(), d_members.ptr(), nm * 4);
    copy_d2h_async(out->chain_of.data(), d_chain_of.ptr(), (u64)n * 4);
    copy_d2h_async(out->fixed.data(), d_fixed_out.ptr(), n);
    copy_d2h_async(out->links.data(), d_links_after.ptr(), (u64)h.n_links_after * sizeof(Link));
    if (with_paths) {
        out->fwd_positions.resize(n); out->rev_positions.resize(n);
        copy_d2h_async(out->fwd_positions.data(), d_fwd.ptr(), (u64)n * 4);
        copy_d2h_async(out->rev_positions.data(), d_rev.ptr(), (u64)n * 4);
    }
    meter.sync_copies();
    out->stats += meter.stats();
    out->seconds_copy = meter.seconds(1);      // (0 where no sequence was copied)
}
