// A finished graph: a merge plan applied to the arrays it was made from, as a read-only product ON THE DEVICE — the order of the S lines
// (graph.unitigs after merge_path's push and retain, graph_simplification.rs:410-485; optionally sorted as renumber_unitigs does,
// unitig_graph.rs:295-315), the sequences gathered in that order, the L lines in get_links_for_gfa order (:333-350) and the P lines, both
// under the printed numbers.  Part of graph_extras.hip (included inside namespace ac; not a translation unit of its own).  The host side is
// finish_host.cpp.
//
// Slots: slot s < n is unitig s + 1, slot n + c is chain c.  A slot is kept when its unitig is alive and in no chain, or when it is a chain.
// Items are the kept slots in ascending slot order — graph.unitigs without renumbering.
//
// Stages of merge_finish_device, all on stream 0:
//   slots       per slot: kept?, length, where its bytes lie (the caller's sequences and the plan's merged ones are one device buffer), depth, type
//   scan        the kept flags: the item of every kept slot; compact
//   (renumber)  three stable radix sorts, least significant key first: depth descending (partial_cmp with -0.0 == 0.0 as an ascending 64-bit
//               key), the first 8 bytes of the sequence, length descending.  Exact for every unitig of up to 8 bases.  What is left open are
//               runs of equal length above 8 and equal first 8 bytes: the TIE GROUPS
//   ties        flag the items of groups with more than one item, scan, compact (the header read-back gives their number m)
//   merge sort  of the m compacted items by (group, sequence from byte 8, depth, item): bit_width(F - 1) passes whatever the data, one
//               wavefront per item and pass; the item finds its rank in the sibling run by a binary search whose comparisons the wavefront
//               makes together — 16 bytes per lane and step, the first difference by ballot.  The item index as the last key makes the order
//               total, so the result is the stable sort of the reference whatever order the radix keys left inside a group
//   scatter     the sorted items back to the places of their group
//   lengths     in final order; scan -> where every sequence begins in the output
//   records     per final unitig: printed number, source, length, offset, depth, type; new_of_old and the final place per slot
//   gather      the sequences, partitioned by OUTPUT bytes: a wavefront owns 4 KB, a lane four 16-byte pieces, as the merge copy does
//   members     per member of the plan: its place in its chain and its strand there
//   link keys   per input link: dropped (dead, a join, its mirror image) or (final place of the source, source strand, target merged?, input
//               index | 2 * chain + sign); radix sort; decode under the printed numbers
//   paths       per entry: the printed number
// Launches follow the key widths and bit_width(F - 1) alone — not group sizes, not the length of a common prefix.
struct FinishCounts { u64 tie_items, n_links, reserved[2]; };
static const int FINISH_BAD_PATH = 0, FINISH_BAD_LINK = 1;      // first_bad[]: lowest index, ~0 = none
static const u32 FINISH_ERR_MEMBERS = 1, FINISH_ERR_INSIDE = 2, FINISH_ERR_PLACE = 4;
static const u64 FINISH_PREFIX_BYTES = 8;

// descending depth as an ascending key: partial_cmp's order on everything but NaN (refused on the host), -0.0 == 0.0
AC_D u64 finish_depth_key(double d) {
    if (d == 0.0) d = 0.0;
    u64 b;
    __builtin_memcpy(&b, &d, 8);
    b = (b >> 63) ? ~b : (b | (1ULL << 63));
    return ~b;
}
AC_D u64 finish_prefix_key(const u8* p, u64 len) {
    u64 k = 0;
    for (u64 i = 0; i < FINISH_PREFIX_BYTES; i++) k = (k << 8) | (i < len ? (u64)p[i] : 0ULL);
    return k;
}

struct FinishSlotFunctor {
    u32 n; u64 n_chains; const u8* alive; const u32* chain_of; const u32* unitig_len; const u64* seq_begin; const double* depth; const u8* type;
    const MergeChainRecord* chains; u64 merged_base; u32* keep; u64* len; u64* src; double* dp; u8* ty;
    AC_D void operator()(u64 s) const {
        if (s < n) {
            keep[s] = ((!alive || alive[s]) && chain_of[s] == MERGE_NONE) ? 1u : 0u;
            len[s] = unitig_len[s]; src[s] = seq_begin ? seq_begin[s] : 0ULL; dp[s] = depth ? depth[s] : 0.0; ty[s] = type ? type[s] : (u8)0;
        } else {
            const MergeChainRecord& c = chains[s - n];
            keep[s] = 1u; len[s] = c.length; src[s] = merged_base + c.seq_off; dp[s] = c.depth; ty[s] = c.type;
        }
    }
};
struct FinishCompactFunctor {
    const u32* keep; const u32* item_of; u64 n_items; u32* item_slot; u32* ord; u32* err;
    AC_D void operator()(u64 s) const {
        if (!keep[s]) return;
        const u64 it = item_of[s];
        if (it >= n_items) { atomic_or32(err, FINISH_ERR_PLACE); return; }
        item_slot[it] = (u32)s; ord[it] = (u32)it;
    }
};

struct FinishItems { const u32* item_slot; const u64* len; const u64* src; const double* dp; const u8* seq; };
struct FinishKeyFunctor {
    int which; FinishItems v; const u32* ord; u64 len_flip; u64* key;
    AC_D void operator()(u64 j) const {
        const u32 s = v.item_slot[ord[j]];
        key[j] = which == 0 ? finish_depth_key(v.dp[s]) : which == 1 ? finish_prefix_key(v.seq + v.src[s], v.len[s]) : len_flip - v.len[s];
    }
};
struct FinishHeadFunctor {
    FinishItems v; const u32* ord; u32* head;
    AC_D void operator()(u64 j) const {
        if (j == 0) { head[j] = 1; return; }
        const u32 s = v.item_slot[ord[j]], p = v.item_slot[ord[j - 1]];
        head[j] = (v.len[s] != v.len[p] || finish_prefix_key(v.seq + v.src[s], v.len[s]) != finish_prefix_key(v.seq + v.src[p], v.len[p])) ? 1u : 0u;
    }
};
struct FinishTieFlagFunctor {
    FinishItems v; const u32* ord; const u32* head; u64 n_items; u32* tie;
    AC_D void operator()(u64 j) const {
        const bool alone = head[j] && (j + 1 == n_items || head[j + 1]);
        tie[j] = (v.len[v.item_slot[ord[j]]] > FINISH_PREFIX_BYTES && !alone) ? 1u : 0u;
    }
};
struct FinishTieCompactFunctor {
    const u32* ord; const u32* group; const u32* tie; const u32* tie_at; u64 n_items; u32* group_of_item; u32* t_item; u32* t_place; FinishCounts* counts;
    AC_D void operator()(u64 j) const {
        group_of_item[ord[j]] = group[j];
        if (j + 1 == n_items) counts->tie_items = (u64)tie_at[j] + tie[j];
        if (!tie[j]) return;
        t_item[tie_at[j]] = ord[j]; t_place[tie_at[j]] = (u32)j;
    }
};

// Bytes [from, len) of two sequences, compared by the whole wavefront (every argument wave-uniform): a lane takes 16 bytes per step, the
// first lane that sees a difference decides.  -1, 0, 1.
AC_D int finish_wave_compare(const u8* a, const u8* b, u64 from, u64 len) {
    const u64 lane = (u64)wv::lane();
    for (u64 base = from; base < len; base += 64 * 16) {      // (wave-uniform: every lane makes every step)
        const u64 o = base + lane * 16;
        int mine = 0;
        if (o < len) {
            const u64 take = len - o < 16 ? len - o : 16;
            if (take == 16) {
                u64 x[2], y[2];
                __builtin_memcpy(x, a + o, 16); __builtin_memcpy(y, b + o, 16);
                const int w = x[0] != y[0] ? 0 : 1;
                if (x[w] != y[w]) {
                    const int byte = ctz64(x[w] ^ y[w]) >> 3;      // (little endian: the lowest differing byte comes first in memory)
                    mine = ((x[w] >> (8 * byte)) & 0xFF) < ((y[w] >> (8 * byte)) & 0xFF) ? -1 : 1;
                }
            } else {
                for (u64 i = 0; i < take && !mine; i++)
                    if (a[o + i] != b[o + i]) mine = a[o + i] < b[o + i] ? -1 : 1;
            }
        }
        const u64 differ = wv::ballot(mine != 0);
        if (differ) return wv::shfl(mine, ctz64(differ));
    }
    return 0;
}
struct FinishTieView { FinishItems v; const u32* group_of_item; };
// the full comparator inside the compacted ties, a strict total order (x, y wave-uniform)
AC_D bool finish_tie_less(const FinishTieView& t, u32 x, u32 y) {
    if (x == y) return false;
    const u32 gx = t.group_of_item[x], gy = t.group_of_item[y];
    if (gx != gy) return gx < gy;
    const u32 sx = t.v.item_slot[x], sy = t.v.item_slot[y];
    const u64 len = t.v.len[sx] < t.v.len[sy] ? t.v.len[sx] : t.v.len[sy];      // (equal inside a group)
    const int c = finish_wave_compare(t.v.seq + t.v.src[sx], t.v.seq + t.v.src[sy], FINISH_PREFIX_BYTES, len);
    if (c) return c < 0;
    const u64 kx = finish_depth_key(t.v.dp[sx]), ky = finish_depth_key(t.v.dp[sy]);
    if (kx != ky) return kx < ky;
    return x < y;
}
// One pass of a bottom-up merge sort by ranks over the m compacted items, one wavefront per item: runs of `run` sorted items are merged
// pairwise; an item of the left run goes behind the right items that are smaller, an item of the right run behind the left items that are
// not larger.
struct FinishTieMergeFunctor {
    FinishTieView t; const u32* in; u32* out; u64 m, run;
    AC_D void operator()(u64 tid, bool) const {
        const u64 i = tid >> 6;
        if (i >= m) return;      // (wave-uniform)
        const u64 pair0 = i / (2 * run) * (2 * run);
        const u64 mid = pair0 + run < m ? pair0 + run : m, end = pair0 + 2 * run < m ? pair0 + 2 * run : m;
        const u32 me = in[i];
        u64 lo, hi, dst;
        if (i < mid) {
            lo = mid; hi = end;
            for (int it = 0; it < 64 && lo < hi; it++) { const u64 q = lo + ((hi - lo) >> 1); if (finish_tie_less(t, in[q], me)) lo = q + 1; else hi = q; }
            dst = i + (lo - mid);
        } else {
            lo = pair0; hi = mid;
            for (int it = 0; it < 64 && lo < hi; it++) { const u64 q = lo + ((hi - lo) >> 1); if (!finish_tie_less(t, me, in[q])) lo = q + 1; else hi = q; }
            dst = pair0 + (i - mid) + (lo - pair0);
        }
        if (wv::lane() == 0 && dst < m) out[dst] = me;
    }
};
struct FinishTieScatterFunctor {
    const u32* sorted; const u32* t_place; u64 n_items; u32* ord;
    AC_D void operator()(u64 t) const { if ((u64)t_place[t] < n_items) ord[t_place[t]] = sorted[t]; }
};

struct FinishLenFunctor {
    FinishItems v; const u32* ord; u64* len_out;
    AC_D void operator()(u64 f) const { len_out[f] = v.len[v.item_slot[ord[f]]]; }
};
struct FinishRecordFunctor {
    FinishItems v; const u32* ord; const u64* out_off; const u8* ty; int renumber; FinishedUnitigRecord* rec; u32* new_of_old; u32* place_of_slot; u32* slot_of_place;
    AC_D void operator()(u64 f) const {
        const u32 s = v.item_slot[ord[f]];
        const u32 number = renumber ? (u32)f + 1u : s + 1u;
        FinishedUnitigRecord& r = rec[f];      // (zeroed: the padding too)
        r.number = number; r.source = s + 1u; r.length = v.len[s]; r.seq_off = out_off[f]; r.depth = v.dp[s]; r.type = ty[s];
        new_of_old[s] = number; place_of_slot[s] = (u32)f; slot_of_place[f] = s;
    }
};

// The sequences in final order, partitioned by output as MergeCopyFunctor is: out_off[f] (ascending, n_items + 1 entries, the last one =
// n_bases) is where final unitig f begins; the wavefront finds the unitigs of its first and last byte by two 64-way searches, the lane
// searches between them only when a piece leaves the unitig of the piece before.  16 bytes inside one unitig are one read and one store.
struct FinishGatherFunctor {
    const u64* out_off; const u32* slot_of_place; const u64* src; u64 n_items; u64 n_bases; const u8* seq; u8* out;
    AC_D void operator()(u64 t, bool valid) const {
        const u64 wave_first = (t >> 6) * MERGE_COPY_WAVE_BYTES;
        if (wave_first >= n_bases) return;      // (wave-uniform)
        const u64 wave_last = wave_first + MERGE_COPY_WAVE_BYTES - 1 < n_bases ? wave_first + MERGE_COPY_WAVE_BYTES - 1 : n_bases - 1;
        const u64 j_first = merge_wave_search(out_off, n_items, wave_first);
        const u64 j_last = merge_wave_search(out_off, n_items, wave_last);
        if (!valid) return;
        u64 j = j_first, m_begin = out_off[j_first], m_end = out_off[j_first + 1];
        const u8* from = nullptr;
        bool loaded = false;
        for (u64 c = 0; c < MERGE_COPY_CHUNKS; c++) {
            const u64 o = wave_first + (c * 64 + (u64)wv::lane()) * 16;
            if (o >= n_bases) break;
            if (o >= m_end) {      // the largest j in [j, j_last] with out_off[j] <= o
                u64 lo = j, hi = j_last + 1;
                for (int it = 0; it < 64 && hi - lo > 1; it++) {
                    const u64 mid = lo + (hi - lo) / 2;
                    if (out_off[mid] <= o) lo = mid; else hi = mid;
                }
                j = lo; m_begin = out_off[j]; m_end = out_off[j + 1]; loaded = false;
            }
            const u64 end = o + 16 < n_bases ? o + 16 : n_bases;
            alignas(16) u8 buf[16];
            u64 pos = o;
            while (pos < end) {
                if (m_end <= pos) { j++; m_begin = m_end; m_end = out_off[j + 1]; loaded = false; continue; }      // (the next unitig; one without bases is passed over)
                if (!loaded) { from = seq + src[slot_of_place[j]]; loaded = true; }
                const u64 within = pos - m_begin;
                const u64 take = (m_end < end ? m_end : end) - pos;
                if (take == 16) __builtin_memcpy(buf, from + within, 16);
                else for (u64 i = 0; i < take; i++) buf[pos - o + i] = from[within + i];
                pos += take;
            }
            if (end - o == 16) *(PrimV16*)(out + o) = *(const PrimV16*)buf;
            else for (u64 i = 0; i < end - o; i++) out[o + i] = buf[i];
        }
    }
};

// ---- the L lines ---------------------------------------------------------------------------------------------------------------------------------
// After merge_path's list pushes and delete_dangling_links, a list of a kept unitig holds its own entries whose target is kept unmerged, in
// input order, then the entries that name merged unitigs, ascending by chain, + before - — but for the merged unitig's own entries in its
// reverse_next, where merge_path appends the loop (-) before the start flip (+).  Every entry that names a merged unitig is the image of an
// input entry that named the chain's first member on its chain strand (+) or its last member on the other strand (-).
struct FinishLinkView { u32 n; const u8* alive; const u32* chain_of; const u32* pos_in; const u8* strand_in; const MergeChainRecord* chains; u64 n_chains; };
// One end of an entry after the merge: 0 = an unmerged unitig, 1 = a merged one at the side the entry may touch, -1 = inside a chain.
AC_D int finish_link_end(const FinishLinkView& v, int64_t e, bool source, u64* slot, bool* fwd, u32* chain) {
    const u32 u = (u32)(e < 0 ? -e : e) - 1u;
    const u32 ch = v.chain_of[u];
    if (ch == MERGE_NONE || (u64)ch >= v.n_chains) { *slot = u; *fwd = e > 0; return 0; }
    const bool along = (v.strand_in[u] != 0) == (e < 0);
    const u32 pos = v.pos_in[u], last = v.chains[ch].members - 1u;
    *chain = ch; *slot = (u64)v.n + ch;
    const bool at_plus = source ? pos == last : pos == 0, at_minus = source ? pos == 0 : pos == last;
    if (along && at_plus) { *fwd = true; return 1; }
    if (!along && at_minus) { *fwd = false; return 1; }
    return -1;
}
// is the entry a join of a chain (member i -> member i + 1 on the chain strands) or the mirror image of one?
AC_D bool finish_link_is_join(const FinishLinkView& v, int64_t a, int64_t b) {
    const u32 ua = (u32)(a < 0 ? -a : a) - 1u, ub = (u32)(b < 0 ? -b : b) - 1u;
    const u32 ca = v.chain_of[ua];
    if (ca == MERGE_NONE || ca != v.chain_of[ub]) return false;
    const bool along_a = (v.strand_in[ua] != 0) == (a < 0), along_b = (v.strand_in[ub] != 0) == (b < 0);
    if (along_a != along_b) return false;
    return along_a ? v.pos_in[ub] == v.pos_in[ua] + 1u : v.pos_in[ua] == v.pos_in[ub] + 1u;
}
static const u64 FINISH_LINK_DROPPED = ~0ULL;
struct FinishLinkKeyFunctor {
    const Link* links; FinishLinkView v; const u32* place_of_slot; u64 n_items; int idx_bits; u64* key; u32* val; u64* first_bad; u32* err;
    AC_D void operator()(u64 i) const {
        key[i] = FINISH_LINK_DROPPED; val[i] = (u32)i;
        LinkEnds e;
        const int kind = link_ends(links[i], v.n, v.alive, &e);
        if (kind == LINK_NO_UNITIG) { atomic_min64(&first_bad[FINISH_BAD_LINK], i); return; }
        if (kind != LINK_OK) return;
        const int64_t a = links[i].a, b = links[i].b;
        if (finish_link_is_join(v, a, b)) return;
        u64 slot_a = 0, slot_b = 0; bool fwd_a = true, fwd_b = true; u32 ch_a = 0, ch_b = 0;
        const int ka = finish_link_end(v, a, true, &slot_a, &fwd_a, &ch_a), kb = finish_link_end(v, b, false, &slot_b, &fwd_b, &ch_b);
        if (ka < 0 || kb < 0) { atomic_or32(err, FINISH_ERR_INSIDE); return; }
        const u64 place = place_of_slot[slot_a];
        if (place >= n_items) { atomic_or32(err, FINISH_ERR_PLACE); return; }
        u64 sign = fwd_b ? 0ULL : 1ULL;
        if (kb == 1 && slot_a == slot_b && !fwd_a) sign ^= 1ULL;      // (the merged unitig's own reverse_next: - before +)
        const u64 idx = kb == 1 ? 2ULL * ch_b + sign : i;
        key[i] = ((((place << 1) | (fwd_a ? 0ULL : 1ULL)) << 1 | (kb == 1 ? 1ULL : 0ULL)) << idx_bits) | idx;
    }
};
struct FinishLinkDecodeFunctor {
    const u64* key; const u32* val; const Link* links; u64 n_links; FinishLinkView v; const u32* new_of_old; Link* out; FinishCounts* counts;
    AC_D void operator()(u64 j) const {
        out[j] = Link{0, 0};
        if (key[j] == FINISH_LINK_DROPPED) return;
        if (j + 1 == n_links || key[j + 1] == FINISH_LINK_DROPPED) counts->n_links = j + 1;
        const u64 i = val[j];
        if (i >= n_links) return;
        u64 slot_a = 0, slot_b = 0; bool fwd_a = true, fwd_b = true; u32 ch = 0;
        finish_link_end(v, links[i].a, true, &slot_a, &fwd_a, &ch); finish_link_end(v, links[i].b, false, &slot_b, &fwd_b, &ch);
        const int32_t na = (int32_t)new_of_old[slot_a], nb = (int32_t)new_of_old[slot_b];
        out[j] = Link{fwd_a ? na : -na, fwd_b ? nb : -nb};
    }
};
struct FinishPathFunctor {
    const int32_t* in; const u32* new_of_old; u64 n_slots; int32_t* out; u64* first_bad;
    AC_D void operator()(u64 j) const {
        const int64_t e = in[j];
        const u64 u = (u64)(e < 0 ? -e : e);
        out[j] = 0;
        if (u == 0 || u > n_slots || new_of_old[u - 1] == 0) { atomic_min64(&first_bad[FINISH_BAD_PATH], j); return; }
        out[j] = e < 0 ? -(int32_t)new_of_old[u - 1] : (int32_t)new_of_old[u - 1];
    }
};

void merge_finish_device(const FinishInput& in, FinishResult* out) {
    const MergeResult& plan = *in.plan;
    const u32 n = in.n_unitigs;
    const u64 nc = plan.chains.size(), nm = plan.members.size(), nl = in.n_links, slots = (u64)n + nc, F = in.unitigs_after, np = in.n_path;
    if (slots == 0 || F == 0) throw DeviceError("finish: nothing to launch (internal error)");
    if (slots > 0x7FFFFFFEULL) throw DeviceError("finish: more unitigs and chains than a signed unitig number can name");
    if (nl >= 0xFFFFFFF0ULL) throw DeviceError("finish: more than 2^32 links");
    u64 max_len = 0, n_bases = 0;
    for (u32 u = 0; u < n; u++)
        if ((!in.alive || in.alive[u]) && plan.chain_of[u] == MERGE_NOT_MERGED) { max_len = std::max<u64>(max_len, in.unitig_len[u]); n_bases += in.unitig_len[u]; }
    for (const MergeChainRecord& c : plan.chains) { max_len = std::max<u64>(max_len, c.length); n_bases += c.length; }
    const int len_bits = bit_width(max_len), place_bits = bit_width(F), idx_bits = std::max(bit_width(nl), bit_width(2 * nc + 1));
    const int link_bits = place_bits + 2 + idx_bits;
    if (link_bits > 63) throw DeviceError("finish: more unitigs and links than a 64-bit link key can order");
    const u32 passes = F > 1 ? (u32)bit_width(F - 1) : 0;
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    double seconds = 0;

    const u64 own_bytes = in.seq_bytes ? in.seq_total : 0;
    DBuf<u8> d_seq(own_bytes + plan.seq.size()), d_alive(in.alive ? n : 0), d_type_in(in.type ? n : 0), d_strand_in(n), d_ty(slots);
    DBuf<u32> d_len_in(n), d_chain_of(n), d_pos_in(n), d_err(2);
    DBuf<u64> d_seq_begin(in.seq_begin ? n : 0), d_first_bad(2);
    DBuf<double> d_depth_in(in.depth ? n : 0), d_dp(slots);
    DBuf<MergeChainRecord> d_chains(nc);
    DBuf<int32_t> d_members(nm), d_path(np), d_path_out(np);
    DBuf<Link> d_links(nl), d_links_out(nl);
    if (own_bytes) copy_h2d(d_seq.ptr(), in.seq_bytes, own_bytes);
    if (plan.seq.size()) copy_h2d(d_seq.ptr() + own_bytes, plan.seq.data(), plan.seq.size());
    if (in.alive) copy_h2d(d_alive.ptr(), in.alive, n);
    if (in.type) copy_h2d(d_type_in.ptr(), in.type, n);
    if (in.depth) copy_h2d(d_depth_in.ptr(), in.depth, (u64)n * 8);
    if (in.seq_begin) copy_h2d(d_seq_begin.ptr(), in.seq_begin, (u64)n * 8);
    copy_h2d(d_len_in.ptr(), in.unitig_len, (u64)n * 4);
    copy_h2d(d_chain_of.ptr(), plan.chain_of.data(), (u64)n * 4);
    copy_h2d(d_chains.ptr(), plan.chains.data(), nc * sizeof(MergeChainRecord));
    copy_h2d(d_members.ptr(), plan.members.data(), nm * 4);
    copy_h2d(d_links.ptr(), in.links, nl * sizeof(Link));
    if (np) copy_h2d(d_path.ptr(), in.path, np * 4);
    const u8* p_alive = in.alive ? d_alive.ptr() : nullptr;

    DBuf<u32> d_keep(slots + 1), d_item_of(slots + 1), d_item_slot(F), d_ord(F), d_head(F), d_group(F), d_tie(F + 1), d_tie_at(F + 1), d_group_of_item(F), d_t_item(F), d_t_item2(F),
        d_t_place(F), d_new_of_old(slots), d_place_of_slot(slots), d_slot_of_place(F), d_link_val(nl);
    DBuf<u64> d_len(slots), d_src(slots), d_key(F), d_len_f(F + 1), d_out_off(F + 1), d_link_key(nl);
    DBuf<FinishedUnitigRecord> d_rec(F);
    DBuf<FinishCounts> d_counts(1);
    DBuf<u8> d_out(n_bases);
    d_keep.fill_bytes(0); d_tie.fill_bytes(0); d_len_f.fill_bytes(0); d_rec.fill_bytes(0); d_counts.fill_bytes(0); d_new_of_old.fill_bytes(0); d_place_of_slot.fill_bytes(0xFF);
    d_err.fill_bytes(0); d_first_bad.fill_bytes(0xFF); d_pos_in.fill_bytes(0); d_strand_in.fill_bytes(0); d_item_slot.fill_bytes(0); d_ord.fill_bytes(0);
    d_t_item.fill_bytes(0); d_t_item2.fill_bytes(0); d_t_place.fill_bytes(0xFF); d_group_of_item.fill_bytes(0);
    const FinishItems items{d_item_slot.ptr(), d_len.ptr(), d_src.ptr(), d_dp.ptr(), d_seq.ptr()};

    meter.begin();
    launch(slots, FinishSlotFunctor{n, nc, p_alive, d_chain_of.ptr(), d_len_in.ptr(), in.seq_begin ? d_seq_begin.ptr() : nullptr, in.depth ? d_depth_in.ptr() : nullptr,
                                    in.type ? d_type_in.ptr() : nullptr, d_chains.ptr(), own_bytes, d_keep.ptr(), d_len.ptr(), d_src.ptr(), d_dp.ptr(), d_ty.ptr()});
    exclusive_scan_u32(d_keep.ptr(), d_item_of.ptr(), slots + 1);
    launch(slots, FinishCompactFunctor{d_keep.ptr(), d_item_of.ptr(), F, d_item_slot.ptr(), d_ord.ptr(), d_err.ptr()});
    u64 m = 0;
    if (in.renumber) {
        const int key_bits[3] = {64, 64, len_bits};
        for (int which = 0; which < 3; which++) {
            launch(F, FinishKeyFunctor{which, items, d_ord.ptr(), (len_bits >= 64 ? ~0ULL : (1ULL << len_bits) - 1ULL), d_key.ptr()});
            sort_pairs_u64_u32(d_key, d_ord, F, key_bits[which]);
        }
        launch(F, FinishHeadFunctor{items, d_ord.ptr(), d_head.ptr()});
        launch(F, FinishTieFlagFunctor{items, d_ord.ptr(), d_head.ptr(), F, d_tie.ptr()});
        inclusive_scan_u32(d_head.ptr(), d_group.ptr(), F);
        exclusive_scan_u32(d_tie.ptr(), d_tie_at.ptr(), F + 1);
        launch(F, FinishTieCompactFunctor{d_ord.ptr(), d_group.ptr(), d_tie.ptr(), d_tie_at.ptr(), F, d_group_of_item.ptr(), d_t_item.ptr(), d_t_place.ptr(), d_counts.ptr()});
        meter.end();
        seconds += meter.take();
        // the header of the first half: how many items the radix keys left open (sizes the merge passes; their number is fixed)
        FinishCounts h;
        { ReadBatch rb; rb.add(&h, d_counts.ptr(), sizeof h); rb.run(); }
        if (h.tie_items > F) throw DeviceError("finish: the device returned an impossible header (internal error)");
        m = h.tie_items;
        meter.begin();
        const FinishTieView view{items, d_group_of_item.ptr()};
        u32* ta = d_t_item.ptr(); u32* tb = d_t_item2.ptr();
        for (u32 p = 0; p < passes; p++) {      // (every pass is launched whatever m: the launches follow F alone)
            launch_full(std::max<u64>(m, 1) * 64, FinishTieMergeFunctor{view, ta, tb, m, 1ULL << p});
            std::swap(ta, tb);
        }
        if (m) launch(m, FinishTieScatterFunctor{ta, d_t_place.ptr(), F, d_ord.ptr()});
        else launch(1, FinishTieScatterFunctor{ta, d_t_place.ptr(), F, d_ord.ptr()});      // (t_place[0] = ~0: nothing is written)
    }
    launch(F, FinishLenFunctor{items, d_ord.ptr(), d_len_f.ptr()});
    exclusive_scan_u64(d_len_f.ptr(), d_out_off.ptr(), F + 1);
    launch(F, FinishRecordFunctor{items, d_ord.ptr(), d_out_off.ptr(), d_ty.ptr(), in.renumber ? 1 : 0, d_rec.ptr(), d_new_of_old.ptr(), d_place_of_slot.ptr(),
                                  d_slot_of_place.ptr()});
    const FinishLinkView lview{n, p_alive, d_chain_of.ptr(), d_pos_in.ptr(), d_strand_in.ptr(), d_chains.ptr(), nc};
    if (nm) launch(nm, MergedPathsMemberFunctor{d_members.ptr(), n, d_chain_of.ptr(), d_chains.ptr(), nc, d_pos_in.ptr(), d_strand_in.ptr(), d_err.ptr()});
    if (nl) {
        launch(nl, FinishLinkKeyFunctor{d_links.ptr(), lview, d_place_of_slot.ptr(), F, idx_bits, d_link_key.ptr(), d_link_val.ptr(), d_first_bad.ptr(), d_err.ptr()});
        sort_pairs_u64_u32(d_link_key, d_link_val, nl, link_bits);
        launch(nl, FinishLinkDecodeFunctor{d_link_key.ptr(), d_link_val.ptr(), d_links.ptr(), nl, lview, d_new_of_old.ptr(), d_links_out.ptr(), d_counts.ptr()});
    }
    if (np) launch(np, FinishPathFunctor{d_path.ptr(), d_new_of_old.ptr(), slots, d_path_out.ptr(), d_first_bad.ptr()});
    meter.end();
    seconds += meter.take();
    if (n_bases) {
        meter.begin();      // the gather alone: seconds_gather
        launch_full((n_bases + MERGE_COPY_WAVE_BYTES - 1) / MERGE_COPY_WAVE_BYTES * 64,
                    FinishGatherFunctor{d_out_off.ptr(), d_slot_of_place.ptr(), d_src.ptr(), F, n_bases, d_seq.ptr(), d_out.ptr()});
        meter.end();
        out->seconds_gather = meter.take();
        seconds += out->seconds_gather;
    }
    // the header: errors, the kept links, the bases the scan counted
    FinishCounts h; u64 first_bad[2] = {~0ULL, ~0ULL}; u32 err[2] = {0, 0}; u64 total = 0;
    {
        ReadBatch rb;
        rb.add(&h, d_counts.ptr(), sizeof h); rb.add(first_bad, d_first_bad.ptr(), sizeof first_bad); rb.add(err, d_err.ptr(), sizeof err); rb.add(&total, d_out_off.ptr() + F, 8);
        rb.run();
    }
    if (first_bad[FINISH_BAD_LINK] < nl) { const u64 i = first_bad[FINISH_BAD_LINK]; throw DeviceError(components_bad_link_message(i, in.links[i].a, in.links[i].b, n)); }
    if (err[0] & FINISH_ERR_MEMBERS) throw DeviceError("finish: the plan's member list does not fit its chains");
    if (err[0] & FINISH_ERR_INSIDE) throw DeviceError("finish: a link touches the inside of a chain: the links are not the ones the plan was made from");
    if ((err[0] & FINISH_ERR_PLACE) || total != n_bases || h.n_links > nl) throw DeviceError("finish: the device returned an impossible header (internal error)");
    if (first_bad[FINISH_BAD_PATH] < np) throw DeviceError(finish_bad_path_entry_message(first_bad[FINISH_BAD_PATH], in.path[first_bad[FINISH_BAD_PATH]]));
    out->unitigs.resize(F); out->seq.resize(n_bases); out->new_of_old.resize(slots); out->links.resize((size_t)h.n_links); out->path_entries.resize(np);
    copy_d2h_async(out->unitigs.data(), d_rec.ptr(), F * sizeof(FinishedUnitigRecord));
    copy_d2h_async(out->seq.data(), d_out.ptr(), n_bases);
    copy_d2h_async(out->new_of_old.data(), d_new_of_old.ptr(), slots * 4);
    copy_d2h_async(out->links.data(), d_links_out.ptr(), (u64)h.n_links * sizeof(Link));
    copy_d2h_async(out->path_entries.data(), d_path_out.ptr(), np * 4);
    meter.sync_copies();
    out->tie_items = m;
    out->stats = meter.stats();
    out->stats.seconds_device = seconds;
}
