// connected_components, component_is_circular_loop, link_count and topology (unitig_graph.rs:478-545, 905-967) with the per-unitig end
// tests of unitig.rs:197-215, 276-293, ON THE DEVICE — part of graph_extras.hip (included inside namespace ac; not a translation unit of
// its own).  The host side (components_host.cpp) adds the totals and runs the topology chain on what comes back.
//
// The graph is what build_links_from_gfa (unitig_graph.rs:91-115) makes of the link entries in their order: an entry (a, b) puts b into
// a's next list (forward_next for a > 0, reverse_next otherwise) and a into b's prev list (forward_prev for b > 0, reverse_prev
// otherwise).  Entries may repeat and their reverse complements may be missing; a unitig that is not alive is in no component and every
// entry touching it is ignored (remove_unitigs_by_number + delete_dangling_links).
//
// Stages, all on stream 0, nothing read by the host in between:
//   init        parent[u] = u
//   census      one pass over the entries: range check, alive filter, the four list lengths per unitig, one target per list (whichever entry
//               stores last: only read where the list has exactly one entry), the "not a hairpin to myself" bits is_isolated_and_linear
//               needs, the entry's canonical key for link_count, and the hook of its two unitigs into one tree
//   jump        ceil(log2 n) + 1 rounds of parent[u] = parent[parent[u]]; a round does nothing once the round before changed nothing
//   roots       checks that every tree is flat now (else the error flag), flags the roots, the per-unitig flag bits
//   scan        root flags -> component index: a component's root is its lowest member, so the indices are connected_components() order
//   label       component_of[u]; the sort key (component index; not alive: n, behind everything)
//   radix sort  unitig numbers by component index; stable, so every member list ascends
//   segments    member offsets, and per component length / open ends / marked / "some degree is not 1", combined over the runs of one
//               component inside a wavefront before they reach the component's counters
//   radix sort  the canonical keys; then distinct keys per component, combined the same way
//   records     one thread per component: the record, and the literal walk of component_is_circular_loop where every degree is 1
//
// Components.  Hooking is lock-free union by index: the larger root is pointed at the smaller one with a compare-and-swap that only
// succeeds on a root, so parent[x] <= x always holds, a root is the lowest number of its tree, and the final labels do not depend on the
// order the hooks ran in.  find() halves its path with atomicMin (a parent word only ever decreases).  Every loop is bounded by n: find
// descends strictly; a failed compare-and-swap means the root it named has since been hooked below itself, so the sum of the two roots
// strictly decreases from one attempt to the next.  No loop waits for another lane.  A bound that is reached sets the error flag.
static const u32 COMP_FN = 0, COMP_RN = 1, COMP_FP = 2, COMP_RP = 3;      // planes of the degree / target arrays
static const u32 COMP_ERR_RANGE = 1, COMP_ERR_BOUND = 2;
static const u32 COMP_DEAD = 0xFFFFFFFFu;
struct CompHeader { u64 n_components, n_alive, first_bad_link, reserved; };

// ---- what the three graph steps share (this file, kernels_merge.inc, kernels_subset.inc) ----
static int bit_width(u64 x) { int b = 0; while (x) { b++; x >>= 1; } return b; }
static u32 jump_rounds(u64 n) { u32 rounds = 1; while (((u64)1 << (rounds - 1)) < n) rounds++; return rounds; }      // ceil(log2 n) + 1: pointer jumping over at most n members
// A link entry's two ends: LINK_NO_UNITIG, LINK_DEAD (it touches a unitig that is not alive: the entry is ignored), or LINK_OK with the two
// unitig indices and the planes of the lists build_links_from_gfa puts the entry into — a's next list, b's prev list.
static const int LINK_OK = 0, LINK_NO_UNITIG = 1, LINK_DEAD = 2;
struct LinkEnds { u32 ua, ub, la, lb; };
AC_D int link_ends(const Link& l, u32 n, const u8* alive, LinkEnds* e) {
    const u32 na = l.na(), nb = l.nb();
    if (na == 0 || nb == 0 || na > n || nb > n) return LINK_NO_UNITIG;
    e->ua = na - 1; e->ub = nb - 1;
    if (alive && (!alive[e->ua] || !alive[e->ub])) return LINK_DEAD;
    e->la = l.a > 0 ? COMP_FN : COMP_RN; e->lb = l.b > 0 ? COMP_FP : COMP_RP;
    return LINK_OK;
}
// The entry in its two lists: their lengths, and one target each — whichever entry stores last, read only where the list has one entry.
AC_D void link_into_lists(const Link& l, const LinkEnds& e, u32 n, u32* deg, int32_t* target) {
    atomic_add32(&deg[(u64)e.la * n + e.ua], 1u); target[(u64)e.la * n + e.ua] = l.b;
    atomic_add32(&deg[(u64)e.lb * n + e.ub], 1u); target[(u64)e.lb * n + e.ub] = l.a;
}
// The key of an entry that takes no part (it sorts behind every real key of two key_bits halves).
AC_D u64 link_key_dropped(int key_bits) { return key_bits == 32 ? ~0ULL : ((1ULL << (2 * key_bits)) - 1ULL); }

AC_D u32 comp_find(u32* parent, u32 x, u32 n, u32* err) {
    for (u32 s = 0; s <= n; s++) {
        const u32 p = atomic_load32(&parent[x]);
        if (p == x) return x;
        const u32 g = atomic_load32(&parent[p]);
        if (g == p) return p;
        atomic_min32(&parent[x], g);
        x = g;
    }
    atomic_or32(err, COMP_ERR_BOUND);
    return x;
}
AC_D void comp_union(u32* parent, u32 a, u32 b, u32 n, u32* err) {
    for (u64 it = 0; it < 2 * (u64)n + 4; it++) {
        a = comp_find(parent, a, n, err); b = comp_find(parent, b, n, err);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }
        if (atomic_cas32(&parent[a], a, b) == a) return;
    }
    atomic_or32(err, COMP_ERR_BOUND);
}

struct CompInitFunctor {
    u32* parent;
    AC_D void operator()(u64 u) const { parent[u] = (u32)u; }
};

struct CompCensusFunctor {
    const Link* links; u32 n; const u8* alive; int key_bits;      // key_bits: bits of one half of a key
    u32* deg; int32_t* target; u32* notself; u32* parent; u64* key; u32* key_unitig; u32* err; CompHeader* hdr;
    AC_D void operator()(u64 i) const {
        const int64_t a = links[i].a, b = links[i].b;
        key[i] = link_key_dropped(key_bits); key_unitig[i] = 0;
        LinkEnds e;
        const int ends = link_ends(links[i], n, alive, &e);
        if (ends == LINK_NO_UNITIG) {
            atomic_or32(err, COMP_ERR_RANGE);
            atomic_min64(&hdr->first_bad_link, i);
            return;
        }
        if (ends == LINK_DEAD) return;
        const u32 ua = e.ua, ub = e.ub;
        const int64_t na = (int64_t)ua + 1, nb = (int64_t)ub + 1;
        link_into_lists(links[i], e, n, deg, target);
        // the notself bits: an entry that is_isolated_and_linear's all() rejects
        if (b != (a > 0 ? -na : na)) atomic_or32(&notself[ua], 1u << e.la);      // forward_next: myself, reverse; reverse_next: myself, forward
        if (a != (b > 0 ? -nb : nb)) atomic_or32(&notself[ub], 1u << e.lb);      // forward_prev: myself, reverse; reverse_prev: myself, forward
        // link_count's one_way entry: the larger of (a, b) and (-b, -a) as tuples, as a key that keeps the tuples' order
        const bool keep = a > -b || (a == -b && b >= -a);
        const int64_t ca = keep ? a : -b, cb = keep ? b : -a;
        key[i] = ((u64)(ca + (int64_t)n) << key_bits) | (u64)(cb + (int64_t)n);
        key_unitig[i] = ua;
        if (ua != ub) comp_union(parent, ua, ub, n, err);
    }
};

struct CompJumpFunctor {
    u32* parent; u32* changed; u32 round;
    AC_D void operator()(u64 u) const {
        if (round && atomic_load32(&changed[round - 1]) == 0) return;
        const u32 p = atomic_load32(&parent[u]);
        const u32 g = atomic_load32(&parent[p]);
        if (g != p) { atomic_min32(&parent[u], g); atomic_or32(&changed[round], 1u); }
    }
};

struct CompRootsFunctor {
    const u32* parent; const u8* alive; u32 n; const u32* deg; const int32_t* target; const u32* notself;
    u32* is_root; u8* flags; u32* err;
    AC_D void operator()(u64 u) const {
        const u32 p = parent[u];
        if (parent[p] != p) atomic_or32(err, COMP_ERR_BOUND);      // (the jump rounds did not flatten this tree)
        const bool live = !alive || alive[u];
        is_root[u] = live && p == (u32)u ? 1u : 0u;
        u8 f = 0;
        if (live) {
            const u32 dfn = deg[(u64)COMP_FN * n + u], drn = deg[(u64)COMP_RN * n + u], dfp = deg[(u64)COMP_FP * n + u];
            const int32_t self = (int32_t)(u + 1);
            if (drn == 0) f |= CUF_OPEN_START;
            if (dfn == 0) f |= CUF_OPEN_END;
            if (drn == 1 && target[(u64)COMP_RN * n + u] == self) f |= CUF_HAIRPIN_START;
            if (dfn == 1 && target[(u64)COMP_FN * n + u] == -self) f |= CUF_HAIRPIN_END;
            const bool circ = dfn == 1 && dfp == 1 && target[(u64)COMP_FN * n + u] == self && target[(u64)COMP_FP * n + u] == self;
            if (circ) f |= CUF_ISOLATED_CIRCULAR;
            if (dfn <= 1 && dfp <= 1 && !circ && notself[u] == 0) f |= CUF_ISOLATED_LINEAR;
        }
        flags[u] = f;
    }
};

struct CompLabelFunctor {
    const u32* parent; const u32* is_root; const u32* root_rank; const u8* alive; u32 n;
    u32* component_of; u64* sort_key; u32* sort_val; CompHeader* hdr;
    AC_D void operator()(u64 u) const {
        const bool live = !alive || alive[u];
        const u32 c = live ? root_rank[parent[u]] : COMP_DEAD;
        component_of[u] = c;
        sort_key[u] = live ? (u64)c : (u64)n;
        sort_val[u] = (u32)u + 1;
        if (u + 1 == n) { hdr->n_components = (u64)root_rank[u] + is_root[u]; hdr->n_alive = n; }      // (n_alive: until the segments find a unitig that is not alive)
    }
};

// The runs of one component inside a wavefront: a lane starts a run when its left neighbour holds another component (the members are sorted
// by component; the links only by their first unitig, where a component may come back later in the wavefront: a run of its own each time).
// Returns the run's number, which ascends across the lanes.
AC_D u32 comp_run_id(u32 c, int lane) {
    const u32 left = (u32)wv::shfl_up((int)c, 1);
    const u64 heads = wv::ballot(lane == 0 || left != c);
    return (u32)prim_popc64(heads & ((2ULL << lane) - 1ULL));
}
// inclusive sum over the lanes of this lane's run up to this lane
AC_D u64 comp_run_sum64(u64 v, u32 run, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = wave_shfl_up64(v, o);
        const u32 tr = (u32)wv::shfl_up((int)run, o);
        if (lane >= o && tr == run) v += t;
    }
    return v;
}

// sorted[j] = (component index, unitig number), ascending
struct CompSegmentsFunctor {
    const u64* sort_key; const u32* sort_val; u32 n; const u32* unitig_len; const u8* marked; const u32* deg;
    u64* member_off; u64* c_length; u64* c_ends_marked; u32* c_not_one; CompHeader* hdr;
    AC_D void operator()(u64 j, bool valid) const {
        const int lane = wv::lane();
        u32 c = COMP_DEAD; u64 len = 0, em = 0, bad = 0;
        if (valid) {
            const u64 k = sort_key[j];
            const bool first_of_key = j == 0 || sort_key[j - 1] != k;
            if (k == (u64)n) { if (first_of_key) hdr->n_alive = j; }
            else {
                c = (u32)k;
                const u32 u = sort_val[j] - 1;
                if (first_of_key) member_off[c] = j;
                const u32 dfn = deg[(u64)COMP_FN * n + u], drn = deg[(u64)COMP_RN * n + u], dfp = deg[(u64)COMP_FP * n + u], drp = deg[(u64)COMP_RP * n + u];
                len = unitig_len ? unitig_len[u] : 0;
                em = (u64)((drn == 0) + (dfn == 0)) | ((u64)(marked && marked[u] ? 1 : 0) << 32);      // two sums below 2^32 each in one word
                bad = (dfn != 1 || drn != 1 || dfp != 1 || drp != 1) ? 1 : 0;
            }
        }
        const u32 run = comp_run_id(c, lane);
        len = comp_run_sum64(len, run, lane); em = comp_run_sum64(em, run, lane); bad = comp_run_sum64(bad, run, lane);
        const u32 next_run = (u32)wv::shfl_down((int)run, 1);
        if (c != COMP_DEAD && (lane == 63 || next_run != run)) {      // the last lane of the run: one atomic per (wavefront, component) and sum
            if (len) atomic_add64(&c_length[c], len);
            if (em) atomic_add64(&c_ends_marked[c], em);
            if (bad) atomic_add32(&c_not_one[c], (u32)bad);
        }
    }
};

// key[j] ascending (dropped entries last), key_unitig[j] = a unitig of the entry
struct CompLinkCountFunctor {
    const u64* key; const u32* key_unitig; u64 n_links; u32 n; int key_bits; const u32* component_of;
    u64* c_links_all; u64* c_links_one_way;
    AC_D void operator()(u64 j, bool valid) const {
        const int lane = wv::lane();
        const u64 dropped = link_key_dropped(key_bits);
        u32 c = COMP_DEAD; u64 counts = 0;      // one_way | all << 32
        if (valid) {
            const u64 k = key[j];
            if (k != dropped) {
                c = component_of[key_unitig[j]];
                if (j == 0 || key[j - 1] != k) {
                    const int64_t ca = (int64_t)(k >> key_bits) - (int64_t)n, cb = (int64_t)(k & ((1ULL << key_bits) - 1ULL)) - (int64_t)n;
                    counts = 1ULL | ((ca == -cb ? 1ULL : 2ULL) << 32);      // its own reverse complement: once in all_links
                }
            }
        }
        // the keys ascend by their first unitig, so a unitig's links — and a component's, where its numbers are neighbours — sit side by side
        const u32 run = comp_run_id(c, lane);
        counts = comp_run_sum64(counts, run, lane);
        const u32 next_run = (u32)wv::shfl_down((int)run, 1);
        if (c != COMP_DEAD && (lane == 63 || next_run != run) && counts) {
            atomic_add64(&c_links_one_way[c], counts & 0xFFFFFFFFULL);
            atomic_add64(&c_links_all[c], counts >> 32);
        }
    }
};

// component c: its record; c == n_components: the end of the member offsets
struct CompRecordsFunctor {
    const CompHeader* hdr; u32 n; const u64* member_off_in; const u32* members; const u64* c_length; const u64* c_ends_marked; const u32* c_not_one;
    const u64* c_links_all; const u64* c_links_one_way; const int32_t* target;
    u64* member_off; u8* stamp; ComponentRecord* records; u32* err;
    AC_D void operator()(u64 c) const {
        const u64 nc = hdr->n_components;
        if (c > nc) return;
        if (c == nc) { member_off[c] = hdr->n_alive; return; }
        const u64 begin = member_off_in[c], end = c + 1 == nc ? hdr->n_alive : member_off_in[c + 1];
        const u32 first = members[begin], size = (u32)(end - begin);
        member_off[c] = begin;
        ComponentRecord& r = records[c];      // (the buffer was zeroed: the padding bytes stay 0)
        r.first = first; r.unitigs = size;
        r.length = c_length[c]; r.links_all = c_links_all[c]; r.links_one_way = c_links_one_way[c];
        r.open_ends = (u32)(c_ends_marked[c] & 0xFFFFFFFFULL); r.marked = (u32)(c_ends_marked[c] >> 32);
        // component_is_circular_loop (unitig_graph.rs:949-967) from (first, +).  A member whose four list lengths are not all 1 makes the
        // reference's walk fail wherever it meets it, and a walk that never meets it cannot have visited the whole component: false either way.
        u8 loop = 0;
        if (c_not_one[c] == 0) {
            u32 num = first, visited = 0;
            bool forward = true, ok = true;
            while (num != first || visited == 0) {
                if (visited > size) { atomic_or32(err, COMP_ERR_BOUND); ok = false; break; }      // (cannot happen: every step stamps a new member)
                if (stamp[num - 1]) { ok = false; break; }
                stamp[num - 1] = 1; visited++;
                const int32_t nx = target[(u64)(forward ? COMP_FN : COMP_RN) * n + (num - 1)];
                num = (u32)(nx < 0 ? -nx : nx); forward = nx > 0;
            }
            loop = ok && visited == size ? 1 : 0;
        }
        r.circular_loop = loop;
    }
};

void components_device(uint32_t n, const Link* links, uint64_t n_links, const uint32_t* unitig_len, const uint8_t* alive, const uint8_t* marked,
                       ComponentsResult* out) {
    *out = ComponentsResult();
    out->n_unitigs = n;
    if (n > 0x7FFFFFFEu) throw DeviceError("components: more unitigs than a signed unitig number can name");
    if (n_links >= 0xFFFFFFF0ULL) throw DeviceError("components: more than 2^32 links");
    if (n == 0) {
        if (n_links) throw DeviceError(components_bad_link_message(0, links[0].a, links[0].b, 0));
        out->member_off.assign(1, 0);
        components_finish(out);
        return;
    }
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    const u64 nl = n_links;
    const int key_bits = bit_width(2 * (u64)n), comp_bits = bit_width((u64)n);
    const u32 rounds = jump_rounds(n);

    DBuf<Link> d_links(nl);
    DBuf<u32> d_len(unitig_len ? n : 0); DBuf<u8> d_alive(alive ? n : 0), d_marked(marked ? n : 0);
    copy_h2d(d_links.ptr(), links, nl * sizeof(Link));
    if (unitig_len) copy_h2d(d_len.ptr(), unitig_len, (u64)n * 4);
    if (alive) copy_h2d(d_alive.ptr(), alive, n);
    if (marked) copy_h2d(d_marked.ptr(), marked, n);
    const u32* p_len = unitig_len ? d_len.ptr() : nullptr;
    const u8* p_alive = alive ? d_alive.ptr() : nullptr;
    const u8* p_marked = marked ? d_marked.ptr() : nullptr;

    DBuf<u32> d_deg((u64)4 * n), d_notself(n), d_parent(n), d_err(2), d_changed(rounds), d_is_root(n), d_root_rank(n), d_component_of(n), d_sort_val(n), d_not_one(n);
    DBuf<int32_t> d_target((u64)4 * n);
    DBuf<u64> d_key(nl), d_sort_key(n), d_off_in(n), d_off((u64)n + 1), d_length(n), d_ends_marked(n), d_links_all(n), d_links_one_way(n);
    DBuf<u32> d_key_unitig(nl);
    DBuf<u8> d_flags(n), d_stamp(n);
    DBuf<CompHeader> d_hdr(1);
    DBuf<ComponentRecord> d_records(n);
    d_deg.fill_bytes(0); d_notself.fill_bytes(0); d_err.fill_bytes(0); d_changed.fill_bytes(0); d_target.fill_bytes(0); d_not_one.fill_bytes(0);
    d_length.fill_bytes(0); d_ends_marked.fill_bytes(0); d_links_all.fill_bytes(0); d_links_one_way.fill_bytes(0); d_stamp.fill_bytes(0);
    d_records.fill_bytes(0); d_off.fill_bytes(0); d_off_in.fill_bytes(0);
    d_hdr.fill_bytes(0xFF);      // first_bad_link: none
    RadixScratch sort_members, sort_links;
    sort_members.prepare(n, comp_bits);
    sort_links.prepare(nl, 2 * key_bits);

    meter.begin();
    launch(n, CompInitFunctor{d_parent.ptr()});
    if (nl) {
        launch(nl, CompCensusFunctor{d_links.ptr(), n, p_alive, key_bits, d_deg.ptr(), d_target.ptr(), d_notself.ptr(), d_parent.ptr(), d_key.ptr(), d_key_unitig.ptr(),
                                     d_err.ptr(), d_hdr.ptr()});
        for (u32 r = 0; r < rounds; r++) launch(n, CompJumpFunctor{d_parent.ptr(), d_changed.ptr(), r});
    }
    launch(n, CompRootsFunctor{d_parent.ptr(), p_alive, n, d_deg.ptr(), d_target.ptr(), d_notself.ptr(), d_is_root.ptr(), d_flags.ptr(), d_err.ptr()});
    exclusive_scan_u32(d_is_root.ptr(), d_root_rank.ptr(), n);
    launch(n, CompLabelFunctor{d_parent.ptr(), d_is_root.ptr(), d_root_rank.ptr(), p_alive, n, d_component_of.ptr(), d_sort_key.ptr(), d_sort_val.ptr(), d_hdr.ptr()});
    sort_pairs_u64_u32(d_sort_key, d_sort_val, n, comp_bits, 0, 0, &sort_members);
    launch_full(n, CompSegmentsFunctor{d_sort_key.ptr(), d_sort_val.ptr(), n, p_len, p_marked, d_deg.ptr(), d_off_in.ptr(), d_length.ptr(), d_ends_marked.ptr(),
                                       d_not_one.ptr(), d_hdr.ptr()});
    if (nl) {
        sort_pairs_u64_u32(d_key, d_key_unitig, nl, 2 * key_bits, 0, 0, &sort_links);
        launch_full(nl, CompLinkCountFunctor{d_key.ptr(), d_key_unitig.ptr(), nl, n, key_bits, d_component_of.ptr(), d_links_all.ptr(), d_links_one_way.ptr()});
    }
    launch((u64)n + 1, CompRecordsFunctor{d_hdr.ptr(), n, d_off_in.ptr(), d_sort_val.ptr(), d_length.ptr(), d_ends_marked.ptr(), d_not_one.ptr(), d_links_all.ptr(),
                                          d_links_one_way.ptr(), d_target.ptr(), d_off.ptr(), d_stamp.ptr(), d_records.ptr(), d_err.ptr()});
    meter.end();
    // the read-back: the header and the error word say how much there is to fetch (the arrays are sized by n; what crosses is sized by the
    // components and the alive unitigs), then everything else behind one synchronisation
    CompHeader h; u32 err[2] = {0, 0};
    {
        ReadBatch rb;
        rb.add(&h, d_hdr.ptr(), sizeof h); rb.add(err, d_err.ptr(), sizeof err);
        rb.run();
    }
    if (err[0] & COMP_ERR_RANGE) {
        const u64 i = h.first_bad_link < nl ? h.first_bad_link : 0;
        throw DeviceError(components_bad_link_message(i, links[i].a, links[i].b, n));
    }
    if (err[0] & COMP_ERR_BOUND) throw DeviceError("components: a loop of the device analysis reached its bound (internal error)");
    if (h.n_components > n || h.n_alive > n || h.n_components > h.n_alive) throw DeviceError("components: the device returned an impossible header (internal error)");
    const size_t nc = (size_t)h.n_components, na = (size_t)h.n_alive;
    out->records.resize(nc); out->component_of.resize(n); out->member_off.resize(nc + 1); out->members.resize(na); out->flags.resize(n);
    copy_d2h_async(out->records.data(), d_records.ptr(), nc * sizeof(ComponentRecord));
    copy_d2h_async(out->component_of.data(), d_component_of.ptr(), (u64)n * 4);
    copy_d2h_async(out->member_off.data(), d_off.ptr(), (nc + 1) * 8);
    copy_d2h_async(out->members.data(), d_sort_val.ptr(), na * 4);
    copy_d2h_async(out->flags.data(), d_flags.ptr(), n);
    meter.sync_copies();
    out->stats = meter.stats();
    components_finish(out);
}
