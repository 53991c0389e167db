// qc_clusters' matrix work (cluster.rs:560-567 with cluster_is_contained_in_another :692-723) for ALL alternatives of a refinement round at
// once, ON THE DEVICE — part of graph_extras.hip (included inside namespace ac after kernels_cluster.inc; not a translation unit of its own).
// The host side (cluster_qc_host.cpp) writes a ClusterQcPlan per evaluation and turns the verdict words into records, metrics and the accept
// walk; the layout of the plan and of the pair bytes is described at ClusterQcPlan.  DESIGN.md §9f.
//
// Once per call
//   bits     C[p][q] = d(a,b) < d(b,a) && d(a,b) < cutoff for a = dfs_tip[p], b = dfs_tip[q]: rows and columns in the tree's left-first
//            depth-first tip order, 64 columns per u64 (one ballot per word).  The two comparisons are the only f64 work on the device.  Every
//            entry of the matrix is looked at exactly once as d(a,b) and checked as the tree entry checks it.
// Per evaluation (the start clustering alone, or all alternatives of one round), a fixed number of launches and one read-back
//   pairs    one wavefront per entry of the plan's pair table: contain = the sum over the rows p of x of popcount(C[p] & columns of y), the
//            lanes striding rows x words; the byte is 2 * contain > size(x) * size(y), in integers (the reference's f64 quotient > 0.5 is that
//            for every total <= 2^28).  A base pair is counted once per round however many alternatives share it.
//   chain    one single-wavefront workgroup per alternative: the too-few-assemblies failures (a flag the host set per node) into the set of
//            clusters "passing so far" (a bit set in LDS, filled by ballots), then c = 1 .. max in order: a cluster that is not trusted looks
//            for the smallest passing y != c whose pair byte says "c is contained in y", 64 candidates per ballot, and leaves the set if
//            there is one.  One word per cluster goes back: fail bits | container << 8.
// No workgroup waits for another one; every loop is bounded by the cluster count or by rows x words of one pair.  Every index is below
// its array's size by construction of the plan: positions j < count <= S, entities < n + 2, tip ranges inside [0, S), words below W.
static const u32 CLUSTER_QC_DEFAULT_PAIR_BATCH = 1u << 24;      // pair entries per launch (AC_CLUSTER_QC_PAIR_BATCH); 4 per workgroup

struct ClusterQcBitsFunctor {
    const double* asym; const u32* dfs_tip; u32 S, W; double cutoff; u64* bits; u32* bad;
    AC_D void operator()(u64 i, bool valid) const {
        const u64 row_bits = (u64)W * 64;
        const u64 p = i / row_bits, q = i % row_bits;
        bool bit = false;
        if (valid && q < S) {
            const u64 a = dfs_tip[p], b = dfs_tip[q];
            const double ab = asym[a * S + b], ba = asym[b * S + a];
            if (!(ab >= 0.0 && ab < cluster_inf())) atomic_or32(bad, 1u);
            bit = ab < ba && ab < cutoff;
        }
        const u64 word = wv::ballot(bit);
        if (valid && wv::lane() == 0) bits[i >> 6] = word;
    }
};

// position j of an alternative's reordered clusters -> base position, or CHILD0 / CHILD1 (ClusterQcPlan::entity with the children marked
// by the two largest values, so that "is a base cluster" is one comparison)
static const u32 CLUSTER_QC_CHILD0 = CLUSTER_QC_NONE - 1, CLUSTER_QC_CHILD1 = CLUSTER_QC_NONE;
AC_D u32 cluster_qc_entity(u32 kpos, u32 ins0, u32 ins1, u32 j) {
    if (j == ins0) return CLUSTER_QC_CHILD0;
    if (j == ins1) return CLUSTER_QC_CHILD1;
    const u32 r = j - (j > ins0 ? 1u : 0u) - (j > ins1 ? 1u : 0u);
    return r + (r >= kpos ? 1u : 0u);
}

AC_KERNEL void __launch_bounds__(256) cluster_qc_pairs_kernel(u64 e0, u64 e1, u32 n, u32 W, const u64* bits, const ClusterQcEntity* base,
                                                              const ClusterQcAlt* alts, u8* contained) {
    const u64 e = e0 + (u64)wv::bid() * 4 + (wv::tid() >> 6);
    if (e >= e1) return;      // (whole wavefronts, here and below: every condition is on e alone)
    const u64 nn = (u64)n * n;
    ClusterQcEntity x, y;
    if (e < nn) {
        const u32 bx = (u32)(e / n), by = (u32)(e % n);
        if (bx == by) return;
        x = base[bx]; y = base[by];
    } else {
        const u64 per = 4ull * n + 2, rest = e - nn;
        const ClusterQcAlt& al = alts[rest / per];
        if (al.kpos == CLUSTER_QC_NONE) return;
        const u32 r = (u32)(rest % per);
        if (r < 2 * n) { const u32 b = r % n; if (b == al.kpos) return; x = al.child[r / n]; y = base[b]; }
        else if (r < 4 * n) { const u32 b = (r - 2 * n) % n; if (b == al.kpos) return; x = base[b]; y = al.child[(r - 2 * n) / n]; }
        else { x = al.child[r - 4 * n]; y = al.child[1 - (r - 4 * n)]; }
    }
    const u32 w0 = y.lo >> 6, w1 = (y.hi - 1) >> 6, nw = w1 - w0 + 1;
    const u32 items = (x.hi - x.lo) * nw;      // (at most S * S / 64 = 2^22)
    u32 contain = 0;
    for (u32 i = (u32)wv::lane(); i < items; i += 64) {
        const u32 p = x.lo + i / nw, w = w0 + i % nw;
        u64 mask = ~0ULL;
        if (w == w0) mask &= ~0ULL << (y.lo & 63);
        if (w == w1 && (y.hi & 63)) mask &= ~0ULL >> (64 - (y.hi & 63));
        contain += (u32)popc64(bits[(u64)p * W + w] & mask);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) contain += (u32)wv::shfl_xor((int)contain, o);
    if (wv::lane() == 0) contained[e] = 2ull * contain > (u64)(x.hi - x.lo) * (y.hi - y.lo) ? 1 : 0;
}

AC_KERNEL void __launch_bounds__(64) cluster_qc_chain_kernel(u32 n, const ClusterQcEntity* base, const ClusterQcAlt* alts, const u8* contained,
                                                             const u32* bad, u32* out) {
    AC_SHARED u32 s_pass[CLUSTER_MAX_SEQS / 32 + 2];
    const u32 a = wv::bid();
    const u32 l = (u32)wv::lane();
    const u32 kpos = alts[a].kpos, ins0 = alts[a].ins0, ins1 = alts[a].ins1;      // (scalars: nothing here indexes a local array)
    const u32 flags0 = alts[a].child[0].flags, flags1 = alts[a].child[1].flags;
    const u32 cnt = n + (kpos != CLUSTER_QC_NONE ? 1u : 0u);
    const u64 off = (u64)n * n + (u64)a * (4ull * n + 2);
    u32* verdict = out + 1 + (u64)a * (n + 1);
    if (a == 0 && l == 0) out[0] = *bad;
    for (u32 j0 = 0; j0 < cnt; j0 += 64) {      // (the same trip count in every lane: the ballot is met by all)
        const u32 j = j0 + l;
        u32 fail = 0;
        if (j < cnt) {
            const u32 ent = cluster_qc_entity(kpos, ins0, ins1, j);
            fail = (ent < n ? base[ent].flags : (ent == CLUSTER_QC_CHILD0 ? flags0 : flags1)) & 2u;
            verdict[j] = fail;
        }
        const u64 pass = wv::ballot(j < cnt && fail == 0);
        if (l == 0) { s_pass[j0 >> 5] = (u32)pass; s_pass[(j0 >> 5) + 1] = (u32)(pass >> 32); }
    }
    wv::block_sync();
    for (u32 c = 0; c < cnt; c++) {
        const u32 ec = cluster_qc_entity(kpos, ins0, ins1, c);
        const u32 flags = ec < n ? base[ec].flags : (ec == CLUSTER_QC_CHILD0 ? flags0 : flags1);
        if (flags & 1u) continue;      // trusted: nothing can fail it
        u32 found = CLUSTER_QC_NONE;
        for (u32 y0 = 0; y0 < cnt; y0 += 64) {
            const u32 y = y0 + l;
            bool hit = false;
            if (y < cnt && y != c && ((s_pass[y >> 5] >> (y & 31)) & 1u)) {
                const u32 ey = cluster_qc_entity(kpos, ins0, ins1, y);
                u64 at;      // (ClusterQcPlan's layout of the pair bytes)
                if (ec < n) at = ey < n ? (u64)ec * n + ey : off + 2ull * n + (u64)(ey - CLUSTER_QC_CHILD0) * n + ec;
                else at = ey < n ? off + (u64)(ec - CLUSTER_QC_CHILD0) * n + ey : off + 4ull * n + (ec - CLUSTER_QC_CHILD0);
                hit = contained[at] != 0;
            }
            const u64 m = wv::ballot(hit);
            if (m) { found = y0 + (u32)__builtin_ctzll(m); break; }
        }
        if (found == CLUSTER_QC_NONE) continue;
        if (l == 0) {
            verdict[c] = (flags & 2u) | 4u | ((found + 1) << 8);
            s_pass[c >> 5] &= ~(1u << (c & 31));
        }
        wv::block_sync();
    }
}

// One call's session: the contain bits on the device, then any number of evaluations.
struct ClusterQcSession {
    u32 S, W;
    DBuf<u64> bits;
    DBuf<u32> bad;
    ClusterQcDeviceStats* st;
    u64 pair_batch;
    StepMeter meter;      // one interval per evaluation

    void evaluate(const ClusterQcPlan& plan, std::vector<u32>* verdicts) {
        Arena& arena = Arena::device();
        const Arena::Mark mark = arena.mark();
        const u32 n = plan.n, A = (u32)plan.alts.size();
        if (n == 0 || n > S || A == 0) throw DeviceError("cluster: an evaluation of " + std::to_string(n) + " clusters and " + std::to_string(A) + " alternatives");
        for (const ClusterQcEntity& x : plan.base) if (x.lo >= x.hi || x.hi > S) throw DeviceError("cluster: a tip range outside the tree");
        for (const ClusterQcAlt& al : plan.alts) {
            if (al.kpos == CLUSTER_QC_NONE) continue;
            if (al.kpos >= n || al.ins0 >= al.ins1 || al.ins1 > n || n + 1 > S) throw DeviceError("cluster: an alternative outside its base clustering");
            for (const ClusterQcEntity& x : al.child) if (x.lo >= x.hi || x.hi > S) throw DeviceError("cluster: a tip range outside the tree");
        }
        const u64 entries = plan.pair_entries(), words = 1 + (u64)A * plan.stride();
        DBuf<ClusterQcEntity> d_base(n);
        DBuf<ClusterQcAlt> d_alts(A);
        DBuf<u8> d_contained(entries);
        DBuf<u32> d_out(words);
        copy_h2d(d_base.ptr(), plan.base.data(), (size_t)n * sizeof(ClusterQcEntity));
        copy_h2d(d_alts.ptr(), plan.alts.data(), (size_t)A * sizeof(ClusterQcAlt));
        meter.begin();
        for (u64 b0 = 0; b0 < entries; b0 += pair_batch) {
            const u64 b1 = std::min(entries, b0 + pair_batch);
            launch_wave_kernel(cluster_qc_pairs_kernel, (b1 - b0 + 3) / 4, 0, b0, b1, n, W, (const u64*)bits.ptr(), (const ClusterQcEntity*)d_base.ptr(),
                               (const ClusterQcAlt*)d_alts.ptr(), d_contained.ptr());
            st->launches++; st->pair_batches++;
        }
        launch_wave_kernel_sized(cluster_qc_chain_kernel, A, 64u, 0, n, (const ClusterQcEntity*)d_base.ptr(), (const ClusterQcAlt*)d_alts.ptr(),
                                 (const u8*)d_contained.ptr(), (const u32*)bad.ptr(), d_out.ptr());
        st->launches++;
        meter.end();
        std::vector<u32> h_out(words);
        copy_d2h(h_out.data(), d_out.ptr(), (size_t)words * 4);
        st->readbacks++; st->evaluations++; st->bytes_read_back += words * 4;
        st->seconds += meter.take();
        st->alternatives += A; st->pairs_counted += plan.pairs_counted();
        arena.rewind(mark);
        if (h_out[0]) throw DeviceError("cluster: the distance matrix holds a NaN, an infinite or a negative value");
        verdicts->assign(h_out.begin() + 1, h_out.end());
    }
};

void cluster_qc_device(const double* asym, uint32_t n, const uint32_t* dfs_tip, double cutoff, const std::function<void(const ClusterQcEvaluate&)>& body,
                       ClusterQcDeviceStats* stats) {
    if (n == 0 || n > CLUSTER_MAX_SEQS) throw DeviceError("cluster: " + std::to_string(n) + " sequences (1 .. " + std::to_string(CLUSTER_MAX_SEQS) + ", ac_cluster_max_seqs)");
    Arena::device().reset();
    ClusterQcSession s;
    s.S = n; s.W = (n + 63) / 64; s.st = stats;
    {
        const char* e = getenv("AC_CLUSTER_QC_PAIR_BATCH");      // (read at every call: the tests lower it)
        const long long v = e ? atoll(e) : 0;
        s.pair_batch = v > 0 ? std::min<u64>((u64)v, (u64)1 << 25) : CLUSTER_QC_DEFAULT_PAIR_BATCH;
    }
    s.bits.alloc((u64)n * s.W);
    s.bad.alloc(1);
    s.bad.fill_bytes(0);
    {   // (the matrix and the tip order are only needed for the bits: their room goes back to the arena)
        const Arena::Mark mark = Arena::device().mark();
        DBuf<double> d_asym((u64)n * n);
        DBuf<u32> d_tip(n);
        copy_h2d(d_asym.ptr(), asym, (size_t)n * n * 8);
        copy_h2d(d_tip.ptr(), dfs_tip, (size_t)n * 4);
        launch_full((u64)n * s.W * 64, ClusterQcBitsFunctor{d_asym.ptr(), d_tip.ptr(), n, s.W, cutoff, s.bits.ptr(), s.bad.ptr()});
        stats->launches++;
        Arena::device().rewind(mark);
    }
    body([&](const ClusterQcPlan& plan, std::vector<uint32_t>* verdicts) { s.evaluate(plan, verdicts); });
}
