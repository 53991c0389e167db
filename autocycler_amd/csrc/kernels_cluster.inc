// upgma (cluster.rs:395-480), the merge loop of `autocycler cluster`, ON THE DEVICE — part of graph_extras.hip (included inside namespace ac
// after neighbours.inc, whose pair-length kernels the graph entry reuses; not a translation unit of its own).  The host side
// (cluster_host.cpp) turns the merges into the tree and does everything after it.
//
// Arithmetic (DESIGN.md §9e; the tests hold it to a plain-Python model bit for bit).  Rows and columns are the sequences in ascending id
// order.  sum[i][j] = max(d(i,j), d(j,i)) at the start and avg = sum; a merge of a < b sets sum[a][X] = sum[a][X] + sum[b][X] (that operand
// order) and avg[a][X] = sum[a][X] / (double)(size(a u b) * size(X)), the product in integers.  Only avg is compared.  No expression here
// can fuse into a multiply-add (there is no product of doubles), and contraction is switched off all the same.
//
// State: sum and avg in full (both mirror halves: every row scan is contiguous), active[S], size[S], a nearest-neighbour cache per row
// (nn_val[r] / nn_col[r]: the minimum of avg[r][c] over the active c > r, the smallest c among equal values; col = NONE when there is no
// such c), the merges, and ClusterStateDev.
//
// Schedule: a merge is three plain launches on the stream, and the host reads nothing until the last merge is done.
//   pick     ONE workgroup reduces (nn_val[r], r) over the active rows — with the cache's smallest-column rule that is get_closest_pair's
//            order (value, a, b) — records the merge, publishes a and b, and only then (after its last read of them) adds size[b] to size[a]
//            and retires b.
//   fold     one thread per active X != a: the update above, both mirror entries.  size[a] is already the merged size, size[X] is untouched.
//   refresh  one wavefront per row r < b: row a, and any row whose cached column is a or b, is scanned again (a wave-strided loop, a
//            shuffle reduction of (value, column)); any other row r < a compares the new avg[r][a] with its cache; rows between a and b
//            whose cache names neither, and rows above b, cannot change.
// No workgroup waits for another one: every loop is bounded by S.  A pick that finds no pair (possible only when the input held a NaN or
// an infinity, which the setup has flagged for the host) publishes NONE, and fold and refresh then do nothing: no index leaves [0, S).
static const u32 CLUSTER_MAX_SEQS = 16384;      // three S x S f64 arrays: 6.4 GB
static const u32 CLUSTER_NONE = 0xFFFFFFFFu;
struct ClusterStateDev {
    u32 a, b;            // the pair the last pick published (rows)
    u32 step;            // merges recorded
    u32 bad;             // the input held a NaN, an infinity or a negative distance
    u64 rescans, compares;
};
struct ClusterMergeDev { u32 a, b; double distance; };

AC_D double cluster_inf() { return __builtin_huge_val(); }
AC_D double cluster_shfl_xor_f64(double v, int m) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    u = wv::shfl_xor64(u, m);
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// (graph entry) the distances from the integer intersection lengths, with the two operations pairwise_distances_device does on the host
struct ClusterQuotientFunctor {
    const u64* ab; u32 S; double* asym;
    AC_D void operator()(u64 i) const {
#pragma clang fp contract(off)
        const u64 a = i / S;
        const double a_len = (double)(u32)ab[a * S + a];
        const double q = (double)ab[i] / a_len;
        asym[i] = 1.0 - q;
    }
};
// make_symmetrical_distances (cluster.rs:177-192) into sum and avg; every entry of the input is checked on the way
struct ClusterSymFunctor {
    const double* asym; u32 S; double* sum; double* avg; ClusterStateDev* st;
    AC_D void operator()(u64 i) const {
        const u64 r = i / S, c = i % S;
        const u64 lo = r < c ? r : c, hi = r < c ? c : r;
        const double own = asym[i];
        if (!(own >= 0.0 && own < cluster_inf())) atomic_or32(&st->bad, 1u);
        const double x = asym[lo * S + hi], y = asym[hi * S + lo];
        const double v = y > x ? y : x;
        sum[i] = v; avg[i] = v;
    }
};
struct ClusterInitFunctor {
    u32* active; u32* size;
    AC_D void operator()(u64 r) const { active[r] = 1; size[r] = 1; }
};

AC_KERNEL void __launch_bounds__(256) cluster_pick_kernel(u32 S, const double* nn_val, const u32* nn_col, u32* active, u32* size, ClusterStateDev* st,
                                                          ClusterMergeDev* merges) {
    AC_SHARED double s_val[4];
    AC_SHARED u32 s_row[4];
    AC_SHARED u32 s_col[4];
    const u32 t = wv::tid();
    double bv = cluster_inf(); u32 br = CLUSTER_NONE, bc = CLUSTER_NONE;
    for (u32 r = t; r < S; r += 256) {      // (ascending rows and a strict comparison: the smallest row among equal values)
        if (!active[r]) continue;
        const u32 c = nn_col[r];
        if (c >= S) continue;
        const double v = nn_val[r];
        if (v < bv) { bv = v; br = r; bc = c; }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = cluster_shfl_xor_f64(bv, o);
        const u32 orow = (u32)wv::shfl_xor((int)br, o), ocol = (u32)wv::shfl_xor((int)bc, o);
        if (ov < bv || (ov == bv && orow < br)) { bv = ov; br = orow; bc = ocol; }
    }
    if (wv::lane() == 0) { s_val[t >> 6] = bv; s_row[t >> 6] = br; s_col[t >> 6] = bc; }
    wv::block_sync();
    if (t != 0) return;
    for (int w = 1; w < 4; w++)
        if (s_val[w] < bv || (s_val[w] == bv && s_row[w] < br)) { bv = s_val[w]; br = s_row[w]; bc = s_col[w]; }
    const u32 step = st->step;
    if (br < bc && bc < S && step + 1 < S) {
        merges[step] = ClusterMergeDev{br, bc, bv};
        st->step = step + 1;
        st->a = br; st->b = bc;
        size[br] += size[bc];
        active[bc] = 0;
    } else {
        st->a = CLUSTER_NONE; st->b = CLUSTER_NONE;
    }
}

struct ClusterFoldFunctor {
    u32 S; double* sum; double* avg; const u32* active; const u32* size; const ClusterStateDev* st;
    AC_D void operator()(u64 x) const {
#pragma clang fp contract(off)
        const u32 a = st->a, b = st->b;
        if (a >= S || b >= S || x == a || !active[x]) return;      // (b itself is retired already)
        const u64 ax = (u64)a * S + x, bx = (u64)b * S + x, xa = x * S + a;
        const double s = sum[ax] + sum[bx];
        const double n = (double)((u64)size[a] * (u64)size[x]);
        const double v = s / n;
        sum[ax] = s; sum[xa] = s;
        avg[ax] = v; avg[xa] = v;
    }
};

// init != 0: every row's cache from scratch (the setup).  Otherwise the rows the merge (st->a, st->b) can have changed.
AC_KERNEL void __launch_bounds__(256) cluster_refresh_kernel(u32 S, int init, const double* avg, const u32* active, double* nn_val, u32* nn_col,
                                                             ClusterStateDev* st) {
    const u32 r = wv::bid() * 4 + (wv::tid() >> 6);
    if (r >= S) return;      // (whole wavefronts, here and below: every condition is on r alone)
    const int l = wv::lane();
    if (!init) {
        const u32 a = st->a, b = st->b;
        if (a >= S || b >= S || r >= b || !active[r]) return;
        const u32 c = nn_col[r];
        if (!(r == a || c == a || c == b)) {
            if (r < a && l == 0) {
                const double v = avg[(u64)r * S + a], cur = nn_val[r];
                if (v < cur || (v == cur && a < c)) { nn_val[r] = v; nn_col[r] = a; }
                atomic_add64(&st->compares, 1);
            }
            return;
        }
    }
    double bv = cluster_inf(); u32 bc = CLUSTER_NONE;
    const double* row = avg + (u64)r * S;
    for (u32 c = r + 1 + (u32)l; c < S; c += 64) {      // (ascending columns and a strict comparison: the smallest column among equal values)
        if (!active[c]) continue;
        const double v = row[c];
        if (v < bv) { bv = v; bc = c; }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = cluster_shfl_xor_f64(bv, o);
        const u32 oc = (u32)wv::shfl_xor((int)bc, o);
        if (ov < bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    if (l == 0) {
        nn_val[r] = bv; nn_col[r] = bc;
        if (!init) atomic_add64(&st->rescans, 1);
    }
}

uint32_t cluster_max_seqs() { return CLUSTER_MAX_SEQS; }

// The loop on a matrix that is on the device already (the arena session is the caller's).
static void cluster_merge_loop(const double* d_asym, u32 S, std::vector<ClusterRowMerge>* merges, ClusterDeviceStats* stats) {
    const u64 SS = (u64)S * S;
    DBuf<double> sum(SS), avg(SS), nn_val(S);
    DBuf<u32> nn_col(S), active(S), size(S);
    DBuf<ClusterStateDev> st(1);
    DBuf<ClusterMergeDev> d_merges(S);      // (S - 1 are written)
    st.fill_bytes(0);
    u32 launches = 0;
    launch(SS, ClusterSymFunctor{d_asym, S, sum.ptr(), avg.ptr(), st.ptr()});
    launch(S, ClusterInitFunctor{active.ptr(), size.ptr()});
    launch_wave_kernel(cluster_refresh_kernel, ((u64)S + 3) / 4, 0, S, 1, (const double*)avg.ptr(), (const u32*)active.ptr(), nn_val.ptr(), nn_col.ptr(), st.ptr());
    launches += 3;
    StepMeter meter;
    meter.begin();
    for (u32 m = 0; m + 1 < S; m++) {
        launch_wave_kernel(cluster_pick_kernel, 1, 0, S, (const double*)nn_val.ptr(), (const u32*)nn_col.ptr(), active.ptr(), size.ptr(), st.ptr(), d_merges.ptr());
        launch(S, ClusterFoldFunctor{S, sum.ptr(), avg.ptr(), active.ptr(), size.ptr(), st.ptr()});
        launch_wave_kernel(cluster_refresh_kernel, ((u64)S + 3) / 4, 0, S, 0, (const double*)avg.ptr(), (const u32*)active.ptr(), nn_val.ptr(), nn_col.ptr(), st.ptr());
        launches += 3;
    }
    meter.end();
    const double seconds = meter.seconds();
    ClusterStateDev h_st;
    std::vector<ClusterMergeDev> h_merges(S);
    copy_d2h(&h_st, st.ptr(), sizeof h_st);
    if (h_st.bad) throw DeviceError("cluster: the distance matrix holds a NaN, an infinite or a negative value");
    if (h_st.step != S - 1) throw DeviceError("cluster: the merge loop ended after " + std::to_string(h_st.step) + " of " + std::to_string(S - 1) + " merges");
    if (S > 1) copy_d2h(h_merges.data(), d_merges.ptr(), (size_t)(S - 1) * sizeof(ClusterMergeDev));
    merges->clear();
    for (u32 m = 0; m + 1 < S; m++) merges->push_back(ClusterRowMerge{h_merges[m].a, h_merges[m].b, h_merges[m].distance});
    if (stats) { stats->seconds = seconds; stats->rescans = h_st.rescans; stats->compares = h_st.compares; stats->launches = launches; }
}

void cluster_merges_device(const double* asym, uint32_t n, std::vector<ClusterRowMerge>* merges, ClusterDeviceStats* stats) {
    if (n == 0 || n > CLUSTER_MAX_SEQS) throw DeviceError("cluster: " + std::to_string(n) + " sequences (1 .. " + std::to_string(CLUSTER_MAX_SEQS) + ", ac_cluster_max_seqs)");
    Arena::device().reset();
    DBuf<double> d_asym((u64)n * n);
    copy_h2d(d_asym.ptr(), asym, (size_t)n * n * 8);
    cluster_merge_loop(d_asym.ptr(), n, merges, stats);
}

void cluster_merges_graph_device(const FinalGraph& g, uint32_t n_seqs, double* asym_out, std::vector<ClusterRowMerge>* merges, ClusterDeviceStats* stats) {
    if (n_seqs > CLUSTER_MAX_SEQS) throw DeviceError("cluster: " + std::to_string(n_seqs) + " sequences (1 .. " + std::to_string(CLUSTER_MAX_SEQS) + ", ac_cluster_max_seqs)");
    DBuf<u64> ab = pair_lengths_device(g, n_seqs);      // (starts the arena session)
    const u64 SS = (u64)n_seqs * n_seqs;
    DBuf<double> d_asym(SS);
    launch(SS, ClusterQuotientFunctor{ab.ptr(), n_seqs, d_asym.ptr()});
    if (asym_out) copy_d2h(asym_out, d_asym.ptr(), SS * 8);
    cluster_merge_loop(d_asym.ptr(), n_seqs, merges, stats);
    if (stats) stats->launches += 3;
}
