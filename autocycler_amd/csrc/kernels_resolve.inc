// global_alignment_distance (resolve.rs:387-418), the quadratic step of `autocycler resolve`, ON THE DEVICE — part of graph_extras.hip
// (included inside namespace ac; not a translation unit of its own).  The host side (resolve_host.cpp) finds the anchors, cuts and
// groups the bridge paths and picks the best path from the distances; here a batch of jobs (two paths of signed unitig numbers each)
// becomes one u32 per job: the last cell of the reference's matrix.
//
// Arithmetic.  u32 as in the reference: D[0][j] / D[i][0] are prefix sums of w(b) / w(a), D[i][j] = min(D[i-1][j-1] + (a_i == b_j ? 0 :
// max(w_i, w_j)), D[i-1][j] + w_i, D[i][j-1] + w_j).  Every cell is at most the sum of the two paths' weights, which the host has
// checked to be below 2^32 for every job it hands over: no addition can wrap.
//
// Schedule (resolve_distance_kernel: one WAVEFRONT per job, four jobs per 256-thread workgroup, no synchronisation between them).  The
// columns are cut into strips of 64, one column per lane (b_j / w(b_j) in registers); a job's strips run one after the other in its
// wavefront.  The rows stream through a strip SKEWED, as in trim's fill kernel: at step g lane l computes row g - l + 1, so its left
// neighbour D[i][j-1] is what lane l - 1 computed one step earlier (one shuffle), its diagonal neighbour the value that shuffle
// delivered the step before, its upper neighbour its own last value.  a_i / w(a_i) travel with the row: they enter at lane 0 and move
// one lane to the right per step (two more shuffles); lane 0 is fed from registers the 64 lanes load together every 64 steps
// (coalesced), read by a shuffle from lane g mod 64.
// A strip's right-edge column is the next strip's left edge: n + 1 u32 in a scratch row of the job's own in device memory.  Lane 63
// stores row i at step i + 62; the row-i value of the PREVIOUS strip was loaded at step 64 floor((i - 1) / 64) <= i - 1 of the same
// strip, so one row serves both directions.  Loads and stores are plain vector accesses of one wavefront, issued in program order.
// No matrix is stored and there is no traceback: only D[n][m] leaves.
static const u32 RESOLVE_MAX_PATH = 65536;
struct ResolveJobDev {
    u64 a_off, b_off;      // first entry of the job's row path / column path in the pool
    u64 edge_off;          // first of its n + 1 scratch values
    u32 n, m;              // rows, columns
};

AC_D u32 resolve_shfl(u32 v, int src) { return (u32)wv::shfl((int)v, src); }

AC_KERNEL void __launch_bounds__(256) resolve_distance_kernel(const ResolveJobDev* jobs, u32 n_jobs, const int32_t* entries, const u32* entry_w,
                                                              u32* edge, u32* dist) {
    const u32 job = wv::bid() * 4 + (wv::tid() >> 6);
    if (job >= n_jobs) return;      // (the whole wavefront)
    const ResolveJobDev J = jobs[job];
    const int l = wv::lane();
    const u32 n = J.n, m = J.m;
    const int32_t* a = entries + J.a_off; const int32_t* b = entries + J.b_off;
    const u32* wa = entry_w + J.a_off; const u32* wb = entry_w + J.b_off;
    if (m == 0) {      // all gaps: D[n][0]
        u32 sum = 0;
        for (u32 i = (u32)l; i < n; i += 64) sum += wa[i];
#pragma unroll
        for (int o = 32; o; o >>= 1) sum += (u32)wv::shfl_xor((int)sum, o);
        if (l == 0) dist[job] = sum;
        return;
    }
    u32* e = edge + J.edge_off;
    const u32 nstrips = (m + 63) / 64;
    const int from = (l + 63) & 63;      // the left neighbour (lane 0 replaces what it receives)
    u32 top_base = 0, result = 0;        // D[0][64 strip]
    for (u32 strip = 0; strip < nstrips; strip++) {
        const u32 j0 = strip * 64 + (u32)l;      // this lane's column, 0-based
        const bool col_valid = j0 < m, last_strip = strip + 1 == nstrips;
        const u32 cols = m - strip * 64 < 64 ? m - strip * 64 : 64;
        int32_t bv = 0; u32 wbv = 0;
        if (col_valid) { bv = b[j0]; wbv = wb[j0]; }
        u32 incl = wbv;      // the top edge: prefix sums of w(b)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const u32 t = (u32)wv::shfl_up((int)incl, o); if (l >= o) incl += t; }
        u32 cur = top_base + incl;      // D[0][j]
        u32 prev_left = top_base;       // lane 0: D[0][64 strip]; the other lanes receive theirs before their first row
        top_base += resolve_shfl(incl, 63);
        const u32 nsteps = n ? n + cols - 1 : 0;
        int32_t av = 0, chunk_a = 0; u32 wav = 0, chunk_w = 0, chunk_e = 0;
        for (u32 g = 0; g < nsteps; g++) {
            if ((g & 63) == 0) {      // rows g + 1 .. g + 64 for lane 0's next 64 steps
                const u32 r = g + (u32)l;
                if (r < n) { chunk_a = a[r]; chunk_w = wa[r]; if (strip) chunk_e = e[r + 1]; }
            }
            u32 left = resolve_shfl(cur, from);
            int32_t av_in = wv::shfl(av, from);
            u32 wav_in = resolve_shfl(wav, from);
            const int q = (int)(g & 63);
            const int32_t a0 = wv::shfl(chunk_a, q);
            const u32 w0 = resolve_shfl(chunk_w, q), e0 = resolve_shfl(chunk_e, q);
            if (l == 0) { av_in = a0; wav_in = w0; left = strip ? e0 : prev_left + w0; }      // (strip 0: D[i][0] = D[i-1][0] + w_i)
            av = av_in; wav = wav_in;
            const u32 i = g + 1 - (u32)l;      // this lane's row, 1-based (wraps for g < l: not valid)
            if (col_valid && g >= (u32)l && i <= n) {
                const u32 sub = prev_left + (av == bv ? 0u : (wav > wbv ? wav : wbv));
                const u32 del = cur + wav, ins = left + wbv;
                u32 v = sub < del ? sub : del;
                v = v < ins ? v : ins;
                cur = v;
                if (l == 63 && !last_strip) e[i] = v;
            }
            prev_left = left;
        }
        if (last_strip) result = resolve_shfl(cur, (int)((m - 1) & 63));
    }
    if (l == 0) dist[job] = result;
}

u32 resolve_max_path() { return RESOLVE_MAX_PATH; }

// A batch of distance jobs through the kernel: dist[i] for pairs[i] of the pool's paths.  weights[u - 1] = w(u); the paths were validated
// and no pair overflows (resolve_host.hpp pair_overflows): the caller's checks.  The longer path goes on the rows or the columns,
// whichever takes fewer steps (the distance is symmetric); the jobs run in descending order of rows x strips; jobs whose scratch rows do
// not fit AC_RESOLVE_BATCH_BYTES together run in several launches (a job larger than that on its own still runs, alone).
void path_distance_batch(const PathPool& pool, const std::vector<PathPair>& pairs, const uint32_t* weights, std::vector<uint32_t>* dist,
                         ResolveDeviceStats* st) {
    const size_t nj = pairs.size();
    dist->assign(nj, 0);
    if (nj == 0) return;
    std::vector<ResolveJobDev> all(nj);
    std::vector<u64> cost(nj);
    for (size_t q = 0; q < nj; q++) {
        if (pairs[q].a >= pool.size() || pairs[q].b >= pool.size()) throw DeviceError("path distances: a pair names a path that does not exist");
        u32 pa = pairs[q].a, pb = pairs[q].b;
        const u64 la = pool.len(pa), lb = pool.len(pb);
        if (la > RESOLVE_MAX_PATH || lb > RESOLVE_MAX_PATH)
            throw DeviceError("path distances: a path of " + std::to_string(std::max(la, lb)) + " entries is above the " + std::to_string(RESOLVE_MAX_PATH) +
                              " this library supports (ac_resolve_max_path)");
        auto steps = [](u64 rows, u64 cols) -> u64 { return cols == 0 ? 0 : (rows == 0 ? 1 : ((cols + 63) / 64) * (rows + 63)); };
        if (steps(lb, la) < steps(la, lb)) std::swap(pa, pb);
        const u64 n = pool.len(pa), m = pool.len(pb);
        all[q] = ResolveJobDev{pool.off[pa], pool.off[pb], 0, (u32)n, (u32)m};
        cost[q] = n * ((m + 63) / 64);
        if (st) { st->cells += n * m; st->jobs++; st->largest_job_cells = std::max(st->largest_job_cells, n * m); }
    }
    std::vector<size_t> order(nj);
    for (size_t q = 0; q < nj; q++) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cost[x] > cost[y]; });
    const u64 budget = knobs().resolve_batch_bytes;
    const size_t MAX_JOBS_PER_LAUNCH = (size_t)1 << 22;
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    // the pool and the weight of every entry, once for all launches
    const u64 n_ent = pool.entries.size();
    std::vector<u32> hw(n_ent);
    for (u64 i = 0; i < n_ent; i++) { const int64_t x = pool.entries[i]; hw[i] = weights[(u32)(x < 0 ? -x : x) - 1]; }
    DBuf<int32_t> d_ent(n_ent + 1); DBuf<u32> d_w(n_ent + 1);
    copy_h2d(d_ent.ptr(), pool.entries.data(), n_ent * 4); copy_h2d(d_w.ptr(), hw.data(), n_ent * 4);
    for (size_t q0 = 0; q0 < nj;) {
        size_t q1 = q0; u64 n_edge = 0;
        std::vector<ResolveJobDev> jd;
        while (q1 < nj && q1 - q0 < MAX_JOBS_PER_LAUNCH) {
            ResolveJobDev j = all[order[q1]];
            const u64 row = (u64)j.n + 1;
            if (q1 > q0 && (n_edge + row) * 4 > budget) break;
            j.edge_off = n_edge; n_edge += row;
            jd.push_back(j);
            q1++;
        }
        const size_t nb = q1 - q0;
        const Arena::Mark mark = arena.mark();
        {
            DBuf<ResolveJobDev> d_jobs(nb); DBuf<u32> d_edge(n_edge + 1), d_dist(nb);
            copy_h2d(d_jobs.ptr(), jd.data(), nb * sizeof(ResolveJobDev));
            meter.begin();
            launch_wave_kernel(resolve_distance_kernel, (nb + 3) / 4, 0, (const ResolveJobDev*)d_jobs.ptr(), (u32)nb, (const int32_t*)d_ent.ptr(),
                               (const u32*)d_w.ptr(), d_edge.ptr(), d_dist.ptr());
            meter.end();
            const double seconds = meter.take();      // (waits for the kernel: the read-back below finds it done)
            if (st) st->seconds_device += seconds;
            const std::vector<u32> hd = to_host(d_dist, nb);
            for (size_t q = q0; q < q1; q++) (*dist)[order[q]] = hd[q - q0];
            if (st) st->launches++;
        }
        arena.rewind(mark);
        q0 = q1;
    }
}
