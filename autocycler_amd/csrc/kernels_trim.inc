// overlap_alignment (trim.rs:366-480), the quadratic step of `autocycler trim`, ON THE DEVICE — part of graph_extras.hip (included inside
// namespace ac; not a translation unit of its own).  The host side (trim_host.cpp) builds the jobs, applies the identity test and turns
// alignments into path slices; here a batch of jobs (paths A, B of n entries each, k = min(max_unitigs, n)) becomes alignment pieces.
//
// Arithmetic.  The reference fills a (k + 1) x (k + 1) f64 matrix with sums of unitig lengths and halves of such sums.  Every finite score
// is a multiple of 0.5 of magnitude < 2^34 (a path's weights add up to less than 2^32: checked), so the DOUBLED score in int64 is the same
// computation: match +2 w(a), mismatch -(w(a) + w(b)), gaps -2 w(a) / -2 w(b).  The cells the reference leaves at -inf (the skipped main
// diagonal of a path against itself) hold TRIM_NEG = -2^61: below every finite score, still below after at most 2 k subtractions, and
// `TRIM_NEG >= finite` is false as `-inf >= finite` is.  No cell is computed FROM a skipped one: a cell's diagonal neighbour lies on its own
// diagonal, and of its upper and left neighbours (which lie on two different diagonals) at most one is skipped and loses the max.
//
// Fill (trim_fill_kernel: one 256-thread workgroup per job, all jobs of a phase in one launch).  Columns are cut into STRIPS of 64 (one
// column per lane, b / w(b) of the column in registers) and strips into BANDS of four (one strip per wavefront).  The rows stream through a
// strip SKEWED: at step g lane l computes row g - l + 1, so that its left neighbour S[i][j-1] is what lane l - 1 computed one step earlier
// (one shuffle), its diagonal neighbour the value that shuffle delivered the step before, and its upper neighbour its own last value.  A
// strip's right-edge column goes to the wavefront of the next strip through an LDS ring; that wavefront runs two phases (2 x 64 steps)
// behind, so that a workgroup barrier per 64 steps is all the synchronisation there is.  The band's last column goes to global memory (8 k
// bytes, two such buffers per job used in turn) and comes back as the left edge of the next band; the last band's is the matrix's right
// edge S[1..k][k], which the traceback scans.  The a / w(a) of the rows and the incoming left edge are staged through LDS rings one or two
// phases ahead by threads that are not the ones reading them in that phase.
// No score is stored.  What the traceback reads is ONE BIT per cell, `S[i-1][j] >= S[i][j-1]` (both known when cell (i, j) is computed),
// kept as the ballots the wavefronts produce: word [strip * (k + 63) + g] holds, in bit l, the bit of cell (g - l + 1, 64 strip + l + 1).
// A wavefront collects the 64 ballots of a phase in registers (lane r keeps step r's) and writes them as one 512-byte vector store.
// (k + 63) * ceil(k / 64) * 8 bytes per job: 3.2 MB at k = 5000, 50 MB at 20 000, 537 MB at TRIM_MAX_K.
//
// Traceback (trim_trace_kernel: one wavefront per job): the 64 lanes find the smallest row that maximises S[i][k] (strict > in row
// order, as the reference's scan), lane 0 walks the bit matrix (trim.rs:433-456) and writes the pieces back to front into the job's 2 k
// piece slots together with the three sums the identity test needs.
static const u32 TRIM_MAX_K = 65536;
static const int TRIM_NW = 4;                       // wavefronts per workgroup = strips per band
static const u32 TRIM_ERING = 256, TRIM_ARING = 1024;      // LDS ring sizes in rows (see the spans in the kernel)
static const int64_t TRIM_NEG = -((int64_t)1 << 61);
struct TrimJobDev {
    u64 in_off;        // first entry of the job's a / b / wa / wb
    u64 bits_off;      // first word of its bit matrix
    u64 edge_off;      // first of its 2 k edge values
    u64 piece_off;     // first of its 2 k piece slots
    u32 n, k, skip, pad;
};
struct TrimHeader { u64 status, count, matches, len_a, len_b; };

AC_KERNEL void __launch_bounds__(256) trim_fill_kernel(const TrimJobDev* jobs, const int32_t* pa, const int32_t* pb, const u32* pwa, const u32* pwb,
                                                       u64* bits, int64_t* edge) {
    AC_SHARED int64_t ering[TRIM_NW + 1][TRIM_ERING];      // [0]: the band's incoming left edge; [w + 1]: the right edge of wavefront w's strip
    AC_SHARED int32_t a_ring[TRIM_ARING];
    AC_SHARED u32 wa_ring[TRIM_ARING];
    const TrimJobDev J = jobs[wv::bid()];
    const u32 tid = wv::tid(), w = tid >> 6;
    const int l = wv::lane();
    const u32 k = J.k, n = J.n;
    if (k == 0) return;
    const int32_t* a = pa + J.in_off; const int32_t* b = pb + J.in_off;
    const u32* wa = pwa + J.in_off; const u32* wb = pwb + J.in_off;
    const u32 nsteps = k + 63, nbands = (k + 255) / 256;
    for (u32 band = 0; band < nbands; band++) {
        const u32 col0 = band * 256, cols = k - col0 < 256 ? k - col0 : 256, nwb = (cols + 63) / 64;
        const int64_t* ein = edge + J.edge_off + ((band & 1) ? 0 : k);
        int64_t* eout = edge + J.edge_off + ((band & 1) ? k : 0);
        const u32 j0 = col0 + w * 64 + (u32)l;      // this lane's column, 0-based
        const bool col_valid = j0 < k, last_col = j0 + 1 == col0 + cols;
        const u32 gj = n - k + j0;
        int32_t bv = 0; int64_t wbv = 0;
        if (col_valid) { bv = b[gj]; wbv = wb[gj]; }
        wv::block_sync();      // (the previous band is done with the rings)
        if (tid < 128) { if (tid < k) { a_ring[tid] = a[tid]; wa_ring[tid] = wa[tid]; } }
        else if (tid < 192) { const u32 i = tid - 128 + 1; if (i <= k) ering[0][i & (TRIM_ERING - 1)] = band ? ein[i - 1] : 0; }
        wv::block_sync();
        int64_t cur = 0, prev_left = 0;      // S[0][j] = 0; the diagonal neighbour of row 1 is S[0][j-1] = 0
        const u32 nphases = (nsteps + 63) / 64 + 2 * (nwb - 1);
        for (u32 p = 0; p < nphases; p++) {
            // staging for later phases: rows 64 (p + 2) .. + 63 of a / w(a) (wavefront 0 reads rows up to 64 p + 63 in phase p; the oldest row
            // still read, by wavefront 3, is 64 p - 447: a span below TRIM_ARING); rows 64 (p + 1) + 1 .. + 64 of the incoming edge (lane 0 of
            // wavefront 0 reads rows 64 p + 1 .. 64 p + 64 now)
            if (tid < 64) { const u32 gi = 64 * (p + 2) + tid; if (gi < k) { a_ring[gi & (TRIM_ARING - 1)] = a[gi]; wa_ring[gi & (TRIM_ARING - 1)] = wa[gi]; } }
            else if (tid < 128) { const u32 i = 64 * (p + 1) + 1 + (tid - 64); if (i <= k) ering[0][i & (TRIM_ERING - 1)] = band ? ein[i - 1] : 0; }
            const u32 q = p - 2 * w;      // this wavefront's own phase (wraps for p < 2 w: not active)
            if (w < nwb && p >= 2 * w && q * 64 < nsteps) {
                u64 keep = 0;
                for (u32 r = 0; r < 64; r++) {
                    const u32 g = q * 64 + r;
                    if (g >= nsteps) break;
                    const int64_t i = (int64_t)g - l + 1;      // this lane's row, 1-based
                    const bool row_valid = i >= 1 && i <= (int64_t)k, act = col_valid && row_valid;
                    const int64_t up = cur;
                    int64_t left = (int64_t)wv::shfl64((unsigned long long)cur, (l + 63) & 63);
                    if (l == 0) left = row_valid ? ering[w][(u32)i & (TRIM_ERING - 1)] : 0;
                    bool bit = false;
                    if (act) {
                        const u32 gi = (u32)i - 1;
                        const int32_t av = a_ring[gi & (TRIM_ARING - 1)];
                        const int64_t wav = wa_ring[gi & (TRIM_ARING - 1)];
                        const int64_t m = prev_left + (av == bv ? 2 * wav : -(wav + wbv));
                        const int64_t d = up - 2 * wav, ins = left - 2 * wbv;
                        int64_t v = m > d ? m : d;
                        v = v > ins ? v : ins;
                        if (J.skip && gi == gj) v = TRIM_NEG;
                        bit = up >= left;
                        cur = v;
                        // (a strip's lane 63 writes rows 64 q - 62 .. 64 q + 1 while the next wavefront reads rows 64 q - 127 .. 64 q - 64)
                        if (l == 63) ering[w + 1][(u32)i & (TRIM_ERING - 1)] = v;
                        if (last_col) eout[i - 1] = v;
                    }
                    prev_left = left;
                    const u64 bal = wv::ballot(bit);
                    if ((u32)l == r) keep = bal;
                }
                const u32 g = q * 64 + (u32)l;
                if (g < nsteps) bits[J.bits_off + (u64)(band * TRIM_NW + w) * nsteps + g] = keep;
            }
            wv::block_sync();
        }
    }
}

AC_KERNEL void __launch_bounds__(64) trim_trace_kernel(const TrimJobDev* jobs, const int32_t* pa, const int32_t* pb, const u32* pwa, const u32* pwb,
                                                      const u64* bits, const int64_t* edge, int32_t* pieces, TrimHeader* hdr) {
    const u32 job = wv::bid();
    const TrimJobDev J = jobs[job];
    const int l = wv::lane();
    const u32 k = J.k, n = J.n;
    if (k == 0) { if (l == 0) hdr[job] = TrimHeader{1, 0, 0, 0, 0}; return; }
    const u32 nbands = (k + 255) / 256, nsteps = k + 63;
    const int64_t* rc = edge + J.edge_off + (((nbands - 1) & 1) ? k : 0);      // S[i][k] at rc[i - 1]
    int64_t best = INT64_MIN; int bi = 0;
    for (u32 i = (u32)l + 1; i <= k; i += 64) { const int64_t v = rc[i - 1]; if (v > best) { best = v; bi = (int)i; } }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int64_t ov = (int64_t)wv::shfl_xor64((unsigned long long)best, o);
        const int oi = wv::shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (l != 0) return;
    if (best <= 0) { hdr[job] = TrimHeader{1, 0, 0, 0, 0}; return; }      // (trim.rs:422: a skipped cell never wins either: TRIM_NEG < 0)
    const int32_t* a = pa + J.in_off; const int32_t* b = pb + J.in_off;
    const u32* wa = pwa + J.in_off; const u32* wb = pwb + J.in_off;
    int32_t* out = pieces + (J.piece_off + 2 * (u64)k) * 4;      // written back to front: piece t of the walk at slot 2 k - 1 - t
    u32 i = (u32)bi, j = k; u64 t = 0, matches = 0, len_a = 0, len_b = 0;
    while (i > 0 && j > 0) {
        const u32 gi = i - 1, gj = n - k + j - 1;
        const int32_t av = a[gi], bv = b[gj];
        out -= 4;
        if (av == bv) {
            out[0] = av; out[1] = (int32_t)gi; out[2] = bv; out[3] = (int32_t)gj;
            matches += wa[gi]; len_a += wa[gi]; len_b += wb[gj];
            i--; j--;
        } else {
            const u32 ln = (j - 1) & 63;
            const u64 word = bits[J.bits_off + (u64)((j - 1) >> 6) * nsteps + (i - 1 + ln)];
            if ((word >> ln) & 1) { out[0] = av; out[1] = (int32_t)gi; out[2] = 0; out[3] = -1; len_a += wa[gi]; i--; }
            else { out[0] = 0; out[1] = -1; out[2] = bv; out[3] = (int32_t)gj; len_b += wb[gj]; j--; }
        }
        t++;
    }
    hdr[job] = TrimHeader{i > 0 ? 2u : 0u, t, matches, len_a, len_b};
}

u32 trim_max_unitigs() { return TRIM_MAX_K; }

// A batch of alignment jobs through the two kernels; jobs that do not fit AC_TRIM_BATCH_BYTES of bit matrices together run in several
// launches (a job larger than that on its own still runs, alone).  weights[u - 1] = w(u); the paths were validated by the caller.
void overlap_alignment_batch(const std::vector<AlignJob>& jobs, const uint32_t* weights, uint32_t max_unitigs, std::vector<AlignOut>* outs,
                             TrimDeviceStats* st) {
    const size_t nj = jobs.size();
    outs->assign(nj, AlignOut());
    std::vector<u32> ks(nj);
    for (size_t q = 0; q < nj; q++) {
        if (jobs[q].a.size() != jobs[q].b.size()) throw DeviceError("overlap alignment: the two paths differ in length");
        const u64 n = jobs[q].a.size(), k = std::min<u64>(n, max_unitigs);
        if (n > 0xFFFFFFFFull || k > TRIM_MAX_K)
            throw DeviceError("overlap alignment: min(max_unitigs, path length) = " + std::to_string(k) + " is above the " + std::to_string(TRIM_MAX_K) +
                              " this library supports (ac_trim_max_unitigs): lower --max_unitigs");
        ks[q] = (u32)k;
    }
    const u64 budget = knobs().trim_batch_bytes;
    Arena& arena = Arena::device();
    arena.reset();
    StepMeter meter;
    for (size_t q0 = 0; q0 < nj;) {
        // the jobs of this launch
        size_t q1 = q0; u64 bit_words = 0, n_in = 0, n_edge = 0, n_piece = 0;
        std::vector<TrimJobDev> jd;
        while (q1 < nj) {
            const u64 k = ks[q1], words = (k + 63) * ((k + 63) / 64);
            if (q1 > q0 && (bit_words + words) * 8 > budget) break;
            jd.push_back(TrimJobDev{n_in, bit_words, n_edge, n_piece, (u32)jobs[q1].a.size(), (u32)k, jobs[q1].skip_diagonal ? 1u : 0u, 0u});
            bit_words += words; n_in += jobs[q1].a.size(); n_edge += 2 * k; n_piece += 2 * k;
            q1++;
        }
        const size_t nb = q1 - q0;
        std::vector<int32_t> ha(n_in), hb(n_in); std::vector<u32> hwa(n_in), hwb(n_in);
        for (size_t q = q0; q < q1; q++) {
            const u64 o = jd[q - q0].in_off;
            for (size_t i = 0; i < jobs[q].a.size(); i++) {
                const int32_t x = jobs[q].a[i], y = jobs[q].b[i];
                ha[o + i] = x; hb[o + i] = y;
                hwa[o + i] = weights[(u32)(x < 0 ? -(int64_t)x : (int64_t)x) - 1]; hwb[o + i] = weights[(u32)(y < 0 ? -(int64_t)y : (int64_t)y) - 1];
            }
        }
        const Arena::Mark mark = arena.mark();
        {
            DBuf<TrimJobDev> d_jobs(nb); DBuf<int32_t> d_a(n_in + 1), d_b(n_in + 1), d_pieces(n_piece * 4 + 4); DBuf<u32> d_wa(n_in + 1), d_wb(n_in + 1);
            DBuf<u64> d_bits(bit_words + 1); DBuf<int64_t> d_edge(n_edge + 1); DBuf<TrimHeader> d_hdr(nb);
            copy_h2d(d_jobs.ptr(), jd.data(), nb * sizeof(TrimJobDev));
            copy_h2d(d_a.ptr(), ha.data(), n_in * 4); copy_h2d(d_b.ptr(), hb.data(), n_in * 4);
            copy_h2d(d_wa.ptr(), hwa.data(), n_in * 4); copy_h2d(d_wb.ptr(), hwb.data(), n_in * 4);
            meter.begin();
            launch_wave_kernel(trim_fill_kernel, nb, 0, (const TrimJobDev*)d_jobs.ptr(), (const int32_t*)d_a.ptr(), (const int32_t*)d_b.ptr(),
                               (const u32*)d_wa.ptr(), (const u32*)d_wb.ptr(), d_bits.ptr(), d_edge.ptr());
            launch_wave_kernel_sized(trim_trace_kernel, nb, 64u, 0, (const TrimJobDev*)d_jobs.ptr(), (const int32_t*)d_a.ptr(), (const int32_t*)d_b.ptr(),
                                     (const u32*)d_wa.ptr(), (const u32*)d_wb.ptr(), (const u64*)d_bits.ptr(), (const int64_t*)d_edge.ptr(), d_pieces.ptr(),
                                     d_hdr.ptr());
            meter.end();
            const double seconds = meter.take();      // (waits for the two kernels: the read-backs below find them done)
            if (st) st->seconds_device += seconds;
            const std::vector<TrimHeader> hdr = to_host(d_hdr, nb);
            for (size_t q = q0; q < q1; q++) {
                const TrimHeader& h = hdr[q - q0];
                const TrimJobDev& j = jd[q - q0];
                AlignOut& o = (*outs)[q];
                o.status = (u32)h.status; o.matches = h.matches; o.len_a = h.len_a; o.len_b = h.len_b;
                if (st) { st->cells += (u64)j.k * j.k; st->jobs++; }
                if (h.status != 0 || h.count == 0) continue;
                if (h.count > 2 * (u64)j.k) throw DeviceError("overlap alignment: internal error (a traceback longer than 2 k)");
                o.pieces.resize(h.count);      // (AlignPiece is four 32-bit words, as the kernel writes them)
                copy_d2h(o.pieces.data(), d_pieces.ptr() + (j.piece_off + 2 * (u64)j.k - h.count) * 4, h.count * 16);
            }
            if (st) st->launches++;
        }
        arena.rewind(mark);
        q0 = q1;
    }
}
