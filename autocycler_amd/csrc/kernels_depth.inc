// Read-based unitig depths (depth.rs:45-76 of `autocycler combine --reads`) ON THE DEVICE — included by graph_depth.hip inside namespace ac.
//
// Text.  Reads (and, for the table build, the unitigs) lie one behind the other with ONE separator position after each; the host packs
// them to 2-bit codes, 32 positions per u64 word (position j of a word in bits 2 j, 2 j + 1), plus a mask plane of one u32 per word whose
// bit j is set for a separator, padding behind the last read, or any byte outside ACGTacgt.  A set mask bit resets a lane's run of valid
// bases, which is all a read boundary or an N needs.  wread[w] = the read that holds position 32 w (the separator counts to the read
// before it), toff[r] = first position of read r, toff[n_reads] = end of the text.
//
// Table.  keys[] (u64, DEPTH_EMPTY = all ones: no key of at most 62 bits takes it, while poly-A / poly-T is the key 0), occ[] (occurrences
// in the assembly: > 1 = a repeat, depth.rs:422-431) and cnt[] (the read tally; starts at 0, which is the reference's reset).  Slots are
// claimed by atomicCAS, linear probing, capacity a power of two of at least twice the inserts.
//
// depth_roll_kernel: one packed word = 32 k-mer END positions per lane, a wavefront covers 2048 positions, a workgroup 8192.  A lane warms
// its forward / reverse-complement k-mer up on the last k - 1 positions of the word before (k - 1 <= 30: one word always suffices) and
// rolls across its own.  MODE 0 inserts every valid k-mer (table build).  MODE 1 is the reads' pass 1: every valid k-mer is looked up, the
// slot it hit (or DEPTH_NOSLOT) is kept per position for pass 2, and k-mers / hits / first / last hit position are summed PER READ: inside
// the lane as segments (a new segment starts when a k-mer belongs to a later read), then across the wavefront — the segments that are still
// open at the lanes' ends are combined by a segmented scan keyed by the read, a read that closes in a lane takes the chain of its
// predecessors — so that one (wavefront, read) pair issues ONE set of atomics whether a wavefront holds fifty 40 bp reads or a 100 kbp read
// spans many workgroups.
// depth_accept: one thread per read, the reference's f64 test (depth.rs:412) and the six ReadTotals as u64.
// depth_commit_kernel (pass 2): positions interleaved across the lanes (coalesced reads of the kept slots); a hit of an accepted read adds
// 1 to its slot.  Equal slots on ADJACENT positions (homopolymer runs: thousands of hits on one slot) are added as one atomic per run.
static const u64 DEPTH_EMPTY = ~0ULL;
static const u32 DEPTH_NOSLOT = 0xFFFFFFFFu;
static const u32 DEPTH_NOREAD = 0xFFFFFFFFu;
static const u32 DEPTH_STRETCH = 32;                      // positions per lane
static const u32 DEPTH_WAVE_TILE = 64 * DEPTH_STRETCH;    // positions per wavefront
struct DepthTable { u64* keys; u32* occ; u32* cnt; u64 mask; };
struct DepthRec { u32 kmers, hits, first, last; };

AC_D u64 depth_hash(u64 x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
AC_D u32 depth_find(const u64* keys, u64 mask, u64 key) {
    u64 s = depth_hash(key) & mask;
    for (u64 n = 0; n <= mask; n++) {
        const u64 have = keys[s];
        if (have == key) return (u32)s;
        if (have == DEPTH_EMPTY) return DEPTH_NOSLOT;
        s = (s + 1) & mask;
    }
    return DEPTH_NOSLOT;
}
// (a key never changes once its slot is claimed: a plain load that sees another key is final, one that sees an empty slot is settled by the CAS)
AC_D void depth_insert(const DepthTable& t, u64 key, u32* err) {
    u64 s = depth_hash(key) & t.mask;
    for (u64 n = 0; n <= t.mask; n++) {
        u64 have = t.keys[s];
        if (have == DEPTH_EMPTY) { have = atomic_cas64(t.keys + s, DEPTH_EMPTY, key); if (have == DEPTH_EMPTY) have = key; }
        if (have == key) { atomic_add32(t.occ + s, 1u); return; }
        s = (s + 1) & t.mask;
    }
    atomic_or32(err, 1u);      // a full table: the capacity rule was broken
}
AC_D void depth_flush(u32 r, const DepthRec& c, u32* rk, u32* rh, u32* rf, u32* rl) {
    if (!c.kmers) return;
    atomic_add32(rk + r, c.kmers);
    if (c.hits) { atomic_add32(rh + r, c.hits); atomic_min32(rf + r, c.first); atomic_max32(rl + r, c.last); }
}

template <int MODE>
AC_KERNEL void __launch_bounds__(256) depth_roll_kernel(const u64* bits, const u32* mask, u64 n_words, u32 k, DepthTable t, const u64* toff,
                                                       const u32* wread, u32* hitslot, u32* rk, u32* rh, u32* rf, u32* rl, u32* err) {
    const u64 w = (u64)wv::bid() * 256 + wv::tid();
    const bool live = w < n_words;
    const u64 kmask = (1ULL << (2 * k)) - 1;
    const u32 shift = 2 * (k - 1);
    u64 fwd = 0, rev = 0; u32 run = 0;
    u32 r = DEPTH_NOREAD, hk = DEPTH_NOREAD; u64 r0 = 0, nb = 0;
    DepthRec head{0, 0, 0xFFFFFFFFu, 0}, cur{0, 0, 0xFFFFFFFFu, 0};
    bool head_closed = false;
    if (live) {
        if (w > 0) {
            const u64 pb = bits[w - 1]; const u32 pm = mask[w - 1];
            for (u32 j = 33 - k; j < 32; j++) {
                if ((pm >> j) & 1) { run = 0; continue; }
                const u64 c = (pb >> (2 * j)) & 3;
                fwd = ((fwd << 2) | c) & kmask; rev = (rev >> 2) | ((3 - c) << shift); run++;
            }
        }
        if (MODE == 1) { r = wread[w]; hk = r; r0 = toff[r]; nb = toff[r + 1]; }
        const u64 b = bits[w]; const u32 m = mask[w];
        for (u32 j = 0; j < 32; j++) {
            u32 slot = DEPTH_NOSLOT;
            if ((m >> j) & 1) run = 0;
            else {
                const u64 c = (b >> (2 * j)) & 3;
                fwd = ((fwd << 2) | c) & kmask; rev = (rev >> 2) | ((3 - c) << shift); run++;
                if (run >= k) {
                    const u64 key = fwd < rev ? fwd : rev;
                    if (MODE == 0) depth_insert(t, key, err);
                    else {
                        const u64 e = w * 32 + j;
                        while (e >= nb) {      // the k-mer belongs to a later read: the segment of the read before it is complete
                            if (!head_closed) { head = cur; head_closed = true; } else depth_flush(r, cur, rk, rh, rf, rl);
                            cur = DepthRec{0, 0, 0xFFFFFFFFu, 0};
                            r++; r0 = nb; nb = toff[r + 1];
                        }
                        cur.kmers++;
                        slot = depth_find(t.keys, t.mask, key);
                        if (slot != DEPTH_NOSLOT) {
                            const u32 i = (u32)(e - (k - 1) - r0);
                            if (!cur.hits) cur.first = i;
                            cur.last = i; cur.hits++;
                        }
                    }
                }
            }
            if (MODE == 1) hitslot[w * 32 + j] = slot;
        }
    }
    if (MODE == 0) return;
    // across the wavefront: the lanes' open segments (key ok; reads ascend with the lanes, so equal keys are neighbours)
    const int lane = wv::lane();
    const u32 ok = r;
    DepthRec sc = cur;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 pk = (u32)wv::shfl_up((int)ok, o);
        const u32 a = (u32)wv::shfl_up((int)sc.kmers, o), h = (u32)wv::shfl_up((int)sc.hits, o);
        const u32 f = (u32)wv::shfl_up((int)sc.first, o), l = (u32)wv::shfl_up((int)sc.last, o);
        if (lane >= o && pk == ok) { sc.kmers += a; sc.hits += h; sc.first = f < sc.first ? f : sc.first; sc.last = l > sc.last ? l : sc.last; }
    }
    const u32 prev_ok = (u32)wv::shfl_up((int)ok, 1);
    const u32 pa = (u32)wv::shfl_up((int)sc.kmers, 1), ph = (u32)wv::shfl_up((int)sc.hits, 1);
    const u32 pf = (u32)wv::shfl_up((int)sc.first, 1), pl = (u32)wv::shfl_up((int)sc.last, 1);
    const u32 next_hk = (u32)wv::shfl_down((int)hk, 1);
    if (!live) return;
    if (head_closed) {      // the read this lane began in ended here: its segment plus the chain the lanes before it carried
        if (lane > 0 && prev_ok == hk) { head.kmers += pa; head.hits += ph; head.first = pf < head.first ? pf : head.first; head.last = pl > head.last ? pl : head.last; }
        depth_flush(hk, head, rk, rh, rf, rl);
    }
    if (lane == 63 || next_hk != ok) depth_flush(ok, sc, rk, rh, rf, rl);      // nobody after this lane carries the chain on
}

AC_D u64 depth_wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += wv::shfl_xor64(v, o);
    return v;
}

// one thread per read: count_one_read's verdict (depth.rs:411-418); totals[0..5] = reads, rejected_reads, read_bases, span_bases, span_kmers, hits
struct DepthAcceptFunctor {
    const u32 *rk, *rh, *rf, *rl; const u64* toff; u8* acc; u64* totals; u32 k;
    AC_D void operator()(u64 i, bool valid) const {
        u64 v[6] = {0, 0, 0, 0, 0, 0};
        if (valid) {
            const u32 kmers = rk[i], hits = rh[i];
            u8 a = 0;
            if (kmers) {
                if ((double)hits < 0.005 * (double)kmers) v[1] = 1;
                else {
                    a = 1;
                    const u64 span = (u64)rl[i] - (u64)rf[i] + 1;
                    v[0] = 1; v[2] = toff[i + 1] - toff[i] - 1; v[3] = span + k - 1; v[4] = span; v[5] = hits;
                }
            }
            acc[i] = a;
        }
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const u64 s = depth_wave_sum64(v[q]);
            if (wv::lane() == 0 && s) atomic_add64(totals + q, s);
        }
    }
};

AC_KERNEL void __launch_bounds__(256) depth_commit_kernel(const u32* hitslot, u64 n_slots, const u64* toff, const u32* wread, const u8* acc, u32* cnt) {
    const int lane = wv::lane();
    const u64 base = (((u64)wv::bid() * 256 + wv::tid()) >> 6) * DEPTH_WAVE_TILE;
    if (base >= n_slots) return;      // (the whole wavefront)
    u32 r = DEPTH_NOREAD; u64 nb = 0;
    for (u32 j = 0; j < DEPTH_STRETCH; j++) {
        const u64 pos = base + (u64)j * 64 + (u64)lane;
        u32 slot = pos < n_slots ? hitslot[pos] : DEPTH_NOSLOT;
        if (slot != DEPTH_NOSLOT) {
            if (r == DEPTH_NOREAD) { r = wread[pos >> 5]; nb = toff[r + 1]; }
            while (pos >= nb) { r++; nb = toff[r + 1]; }
            if (!acc[r]) slot = DEPTH_NOSLOT;
        }
        const u32 prev = (u32)wv::shfl_up((int)slot, 1);
        const bool first_of_run = lane == 0 || prev != slot;
        const u64 starts = wv::ballot(first_of_run);
        if (first_of_run && slot != DEPTH_NOSLOT) {
            const u64 rest = lane == 63 ? 0 : (starts >> (lane + 1));
            const u32 n = rest ? (u32)__builtin_ctzll(rest) + 1 : (u32)(64 - lane);
            atomic_add32(cnt + slot, n);
        }
    }
}

struct DepthInsertKeysFunctor {      // the junction k-mers: canonical values, one occurrence each
    DepthTable t; const u64* keys; u32* err;
    AC_D void operator()(u64 i) const { depth_insert(t, keys[i], err); }
};
struct DepthLookupFunctor {          // ac_depth_kmer_counts and the context k-mers of ac_depth_finish
    DepthTable t; const u64* keys; u32 k; u8* present; u32* occ; u32* cnt;
    AC_D void operator()(u64 i) const {
        const u64 key = keys[i];
        const u32 s = (key >> (2 * k)) ? DEPTH_NOSLOT : depth_find(t.keys, t.mask, key);
        present[i] = s != DEPTH_NOSLOT;
        occ[i] = s != DEPTH_NOSLOT ? t.occ[s] : 0;
        cnt[i] = s != DEPTH_NOSLOT ? t.cnt[s] : 0;
    }
};
struct DepthGatherFunctor {          // per assembly position: the read count of its k-mer and 0 = unique, 1 = repeat, 2 = no k-mer ends here
    DepthTable t; const u32* slot; u64 first; u32* cnt; u8* flag;
    AC_D void operator()(u64 i) const {
        const u32 s = slot[first + i];
        cnt[i] = s != DEPTH_NOSLOT ? t.cnt[s] : 0;
        flag[i] = s != DEPTH_NOSLOT ? (t.occ[s] > 1 ? 1 : 0) : 2;
    }
};
struct DepthCensusFunctor {          // out[0] = distinct k-mers, out[1] = repeats
    DepthTable t; u64* out;
    AC_D void operator()(u64 i, bool valid) const {
        const bool used = valid && t.keys[i] != DEPTH_EMPTY;
        const u64 d = depth_wave_sum64(used ? 1 : 0), rp = depth_wave_sum64(used && t.occ[i] > 1 ? 1 : 0);
        if (wv::lane() == 0) { if (d) atomic_add64(out, d); if (rp) atomic_add64(out + 1, rp); }
    }
};
