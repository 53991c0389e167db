// Read-based unitig depths (ac_depth_*): the device side of set_read_depths (depth.rs:45-76).  A translation unit of its own: the k-mer
// table lives as long as the caller's handle, across any number of graph builds, so nothing here comes from the build arena (which every
// build resets) — the engine owns plain device allocations and frees them with the handle.  Timing is a StepMeter of the engine's own
// (device_rt.hpp: its events are not from the 64-entry event ring, whose entries a long-lived user would see recycled under it).
#include "graph_depth.hpp"

#include <thread>

#include "device_rt.hpp"

namespace ac {

#include "kernels_depth.inc"

namespace {

template <class T> struct OwnedDev {      // device memory that belongs to the engine
    T* p = nullptr; size_t cap = 0;
    OwnedDev() {}
    OwnedDev(const OwnedDev&) = delete;
    OwnedDev& operator=(const OwnedDev&) = delete;
    ~OwnedDev() { release(); }
    void release() {
        if (!p) return;
#ifdef AC_EMU
        free(p);
#else
        (void)hipFree(p);
#endif
        p = nullptr; cap = 0;
    }
    T* ensure(size_t n) {
        if (n == 0) n = 1;
        if (n <= cap) return p;
        release();
#ifdef AC_EMU
        p = (T*)malloc(n * sizeof(T));
        if (!p) throw DeviceError("out of memory");
#else
        flush_fills();
        AC_HIP_CHECK(hipMalloc((void**)&p, n * sizeof(T)));
#endif
        cap = n;
        return p;
    }
    void fill(int byte, size_t n) {
        if (!n) return;
#ifdef AC_EMU
        memset(p, byte, n * sizeof(T));
#else
        flush_fills();
        AC_HIP_CHECK(hipMemsetAsync(p, byte, n * sizeof(T), 0));
#endif
    }
};
template <class T> struct OwnedPinned {      // the staging side of an upload
    T* p = nullptr; size_t cap = 0;
    OwnedPinned() {}
    OwnedPinned(const OwnedPinned&) = delete;
    OwnedPinned& operator=(const OwnedPinned&) = delete;
    ~OwnedPinned() { release(); }
    void release() {
        if (!p) return;
#ifdef AC_EMU
        free(p);
#else
        (void)hipHostFree(p);
#endif
        p = nullptr; cap = 0;
    }
    T* ensure(size_t n) {
        if (n == 0) n = 1;
        if (n <= cap) return p;
        release();
#ifdef AC_EMU
        p = (T*)malloc(n * sizeof(T));
        if (!p) throw DeviceError("out of memory");
#else
        AC_HIP_CHECK(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
#endif
        cap = n;
        return p;
    }
};

struct DepthCodes {      // byte -> 2-bit code, 4 = masked (anything outside ACGTacgt: depth.rs:434-442)
    u8 c[256];
    DepthCodes() {
        memset(c, 4, sizeof c);
        c[(u8)'A'] = c[(u8)'a'] = 0; c[(u8)'C'] = c[(u8)'c'] = 1; c[(u8)'G'] = c[(u8)'g'] = 2; c[(u8)'T'] = c[(u8)'t'] = 3;
    }
};
const DepthCodes& depth_codes() { static const DepthCodes t; return t; }

// Words [w0, w1) of the packed text of `nr` sequences: sequence r = src(r) of toff[r + 1] - toff[r] - 1 bytes at positions toff[r] ..
template <class Src> void depth_pack_range(const Src& src, const u64* toff, u64 nr, u64 w0, u64 w1, u64* bits, u32* mask, u32* wread) {
    const u8* code = depth_codes().c;
    u64 r = (u64)(std::upper_bound(toff, toff + nr + 1, w0 * 32) - toff);
    r = r ? r - 1 : 0;
    if (r >= nr) r = nr - 1;
    const u8* s = src(r);
    for (u64 w = w0; w < w1; w++) {
        u64 pos = w * 32;
        while (r + 1 < nr && pos >= toff[r + 1]) { r++; s = src(r); }
        wread[w] = (u32)r;
        u64 b = 0; u32 m = 0;
        if (pos + 32 < toff[r + 1]) {      // the whole word inside one sequence
            const u8* q = s + (pos - toff[r]);
            for (u32 j = 0; j < 32; j++) { const u32 c = code[q[j]]; b |= (u64)(c & 3) << (2 * j); m |= (c >> 2) << j; }
        } else {
            u64 rr = r; const u8* ss = s;
            for (u32 j = 0; j < 32; j++, pos++) {
                while (rr + 1 < nr && pos >= toff[rr + 1]) { rr++; ss = src(rr); }
                if (pos + 1 >= toff[rr + 1]) { m |= 1u << j; continue; }      // the separator, or padding behind the last sequence
                const u32 c = code[ss[pos - toff[rr]]];
                b |= (u64)(c & 3) << (2 * j); m |= (c >> 2) << j;
            }
        }
        bits[w] = b; mask[w] = m;
    }
}
template <class Src> void depth_pack(const Src& src, const u64* toff, u64 nr, u64 n_words, u64* bits, u32* mask, u32* wread) {
    const unsigned hw = std::thread::hardware_concurrency();
    const u64 T = std::max<u64>(1, std::min<u64>({(u64)16, (u64)(hw ? hw : 1), n_words >> 14}));
    if (T == 1) { depth_pack_range(src, toff, nr, 0, n_words, bits, mask, wread); return; }
    std::vector<std::thread> pool;
    for (u64 t = 1; t < T; t++)
        pool.emplace_back([&, t] { depth_pack_range(src, toff, nr, n_words * t / T, n_words * (t + 1) / T, bits, mask, wread); });
    depth_pack_range(src, toff, nr, 0, n_words / T, bits, mask, wread);
    for (auto& th : pool) th.join();
}

}  // namespace

struct DepthEngine::Impl {
    u32 k = 0;
    DepthTable t{nullptr, nullptr, nullptr, 0};
    OwnedDev<u64> keys; OwnedDev<u32> occ, cnt, err; OwnedDev<u64> d_totals;
    // one text at a time (the assembly first, then each batch of reads): packed planes, read tables, per-read sums
    OwnedDev<u64> d_bits, d_toff; OwnedDev<u32> d_mask, d_wread, d_hitslot, d_rk, d_rh, d_rf, d_rl; OwnedDev<u8> d_acc;
    OwnedPinned<u64> h_bits; OwnedPinned<u32> h_mask, h_wread;
    OwnedDev<u32> asm_slot;                     // the slot of the k-mer that ends at each assembly position
    std::vector<u64> asm_toff;                  // all unitigs of all graphs, one behind the other
    std::vector<u32> graph_first;               // graph g's unitigs are [graph_first[g], graph_first[g + 1])
    std::vector<DepthGraphPlan> plans;
    OwnedDev<u64> d_q; OwnedDev<u8> d_present; OwnedDev<u32> d_qocc, d_qcnt;      // lookups
    DepthTotals tot;
    StepMeter meter;      // one interval per batch of reads

    struct Text { u64 n_words, n_seqs; };
    template <class Src> Text upload_text(const Src& src, const std::vector<u64>& toff) {
        const u64 nr = toff.size() - 1, n_pos = toff[nr], n_words = (n_pos + 31) / 32;
        depth_pack(src, toff.data(), nr, n_words, h_bits.ensure(n_words), h_mask.ensure(n_words), h_wread.ensure(n_words));
        copy_h2d(d_bits.ensure(n_words), h_bits.p, n_words * 8);
        copy_h2d(d_mask.ensure(n_words), h_mask.p, n_words * 4);
        copy_h2d(d_wread.ensure(n_words), h_wread.p, n_words * 4);
        copy_h2d(d_toff.ensure(nr + 1), toff.data(), (nr + 1) * 8);
        stream_sync();      // (toff is the caller's pageable vector; the staging planes are packed anew for the next text)
        return Text{n_words, nr};
    }
    void reset_read_sums(u64 nr) {
        d_rk.ensure(nr); d_rh.ensure(nr); d_rf.ensure(nr); d_rl.ensure(nr); d_acc.ensure(nr);
        d_rk.fill(0, nr); d_rh.fill(0, nr); d_rl.fill(0, nr); d_rf.fill(0xFF, nr);
    }
    template <int MODE> void roll(const Text& x, u32* hitslot) {
        launch_wave_kernel(depth_roll_kernel<MODE>, (x.n_words + 255) / 256, 0, (const u64*)d_bits.p, (const u32*)d_mask.p, x.n_words, k, t,
                           (const u64*)d_toff.p, (const u32*)d_wread.p, hitslot, d_rk.p, d_rh.p, d_rf.p, d_rl.p, err.p);
    }
    void check_err(const char* what) {
        if (read_scalar(err.p)) throw DeviceError(std::string("read depths: internal error (the k-mer table filled up during ") + what + ")");
    }
};

DepthEngine::DepthEngine(uint32_t k, const std::vector<DepthGraphView>& graphs, std::vector<DepthGraphPlan>&& plans) : impl_(new Impl) {
    Impl& m = *impl_;
    m.k = k;
    m.plans = std::move(plans);
    std::vector<const u8*> seq;
    m.asm_toff.assign(1, 0);
    m.graph_first.assign(1, 0);
    u64 n_junction = 0;
    for (size_t g = 0; g < graphs.size(); g++) {
        for (u32 u = 0; u < graphs[g].n_unitigs; u++) {
            seq.push_back(graphs[g].seq_bytes + graphs[g].seq_begin[u]);
            m.asm_toff.push_back(m.asm_toff.back() + graphs[g].seq_len[u] + 1);
        }
        if (seq.size() >= 0xFFFFFFF0ull) throw DeviceError("read depths: too many unitigs");
        m.graph_first.push_back((u32)seq.size());
        n_junction += m.plans[g].junction.size();
    }
    const u64 n_pos = m.asm_toff.back();
    u64 cap = 64;
    while (cap < 2 * (n_pos + n_junction)) cap <<= 1;
    if (cap > ((u64)1 << 31)) throw DeviceError("read depths: the consensus assembly is too large for a table of 2^31 slots");
    m.t = DepthTable{m.keys.ensure(cap), m.occ.ensure(cap), m.cnt.ensure(cap), cap - 1};
    m.keys.fill(0xFF, cap); m.occ.fill(0, cap); m.cnt.fill(0, cap);
    m.err.ensure(1); m.err.fill(0, 1);
    m.d_totals.ensure(8); m.d_totals.fill(0, 8);
    m.tot.table_slots = cap;
    if (!seq.empty()) {
        const Impl::Text x = m.upload_text([&](u64 r) { return seq[r]; }, m.asm_toff);
        m.reset_read_sums(x.n_seqs);
        m.roll<0>(x, nullptr);
        for (size_t g = 0; g < graphs.size(); g++) {
            const std::vector<u64>& jk = m.plans[g].junction;
            if (jk.empty()) continue;
            copy_h2d(m.d_q.ensure(jk.size()), jk.data(), jk.size() * 8);
            launch((u64)jk.size(), DepthInsertKeysFunctor{m.t, (const u64*)m.d_q.p, m.err.p});
            stream_sync();
        }
        m.check_err("its build");
        m.roll<1>(x, m.asm_slot.ensure(x.n_words * 32));      // every assembly position's slot, kept for ac_depth_finish
    }
    launch_full(cap, DepthCensusFunctor{m.t, m.d_totals.p + 6});
    u64 census[2];
    copy_d2h(census, m.d_totals.p + 6, 16);
    m.tot.distinct_kmers = census[0]; m.tot.repeat_kmers = census[1];
}
DepthEngine::~DepthEngine() {
#ifndef AC_EMU
    (void)hipDeviceSynchronize();
#endif
}

uint32_t DepthEngine::n_graphs() const { return (uint32_t)impl_->graph_first.size() - 1; }
uint32_t DepthEngine::n_unitigs(uint32_t g) const { return impl_->graph_first[g + 1] - impl_->graph_first[g]; }

void DepthEngine::add_reads(const uint8_t* bases, const uint64_t* off, uint64_t n_reads) {
    Impl& m = *impl_;
    u64 budget = (u64)1 << 28;      // text positions (read bytes + one separator each) per batch: 4 bytes of kept slot per position on the device
    if (const char* e = getenv("AC_DEPTH_BATCH_BYTES")) { const long long v = atoll(e); if (v > 0 && (u64)v < budget) budget = (u64)v; }
    std::vector<u64> toff;
    for (u64 r0 = 0; r0 < n_reads;) {
        toff.assign(1, 0);
        u64 r1 = r0;
        while (r1 < n_reads && r1 - r0 < 0x7FFFFFFFull) {      // whole reads; a read longer than the budget is a batch of its own
            const u64 len = off[r1 + 1] - off[r1];
            if (len >= 0xFFFFFFF0ull) throw DeviceError("read " + std::to_string(r1 + 1) + " is longer than 2^32 bases");
            if (r1 > r0 && toff.back() + len + 1 > budget) break;
            toff.push_back(toff.back() + len + 1);
            r1++;
        }
        const Impl::Text x = m.upload_text([&](u64 r) { return bases + off[r0 + r]; }, toff);
        m.reset_read_sums(x.n_seqs);
        m.d_hitslot.ensure(x.n_words * 32);
        m.meter.begin();
        m.roll<1>(x, m.d_hitslot.p);
        launch_full(x.n_seqs, DepthAcceptFunctor{m.d_rk.p, m.d_rh.p, m.d_rf.p, m.d_rl.p, m.d_toff.p, m.d_acc.p, m.d_totals.p, m.k});
        launch_wave_kernel(depth_commit_kernel, (x.n_words * 32 + 4 * DEPTH_WAVE_TILE - 1) / (4 * DEPTH_WAVE_TILE), 0, (const u32*)m.d_hitslot.p,
                           x.n_words * 32, (const u64*)m.d_toff.p, (const u32*)m.d_wread.p, (const u8*)m.d_acc.p, m.t.cnt);
        m.meter.end();
        m.tot.seconds_device += m.meter.take();      // (waits for the batch: the staging planes are packed anew for the next one)
        m.tot.batches++; m.tot.launches += 3;
        r0 = r1;
    }
}

DepthTotals DepthEngine::totals() {
    Impl& m = *impl_;
    u64 v[6];
    copy_d2h(v, m.d_totals.p, sizeof v);
    m.tot.reads = v[0]; m.tot.rejected_reads = v[1]; m.tot.read_bases = v[2]; m.tot.span_bases = v[3]; m.tot.span_kmers = v[4]; m.tot.hits = v[5];
    return m.tot;
}

void DepthEngine::kmer_counts(const uint64_t* kmers, uint64_t n, uint8_t* present, uint32_t* occurrences, uint32_t* read_count) {
    Impl& m = *impl_;
    if (!n) return;
    copy_h2d(m.d_q.ensure(n), kmers, n * 8);
    m.d_present.ensure(n); m.d_qocc.ensure(n); m.d_qcnt.ensure(n);
    launch(n, DepthLookupFunctor{m.t, (const u64*)m.d_q.p, m.k, m.d_present.p, m.d_qocc.p, m.d_qcnt.p});
    if (present) copy_d2h_async(present, m.d_present.p, n);
    if (occurrences) copy_d2h_async(occurrences, m.d_qocc.p, n * 4);
    if (read_count) copy_d2h_async(read_count, m.d_qcnt.p, n * 4);
    stream_sync();
}

void DepthEngine::finish(uint32_t g, double* depth, uint8_t* has_depth) {
    Impl& m = *impl_;
    const DepthTotals tt = totals();
    if (tt.reads == 0) throw DeviceError("no reads were found in the reads added so far which match the consensus assembly");
    const double scale = tt.hits > 0 ? (double)tt.span_bases / (double)tt.hits : 0.0;
    const u32 u0 = m.graph_first[g], u1 = m.graph_first[g + 1];
    const u64 p0 = m.asm_toff[u0], np = m.asm_toff[u1] - p0;
    std::vector<u32> cnt(np); std::vector<u8> flag(np);
    if (np) {
        m.d_qcnt.ensure(np); m.d_present.ensure(np);
        launch(np, DepthGatherFunctor{m.t, (const u32*)m.asm_slot.p, p0, m.d_qcnt.p, m.d_present.p});
        copy_d2h_async(cnt.data(), m.d_qcnt.p, np * 4);
        copy_d2h_async(flag.data(), m.d_present.p, np);
        stream_sync();
    }
    const DepthGraphPlan& plan = m.plans[g];
    const u64 nq = plan.kmers.size();
    std::vector<u8> q_present(nq); std::vector<u32> q_occ(nq), q_cnt(nq);
    kmer_counts(plan.kmers.data(), nq, q_present.data(), q_occ.data(), q_cnt.data());
    std::vector<u32> counts;
    for (u32 u = u0; u < u1; u++) {      // tig_kmer_counts (depth.rs:317-342): own positions ascending, then the context offsets ascending
        counts.clear();
        const u64 len = m.asm_toff[u + 1] - m.asm_toff[u] - 1, base = m.asm_toff[u] - p0;
        if (len >= m.k)
            for (u64 i = 0; i + m.k <= len; i++) { const u64 e = base + i + m.k - 1; if (flag[e] == 0) counts.push_back(cnt[e]); }
        for (u64 c = plan.ctx_begin[u - u0]; c < plan.ctx_begin[u - u0 + 1]; c++) {
            const DepthContext& cx = plan.ctx[c];
            bool repeat = false; u32 sum = 0;
            for (u64 q = cx.first; q < cx.first + cx.count; q++) {
                if (q_present[q] && q_occ[q] > 1) { repeat = true; break; }
                if (q_present[q]) sum += q_cnt[q];
            }
            if (!repeat) counts.push_back(sum);
        }
        double mean = 0.0;
        const bool has = depth_clipped_mean(counts, &mean);
        depth[u - u0] = has ? mean * scale : 0.0;
        has_depth[u - u0] = has ? 1 : 0;
    }
}

}  // namespace ac
