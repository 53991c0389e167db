// Data-in / data-out test hooks of the device runtime itself (device_rt.hpp): the arena, the fused fills, the read-backs, the launchers, the
// atomic wrappers with wave_alloc32 / wave_add64, and the side stream with its event ring.  Each hook runs ONE facility on the caller's data and
// hands the result back; the reference lives in tests/runtime_cases.py as plain numpy / Python (ac_selftest_* of the C ABI; included by
// graph_build.hip next to selftest_prims.inc, compiled for the device and for the emulation alike).  Every bad argument is a host-side throw
// before any launch.  Not covered from here: fills above FILL_MAX_TILES tiles (128 GB), grids that need a third launch, multi-device contexts.

namespace selftest {

inline size_t round256(size_t b) { b = (b + 255) & ~(size_t)255; return b ? b : 256; }
inline u32 launches_now() { return rt_counters().launches; }
inline u32 readbacks_now() { return rt_counters().readbacks; }

struct StoreByteFunctor { u8* p; u8 v; AC_D void operator()(u64 i) const { p[i] = v; } };
struct StoreByteFullFunctor { u8* p; u8 v; AC_D void operator()(u64 i, bool valid) const { if (valid) p[i] = v; } };
struct StoreWordFunctor { u64* p; u64 v; AC_D void operator()(u64 i) const { p[i] = v; } };
struct RampFunctor { u32* p; u32 seed; AC_D void operator()(u64 i) const { p[i] = (u32)i * 2654435761u + seed; } };
template <int UNUSED> AC_KERNEL void __launch_bounds__(256) store_byte_kernel(u8* p, u64 n, u8 v) {
    const u64 i = (u64)wv::bid() * 256 + wv::tid();
    if (i < n) p[i] = v;
}

// ---- fills ----
enum FillKind { FK_ALL = 0, FK_FROM, FK_FIRST, FK_SIDE_STREAM, FK_COUNT };
enum FillTrigger { FT_NONE = 0, FT_LAUNCH, FT_LAUNCH_FULL, FT_LAUNCH_WAVE, FT_COPY_H2D, FT_COPY_D2H, FT_COPY_D2D, FT_STREAM_SYNC, FT_REWIND, FT_AFTER_MAIN, FT_MAIN_EVENT, FT_COUNT };
struct FillSpan {      // sentinel, region 0, sentinel, region 1, ..., sentinel: one run of arena memory
    std::vector<DBuf<u8>> region;
    u8* base = nullptr; size_t bytes = 0;
    void alloc(const uint64_t* regions, u64 n_regions, u64 span_bytes) {
        size_t need = 256;
        for (u64 i = 0; i < n_regions; i++) need += round256(regions[4 * i]) + 256;
        if (need != span_bytes) throw DeviceError("selftest fills: the span is " + std::to_string(need) + " bytes, the caller says " + std::to_string(span_bytes));
        Arena::device().reserve(need + 4096);      // (+ the trigger's scratch)
        base = (u8*)Arena::device().alloc(256);
        size_t o = 256;
        region.clear(); region.resize(n_regions);
        for (u64 i = 0; i < n_regions; i++) {
            region[i].alloc(regions[4 * i]);
            if ((u8*)region[i].ptr() != base + o) throw DeviceError("selftest fills: the arena did not hand out one run of memory");
            o += round256(regions[4 * i]);
            if ((u8*)Arena::device().alloc(256) != base + o) throw DeviceError("selftest fills: the arena did not hand out one run of memory");
            o += 256;
        }
        bytes = o;
    }
    void queue(const uint64_t* regions) {
        for (size_t i = 0; i < region.size(); i++) {
            const u64 kind = regions[4 * i + 1], arg = regions[4 * i + 2]; const int byte = (int)(regions[4 * i + 3] & 0xFF);
            if (kind == FK_ALL) region[i].fill_bytes(byte);
            else if (kind == FK_FROM) region[i].fill_bytes_from(arg, byte);
            else if (kind == FK_FIRST) region[i].fill_bytes_first(arg, byte);
            else region[i].fill_bytes(byte, SideStream::get().stream());
        }
    }
};

// ---- launchers: every logical thread adds to the slots of its workgroup, (tid / 256) mod 1024 — {threads, sum of tid, xor of tid, lanes
// beyond n}.  No per-thread memory; a wavefront whose 64 lanes all arrived reduces first and issues one atomic per word (as wave_add64 does) ----
static const u32 LAUNCH_SLOTS = 1024;
AC_D void slots_add_lane(u64* slots, u64 tid, bool valid) {      // one lane on its own
    u64* s = slots + 4 * ((tid >> 8) & (LAUNCH_SLOTS - 1));
    if (valid) { atomic_add64(s + 0, 1); atomic_add64(s + 1, tid); atomic_xor64(s + 2, tid); }
    else atomic_add64(s + 3, 1);
}
AC_D void slots_add_wave(u64* slots, u64 tid, bool valid) {      // all 64 lanes of a wavefront together
    const u64 ok = wv::ballot(valid);
    u64 sum = valid ? tid : 0, x = valid ? tid : 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) { sum += wv::shfl_xor64(sum, o); x ^= wv::shfl_xor64(x, o); }
    if (wv::lane() != 0) return;
    u64* s = slots + 4 * ((tid >> 8) & (LAUNCH_SLOTS - 1));
    const u64 n_ok = (u64)__builtin_popcountll(ok);
    if (n_ok) { atomic_add64(s + 0, n_ok); atomic_add64(s + 1, sum); atomic_xor64(s + 2, x); }
    if (n_ok != 64) atomic_add64(s + 3, 64 - n_ok);
}
struct SlotsFunctor {      // launch(): lanes beyond n never get here, and the emulation runs the threads one by one
    u64* slots; u64 n;
    AC_D void operator()(u64 tid) const {
#ifndef AC_EMU
        if ((tid | 63) < n) { slots_add_wave(slots, tid, true); return; }      // (wave-uniform: a wavefront holds 64 consecutive tids from a multiple of 64)
#endif
        slots_add_lane(slots, tid, true);
    }
};
struct SlotsFullFunctor { u64* slots; AC_D void operator()(u64 tid, bool valid) const { slots_add_wave(slots, tid, valid); } };
template <int UNUSED> AC_KERNEL void __launch_bounds__(256) slots_kernel(u64* slots, u64 n) {
    const u64 tid = (u64)wv::bid() * 256 + wv::tid();
    slots_add_wave(slots, tid, tid < n);
}

// ---- atomics: 64 workgroups of 256 threads; thread t works on word target[t] with operand[t] ----
enum AtomicOp { AO_ADD32 = 0, AO_ADD64, AO_MIN32, AO_MAX32, AO_MIN64, AO_MAX64, AO_OR32, AO_OR64, AO_XOR64, AO_FETCH_OR32, AO_FETCH_AND32, AO_CAS32, AO_CAS64,
                AO_LOAD32, AO_WAVE_ALLOC32, AO_WAVE_ADD64, AO_COUNT };
static const u32 ATOMIC_THREADS = 64 * 256;
template <int UNUSED> AC_KERNEL void __launch_bounds__(256) atomics_kernel(int op, u32* w32, u64* w64, const u64* operand, const u32* target, u64 expected, u64* ret) {
    const u32 t = wv::bid() * 256 + wv::tid();
    const u64 v = operand[t]; const u32 w = target[t];
    u64 r = 0;
    switch (op) {
        case AO_ADD32: r = atomic_add32(w32 + w, (u32)v); break;
        case AO_ADD64: r = atomic_add64(w64 + w, v); break;
        case AO_MIN32: atomic_min32(w32 + w, (u32)v); break;
        case AO_MAX32: atomic_max32(w32 + w, (u32)v); break;
        case AO_MIN64: r = atomic_min64(w64 + w, v); break;
        case AO_MAX64: atomic_max64(w64 + w, v); break;
        case AO_OR32: atomic_or32(w32 + w, (u32)v); break;
        case AO_OR64: atomic_or64(w64 + w, v); break;
        case AO_XOR64: atomic_xor64(w64 + w, v); break;
        case AO_FETCH_OR32: r = atomic_fetch_or32(w32 + w, (u32)v); break;
        case AO_FETCH_AND32: r = atomic_fetch_and32(w32 + w, (u32)v); break;
        case AO_CAS32: r = atomic_cas32(w32 + w, (u32)expected, (u32)v); break;
        case AO_CAS64: r = atomic_cas64(w64 + w, expected, v); break;
        case AO_LOAD32: r = atomic_load32(w32 + w); break;
        case AO_WAVE_ALLOC32: r = wave_alloc32(w32 + w, (u32)v); break;
        case AO_WAVE_ADD64: wave_add64(w64 + w, (u32)v); break;
        default: break;
    }
    ret[t] = r;
}

}  // namespace selftest

// regions: n_regions x {bytes, kind (FillKind), arg (from / upto), byte}.  span: in = the pattern the whole span gets by ONE copy_h2d, out = the
// span afterwards (sentinels and rounding slack included).  mode 0: queue the fills, fire the trigger, read back; mode 1 (drop on reset):
// queue the fills, reset the arena, allocate the same again, upload the pattern, synchronise, read back.  launches_out = the launch counter
// {after the queueing, after the trigger} counted from before the queueing.
void selftest_fills(const uint64_t* regions, uint64_t n_regions, int trigger, int mode, uint8_t* span, uint64_t span_bytes, uint32_t* launches_out) {
    Arena& arena = Arena::device();
    arena.reset();
    if (!regions || !span || !launches_out) throw DeviceError("null pointer");
    if (n_regions == 0 || n_regions > 4096) throw DeviceError("selftest fills: 1 to 4096 regions");
    if (trigger < 0 || trigger >= selftest::FT_COUNT) throw DeviceError("selftest fills: unknown trigger");
    if (mode != 0 && mode != 1) throw DeviceError("selftest fills: unknown mode");
    for (u64 i = 0; i < n_regions; i++) {
        if (regions[4 * i] > ((u64)1 << 30)) throw DeviceError("selftest fills: a region of more than 1 GB");
        if (regions[4 * i + 1] >= (u64)selftest::FK_COUNT) throw DeviceError("selftest fills: unknown kind");
    }
    selftest::FillSpan sp;
    sp.alloc(regions, n_regions, span_bytes);
    DBuf<u8> scratch(1024);
    SideStream& side = SideStream::get();
    SideStream::Guard side_guard;
    if (mode == 0) {
        copy_h2d(sp.base, span, sp.bytes);
        copy_h2d(scratch.ptr(), span, 256);
        stream_sync();      // (the side stream's fills need no event behind the upload; the queue is empty from here)
    }
    const u32 l0 = selftest::launches_now();
    sp.queue(regions);
    launches_out[0] = selftest::launches_now() - l0;
    if (mode == 1) {
        side.sync();
        arena.reset();
        sp.alloc(regions, n_regions, span_bytes);
        copy_h2d(sp.base, span, sp.bytes);
        stream_sync();
        launches_out[1] = selftest::launches_now() - l0;
    } else {
        u8 host4[256];
        const Arena::Mark mk = arena.mark();
        switch (trigger) {
            case selftest::FT_LAUNCH: launch(256, selftest::StoreByteFunctor{scratch.ptr() + 256, 1}); break;
            case selftest::FT_LAUNCH_FULL: launch_full(200, selftest::StoreByteFullFunctor{scratch.ptr() + 256, 2}); break;
            case selftest::FT_LAUNCH_WAVE: launch_wave_kernel(selftest::store_byte_kernel<0>, 1, 0, scratch.ptr() + 256, (u64)256, (u8)3); break;
            case selftest::FT_COPY_H2D: copy_h2d(scratch.ptr() + 512, span, 256); break;
            case selftest::FT_COPY_D2H: copy_d2h(host4, scratch.ptr(), 256); break;
            case selftest::FT_COPY_D2D: copy_d2d(scratch.ptr() + 768, scratch.ptr(), 256); break;
            case selftest::FT_STREAM_SYNC: stream_sync(); break;
            case selftest::FT_REWIND: arena.rewind(mk); break;
            case selftest::FT_AFTER_MAIN: side.after_main(); break;
            case selftest::FT_MAIN_EVENT: SideStream::wait_event(side.main_event()); break;
            default: break;
        }
        launches_out[1] = selftest::launches_now() - l0;
        side.sync();
    }
    // the whole span comes back by one plain copy (no mailbox, no scratch page: those are the other hook's subject)
    copy_d2h_async(span, sp.base, sp.bytes);
    stream_sync();
}

// Order: fill a buffer of n bytes with byte1; a functor overwrites [w_lo, w_hi) with w_val; a second fill, fill_bytes_from(from2, byte2); a
// third, fill_bytes_first(upto3, byte3).  out = the n bytes: the sequential result.
void selftest_fill_order(uint64_t n, int byte1, uint64_t w_lo, uint64_t w_hi, int w_val, uint64_t from2, int byte2, uint64_t upto3, int byte3, uint8_t* out) {
    Arena::device().reset();
    if (!out) throw DeviceError("null pointer");
    if (n == 0 || n > ((u64)1 << 30) || w_lo > w_hi || w_hi > n) throw DeviceError("selftest fill order: ranges out of bounds");
    DBuf<u8> b(n);
    b.fill_bytes(byte1);
    launch(w_hi - w_lo, selftest::StoreByteFunctor{b.ptr() + w_lo, (u8)w_val});
    b.fill_bytes_from(from2, byte2);
    b.fill_bytes_first(upto3, byte3);
    copy_d2h(out, b.ptr(), n);
    stream_sync();
}

// path 0: one copy_d2h per item; 1: one ReadBatch of all items (an add of zero bytes included where an item has none); 2: one ReadBatch object,
// the first half of the items, run(), the second half, run(); 3: to_host_ptr per item; 4: read_scalar per item (4 or 8 bytes, aligned to
// that); 5: copy_d2h per item on the side stream behind after_main().  items: n_items x {offset, bytes} into the uploaded data; out: the items
// one behind the other.  counters_out = {launches, read-backs} of the fetches alone.
void selftest_readback(const uint8_t* data, uint64_t n_data, int path, const uint64_t* items, uint64_t n_items, uint8_t* out, uint32_t* counters_out) {
    Arena::device().reset();
    if (!data || !items || !out || !counters_out) throw DeviceError("null pointer");
    if (n_data == 0 || n_data > ((u64)1 << 28)) throw DeviceError("selftest readback: 1 byte to 256 MB of data");
    if (path < 0 || path > 5) throw DeviceError("selftest readback: unknown path");
    for (u64 i = 0; i < n_items; i++) {
        const u64 o = items[2 * i], b = items[2 * i + 1];
        if (o > n_data || b > n_data - o) throw DeviceError("selftest readback: an item lies outside the data");
        if (path == 4 && ((b != 4 && b != 8) || o % b)) throw DeviceError("selftest readback: a scalar is 4 or 8 aligned bytes");
    }
    DBuf<u8> d(n_data);
    copy_h2d(d.ptr(), data, n_data);
    stream_sync();
    SideStream::Guard side_guard;
    const u32 l0 = selftest::launches_now(), r0 = selftest::readbacks_now();
    std::vector<u8*> dst(n_items);
    { u64 o = 0; for (u64 i = 0; i < n_items; i++) { dst[i] = out + o; o += items[2 * i + 1]; } }
    if (path == 1 || path == 2) {
        ReadBatch rb;
        const u64 half = path == 2 ? n_items / 2 : n_items;
        for (u64 i = 0; i < half; i++) rb.add(dst[i], d.ptr() + items[2 * i], items[2 * i + 1]);
        rb.run();
        if (path == 2) {
            for (u64 i = half; i < n_items; i++) rb.add(dst[i], d.ptr() + items[2 * i], items[2 * i + 1]);
            rb.run();
        }
    } else {
        stream_t s = 0;
        if (path == 5) { SideStream& side = SideStream::get(); s = side.stream(); side.after_main(); }
        for (u64 i = 0; i < n_items; i++) {
            const u8* src = d.ptr() + items[2 * i]; const u64 b = items[2 * i + 1];
            if (path == 3) { std::vector<u8> v = to_host_ptr(src, b); if (b) memcpy(dst[i], v.data(), b); }
            else if (path == 4 && b == 4) { const u32 v = read_scalar((const u32*)src); memcpy(dst[i], &v, 4); }
            else if (path == 4) { const u64 v = read_scalar((const u64*)src); memcpy(dst[i], &v, 8); }
            else copy_d2h(dst[i], src, b, s);
        }
    }
    counters_out[0] = selftest::launches_now() - l0; counters_out[1] = selftest::readbacks_now() - r0;
    stream_sync();
}

// n fetches of one device word in a row, each behind a functor launch that wrote value[i] there -> out[i].  counters_out as above (launches
// include the n functor launches).
void selftest_scalar_chain(const uint64_t* values, uint64_t n, uint64_t* out, uint32_t* counters_out) {
    Arena::device().reset();
    if (!values || !out || !counters_out) throw DeviceError("null pointer");
    if (n > 100000) throw DeviceError("selftest scalar chain: at most 100000 fetches");
    DBuf<u64> w(1, true);
    stream_sync();
    const u32 l0 = selftest::launches_now(), r0 = selftest::readbacks_now();
    for (u64 i = 0; i < n; i++) {
        launch(1, selftest::StoreWordFunctor{w.ptr(), values[i]});
        out[i] = read_scalar(w.ptr());
    }
    counters_out[0] = selftest::launches_now() - l0; counters_out[1] = selftest::readbacks_now() - r0;
    stream_sync();
}

// ops: n_ops x {code, arg}: 0 alloc(arg bytes), 1 mark, 2 rewind(mark number arg), 3 reset, 4 reserve(arg), 5 release_all, 6 set_grow(arg).
// The program starts on an EMPTY arena (release_all) and ends with release_all and the arena's own grow step.  totals_out: n_ops x {capacity,
// total_used, peak} after each op.  allocs_out: per alloc, in order, {block ordinal, offset in the block, address}.  After every alloc a device
// functor writes the allocation's ordinal (its low byte) into every byte of it; at the end every allocation with live[ordinal] != 0 is read
// back: wrong_out[ordinal] = the number of its bytes that do not hold the ordinal (untouched for the others).
void selftest_arena(const uint64_t* ops, uint64_t n_ops, uint64_t* totals_out, uint64_t* allocs_out, const uint8_t* live, uint64_t* wrong_out) {
    Arena& arena = Arena::device();
    arena.reset();
    if (!ops || !totals_out || !allocs_out || !live || !wrong_out) throw DeviceError("null pointer");
    if (n_ops > 10000) throw DeviceError("selftest arena: at most 10000 ops");
    u64 n_marks = 0, asked = 0;
    for (u64 i = 0; i < n_ops; i++) {
        const u64 code = ops[2 * i], arg = ops[2 * i + 1];
        if (code > 6) throw DeviceError("selftest arena: unknown op");
        if (code == 1) n_marks++;
        if (code == 2 && arg >= n_marks) throw DeviceError("selftest arena: rewind to a mark that was not taken");
        if ((code == 0 || code == 4 || code == 6) && arg > ((u64)64 << 20)) throw DeviceError("selftest arena: more than 64 MB in one op");
        if (code == 0 || code == 4) asked += arg + 256;
        if (code == 6 && arg == 0) throw DeviceError("selftest arena: a grow step of 0");
    }
    if (asked > ((u64)1 << 30)) throw DeviceError("selftest arena: the program asks for more than 1 GB");
    const size_t grow0 = arena.grow();
    struct Restore { Arena& a; size_t g; ~Restore() { a.release_all(); a.set_grow(g); } } restore{arena, grow0};
    stream_sync();
    arena.release_all();
    struct Al { u8* p; size_t bytes; };
    std::vector<Al> allocs; std::vector<Arena::Mark> marks;
    for (u64 i = 0; i < n_ops; i++) {
        const u64 code = ops[2 * i], arg = ops[2 * i + 1];
        if (code == 0) {
            u8* p = (u8*)arena.alloc(arg);
            size_t blk = 0, off = 0, used = 0;
            if (!arena.locate(p, &blk, &off, &used)) throw DeviceError("selftest arena: an allocation outside every block");
            const u64 ord = allocs.size();
            allocs_out[3 * ord] = blk; allocs_out[3 * ord + 1] = off; allocs_out[3 * ord + 2] = (u64)(uintptr_t)p;
            const size_t bytes = selftest::round256(arg);
            if (off + bytes > used) throw DeviceError("selftest arena: an allocation beyond what its block has handed out");
            launch(bytes, selftest::StoreByteFunctor{p, (u8)ord});
            allocs.push_back(Al{p, bytes});
        } else if (code == 1) marks.push_back(arena.mark());
        else if (code == 2) arena.rewind(marks[arg]);
        else if (code == 3) { stream_sync(); arena.reset(); }            // (a coalescing reset frees blocks: nothing may still be writing them)
        else if (code == 4) { stream_sync(); arena.reserve(arg); }
        else if (code == 5) { stream_sync(); arena.release_all(); }
        else arena.set_grow(arg);
        totals_out[3 * i] = arena.capacity(); totals_out[3 * i + 1] = arena.total_used(); totals_out[3 * i + 2] = arena.peak();
    }
    std::vector<u8> host;
    for (size_t a = 0; a < allocs.size(); a++) {
        if (!live[a]) continue;
        size_t blk = 0, off = 0, used = 0;      // the caller's model says "live": read it only if the arena agrees that the bytes are handed out
        if (!arena.locate(allocs[a].p, &blk, &off, &used) || off + allocs[a].bytes > used) throw DeviceError("selftest arena: allocation " + std::to_string(a) + " is not live");
        host.resize(allocs[a].bytes);
        copy_d2h(host.data(), allocs[a].p, allocs[a].bytes);
        u64 wrong = 0;
        for (u8 b : host) wrong += b != (u8)a;
        wrong_out[a] = wrong;
    }
    stream_sync();
}

// which 0: launch, 1: launch_full, 2: launch_wave_kernel over n logical threads -> slots_out[1024 x 4] = per slot {threads, sum of tid, xor of
// tid, lanes beyond n}.  which 3: launch_wave_kernel_sized with n BLOCKS, which must refuse ("grid too large") or, for 0 blocks, return:
// slots_out stays zero.  info_out = {1 if "grid too large" was thrown, launches counted}.
void selftest_launch(int which, uint64_t n, uint64_t* slots_out, uint32_t* info_out) {
    Arena::device().reset();
    if (!slots_out || !info_out) throw DeviceError("null pointer");
    if (which < 0 || which > 3) throw DeviceError("selftest launch: unknown launcher");
    if (which != 3 && n > ((u64)1 << 32)) throw DeviceError("selftest launch: at most 2^32 threads");
    if (which == 3 && n != 0 && n <= 0xFFFFFFULL) throw DeviceError("selftest launch: the sized form is only asked for grids it must not launch");
#ifdef AC_EMU
    if (which != 3 && n > ((u64)1 << 24)) throw DeviceError("selftest launch: too many threads for the emulation");
#endif
    DBuf<u64> slots(selftest::LAUNCH_SLOTS * 4, true);
    stream_sync();
    const u32 l0 = selftest::launches_now();
    info_out[0] = 0;
    if (which == 0) launch(n, selftest::SlotsFunctor{slots.ptr(), n});
    else if (which == 1) launch_full(n, selftest::SlotsFullFunctor{slots.ptr()});
    else if (which == 2) launch_wave_kernel(selftest::slots_kernel<0>, (n + 255) / 256, 0, slots.ptr(), n);
    else {
        try { launch_wave_kernel_sized(selftest::slots_kernel<0>, n, 256u, 0, slots.ptr(), (u64)0); }
        catch (const DeviceError& e) { if (std::string(e.what()) == "grid too large") info_out[0] = 1; else throw; }
    }
    info_out[1] = selftest::launches_now() - l0;
    copy_d2h_async(slots_out, slots.ptr(), selftest::LAUNCH_SLOTS * 4 * 8);
    stream_sync();
}

// One kernel of 64 workgroups x 256 threads: thread t runs `op` (AtomicOp) with operand[t] on word target[t] (below n_words) of n_words words
// that start as `init`; expected: what the compare-and-swaps compare with.  AO_LOAD32: an earlier launch stores init + w into word w, the
// kernel loads.  words_out[n_words] = the words afterwards (32-bit words widened), returns_out[16384] = what each thread's call returned (0
// for the forms that return nothing).
void selftest_atomics(int op, uint64_t init, uint64_t expected, const uint64_t* operand, const uint32_t* target, uint32_t n_words, uint64_t* words_out, uint64_t* returns_out) {
    Arena::device().reset();
    if (!operand || !target || !words_out || !returns_out) throw DeviceError("null pointer");
    if (op < 0 || op >= selftest::AO_COUNT) throw DeviceError("selftest atomics: unknown op");
    if (n_words == 0 || n_words > 65536) throw DeviceError("selftest atomics: 1 to 65536 words");
    const u32 T = selftest::ATOMIC_THREADS;
    for (u32 t = 0; t < T; t++) if (target[t] >= n_words) throw DeviceError("selftest atomics: a target beyond the words");
    const bool is32 = op == selftest::AO_ADD32 || op == selftest::AO_MIN32 || op == selftest::AO_MAX32 || op == selftest::AO_OR32 || op == selftest::AO_FETCH_OR32 ||
                      op == selftest::AO_FETCH_AND32 || op == selftest::AO_CAS32 || op == selftest::AO_LOAD32 || op == selftest::AO_WAVE_ALLOC32;
    if (op == selftest::AO_WAVE_ALLOC32 || op == selftest::AO_WAVE_ADD64) {      // one counter per wavefront at most: the helpers take a wave-uniform counter
        for (u32 t = 0; t < T; t++) if (target[t] != target[t & ~63u]) throw DeviceError("selftest atomics: the wave helpers take one counter per wavefront");
    }
    std::vector<u32> h32(n_words); std::vector<u64> h64(n_words);
    for (u32 w = 0; w < n_words; w++) { h32[w] = (u32)init; h64[w] = init; }
    DBuf<u32> w32(n_words), tg(T); DBuf<u64> w64(n_words), opd(T), ret(T);
    copy_h2d(w32.ptr(), h32.data(), (size_t)n_words * 4); copy_h2d(w64.ptr(), h64.data(), (size_t)n_words * 8);
    copy_h2d(opd.ptr(), operand, (size_t)T * 8); copy_h2d(tg.ptr(), target, (size_t)T * 4);
    ret.fill_bytes(0xFF);
    if (op == selftest::AO_LOAD32) launch(n_words, selftest::RampFunctor{w32.ptr(), (u32)init});
    launch_wave_kernel(selftest::atomics_kernel<0>, T / 256, 0, op, w32.ptr(), w64.ptr(), (const u64*)opd.ptr(), (const u32*)tg.ptr(), expected, ret.ptr());
    copy_d2h_async(returns_out, ret.ptr(), (size_t)T * 8);
    if (is32) { copy_d2h_async(h32.data(), w32.ptr(), (size_t)n_words * 4); stream_sync(); for (u32 w = 0; w < n_words; w++) words_out[w] = h32[w]; }
    else copy_d2h_async(words_out, w64.ptr(), (size_t)n_words * 8);
    stream_sync();
}

// mode 0: a functor on stream 0 writes n_words words (word i = i * 2654435761 + seed), after_main(which), copy_d2h_async on stream(which),
// mark(which), wait_event -> out_words.  mode 1: the same through main_event() + wait_event + a copy on stream(which) + mark(which) + wait_event.
void selftest_side_order(int mode, int which, uint32_t seed, uint64_t n_words, uint32_t* out_words) {
    Arena::device().reset();
    if (!out_words) throw DeviceError("null pointer");
    if (mode != 0 && mode != 1) throw DeviceError("selftest side: unknown mode");
    if (which != 0 && which != 1) throw DeviceError("selftest side: stream 0 or 1");
    if (n_words == 0 || n_words > ((u64)1 << 26)) throw DeviceError("selftest side: 1 to 2^26 words");
    DBuf<u32> b(n_words);
    HostBlock pinned = PinnedPool::get().alloc(n_words * 4);
    memset(pinned.p, 0, n_words * 4);
    SideStream& side = SideStream::get();
    SideStream::Guard side_guard;
    const stream_t s = side.stream(which);
    stream_sync();
    launch(n_words, selftest::RampFunctor{b.ptr(), seed});
    if (mode == 0) side.after_main(which);
    else SideStream::wait_event(side.main_event());
    copy_d2h_async(pinned.p, b.ptr(), n_words * 4, s);
    SideStream::wait_event(side.mark(which));
    memcpy(out_words, pinned.p, n_words * 4);      // (no further synchronisation: the waited-for event is all that orders this read)
    side.sync();
    stream_sync();
}

// The event ring's bookkeeping.  op 0: read and clear -> out = {events_taken, recycled_waits}.  op 1: the hook's own program — clear, take one
// handle (kinds[0]: 0 main_event, 1 mark), take n_more further events (kinds[1 + i]: 0 main_event, 1 mark, 2 after_main), wait for the first
// handle, read and clear -> out.
void selftest_event_ring(int op, const uint8_t* kinds, uint32_t n_more, uint64_t* out) {
    Arena::device().reset();
    if (!out) throw DeviceError("null pointer");
    if (op != 0 && op != 1) throw DeviceError("selftest ring: unknown op");
    SideStream& side = SideStream::get();
    if (op == 1) {
        if (!kinds) throw DeviceError("null pointer");
        if (n_more > 1000) throw DeviceError("selftest ring: at most 1000 further events");
        if (kinds[0] > 1) throw DeviceError("selftest ring: the handle is a main_event or a mark");
        for (u32 i = 0; i < n_more; i++) if (kinds[1 + i] > 2) throw DeviceError("selftest ring: unknown event kind");
        SideStream::Guard side_guard;
        (void)side.take_ring_counts();
        void* h = kinds[0] == 0 ? side.main_event() : side.mark();
        for (u32 i = 0; i < n_more; i++) {
            if (kinds[1 + i] == 0) (void)side.main_event();
            else if (kinds[1 + i] == 1) (void)side.mark();
            else side.after_main();
        }
        SideStream::wait_event(h);
    }
    const SideStream::RingCounts c = side.take_ring_counts();
    out[0] = c.events_taken; out[1] = c.recycled_waits;
    stream_sync();
}
