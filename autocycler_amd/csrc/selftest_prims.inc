// Data-in / data-out test hooks of the device primitives (device_prims.hpp) and of the wave layer (wave_rt.hpp): each runs ONE primitive on
// the caller's arrays and hands its output arrays back, so that the reference lives in the tests as plain numpy / Python integers and a new
// case costs no C++ (ac_selftest_* of the C ABI; included by graph_build.hip, compiled for the device and for the emulation alike).
// Not covered from here: scan totals of 2^46 and more (the state word holds 46 value bits: device_prims.hpp), more than 2^32 items.

namespace selftest {

template <class T> struct Shifted {      // n items that start `mis` elements behind a 16-byte boundary (the arena hands out 256-byte boundaries)
    DBuf<T> buf; T* p;
    Shifted(size_t n, int mis) : buf(n + 16 / sizeof(T)), p(buf.ptr() + mis) {}
};
template <class T, int OP, bool INCL> void scan_case(const void* in, u64 n, bool in_place, int mis_in, int mis_out, void* out) {
    if (mis_in < 0 || mis_out < 0 || (size_t)mis_in >= 16 / sizeof(T) || (size_t)mis_out >= 16 / sizeof(T)) throw DeviceError("selftest scan: misalignment out of range");
    Shifted<T> a(n, mis_in), o(n, mis_out);
    copy_h2d(a.p, in, n * sizeof(T));
    T* dst = in_place ? a.p : o.p;
    scan_launch<T, OP, INCL>(a.p, dst, n, 0);
    copy_d2h(out, dst, n * sizeof(T));
}

struct MinU64 { AC_HD u64 operator()(u64 a, u64 b) const { return b < a ? b : a; } };
struct ArgSmaller { const u64* v; AC_HD u32 operator()(u32 a, u32 b) const { return v[b] < v[a] ? b : a; } };      // the index of the smaller value, the first argument on ties
struct PairKey { u64 a; u32 b; u32 pad; };
struct PairLess { AC_HD bool operator()(const PairKey& x, const PairKey& y) const { return x.a != y.a ? x.a < y.a : x.b < y.b; } };
struct ValueLess { const u64* v; AC_HD bool operator()(u32 x, u32 y) const { return v[x] < v[y]; } };

// ---- the wave layer, primitive by primitive: one workgroup of 256 threads; thread t returns before any cross-lane operation if bit t of
// `live` is clear, the others run `program` and write out[t] ----
enum WaveProgram {
    WP_BALLOT = 0, WP_ALL, WP_UNIFORM, WP_SHFL, WP_SHFL64, WP_SHFL_XOR, WP_SHFL_XOR64, WP_SHFL_UP, WP_SHFL_DOWN,
    WP_GRP_BALLOT16, WP_GRP_SHFL16, WP_GRP_BALLOT64, WP_GRP_SHFL64, WP_BLOCK_SYNC,
    // distances the compiler sees as constants (it may pick another instruction for them than for a distance in a register)
    WP_SHFL_UP_1, WP_SHFL_DOWN_1, WP_SHFL_XOR_1, WP_SHFL_XOR_32, WP_SHFL_XOR64_16, WP_SHFL_UP_16, WP_SHFL_DOWN_32, WP_COUNT
};
template <int UNUSED> AC_KERNEL void __launch_bounds__(256) wave_program_kernel(int program, const u64* in, const int* aux, const u64* live, u64* out) {
    AC_SHARED u64 s_x[256];
    const unsigned t = wv::tid();
    const bool alive = (live[t >> 6] >> (t & 63)) & 1;
    const u64 v64 = in[t];
    const int v = (int)(u32)v64, a = aux[t], a0 = aux[0];
    if (program == WP_BLOCK_SYNC) s_x[t] = alive ? v64 : ~v64;      // (a returned thread leaves its word behind: no cross-lane operation yet)
    if (!alive) return;
    const int gs16 = (int)(t & 63 & ~15u);
    u64 r = 0;
    switch (program) {
        case WP_BALLOT: r = wv::ballot((a & 1) != 0); break;
        case WP_ALL: r = wv::all((a & 1) != 0) ? 1 : 0; break;
        case WP_UNIFORM: r = (u32)wv::uniform(v); break;
        case WP_SHFL: r = (u32)wv::shfl(v, a); break;
        case WP_SHFL64: r = wv::shfl64(v64, a); break;
        case WP_SHFL_XOR: r = (u32)wv::shfl_xor(v, a0); break;
        case WP_SHFL_XOR64: r = wv::shfl_xor64(v64, a0); break;
        case WP_SHFL_UP: r = (u32)wv::shfl_up(v, a0); break;
        case WP_SHFL_DOWN: r = (u32)wv::shfl_down(v, a0); break;
        case WP_GRP_BALLOT16: r = wv::grp_ballot<16>((a & 1) != 0, gs16); break;
        case WP_GRP_SHFL16: r = (u32)wv::grp_shfl<16>(v, a, gs16); break;
        case WP_GRP_BALLOT64: r = wv::grp_ballot<64>((a & 1) != 0, 0); break;
        case WP_GRP_SHFL64: r = (u32)wv::grp_shfl<64>(v, a, 0); break;
        case WP_BLOCK_SYNC: {      // two exchanges through LDS between the wavefronts, each ordered by barriers alone
            wv::block_sync();
            const u64 x = s_x[(t + (unsigned)a0) & 255u];
            wv::block_sync();
            s_x[t] = x + 1;
            wv::block_sync();
            r = x + 3 * s_x[(t + 2 * (unsigned)a0) & 255u];
            break;
        }
        case WP_SHFL_UP_1: r = (u32)wv::shfl_up(v, 1); break;
        case WP_SHFL_DOWN_1: r = (u32)wv::shfl_down(v, 1); break;
        case WP_SHFL_XOR_1: r = (u32)wv::shfl_xor(v, 1); break;
        case WP_SHFL_XOR_32: r = (u32)wv::shfl_xor(v, 32); break;
        case WP_SHFL_XOR64_16: r = wv::shfl_xor64(v64, 16); break;
        case WP_SHFL_UP_16: r = (u32)wv::shfl_up(v, 16); break;
        case WP_SHFL_DOWN_32: r = (u32)wv::shfl_down(v, 32); break;
        default: break;
    }
    out[t] = r;
}

}  // namespace selftest

// kind: 0 u32 inclusive add, 1 u32 exclusive add, 2 u32 inclusive max, 3 u64 exclusive add
void selftest_scan(int kind, const void* in, uint64_t n, bool in_place, int misalign_in, int misalign_out, void* out) {
    Arena::device().reset();
    if (n && (!in || !out)) throw DeviceError("null pointer");
    switch (kind) {
        case 0: selftest::scan_case<u32, SCAN_ADD, true>(in, n, in_place, misalign_in, misalign_out, out); break;
        case 1: selftest::scan_case<u32, SCAN_ADD, false>(in, n, in_place, misalign_in, misalign_out, out); break;
        case 2: selftest::scan_case<u32, SCAN_MAX, true>(in, n, in_place, misalign_in, misalign_out, out); break;
        case 3: selftest::scan_case<u64, SCAN_ADD, false>(in, n, in_place, misalign_in, misalign_out, out); break;
        default: throw DeviceError("selftest scan: unknown kind");
    }
    stream_sync();
}

// val_kind 0: u32 values (sort_pairs_u64_u32), 1: i32 values (sort_pairs_u64_i32, which takes no prepared scratch).  prep_n != 0: a
// RadixScratch prepared with (prep_n, prep_bits) is handed in; prep_reuse: ... after another sort has already used it up.
void selftest_radix(const uint64_t* keys, const void* vals, uint64_t n, int begin_bit, int end_bit, int val_kind, uint64_t prep_n, int prep_bits, bool prep_reuse,
                    uint64_t* keys_out, void* vals_out) {
    Arena::device().reset();
    if (n && (!keys || !vals || !keys_out || !vals_out)) throw DeviceError("null pointer");
    if (begin_bit < 0 || end_bit > 64) throw DeviceError("selftest radix: bits out of range");
    if (val_kind != 0 && val_kind != 1) throw DeviceError("selftest radix: unknown value kind");
    if (val_kind == 1 && prep_n) throw DeviceError("selftest radix: the i32 form takes no prepared scratch");
    DBuf<u64> dk(n);
    copy_h2d(dk.ptr(), keys, n * 8);
    if (val_kind == 0) {
        DBuf<u32> dv(n);
        RadixScratch rs;
        if (prep_n) rs.prepare(prep_n, prep_bits);
        if (prep_n && prep_reuse) {
            DBuf<u64> k0(n); DBuf<u32> v0(n);
            copy_h2d(k0.ptr(), keys, n * 8); copy_h2d(v0.ptr(), vals, n * 4);
            sort_pairs_u64_u32(k0, v0, n, end_bit, 0, begin_bit, &rs);
        }
        copy_h2d(dv.ptr(), vals, n * 4);
        sort_pairs_u64_u32(dk, dv, n, end_bit, 0, begin_bit, prep_n ? &rs : nullptr);
        copy_d2h(vals_out, dv.ptr(), n * 4);
    } else {
        DBuf<int32_t> dv(n);
        copy_h2d(dv.ptr(), vals, n * 4);
        sort_pairs_u64_i32(dk, dv, n, end_bit, 0, begin_bit);
        copy_d2h(vals_out, dv.ptr(), n * 4);
    }
    copy_d2h(keys_out, dk.ptr(), n * 8);
    stream_sync();
}

// op 0: reduce_by_segment, u64 minimum -> out = u64[n_segments]; op 1: segment_argmin, the index of the smaller value (the lower index on
// ties) -> out = u32[n_segments].  Entries no segment wrote keep all their bits set.  deferred_err: the error-word form; *err_out = the word.
void selftest_segments(int op, const uint32_t* seg, const uint64_t* vals, uint64_t n, uint64_t n_segments, bool deferred_err, void* out, uint32_t* err_out) {
    Arena::device().reset();
    if ((n && (!seg || !vals)) || (n_segments && !out) || !err_out) throw DeviceError("null pointer");
    if (op != 0 && op != 1) throw DeviceError("selftest segments: unknown op");
    DBuf<u32> ds(n), err(1, true); DBuf<u64> dv(n);
    copy_h2d(ds.ptr(), seg, n * 4); copy_h2d(dv.ptr(), vals, n * 8);
    u32* e = deferred_err ? err.ptr() : nullptr;
    if (op == 0) {
        DBuf<u64> o(n_segments);
        o.fill_bytes(0xFF);
        reduce_by_segment(ds.ptr(), dv.ptr(), n, o.ptr(), n_segments, selftest::MinU64(), e);
        copy_d2h(out, o.ptr(), n_segments * 8);
    } else {
        DBuf<u32> o(n_segments);
        o.fill_bytes(0xFF);
        segment_argmin(ds.ptr(), n, o.ptr(), n_segments, selftest::ArgSmaller{dv.ptr()}, e);
        copy_d2h(out, o.ptr(), n_segments * 4);
    }
    *err_out = read_scalar(err.ptr());
    stream_sync();
}

// form 0: sort_by_key_cmp, keys (a[i], b[i]) compared field by field, payload vals[i] -> a_out, b_out, vals_out; form 1: sort_keys_cmp of
// the indices vals[i] (each below n) by a[index] -> vals_out.
void selftest_sort_cmp(int form, const uint64_t* a, const uint32_t* b, const uint32_t* vals, uint64_t n, uint64_t* a_out, uint32_t* b_out, uint32_t* vals_out) {
    Arena::device().reset();
    if (n && (!a || !vals || !vals_out)) throw DeviceError("null pointer");
    if (n >= 0xFFFFFFF0ULL) throw DeviceError("selftest sort: too many items");
    if (form == 0) {
        if (n && (!b || !a_out || !b_out)) throw DeviceError("null pointer");
        std::vector<selftest::PairKey> hk(n);
        for (u64 i = 0; i < n; i++) hk[i] = selftest::PairKey{a[i], b[i], 0};
        DBuf<selftest::PairKey> dk(n); DBuf<u32> dv(n);
        copy_h2d(dk.ptr(), hk.data(), n * sizeof(selftest::PairKey)); copy_h2d(dv.ptr(), vals, n * 4);
        sort_by_key_cmp(dk, dv, n, selftest::PairLess());
        copy_d2h(hk.data(), dk.ptr(), n * sizeof(selftest::PairKey)); copy_d2h(vals_out, dv.ptr(), n * 4);
        for (u64 i = 0; i < n; i++) { a_out[i] = hk[i].a; b_out[i] = hk[i].b; }
    } else if (form == 1) {
        for (u64 i = 0; i < n; i++) if (vals[i] >= n) throw DeviceError("selftest sort: index out of range");
        DBuf<u64> dv(n); DBuf<u32> idx(n);
        copy_h2d(dv.ptr(), a, n * 8); copy_h2d(idx.ptr(), vals, n * 4);
        sort_keys_cmp(idx, n, selftest::ValueLess{dv.ptr()});
        copy_d2h(vals_out, idx.ptr(), n * 4);
    } else throw DeviceError("selftest sort: unknown form");
    stream_sync();
}

// op 0: read; 1: the epoch forward to `value` (below 2^16); 2: invalidate().  out = {cap, epoch, tickets} of the calling thread's pool afterwards.
void selftest_scan_pool(int op, uint64_t value, uint64_t* out) {
    if (!out) throw DeviceError("null pointer");
    ScanPool& pool = scan_pool();
    if (op == 1) {
        if (value < pool.epoch || value >= (1ULL << 16)) throw DeviceError("selftest scan pool: the epoch only goes forward and stays below 2^16");
        pool.epoch = value;
    } else if (op == 2) pool.invalidate();
    else if (op != 0) throw DeviceError("selftest scan pool: unknown op");
    out[0] = pool.cap; out[1] = pool.epoch; out[2] = pool.tickets;
}

// out_u64[t] of a thread that returned keeps the value the caller put there.
void selftest_wave(int program, const uint64_t* in_u64, const int32_t* aux_i32, const uint64_t* live_mask, uint64_t* out_u64) {
    Arena::device().reset();
    if (!in_u64 || !aux_i32 || !live_mask || !out_u64) throw DeviceError("null pointer");
    if (program < 0 || program >= selftest::WP_COUNT) throw DeviceError("selftest wave: unknown program");
    DBuf<u64> in(256), live(4), out(256); DBuf<int> aux(256);
    copy_h2d(in.ptr(), in_u64, 256 * 8); copy_h2d(aux.ptr(), aux_i32, 256 * 4); copy_h2d(live.ptr(), live_mask, 4 * 8); copy_h2d(out.ptr(), out_u64, 256 * 8);
    launch_wave_kernel(selftest::wave_program_kernel<0>, 1, 0, program, (const u64*)in.ptr(), (const int*)aux.ptr(), (const u64*)live.ptr(), out.ptr());
    copy_d2h(out_u64, out.ptr(), 256 * 8);
    stream_sync();
}
