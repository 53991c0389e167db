"""The device primitives (csrc/device_prims.hpp) and the wave layer (csrc/wave_rt.hpp) one by one, through the data-in / data-out hooks
ac_selftest_* : every expected array is plain numpy / Python integer code, every comparison exact equality.

lib_path = None: the product library (the MI355X); otherwise the CPU emulation's.  `gpu` adds the sizes only the device can afford.
SCAN_TILE = 4096 items (a scan looks back 64 tiles per round), RS_TILE = 2048 items (a sort looks back 1 + 16 tiles per round)."""
import numpy as np

from autocycler_amd import _capi

EDGE_SIZES = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 17 * 2048 + 1, 64 * 4096 + 1)
GPU_SIZES = (129 * 4096 + 5, 1_000_003)      # a third look-back round of the scan; a million and three
SCAN_TILE = 4096
U32, U64 = np.uint32, np.uint64
M32 = 0xFFFFFFFF


def sizes(gpu):
    return EDGE_SIZES + (GPU_SIZES if gpu else ())


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {i} of {got.size}: got {got[i]}, expected {want[i]}")


# ---- scans -----------------------------------------------------------------------------------------------------------------------
def exclusive(c):
    """inclusive sums -> exclusive ones, staying in uint64 (a concatenation with a Python 0 would go through float64)"""
    x = np.zeros_like(c)
    x[1:] = c[:-1]
    return x


def scan_ref(kind, a):
    a = np.asarray(a)
    if kind == "incl_max_u32":
        return np.maximum.accumulate(a) if a.size else a.copy()
    c = np.cumsum(a.astype(U64), dtype=U64)      # u64 items: totals below 2^46; u32 items: at most 2^24 + 1 of them — no wrap in 64 bits
    if kind == "excl_add_u64":
        return exclusive(c)
    if kind == "excl_add_u32":
        c = exclusive(c)
    return (c & U64(M32)).astype(U32)      # a u32 add scan is exact modulo 2^32


def u64_values(n, rng):
    """n values whose grand total is 2^46 - 1, one below the documented limit of the scans."""
    if n == 0:
        return np.zeros(0, dtype=U64)
    v = rng.integers(0, (1 << 46) // n, size=n, dtype=U64)
    v[-1] = 0
    v[rng.integers(0, n)] += U64((1 << 46) - 1 - int(v.sum(dtype=U64)))
    assert int(v.sum(dtype=U64)) == (1 << 46) - 1
    return v


def scan_inputs(kind, n, rng):
    """name -> input array, for one kind and one size"""
    if kind == "excl_add_u64":
        return {"total 2^46 - 1": u64_values(n, rng)}
    full = rng.integers(0, 1 << 32, size=n, dtype=U64).astype(U32)
    if kind != "incl_max_u32":
        return {"full range": full}
    small = rng.integers(0, 1 << 20, size=n, dtype=U64).astype(U32)
    first_of_tile = small.copy(); last_of_tile = small.copy()
    if n:
        first_of_tile[SCAN_TILE if n > SCAN_TILE else 0] = M32      # the first item of a tile (of the second one where there is one)
        last_of_tile[min(SCAN_TILE - 1, n - 1)] = M32               # the last item of the first tile: carried through every look-back
    return {"ramp": np.arange(n, dtype=U32), "strictly decreasing": (M32 - np.arange(n, dtype=U64)).astype(U32),
            "spike on a tile's first item": first_of_tile, "spike on a tile's last item": last_of_tile, "full range": full}


IN_PLACE_SIZES = (1, 257, 4096, 4097, 17 * 2048 + 1)


def scan_every_size(lib_path, kind, gpu):
    rng = np.random.default_rng(4600 + _capi.SCAN_KINDS[kind])
    for n in sizes(gpu):
        for name, a in scan_inputs(kind, n, rng).items():
            same(_capi.selftest_scan(kind, a, lib_path=lib_path), scan_ref(kind, a), f"{kind}, {name}, n = {n}")
        if n in IN_PLACE_SIZES or n == sizes(gpu)[-1]:
            for name, a in scan_inputs(kind, n, rng).items():
                same(_capi.selftest_scan(kind, a, in_place=True, lib_path=lib_path), scan_ref(kind, a), f"{kind} in place, {name}, n = {n}")


def scan_misaligned(lib_path, kind):
    """the pointers one element behind a 16-byte boundary: whole tiles then take the element-wise loads / stores"""
    rng = np.random.default_rng(77)
    n = 2 * SCAN_TILE + 17
    a = list(scan_inputs(kind, n, rng).values())[-1]
    for mi in (0, 1):
        for mo in (0, 1):
            same(_capi.selftest_scan(kind, a, misalign_in=mi, misalign_out=mo, lib_path=lib_path), scan_ref(kind, a), f"{kind}, misaligned in {mi} out {mo}")
    same(_capi.selftest_scan(kind, a, in_place=True, misalign_in=1, lib_path=lib_path), scan_ref(kind, a), f"{kind}, misaligned in place")


# ---- radix sort ------------------------------------------------------------------------------------------------------------------
WINDOWS = ((0, 64), (0, 5), (0, 33), (1, 9), (7, 16), (8, 16), (13, 40), (40, 64), (56, 64), (63, 64), (61, 64), (58, 64), (52, 64))


def window_mask(b, e):
    return U64(((1 << (e - b)) - 1) << b)


def digits(keys, b, e):
    return (keys & window_mask(b, e)) >> U64(b)


def radix_ref(keys, vals, b, e):
    order = np.argsort(digits(keys, b, e), kind="stable")
    return keys[order], vals[order]


def rand_keys(n, rng):
    return rng.integers(0, 1 << 64, size=n, dtype=U64)


def key_shapes(n, b, e, rng):
    """name -> keys: every shape random over the bits OUTSIDE the window too (they must neither move nor steer the order)"""
    r = rand_keys(n, rng)
    outside = r & ~window_mask(b, e)
    span = (1 << (e - b)) - 1
    ramp = (np.arange(n, dtype=U64) * U64(max(span // max(n, 1), 1))) & U64(span)      # ascending inside the window (wraps where it is narrow)
    seven = rand_keys(7, rng)
    return {"uniform": r, "seven values": seven[rng.integers(0, 7, size=n)] if n else r,
            "sorted": outside | (np.sort(ramp) << U64(b)), "reverse sorted": outside | (np.sort(ramp)[::-1] << U64(b)),
            "equal inside the window": outside | (rand_keys(1, rng)[0] & window_mask(b, e))}


def check_radix(lib_path, keys, b, e, what, vals=None, **prep):
    vals = np.arange(keys.size, dtype=U32) if vals is None else vals      # the original index: stability is visible
    gk, gv = _capi.selftest_radix(keys, vals, b, e, lib_path=lib_path, **prep)
    wk, wv = radix_ref(keys, vals, b, e)
    same(gv, wv, f"radix values, {what}, n = {keys.size}, bits [{b}, {e})")
    same(gk, wk, f"radix keys, {what}, n = {keys.size}, bits [{b}, {e})")


def radix_window(lib_path, window, gpu):
    """one (begin_bit, end_bit) at sizes of one, two and three tiles (the device: 17 tiles + 1 and a million and three as well)"""
    b, e = window
    rng = np.random.default_rng(1000 + 64 * b + e)
    for n in (257, 2049, 4097) + ((17 * 2048 + 1, 1_000_003) if gpu else ()):
        for name, keys in key_shapes(n, b, e, rng).items():
            if n > 4097 and name not in ("uniform", "seven values"):
                continue
            check_radix(lib_path, keys, b, e, name)


def radix_one_size(lib_path, n, gpu):
    """all 64 bits (on the device; under the emulation up to 17 tiles + 1: eight passes over 129 tiles cost it seconds), one of the other
    windows in turn, and from the second look-back round on the pipeline's 64 - keep"""
    rng = np.random.default_rng(2000 + n % 1000)
    if gpu or n <= 17 * 2048 + 1:
        check_radix(lib_path, rand_keys(n, rng), 0, 64, "uniform")
    b, e = WINDOWS[1 + sizes(True).index(n) % (len(WINDOWS) - 1)]
    check_radix(lib_path, rand_keys(n, rng), b, e, "uniform")
    if n > 17 * 2048:
        for b, e in ((61, 64), (58, 64), (52, 64)):
            check_radix(lib_path, rand_keys(n, rng), b, e, "uniform")


def trivial_pass_keys(n, b, e, trivial, rng):
    """keys whose digit `p` (8 bits from begin_bit + 8 p, fewer in the last one) is the same in every key for p in `trivial`, random elsewhere"""
    keys = rand_keys(n, rng)
    for p in trivial:
        lo = b + 8 * p
        m = window_mask(lo, min(lo + 8, e))
        keys = (keys & ~m) | (rand_keys(1, rng)[0] & m)
    return keys


def radix_trivial_passes(lib_path, gpu):
    """exactly the first, a middle, the last, or every pass the identity, with odd and even numbers of passes: which of the two buffers the
    result ends in depends on all of them"""
    rng = np.random.default_rng(3)
    n = 100_003 if gpu else 4097
    for b, e in ((0, 64), (0, 33), (13, 40), (40, 64), (7, 16), (8, 16)):      # 8, 5, 4, 3, 2 and 1 passes
        passes = (e - b + 7) // 8
        for trivial in {(0,), (passes // 2,), (passes - 1,), tuple(range(passes)), tuple(range(1, passes)), tuple(range(passes - 1))}:
            check_radix(lib_path, trivial_pass_keys(n, b, e, trivial, rng), b, e, f"passes {trivial} of {passes} trivial")


def radix_i32_values(lib_path, gpu):
    rng = np.random.default_rng(4)
    for n in (1, 2, 2049, 4097) + ((1_000_003,) if gpu else ()):
        vals = (np.arange(n, dtype=np.int64) - n // 2).astype(np.int32)      # negative ones among them
        for b, e in ((0, 64), (58, 64), (13, 40)):
            keys = rand_keys(n, rng)
            gk, gv = _capi.selftest_radix(keys, vals, b, e, lib_path=lib_path)
            wk, wv = radix_ref(keys, vals, b, e)
            assert gv.dtype == np.int32
            same(gv, wv, f"radix i32 values, n = {n}, bits [{b}, {e})"); same(gk, wk, f"radix keys (i32 values), n = {n}, bits [{b}, {e})")


def radix_prepared_scratch(lib_path, gpu):
    rng = np.random.default_rng(5)
    for n in (2, 2049, 3 * 2048 + 5) + ((100_003,) if gpu else ()):
        for b, e in ((0, 64), (13, 40), (61, 64), (55, 64)):      # 8 passes, 4, and the 3-bit and 9-bit sorts
            bits = e - b
            preps = {"exact fit": dict(prep_n=n, prep_bits=bits), "three times n": dict(prep_n=3 * n, prep_bits=bits),
                     "too small in n": dict(prep_n=max(n // 2, 1), prep_bits=bits), "used by another sort before": dict(prep_n=n, prep_bits=bits, prep_reuse=True),
                     "three times n, used before": dict(prep_n=3 * n, prep_bits=max(bits, 32), prep_reuse=True)}
            if bits < 32:
                preps["prepared for 32 bits"] = dict(prep_n=n, prep_bits=32)
            if bits > 8:
                preps["too small in bits"] = dict(prep_n=n, prep_bits=8)
            for name, prep in preps.items():
                check_radix(lib_path, rand_keys(n, rng), b, e, f"prepared scratch: {name}", **prep)
                if name in ("exact fit", "used by another sort before"):
                    check_radix(lib_path, trivial_pass_keys(n, b, e, (0,), rng), b, e, f"prepared scratch: {name}, first pass trivial", **prep)


# ---- segmented reduce and arg-min ------------------------------------------------------------------------------------------------
def segment_shapes(n, rng):
    """name -> segment lengths that add up to n"""
    shapes = {"all of length one": [1] * n, "one segment": [n]}
    lens, left = [], n
    for cut in (255, 1, 1, 254, 1, 1):      # boundaries at 255, 256, 257 and at 511, 512, 513: on each side of a 256-thread block boundary
        if left >= cut:
            lens.append(cut); left -= cut
    while left:
        c = int(min(left, rng.integers(1, 600)))
        lens.append(c); left -= c
    shapes["random lengths"] = lens
    return shapes


def segments_ref(op, lens, vals):
    starts = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    if op == "min":
        return np.minimum.reduceat(vals, starts).astype(U64)
    ids = np.repeat(np.arange(len(lens)), lens)
    return np.lexsort((np.arange(vals.size), vals, ids))[starts].astype(U32)      # per segment the smallest value, the lowest index among equals


def segments(lib_path, op, gpu):
    rng = np.random.default_rng(6 + (op == "min"))
    for n in (1, 255, 256, 257, 1000, 5003) + ((100_003,) if gpu else ()):
        for name, lens in segment_shapes(n, rng).items():
            for vals in (rand_keys(n, rng), rng.integers(0, 4, size=n, dtype=U64)):      # full range; ties everywhere
                want = segments_ref(op, lens, vals)
                for first_id in (0, 7, 0xFFF00000):
                    seg = (np.repeat(np.arange(len(lens), dtype=U64), lens) + U64(first_id)).astype(U32)
                    for deferred in (False, True):
                        got, err = _capi.selftest_segments(op, seg, vals, len(lens), deferred_err=deferred, lib_path=lib_path)
                        same(got, want, f"segment {op}, {name}, n = {n}, first id {first_id}, deferred {deferred}")
                        assert err == 0, (op, name, n, err)


def segments_count_mismatch(lib_path, op):
    """an n_segments that disagrees with the data: bit 128 of the error word in the deferred form, an error return in the immediate one"""
    import pytest
    rng = np.random.default_rng(8)
    lens = segment_shapes(1500, rng)["random lengths"]
    seg = np.repeat(np.arange(len(lens), dtype=U32), lens)
    vals = rand_keys(1500, rng)
    want = segments_ref(op, lens, vals)
    for wrong in (len(lens) + 1, len(lens) - 1):
        got, err = _capi.selftest_segments(op, seg, vals, wrong, deferred_err=True, lib_path=lib_path)
        assert err & 128, (op, wrong, err)
        m = min(wrong, len(lens))
        same(got[:m], want[:m], f"segment {op} with a wrong count {wrong}: the segments that fit")      # (and nothing written past the end: the hook's buffer has `wrong` entries)
        assert (got[m:] == np.iinfo(got.dtype).max).all()
        with pytest.raises(_capi.AutocyclerError, match="segment count mismatch"):
            _capi.selftest_segments(op, seg, vals, wrong, deferred_err=False, lib_path=lib_path)
    assert _capi.selftest_segments(op, seg, vals, len(lens), deferred_err=True, lib_path=lib_path)[1] == 0


# ---- comparator sorts ------------------------------------------------------------------------------------------------------------
CMP_SIZES = (0, 1, 2, 3, 1000, 1024, 1025, 4097)      # not a power of two; just above one: the last merge pair's right run is empty


def sort_pairs_cmp(lib_path, gpu):
    rng = np.random.default_rng(9)
    for n in CMP_SIZES + ((65_537, 100_003) if gpu else ()):
        a = rng.integers(0, 5, size=n, dtype=U64) * U64(0x0123456789ABCDEF)      # duplicate-heavy in both fields
        b = rng.integers(0, 3, size=n, dtype=U64).astype(U32) * U32(0x80000001)
        vals = np.arange(n, dtype=U32)
        order = np.array(sorted(range(n), key=lambda i: (int(a[i]), int(b[i]))), dtype=np.int64)      # Python's sort is stable
        ga, gb, gv = _capi.selftest_sort_pairs_cmp(a, b, vals, lib_path=lib_path)
        same(gv, vals[order], f"sort_by_key_cmp payload, n = {n}"); same(ga, a[order], f"sort_by_key_cmp field a, n = {n}"); same(gb, b[order], f"sort_by_key_cmp field b, n = {n}")


def sort_indices_cmp(lib_path, gpu):
    rng = np.random.default_rng(10)
    for n in CMP_SIZES + ((65_537, 100_003) if gpu else ()):
        values = rng.integers(0, 9, size=n, dtype=U64) << U64(40)
        idx = rng.permutation(n).astype(U32)
        want = np.array(sorted(idx.tolist(), key=lambda i: int(values[i])), dtype=U32)
        same(_capi.selftest_sort_indices_cmp(values, idx, lib_path=lib_path), want, f"sort_keys_cmp, n = {n}")


# ---- the scan state pool ---------------------------------------------------------------------------------------------------------
def pool_epoch_wrap(lib_path):
    rng = np.random.default_rng(11)
    tiles = 70
    tiny = np.arange(5, dtype=U32)
    _capi.selftest_scan("excl_add_u32", tiny, lib_path=lib_path)      # (the pool exists from its first scan on; one that a failed call left invalidated starts over here)
    while _capi.selftest_scan_pool("read", lib_path=lib_path)["epoch"] >= (1 << 16) - 3:
        _capi.selftest_scan("excl_add_u32", tiny, lib_path=lib_path)
    before = _capi.selftest_scan_pool("read", lib_path=lib_path)
    at = _capi.selftest_scan_pool("advance", (1 << 16) - 3, lib_path=lib_path)
    assert at["epoch"] == (1 << 16) - 3 and at["cap"] == before["cap"]
    kinds = list(_capi.SCAN_KINDS)
    for i in range(6):
        kind = kinds[i % 4]
        n = tiles * SCAN_TILE - i      # (70 tiles each, different data)
        a = list(scan_inputs(kind, n, rng).values())[-1]
        same(_capi.selftest_scan(kind, a, lib_path=lib_path), scan_ref(kind, a), f"scan {i} across the epoch wrap ({kind})")
    after = _capi.selftest_scan_pool("read", lib_path=lib_path)
    # epochs 2^16 - 2 and 2^16 - 1, then the wrap: the third scan got epoch 1 of a cleared pool, the sixth epoch 4, and the tickets are theirs alone
    assert after["epoch"] == 4 and after["tickets"] == 4 * tiles and after["cap"] == before["cap"], after


def pool_invalidate(lib_path):
    rng = np.random.default_rng(12)
    a = list(scan_inputs("incl_add_u32", 3 * SCAN_TILE, rng).values())[-1]
    same(_capi.selftest_scan("incl_add_u32", a, lib_path=lib_path), scan_ref("incl_add_u32", a), "scan before invalidate()")
    assert _capi.selftest_scan_pool("invalidate", lib_path=lib_path)["epoch"] >= 1 << 16
    for kind, tiles in (("incl_max_u32", 7), ("excl_add_u64", 2)):
        a = list(scan_inputs(kind, tiles * SCAN_TILE - 9, rng).values())[-1]
        same(_capi.selftest_scan(kind, a, lib_path=lib_path), scan_ref(kind, a), f"scan after invalidate() ({kind})")
    after = _capi.selftest_scan_pool("read", lib_path=lib_path)
    assert after["epoch"] == 2 and after["tickets"] == 9, after


def pool_growth(lib_path):
    """(the device only: 16.7 M items) more tiles than the pool has words: a new, cleared pool; then a small scan in the grown pool"""
    import time
    rng = np.random.default_rng(13)
    cap = _capi.selftest_scan_pool("read", lib_path=lib_path)["cap"]
    n = SCAN_TILE * SCAN_TILE + 1
    assert cap < n // SCAN_TILE + 2, "the pool already holds a scan of this size"
    a = rng.integers(0, 1 << 32, size=n, dtype=U64).astype(U32)
    t0 = time.perf_counter()
    got = _capi.selftest_scan("excl_add_u32", a, lib_path=lib_path)
    print(f"growth scan of {n} items (copies included): {time.perf_counter() - t0:.3f} s")
    same(got, scan_ref("excl_add_u32", a), "the scan that grows the pool")
    b = np.array([5, 4, 3, 2, 1], dtype=U32)
    same(_capi.selftest_scan("excl_add_u32", b, lib_path=lib_path), scan_ref("excl_add_u32", b), "five items in the grown pool")
    assert _capi.selftest_scan_pool("read", lib_path=lib_path)["cap"] > cap


# ---- the wave layer --------------------------------------------------------------------------------------------------------------
# A plain model of what wave_rt.hpp documents: a ballot has the bits of the live lanes whose predicate holds; a shfl source is taken modulo
# the width; shfl_up / shfl_down / shfl_xor out of range give the lane's own value; the grp_* forms see only their G lanes; a returned lane
# takes part in nothing.  What a shuffle reads from a lane that has RETURNED is model(...)[1], see RETURNED_LANE_READS.
(WP_BALLOT, WP_ALL, WP_UNIFORM, WP_SHFL, WP_SHFL64, WP_SHFL_XOR, WP_SHFL_XOR64, WP_SHFL_UP, WP_SHFL_DOWN, WP_GRP_BALLOT16, WP_GRP_SHFL16,
 WP_GRP_BALLOT64, WP_GRP_SHFL64, WP_BLOCK_SYNC, WP_SHFL_UP_1, WP_SHFL_DOWN_1, WP_SHFL_XOR_1, WP_SHFL_XOR_32, WP_SHFL_XOR64_16, WP_SHFL_UP_16,
 WP_SHFL_DOWN_32) = range(21)      # WaveProgram, csrc/selftest_prims.inc
PROGRAM_NAMES = ("ballot", "all", "uniform", "shfl", "shfl64", "shfl_xor", "shfl_xor64", "shfl_up", "shfl_down", "grp_ballot<16>", "grp_shfl<16>",
                 "grp_ballot<64>", "grp_shfl<64>", "block_sync", "shfl_up by constant 1", "shfl_down by constant 1", "shfl_xor by constant 1",
                 "shfl_xor by constant 32", "shfl_xor64 by constant 16", "shfl_up by constant 16", "shfl_down by constant 32")
CONSTANT_FORMS = {WP_SHFL_UP_1: (WP_SHFL_UP, 1), WP_SHFL_DOWN_1: (WP_SHFL_DOWN, 1), WP_SHFL_XOR_1: (WP_SHFL_XOR, 1), WP_SHFL_XOR_32: (WP_SHFL_XOR, 32),
                  WP_SHFL_XOR64_16: (WP_SHFL_XOR64, 16), WP_SHFL_UP_16: (WP_SHFL_UP, 16), WP_SHFL_DOWN_32: (WP_SHFL_DOWN, 32)}
M64 = (1 << 64) - 1
OUT_INIT = [0xDEAD000000000000 + t for t in range(256)]
WAVE_IN = [(((0xA0000000 + 0x10001 * t) << 32) | (0x50000000 + 7 * t + ((t * t) << 12))) & M64 for t in range(256)]      # high and low words differ, all distinct
RETURNED_LANE_READS = 0      # what a shuffle whose source lane has returned delivers: measured on the MI355X for every program below, the
                             # constant distances included, and what the emulation answers


def _each_wave(pattern):
    return [pattern & M64] * 4


LIVE_MASKS = {"all lanes live": _each_wave(M64), "one lane group of 16 returned": _each_wave(M64 & ~(0xFFFF << 16)),
              "alternate lanes returned": _each_wave(0x5555555555555555), "lane 0 returned": _each_wave(M64 & ~1),
              "lanes 32 to 63 returned": _each_wave(0xFFFFFFFF), "one whole wavefront returned": [M64, M64, 0, M64]}


def model(program, inp, aux, live_mask):
    """-> (out[256], from_returned[256]): out_u64 as documented, with RETURNED_LANE_READS where a shuffle's source lane has returned;
    from_returned marks those entries"""
    live = [bool((live_mask[t >> 6] >> (t & 63)) & 1) for t in range(256)]
    out, flagged = list(OUT_INIT), [False] * 256
    if program in CONSTANT_FORMS:
        program, d = CONSTANT_FORMS[program]
        aux = [d] * 256
    lo = lambda x: x & M32
    wide = program in (WP_SHFL64, WP_SHFL_XOR64)
    if program == WP_BLOCK_SYNC:
        s1 = [inp[t] if live[t] else inp[t] ^ M64 for t in range(256)]
        x = [s1[(t + aux[0]) & 255] for t in range(256)]
        s2 = [(x[t] + 1) & M64 if live[t] else s1[t] for t in range(256)]
        for t in range(256):
            if live[t]:
                out[t] = (x[t] + 3 * s2[(t + 2 * aux[0]) & 255]) & M64
        return out, flagged
    for t in range(256):
        if not live[t]:
            continue
        w0, l = t & ~63, t & 63
        if program in (WP_BALLOT, WP_GRP_BALLOT64):
            out[t] = sum(1 << i for i in range(64) if live[w0 + i] and aux[w0 + i] & 1)
        elif program == WP_GRP_BALLOT16:
            g0 = w0 + (l & ~15)
            out[t] = sum(1 << i for i in range(16) if live[g0 + i] and aux[g0 + i] & 1)
        elif program == WP_ALL:
            out[t] = int(all(aux[w0 + i] & 1 for i in range(64) if live[w0 + i]))
        elif program == WP_UNIFORM:
            out[t] = lo(inp[next(w0 + i for i in range(64) if live[w0 + i])])
        else:
            if program in (WP_SHFL, WP_SHFL64, WP_GRP_SHFL64):
                src = w0 + aux[t] % 64      # (Python's %: never negative)
            elif program == WP_GRP_SHFL16:
                src = w0 + (l & ~15) + aux[t] % 16
            elif program in (WP_SHFL_XOR, WP_SHFL_XOR64):
                s = l ^ aux[0]
                src = w0 + s if 0 <= s < 64 else t
            elif program == WP_SHFL_UP:
                src = t - aux[0] if l - aux[0] >= 0 else t
            elif program == WP_SHFL_DOWN:
                src = t + aux[0] if l + aux[0] < 64 else t
            else:
                raise ValueError(program)
            if live[src]:
                out[t] = inp[src] if wide else lo(inp[src])
            else:
                out[t], flagged[t] = RETURNED_LANE_READS, True
    return out, flagged


def wave_aux_sets(program, rng):
    """the aux arrays one program is run with"""
    if program in (WP_BALLOT, WP_ALL, WP_GRP_BALLOT16, WP_GRP_BALLOT64):
        return [[1] * 256, [0] * 256, [int(x) for x in rng.integers(0, 2, size=256)], [int(t % 64 != 37) for t in range(256)], [int(t % 16 == 3) for t in range(256)]]
    if program in (WP_SHFL, WP_SHFL64, WP_GRP_SHFL16, WP_GRP_SHFL64):      # negative sources and sources >= 64 among them
        return [[int(x) for x in rng.integers(-70, 140, size=256)], [0] * 256, [63 - (t & 63) for t in range(256)], [(t & 63) + 64 for t in range(256)], [-1 - (t & 7) for t in range(256)]]
    if program in (WP_SHFL_XOR, WP_SHFL_XOR64):
        return [[m] * 256 for m in (0, 1, 2, 4, 8, 16, 32, 5, 63, 64)]
    if program in (WP_SHFL_UP, WP_SHFL_DOWN):
        return [[d] * 256 for d in range(65)]
    if program == WP_BLOCK_SYNC:
        return [[d] * 256 for d in (0, 1, 64, 65, 128, 191, 255)]
    return [[0] * 256]      # the constant forms take nothing


def wave_program(lib_path, program):
    """one program under every live mask: the library's result == the model's, entry by entry"""
    rng = np.random.default_rng(100 + program)
    for mask_name, mask in LIVE_MASKS.items():
        for aux in wave_aux_sets(program, rng):
            want, _ = model(program, WAVE_IN, aux, mask)
            got = _capi.selftest_wave(program, WAVE_IN, aux, mask, OUT_INIT, lib_path=lib_path)
            same(got, np.array(want, dtype=U64), f"{PROGRAM_NAMES[program]}, {mask_name}, aux[0..3] = {aux[:4]}")
