"""The device runtime (csrc/device_rt.hpp) facility by facility, through the data-in / data-out hooks of csrc/selftest_runtime.inc: the arena,
the fused fills, the read-backs, the launchers, the atomic wrappers with wave_alloc32 / wave_add64, the side stream and its event ring.  Every
expected value is plain numpy / Python integer code, every comparison exact equality.

lib_path = None: the product library (the MI355X); otherwise the CPU emulation's, where a fill is a memset, a read-back a memcpy and an atomic a
plain read-modify-write: there the cases pin the hooks and the models, and the arena and the ring's bookkeeping, which are the same code."""
import os

import numpy as np

from autocycler_amd import _capi
from prim_cases import same

U8, U32, U64 = np.uint8, np.uint32, np.uint64
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
FILL_MAX = 16                       # device_rt.hpp: fills per fused launch
MAIL_CAP = 64 << 10                 # Mailbox::CAP
MAIL_MAX_ITEMS = 6
N_EV = 64                           # SideStream::N_EV
MAX_LAUNCH_BLOCKS = 1 << 23
T = _capi.ATOMIC_THREADS


def on_device(lib_path):
    return lib_path is None


def mailbox_on():
    return os.environ.get("AC_NO_MAILBOX") is None


def round256(b):
    return max(256, (b + 255) & ~255)


# ---- 1. fused fills ----------------------------------------------------------------------------------------------------------------------
FILL_SIZES = (1, 15, 16, 17, 255, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 5, (1 << 20) + 3)      # the 16-byte vector, the 4096-byte lane stride, the 16 KB tile
FILL_BYTES = (0x00, 0xFF, 0x5A)
REGION_COUNTS = (1, 15, 16, 17, 33, 40)      # FILL_MAX = 16: zero, one and two forced flushes


def fill_args(n):
    return [a for a in (0, 1, 15, 16, 17, n - 1, n, n + 1) if a >= 0]


def pattern(n):
    i = np.arange(n, dtype=U64)
    return ((i * U64(131) + (i >> U64(8)) * U64(7) + U64(13)) & U64(0xFF)).astype(U8)


def fills_model(regions, pat):
    """-> (the span after the fills, the number of fills that went into the queue of stream 0)"""
    out = pat.copy()
    off, queued = 256, 0
    for n, kind, arg, byte in regions:
        lo, hi = 0, n
        if kind == "from":
            lo = arg & ~15
        elif kind == "first":
            hi = min(n, arg)
        if lo < hi:
            out[off + lo:off + hi] = byte
            queued += kind != "side_stream"
        off += round256(n) + 256
    assert off == out.size
    return out, queued


def span_bytes(regions):
    return 256 + sum(round256(r[0]) + 256 for r in regions)


def run_fills(lib_path, regions, trigger, own_launches=0, drop=False, expect_queued=None):
    pat = pattern(span_bytes(regions))
    got, (l_queue, l_trigger) = _capi.selftest_fills(regions, trigger, pat, drop_on_reset=drop, lib_path=lib_path)
    want, queued = fills_model(regions, pat)
    assert expect_queued is None or queued == expect_queued, (queued, expect_queued)
    same(got, pat if drop else want, f"{len(regions)} regions, trigger {trigger}{', dropped' if drop else ''}")
    if on_device(lib_path):      # (the emulation fills at once and counts no launches)
        forced = (queued - 1) // FILL_MAX if queued else 0
        pending = queued - forced * FILL_MAX
        assert l_queue == forced, (l_queue, forced)
        if drop:
            assert l_trigger == forced, "a dropped fill was launched"
        else:
            assert l_trigger == forced + (1 if pending and trigger != "none" else 0) + own_launches, (trigger, l_trigger, forced, pending, own_launches)


def mixed_regions(count, sizes, kinds=("all", "from", "first")):
    out = []
    for i in range(count):
        n = sizes[i % len(sizes)]
        kind = kinds[i % len(kinds)]
        args = [a for a in fill_args(n) if (kind == "from" and (a & ~15) < n) or (kind == "first" and a > 0)] or [0]      # (no empty fill: it would not enter the queue)
        arg = args[(i // len(kinds)) % len(args)]
        out.append((n, kind, arg, FILL_BYTES[(i + i // 3) % 3]))
    return out


def fill_every_size(lib_path, kind):
    if kind in ("all", "side_stream"):
        regions = [(n, kind, 0, FILL_BYTES[i % 3]) for i, n in enumerate(FILL_SIZES)]
    else:
        regions = [(n, kind, a, FILL_BYTES[(i + j) % 3]) for i, n in enumerate(FILL_SIZES) for j, a in enumerate(fill_args(n))]
    run_fills(lib_path, regions, "none")
    run_fills(lib_path, list(reversed(regions)), "stream_sync")


def fill_region_count(lib_path, count):
    run_fills(lib_path, mixed_regions(count, FILL_SIZES), "none", expect_queued=count)
    run_fills(lib_path, mixed_regions(count, FILL_SIZES[:-1]), "stream_sync", expect_queued=count)


def trigger_launches(trigger):
    """the launches the trigger itself counts (besides the flush)"""
    if trigger in ("launch", "launch_full", "launch_wave_kernel"):
        return 1
    return 1 if trigger == "copy_d2h" and mailbox_on() else 0      # (256 bytes: the mailbox's publishing kernel)


def fill_trigger(lib_path, trigger):
    sizes = FILL_SIZES[:-2]
    run_fills(lib_path, mixed_regions(17, sizes), trigger, trigger_launches(trigger))      # one forced flush, one fill pending
    run_fills(lib_path, mixed_regions(3, sizes, kinds=("side_stream", "all", "side_stream")), trigger, trigger_launches(trigger))
    if trigger != "none":      # nothing queued on stream 0: the trigger launches nothing for the fills
        run_fills(lib_path, [(4097, "side_stream", 0, 0x5A), (17, "from", 33, 0xFF), (15, "first", 0, 0x00)], trigger, trigger_launches(trigger))


def fill_drop_on_reset(lib_path):
    for count in (1, 16, 17, 33):
        run_fills(lib_path, mixed_regions(count, FILL_SIZES[:-1], kinds=("all", "from", "first", "side_stream")), "none", drop=True)


ORDER_CASES = (      # n, byte1, w_lo, w_hi, w_val, from2, byte2, upto3, byte3
    (4097, 0xFF, 100, 3000, 0x11, 2049, 0x5A, 50, 0x00),
    (16385, 0x00, 0, 16385, 0x22, 16384, 0xFF, 17, 0x5A),
    (3 * 16384 + 5, 0x5A, 16383, 16401, 0x33, 16390, 0x00, 16384, 0xFF),
    (17, 0xFF, 1, 16, 0x44, 16, 0x00, 1, 0x5A),
)


def fill_order(lib_path):
    for n, b1, lo, hi, wv, f2, b2, u3, b3 in ORDER_CASES:
        want = np.full(n, b1, dtype=U8)
        want[lo:hi] = wv
        want[f2 & ~15:] = b2
        want[:min(n, u3)] = b3
        same(_capi.selftest_fill_order(n, b1, lo, hi, wv, f2, b2, u3, b3, lib_path=lib_path), want, f"fill order, n = {n}")


# ---- 2. read-backs -----------------------------------------------------------------------------------------------------------------------
D2H_SIZES = (1, 2, 3, 4, 5, 7, 8, 12, 63, 64, 65, 4096, 65535, 65536, 65537, 65536 + 4096)
MISALIGN = (0, 1, 2, 4, 8)
BATCH_SIZES = (1, 63, 64, 65, 200, 4096)
N_DATA = 400_000
_DATA = None


def data():
    global _DATA
    if _DATA is None:
        _DATA = np.random.default_rng(8101).integers(0, 256, size=N_DATA, dtype=U8)
        _DATA.setflags(write=False)
    return _DATA


def fetch_counts(nbytes, items=1):
    """(launches, read-backs) of one fetch: the mailbox publishes with one kernel; the scratch page and the plain copy launch nothing"""
    if nbytes == 0:
        return 0, 0
    if mailbox_on() and nbytes <= MAIL_CAP and items <= MAIL_MAX_ITEMS:
        return 1, 1
    return 0, 1


def check_items(lib_path, path, items, counts, what):
    got, launches, readbacks = _capi.selftest_readback(data(), path, items, lib_path=lib_path)
    for (off, n), g in zip(items, got):
        same(g, data()[off:off + n], f"{what}: item ({off}, {n}) by {path}")
    if on_device(lib_path):
        assert (launches, readbacks) == counts, (what, path, launches, readbacks, counts)


def spread(i, n, mis):
    """a 256-aligned offset that differs from item to item, plus the misalignment"""
    return ((i * 7919 * 256) % (N_DATA - n - 512)) // 256 * 256 + mis


def d2h_single(lib_path, path="copy_d2h"):
    items = [(spread(i * 5 + j, n, mis), n) for i, n in enumerate(D2H_SIZES) for j, mis in enumerate(MISALIGN)]
    counts = tuple(sum(c) for c in zip(*(fetch_counts(n) for _, n in items)))
    check_items(lib_path, path, items, counts, "every size at every misalignment")


def padded(n):
    return (n + 63) & ~63


def batch_cases():
    pairs = [(a, b) for a in BATCH_SIZES for b in BATCH_SIZES]      # each size behind each
    flat = [n for p in pairs for n in p]
    cases = {f"sizes {flat[i:i + 6]}": flat[i:i + 6] for i in range(0, len(flat), 6)}
    cases["one item"] = [65]
    cases["six items"] = [63, 1, 65, 64, 200, 4096]
    cases["seven items"] = [63, 1, 65, 64, 200, 4096, 63]
    cases["padded total = CAP"] = [MAIL_CAP - 4096 - 64, 4096, 63]
    cases["padded total = CAP + 64"] = [MAIL_CAP - 4096 - 64, 4096, 65]
    cases["an add of zero bytes"] = [65, 0, 63, 0]
    cases["nothing but zero bytes"] = [0, 0]
    return cases


def batch(lib_path):
    for name, sizes in batch_cases().items():
        items = [(spread(3 * i + len(sizes), n, (1, 0, 8, 4, 2, 0, 1)[i % 7]), n) for i, n in enumerate(sizes)]
        real = [n for n in sizes if n]
        total = sum(padded(n) for n in real)
        counts = (0, 0) if not real else (1, 1) if mailbox_on() and total <= MAIL_CAP and len(real) <= MAIL_MAX_ITEMS else (0, 1)
        check_items(lib_path, "batch", items, counts, name)


def batch_run_twice(lib_path):
    sizes = [65, 63, 4096, 1, 200, 64, 64, 65]
    items = [(spread(11 * i, n, i % 3), n) for i, n in enumerate(sizes)]
    one = (1, 1) if mailbox_on() else (0, 1)
    check_items(lib_path, "batch_twice", items, (2 * one[0], 2 * one[1]), "one ReadBatch, run twice")


def large_then_small(lib_path):
    for first in (MAIL_CAP, MAIL_CAP + 4096):
        items = [(0, first), (first + 1024, 100), (200_001, 7), (100_000, 64)]
        counts = tuple(sum(c) for c in zip(*(fetch_counts(n) for _, n in items)))
        check_items(lib_path, "copy_d2h", items, counts, "a large fetch, then smaller ones of other content")
        check_items(lib_path, "to_host", items, counts, "a large fetch, then smaller ones of other content")


def scalars(lib_path):
    items = [(8 * i, 8 if i % 2 else 4) for i in range(40)]
    one = fetch_counts(8)
    check_items(lib_path, "read_scalar", items, (40 * one[0], 40 * one[1]), "read_scalar")


def scalar_chain(lib_path):
    values = np.random.default_rng(8102).integers(0, 1 << 63, size=300, dtype=U64) * U64(2) + U64(1)
    got, launches, readbacks = _capi.selftest_scalar_chain(values, lib_path=lib_path)
    same(got, values, "300 scalar fetches, each behind a launch that wrote a new value")
    if on_device(lib_path):
        one = fetch_counts(8)
        assert (launches, readbacks) == (300 + 300 * one[0], 300 * one[1]), (launches, readbacks)


def side_stream_fetch(lib_path):
    items = [(spread(1, 4096, 4), 4096), (spread(2, 65537, 1), 65537), (spread(3, 7, 0), 7)]
    counts = tuple(sum(c) for c in zip(*(fetch_counts(n) for _, n in items)))
    check_items(lib_path, "side_stream", items, counts, "fetches on the side stream behind after_main")


def readback_all(lib_path):
    """the whole list: what the two child processes of the GPU suite run with the mailbox and the scratch page switched off"""
    d2h_single(lib_path); d2h_single(lib_path, "to_host")
    batch(lib_path); batch_run_twice(lib_path); large_then_small(lib_path); scalars(lib_path); scalar_chain(lib_path); side_stream_fetch(lib_path)


def readback_bad_arguments(lib_path):
    for path, items in (("copy_d2h", [(N_DATA - 4, 5)]), ("read_scalar", [(4, 8)]), ("read_scalar", [(0, 2)])):
        try:
            _capi.selftest_readback(data(), path, items, lib_path=lib_path)
        except Exception as e:
            assert "selftest readback" in str(e), e
        else:
            raise AssertionError(f"{path} {items} was not refused")


# ---- 3. the arena ------------------------------------------------------------------------------------------------------------------------
MB = 1 << 20
COALESCE_SLACK = 256 << 20


class ArenaModel:
    """Arena of device_rt.hpp restated: 256-byte rounding (zero bytes take 256), first fit forwards from the current block, a new block of
    max(bytes, grow), rewind empties all later blocks, a mark on an empty arena rewinds to nothing, reset coalesces only more than one block."""

    def __init__(self):
        self.blocks = []      # [cap, used]
        self.grow = 64 * MB
        self.peak = 0
        self.cur = 0
        self.live = []        # per allocation: (block identity, offset, bytes) or None once dead
        self.ids = []         # identity of each block (a coalesce / release makes new ones)
        self.next_id = 0
        self.marks = []

    def used(self):
        return sum(b[1] for b in self.blocks)

    def cap(self):
        return sum(b[0] for b in self.blocks)

    def new_block(self, cap):
        self.blocks.append([cap, 0]); self.ids.append(self.next_id); self.next_id += 1

    def kill(self, pred):
        self.live = [None if a is not None and pred(a) else a for a in self.live]

    def apply(self, op, arg):
        """-> (block ordinal, offset) for an alloc, else None"""
        placed = None
        if op == "alloc":
            b = round256(arg)
            i = self.cur
            while i < len(self.blocks) and self.blocks[i][1] + b > self.blocks[i][0]:
                i += 1
            if i == len(self.blocks):
                self.new_block(max(b, self.grow))
            self.cur = i
            placed = (i, self.blocks[i][1])
            self.live.append((self.ids[i], self.blocks[i][1], b))
            self.blocks[i][1] += b
            self.peak = max(self.peak, self.used())
        elif op == "mark":
            self.marks.append(None if not self.blocks else (self.cur, self.blocks[self.cur][1]))
        elif op == "rewind":
            m = self.marks[arg]
            if self.blocks:
                self.cur, keep = (0, 0) if m is None else m
                self.blocks[self.cur][1] = keep
                for b in self.blocks[self.cur + 1:]:
                    b[1] = 0
                order = {bid: i for i, bid in enumerate(self.ids)}
                self.kill(lambda a: order[a[0]] > self.cur or (order[a[0]] == self.cur and a[1] >= keep))
        elif op == "reset":
            last_peak, total = self.peak, self.cap()
            self.peak = self.cur = 0
            self.kill(lambda a: True)
            if len(self.blocks) > 1:
                if last_peak:
                    total = min(total, last_peak + last_peak // 8 + COALESCE_SLACK)
                self.blocks, self.ids = [], []
                self.new_block(total)
            else:
                for b in self.blocks:
                    b[1] = 0
        elif op == "reserve":
            if not (self.cap() >= arg or self.used() != 0):
                self.blocks, self.ids, self.cur = [], [], 0
                self.new_block(arg)
        elif op == "release_all":
            self.kill(lambda a: True)
            self.blocks, self.ids, self.cur = [], [], 0
        elif op == "set_grow":
            self.grow = arg
        else:
            raise ValueError(op)
        return placed


def arena_program(lib_path, ops, what):
    m = ArenaModel()
    want_totals, want_place = [], []
    for op, arg in ops:
        p = m.apply(op, arg)
        if p is not None:
            want_place.append(p)
        want_totals.append((m.cap(), m.used(), m.peak))
    live = [a is not None for a in m.live]
    totals, allocs, wrong = _capi.selftest_arena(ops, live, lib_path=lib_path)
    same(totals.ravel(), np.array(want_totals, dtype=U64).ravel(), f"{what}: capacity / used / peak after every op (three numbers each)")
    same(allocs[:, :2].ravel(), np.array(want_place, dtype=U64).ravel(), f"{what}: block and offset of every allocation (two numbers each)")
    sizes = [round256(arg) for op, arg in ops if op == "alloc"]
    spans = sorted((int(allocs[i, 2]), int(allocs[i, 2]) + sizes[i], i) for i in range(len(sizes)) if live[i])
    for (lo0, hi0, i0), (lo1, hi1, i1) in zip(spans, spans[1:]):
        assert hi0 <= lo1, f"{what}: live allocations {i0} and {i1} overlap"
    for i, is_live in enumerate(live):
        assert wrong[i] == (0 if is_live else -1), f"{what}: allocation {i} lost {wrong[i]} of its bytes"
    return m


ARENA_PROGRAMS = {
    "a request larger than grow": [("set_grow", MB), ("alloc", 1), ("alloc", 5 * MB), ("alloc", 0), ("alloc", MB - 512), ("alloc", 257)],
    "rewind two blocks back, then a request that skips a block": [
        ("set_grow", MB), ("alloc", 1000), ("mark", 0), ("alloc", MB), ("alloc", 3 * MB), ("alloc", 600_000), ("alloc", 600_000), ("rewind", 0),
        ("alloc", 100), ("alloc", 2 * MB), ("alloc", 900_000), ("alloc", 5 * MB), ("alloc", 3 * MB)],
    "rewind to an empty-arena mark": [("set_grow", MB), ("mark", 0), ("alloc", 300), ("alloc", 2 * MB), ("rewind", 0), ("alloc", 2 * MB), ("alloc", 5), ("mark", 0),
                                      ("alloc", MB), ("rewind", 1), ("alloc", 256), ("rewind", 0), ("alloc", 7)],
    "nested marks rewound innermost first": [("set_grow", MB), ("alloc", 10), ("mark", 0), ("alloc", 700_000), ("mark", 0), ("alloc", 700_000), ("mark", 0), ("alloc", 4 * MB),
                                             ("rewind", 2), ("alloc", 100_000), ("rewind", 1), ("alloc", 500_000), ("rewind", 0), ("alloc", MB), ("alloc", 1)],
    "reset with one block": [("set_grow", MB), ("alloc", 5000), ("alloc", 70_000), ("reset", 0), ("alloc", 300), ("alloc", MB)],
    "reset with three blocks": [("set_grow", MB), ("alloc", 900_000), ("alloc", 900_000), ("alloc", 2 * MB), ("reset", 0), ("alloc", 3 * MB), ("alloc", 900_000),
                                ("alloc", 1), ("reset", 0), ("alloc", 12)],
    "reserve on a used arena and on a fresh one": [("set_grow", MB), ("reserve", 3 * MB), ("alloc", 2 * MB), ("reserve", 8 * MB), ("alloc", 2 * MB), ("release_all", 0),
                                                   ("reserve", 300), ("reserve", 200), ("alloc", 200), ("alloc", 200), ("reset", 0), ("reserve", 4 * MB), ("alloc", 3 * MB)],
}


def random_arena_program(seed):
    rng = np.random.default_rng(seed)
    ops, marks, total = [("set_grow", MB)], 0, 0
    for _ in range(int(rng.integers(5, 40))):
        r = rng.random()
        if r < 0.55 and total < 40 * MB:
            c = rng.random()
            b = int(rng.integers(0, 65536)) if c < 0.7 else int(rng.integers(65536, MB + 4096)) if c < 0.95 else int(rng.integers(MB, 5 * MB + 1))
            ops.append(("alloc", b)); total += b
        elif r < 0.70:
            ops.append(("mark", 0)); marks += 1
        elif r < 0.85 and marks:
            ops.append(("rewind", int(rng.integers(0, marks))))
        elif r < 0.90:
            ops.append(("reset", 0))
        elif r < 0.94:
            ops.append(("reserve", int(rng.integers(1, 6 * MB))))
        elif r < 0.96:
            ops.append(("release_all", 0))
        else:
            ops.append(("set_grow", int(rng.integers(1, 4)) * MB // 2))
    return ops


def marks_stay_valid(ops):
    """Marks are a stack: a rewind ends the life of every mark taken after the one it goes back to, and a reset / release / reserve that of all
    of them (the blocks they name may be gone).  The runtime's callers never rewind to a dead mark, nor do the random programs."""
    out, valid = [], []
    for op, arg in ops:
        if op == "mark":
            valid.append(True)
        elif op in ("reset", "release_all", "reserve"):
            valid = [False] * len(valid)
        elif op == "rewind" and not valid[arg]:
            continue
        elif op == "rewind":
            valid[arg + 1:] = [False] * (len(valid) - arg - 1)
        out.append((op, arg))
    return out


def arena_random(lib_path, seeds):
    for seed in seeds:
        arena_program(lib_path, marks_stay_valid(random_arena_program(seed)), f"random program {seed}")


def arena_bad_arguments(lib_path):
    for ops in ([("rewind", 0)], [("mark", 0), ("rewind", 1)], [("alloc", 65 * MB)], [("set_grow", 0)]):
        try:
            _capi.selftest_arena(ops, [False] * sum(o == "alloc" for o, _ in ops), lib_path=lib_path)
        except Exception as e:
            assert "selftest arena" in str(e), e
        else:
            raise AssertionError(f"{ops} was not refused")
    try:      # an allocation the arena has rewound over is not read, whatever the caller says
        _capi.selftest_arena([("mark", 0), ("alloc", 100), ("rewind", 0)], [True], lib_path=lib_path)
    except Exception as e:
        assert "is not live" in str(e), e
    else:
        raise AssertionError("a dead allocation was read")


# ---- 4. the launchers --------------------------------------------------------------------------------------------------------------------
LAUNCH_SIZES = (0, 1, 63, 64, 255, 256, 257, 65_537)
LAUNCH_BIG = (1 << 31) + 257      # just above MAX_LAUNCH_BLOCKS * 256: the second launch, with base 2^31


def slots_model(n, full):
    """closed form: slot s of (workgroup mod 1024) = {threads, sum of indices mod 2^64, xor of indices, lanes beyond n}"""
    out = np.zeros((_capi.LAUNCH_SLOTS, 4), dtype=U64)
    blocks = (n + 255) // 256
    if blocks == 0:
        return out
    b = np.arange(blocks, dtype=U64)
    cnt = np.full(blocks, 256, dtype=U64)
    cnt[-1] = U64(n - 256 * (blocks - 1))
    first = b * U64(256)
    total = cnt * first + cnt * (cnt - U64(1)) // U64(2)      # sum of first .. first + cnt - 1 (below 2^64 for every n here)
    x = np.zeros(blocks, dtype=U64)                            # xor of a full, aligned block of 256 indices is 0
    last = 0
    for t in range(256 * (blocks - 1), n):
        last ^= t
    x[-1] = U64(last)
    slot = (b % U64(_capi.LAUNCH_SLOTS)).astype(np.int64)
    np.add.at(out[:, 0], slot, cnt)
    np.add.at(out[:, 1], slot, total)
    np.bitwise_xor.at(out[:, 2], slot, x)
    if full:
        out[(blocks - 1) % _capi.LAUNCH_SLOTS, 3] = U64(256 * blocks - n)
    return out


def launcher(lib_path, which, n):
    slots, refused, launches = _capi.selftest_launch(which, n, lib_path=lib_path)
    assert not refused
    same(slots.ravel(), slots_model(n, which != "launch").ravel(), f"{which} over {n} threads (four numbers per slot)")
    if on_device(lib_path):
        blocks = (n + 255) // 256
        want = 0 if n == 0 else 1 if which == "launch_wave_kernel" else (blocks + MAX_LAUNCH_BLOCKS - 1) // MAX_LAUNCH_BLOCKS
        assert launches == want, (which, n, launches, want)


def launcher_grid_limits(lib_path):
    slots, refused, launches = _capi.selftest_launch("sized", 1 << 24, lib_path=lib_path)
    assert refused and launches == 0 and not slots.any(), "2^24 blocks: 'grid too large', nothing launched"
    slots, refused, launches = _capi.selftest_launch("sized", 0, lib_path=lib_path)
    assert not refused and launches == 0 and not slots.any(), "0 blocks: returns, nothing launched"


# ---- 5. atomics, wave_alloc32, wave_add64 ------------------------------------------------------------------------------------------------
N_WORDS = 5      # a handful of contended words


def atomic_inputs(seed, bits):
    rng = np.random.default_rng(seed)
    operand = rng.integers(0, 1 << 63, size=T, dtype=U64) * U64(2) + rng.integers(0, 2, size=T, dtype=U64)
    if bits == 32:
        operand &= U64(M32)
    target = rng.integers(0, N_WORDS, size=T, dtype=U64).astype(U32)
    return operand, target


def fold(op, init, operand, target, bits):
    mask = M32 if bits == 32 else M64
    words = [init & mask] * N_WORDS
    for v, w in zip(operand.tolist(), target.tolist()):
        words[w] = op(words[w], v) & mask
    return np.array(words, dtype=U64)


FINAL_OPS = {      # name -> (bits, the fold, initial values)
    "add32": (32, lambda a, b: a + b, (0, 0xFFFFFF00)), "add64": (64, lambda a, b: a + b, (0, M64 - 1000)),
    "min32": (32, min, (M32, 0x80000000)), "max32": (32, max, (0, 0x7FFFFFFF)),
    "min64": (64, min, (M64, 1 << 63)), "max64": (64, max, (0, (1 << 63) - 1)),
    "or32": (32, lambda a, b: a | b, (0, 0x0F0F0000)), "or64": (64, lambda a, b: a | b, (0, 0xF0 << 56)),
    "xor64": (64, lambda a, b: a ^ b, (0, 0x0123456789ABCDEF)),
    "fetch_or32": (32, lambda a, b: a | b, (0, 0x00FF0000)), "fetch_and32": (32, lambda a, b: a & b, (M32, 0xFFFF00FF)),
}


def atomic_final_value(lib_path, name):
    bits, op, inits = FINAL_OPS[name]
    for k, init in enumerate(inits):
        operand, target = atomic_inputs(8200 + 7 * k + _capi.ATOMIC_OPS[name], bits)
        if name in ("or32", "or64", "fetch_or32"):      # sparse bits, or every word saturates
            operand = U64(1) << (operand % U64(bits))
        if name == "fetch_and32":
            operand = U64(M32) ^ (U64(1) << (operand % U64(32)))
            operand[target == 0] = U64(M32)             # one word keeps all its bits
        words, ret = _capi.selftest_atomics(name, init, operand, target, N_WORDS, lib_path=lib_path)
        want = fold(op, init, operand, target, bits)
        same(words, want, f"{name} from {init:#x}: the words afterwards")
        if name == "min64":      # each return is a value the word held: between the final minimum and init
            assert (ret >= want[target]).all() and (ret <= U64(init)).all(), name
        if name in ("fetch_or32", "fetch_and32"):      # bit by bit between init and the final word
            lo, hi = (U64(init), want[target]) if name == "fetch_or32" else (want[target], U64(init))
            assert ((ret & lo) == lo).all() and ((ret | hi) == hi).all(), name
            # the OLD value: whoever changed a bit first saw it unchanged — those threads' bits are exactly the bits that changed
            bit = operand if name == "fetch_or32" else operand ^ U64(M32)
            firsts = (ret & bit) == (U64(0) if name == "fetch_or32" else bit)
            changed = np.zeros(N_WORDS, dtype=U64)
            np.bitwise_or.at(changed, target[firsts], bit[firsts])
            same(changed, want ^ U64(init), f"{name}: the bits whose first change a thread saw")


def atomic_add_returns(lib_path, name):
    """a constant addend: the returns on one word are exactly the multiset {init + i * c}"""
    bits = 32 if name == "add32" else 64
    mask = M32 if bits == 32 else M64
    for init, c in ((5, 1), (mask - 70_000, 13), (0, mask)):      # the last: adding -1
        _, target = atomic_inputs(8300, bits)
        words, ret = _capi.selftest_atomics(name, init, np.full(T, c, dtype=U64), target, N_WORDS, lib_path=lib_path)
        for w in range(N_WORDS):
            cnt = int((target == w).sum())
            assert int(words[w]) == (init + cnt * c) & mask, (name, w)
            want = np.sort(np.array([(init + i * c) & mask for i in range(cnt)], dtype=U64))
            same(np.sort(ret[target == w]), want, f"{name} + {c:#x} from {init:#x}: the returned old values of word {w}")


def atomic_cas_claims(lib_path, name):
    n_slots, sentinel = 1000, (0xFFFFFFFF if name == "cas32" else 0xFFFFFFFFFFFFFFFF)
    rng = np.random.default_rng(8400)
    target = rng.integers(0, n_slots, size=T, dtype=U64).astype(U32)
    target[:n_slots] = np.arange(n_slots, dtype=U32)      # every slot has a claimant
    operand = rng.permutation(T).astype(U64) + U64(1)     # distinct, never the sentinel
    words, ret = _capi.selftest_atomics(name, sentinel, operand, target, n_slots, expected=sentinel, lib_path=lib_path)
    won = ret == U64(sentinel)
    assert int(won.sum()) == n_slots, f"{name}: {int(won.sum())} threads saw the sentinel, {n_slots} slots"
    assert np.array_equal(np.sort(target[won]), np.arange(n_slots, dtype=U32)), f"{name}: a slot was claimed twice"
    got = np.zeros(n_slots, dtype=U64)
    got[target[won]] = operand[won]
    same(words, got, f"{name}: each slot holds the operand of the thread that claimed it")
    lost = ~won
    assert np.array_equal(ret[lost], got[target[lost]]), f"{name}: a loser saw something else than the winner's value"


def atomic_load(lib_path):
    rng = np.random.default_rng(8500)
    n_words = 4096
    target = rng.integers(0, n_words, size=T, dtype=U64).astype(U32)
    init = 0x9E3779B9
    words, ret = _capi.selftest_atomics("load32", init, np.zeros(T, dtype=U64), target, n_words, lib_path=lib_path)
    stored = (np.arange(n_words, dtype=U64) * U64(2654435761) + U64(init)) & U64(M32)
    same(words, stored, "the words an earlier launch stored")
    same(ret, stored[target], "atomic_load32 of them")


def wave_alloc(lib_path):
    rng = np.random.default_rng(8600)
    amounts = rng.integers(0, 50, size=T, dtype=U64)
    amounts[rng.random(T) < 0.3] = 0
    amounts[64 * 5:64 * 7] = 0        # whole wavefronts of 0
    amounts[64 * 255:] = 0
    for name, amt, init in (("mixed", amounts, 0), ("from a running counter", amounts, 12345), ("all zero", np.zeros(T, dtype=U64), 777)):
        words, off = _capi.selftest_atomics("wave_alloc32", init, amt, np.zeros(T, dtype=U32), 1, lib_path=lib_path)
        total = int(amt.sum())
        assert int(words[0]) == init + total, f"wave_alloc32 {name}: the counter ends at {int(words[0])}, expected {init + total}"
        taken = amt > 0
        order = np.argsort(off[taken], kind="stable")
        lo, n = off[taken][order], amt[taken][order]
        if total:      # the ranges [off, off + amount) are disjoint and tile [init, init + total)
            assert int(lo[0]) == init and np.array_equal(lo[1:], (lo + n)[:-1]) and int(lo[-1] + n[-1]) == init + total, f"wave_alloc32 {name}: the ranges do not tile"
        w = np.arange(T) // 64      # within a wavefront the lanes' ranges follow one another in lane order
        for wave in (0, 1, 5, 100, 255):
            o, a = off[w == wave], amt[w == wave]
            assert np.array_equal(o[1:], (o + a)[:-1]), f"wave_alloc32 {name}: wavefront {wave}"


def wave_add(lib_path):
    rng = np.random.default_rng(8700)
    v = rng.integers(0, 1 << 25, size=T, dtype=U64)      # a wavefront's total stays below 2^32 (the helper adds in 32 bits)
    v[64 * 9:64 * 11] = 0
    target = (np.arange(T) // 64 % 3).astype(U32)
    for init in (0, M64 - 5):
        words, _ = _capi.selftest_atomics("wave_add64", init, v, target, 3, lib_path=lib_path)
        want = np.array([(init + int(v[target == w].sum())) & M64 for w in range(3)], dtype=U64)
        same(words, want, f"wave_add64 from {init:#x}")


def atomics_bad_arguments(lib_path):
    for kw in (dict(op="add32", target=np.full(T, N_WORDS, dtype=U32)), dict(op="wave_alloc32", target=(np.arange(T) % 2).astype(U32))):
        try:
            _capi.selftest_atomics(kw["op"], 0, np.zeros(T, dtype=U64), kw["target"], N_WORDS, lib_path=lib_path)
        except Exception as e:
            assert "selftest atomics" in str(e), e
        else:
            raise AssertionError(f"{kw['op']} was not refused")


# ---- 6. the side stream and its event ring -----------------------------------------------------------------------------------------------
SIDE_WORDS = 1 << 20      # a 4 MB buffer


def side_order(lib_path, mode, which):
    seed = 0xABCD0000 + 17 * which + (mode == "main_event")
    got = _capi.selftest_side_order(mode, which, seed, SIDE_WORDS, lib_path=lib_path)
    want = ((np.arange(SIDE_WORDS, dtype=U64) * U64(2654435761) + U64(seed)) & U64(M32)).astype(U32)
    same(got, want, f"what the host saw behind {mode} on side stream {which}")


def ring_program(lib_path):
    """a handle stays valid until N_EV more events were taken"""
    mix = ["main_event", "mark", "after_main"]
    for first in ("main_event", "mark"):
        for more, recycled in ((0, 0), (N_EV - 1, 0), (N_EV, 1), (N_EV + 5, 1), (2 * N_EV + 1, 1)):
            r = _capi.selftest_event_ring([first] + [mix[i % 3] for i in range(more)], lib_path=lib_path)
            assert r == dict(events_taken=1 + more, recycled_waits=recycled), (first, more, r)
    assert _capi.selftest_event_ring(lib_path=lib_path) == dict(events_taken=0, recycled_waits=0), "reading clears"
