// The guard's own check (kernel_bounds_check selfcheck): after a few DBuf allocations the sanitizer is ASKED which bytes are poisoned —
// nothing outside an allocation is ever dereferenced, so nothing is provoked.  The only part of the bounds check that includes the runtime
// (csrc/device_rt.hpp); everything else goes through the C ABI.
#include "device_rt.hpp"

#if !defined(AC_ARENA_GUARD)
#error "built with -DAC_ARENA_GUARD=1 or 2 (csrc/Makefile: kernel_bounds_check)"
#endif
#include <sanitizer/asan_interface.h>

using namespace ac;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)
static bool poisoned(const void* p) { return __asan_address_is_poisoned(p) != 0; }
static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// the rule of Arena::alloc: [p, p + bytes) addressable, the rounding tail and the red zone behind it poisoned, the next allocation behind both
template <class T> static void check_alloc(const DBuf<T>& b, const void* next) {
    const char* p = (const char*)b.ptr();
    const size_t bytes = b.bytes();
    CHECK(!poisoned(p)); CHECK(!poisoned(p + bytes - 1));
    CHECK(__asan_region_is_poisoned((void*)p, bytes) == nullptr);
    CHECK(poisoned(p + bytes));                                  // the first byte behind the last one asked for
    if (round256(bytes) > bytes) CHECK(poisoned(p + round256(bytes) - 1));      // the last byte of the rounding tail
    CHECK(poisoned(p + round256(bytes)));                        // the first byte of the red zone
    CHECK(poisoned(p + round256(bytes) + Arena::RED_ZONE - 1));
    if (next) CHECK((const char*)next == p + round256(bytes) + Arena::RED_ZONE);
}

int guard_selfcheck() {
    const bool strict = AC_ARENA_GUARD >= 2;
    CHECK(Arena::RED_ZONE >= 256);
    Arena& a = Arena::device();
    a.release_all();
    a.set_grow((size_t)1 << 20);
    {
        DBuf<u8> b1(1), b255(255), b256(256), b257(257);
        DBuf<u32> w3(3);
        DBuf<u64> q(1000);
        DBuf<u8> none(0);      // (an empty DBuf still takes one element)
        check_alloc(b1, b255.ptr()); check_alloc(b255, b256.ptr()); check_alloc(b256, b257.ptr()); check_alloc(b257, w3.ptr()); check_alloc(w3, q.ptr());
        check_alloc(q, none.ptr());
        CHECK(!poisoned(none.ptr())); CHECK(poisoned(none.ptr() + 1));
        // a request beyond the block's rest opens a new block: all of it poisoned but the request
        DBuf<u8> big((size_t)3 << 20);
        check_alloc(big, nullptr);
        size_t blk = 0, off = 0, used = 0;
        CHECK(a.locate(big.ptr(), &blk, &off, &used) && blk == 1 && off == 0);

        // mark / rewind: level 1 leaves rewound space as it is until it goes out again, level 2 poisons it at once
        const Arena::Mark m = a.mark();
        DBuf<u8> x(100); DBuf<u32> y(5000);
        const u8* xp = x.ptr(); const u32* yp = y.ptr();
        a.rewind(m);
        CHECK(poisoned(xp) == strict); CHECK(poisoned(xp + 99) == strict);
        CHECK(poisoned(yp) == strict); CHECK(poisoned(yp + 4999) == strict);
        CHECK(poisoned(xp + 100)); CHECK(poisoned(yp + 5000));      // tails and red zones stay poisoned at either level
        Arena::keep_readable(yp, 100 * 4);                          // the annotated exception: these bytes, no more
        CHECK(!poisoned(yp) && !poisoned(yp + 99));
        CHECK(poisoned(yp + 100) == strict);
        DBuf<u8> z(10);                                             // rewound space handed out again: the rule of alloc
        CHECK(z.ptr() == xp);
        check_alloc(z, nullptr);
        CHECK(poisoned(xp + 10) && poisoned(xp + 99));

        // a rewind across blocks
        const Arena::Mark m2 = a.mark();
        DBuf<u8> far((size_t)2 << 20);
        const u8* fp = far.ptr();
        CHECK(a.locate(fp, &blk, &off, &used) && blk == 3 && off == 0);      // (x, y and z live in block 2: block 1 is full to the byte)
        a.rewind(m2);
        CHECK(poisoned(fp) == strict); CHECK(poisoned(fp + ((size_t)2 << 20) - 1) == strict);

        // reset: everything is poisoned again
        const u8* p1 = b1.ptr(); const u64* pq = q.ptr(); const u8* pb = big.ptr();
        a.reset();
        CHECK(a.locate(p1, &blk, &off, &used) == false || poisoned(p1));      // (several blocks coalesce on reset: the old ones are gone)
        DBuf<u8> first(64);
        CHECK(a.locate(first.ptr(), &blk, &off, &used) && blk == 0 && off == 0);
        CHECK(poisoned(first.ptr() + 64));
        CHECK(poisoned((const char*)first.ptr() + a.capacity() - 1));
        (void)pq; (void)pb;
        a.reset();                                                  // one block now: it is kept, and poisoned
        CHECK(poisoned(first.ptr())); CHECK(poisoned(first.ptr() + 63));
    }
    a.release_all();
    a.set_grow((size_t)64 << 20);
    {   // the pinned pool: what lies behind the block's stated size, up to the 4096-byte rounding of the emulation's allocation, is poisoned
        HostBlock h = PinnedPool::get().alloc(1000);
        const char* p = (const char*)h.p;
        CHECK(h.bytes >= 1000 && h.bytes % 4096 != 0);
        CHECK(__asan_region_is_poisoned((void*)p, h.bytes) == nullptr);
        CHECK(poisoned(p + h.bytes)); CHECK(poisoned(p + ((h.bytes + 4095) & ~(size_t)4095) - 1));
    }
    PinnedPool::get().trim();
    if (failures) { printf("guard selfcheck (level %d): %d FAILED\n", (int)AC_ARENA_GUARD, failures); return 1; }
    printf("guard selfcheck (level %d): OK\n", (int)AC_ARENA_GUARD);
    return 0;
}
