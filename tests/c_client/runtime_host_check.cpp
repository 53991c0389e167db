// The arena of csrc/device_rt.hpp on the host alone (-DAC_EMU: malloc for hipMalloc), replaying a fixed subset of the programs of
// tests/runtime_cases.py against numbers worked out by hand from the arena's rules — built under the address and undefined-behaviour
// sanitizers (every block is a malloc of its own, so a byte written outside an allocation's block is reported):
//   g++ -std=c++17 -g -O1 -DAC_EMU -fsanitize=address,undefined -I autocycler_amd/csrc tests/c_client/runtime_host_check.cpp -o runtime_host_check -pthread
// (`make runtime_host_check` in autocycler_amd/csrc; tests/test_runtime_emu.py builds and runs it).  CPU only.
#define AC_EMU_DEFINE_CTX_SWITCH
#include "device_rt.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ac;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static const size_t MB = (size_t)1 << 20;

struct Placed { u8* p; size_t bytes; u8 tag; };
static std::vector<Placed> g_live;
static u8* take(Arena& a, size_t bytes, size_t want_block, size_t want_off) {
    u8* p = (u8*)a.alloc(bytes);
    size_t blk = 0, off = 0, used = 0;
    CHECK(a.locate(p, &blk, &off, &used));
    CHECK(blk == want_block); CHECK(off == want_off);
    const size_t rounded = bytes ? (bytes + 255) & ~(size_t)255 : 256;
    CHECK(off + rounded <= used);
    const u8 tag = (u8)(g_live.size() + 1);
    memset(p, tag, rounded);      // (the sanitizer watches every byte of it)
    g_live.push_back(Placed{p, rounded, tag});
    return p;
}
static void check_live(size_t keep) {      // the first `keep` allocations still hold their tags
    for (size_t i = 0; i < keep && i < g_live.size(); i++)
        for (size_t b = 0; b < g_live[i].bytes; b += 97) CHECK(g_live[i].p[b] == g_live[i].tag);
}
static void totals(const Arena& a, size_t cap, size_t used, size_t peak) { CHECK(a.capacity() == cap); CHECK(a.total_used() == used); CHECK(a.peak() == peak); }

int main() {
    {      // a request larger than grow; zero bytes take 256
        Arena a; a.set_grow(MB); g_live.clear();
        take(a, 1, 0, 0);
        take(a, 5 * MB, 1, 0);
        take(a, 0, 2, 0);                              // (block 1 is full to the byte: a third block)
        take(a, MB - 512, 2, 256);
        take(a, 257, 3, 0);
        totals(a, MB + 5 * MB + MB + MB, 256 + 5 * MB + 256 + (MB - 512) + 512, 256 + 5 * MB + 256 + (MB - 512) + 512);
        check_live(5);
    }
    {      // rewind two blocks back, then a request that skips a block
        Arena a; a.set_grow(MB); g_live.clear();
        take(a, 1000, 0, 0);
        const Arena::Mark m = a.mark();
        take(a, MB, 1, 0);
        take(a, 3 * MB, 2, 0);
        take(a, 600000, 3, 0);                         // (first fit looks forwards from the current block only)
        a.rewind(m);
        totals(a, 6 * MB, 1024, 1024 + MB + 3 * MB + 600064);
        check_live(1);
        take(a, 100, 0, 1024);
        take(a, 2 * MB, 2, 0);                         // skips block 1 (1 MB)
        take(a, 900000, 2, 2 * MB);
        take(a, 5 * MB, 4, 0);
        check_live(1);
    }
    {      // an empty-arena mark; nested marks rewound innermost first
        Arena a; a.set_grow(MB); g_live.clear();
        const Arena::Mark empty = a.mark();
        CHECK(empty.empty);
        take(a, 300, 0, 0);
        const Arena::Mark m1 = a.mark();
        take(a, 700000, 0, 512);
        const Arena::Mark m2 = a.mark();
        take(a, 4 * MB, 1, 0);
        a.rewind(m2);
        totals(a, 5 * MB, 512 + 700160, 512 + 700160 + 4 * MB);
        take(a, 100000, 0, 512 + 700160);
        a.rewind(m1);
        check_live(1);
        take(a, MB, 1, 0);
        a.rewind(empty);
        totals(a, 5 * MB, 0, 512 + 700160 + 4 * MB);
        take(a, 7, 0, 0);
    }
    {      // reset with one block keeps it; with three blocks it coalesces: capacity = min(sum, peak + peak / 8 + 256 MB)
        Arena a; a.set_grow(MB); g_live.clear();
        take(a, 5000, 0, 0);
        a.reset();
        totals(a, MB, 0, 0);
        take(a, 900000, 0, 0); take(a, 900000, 1, 0); take(a, 2 * MB, 2, 0);
        a.reset();
        totals(a, 4 * MB, 0, 0);
        g_live.clear();
        take(a, 3 * MB, 0, 0); take(a, 900000, 0, 3 * MB); take(a, 400000, 1, 0);
    }
    {      // reserve: no effect on a used arena or a large enough one, one block on a fresh one
        Arena a; a.set_grow(MB); g_live.clear();
        a.reserve(3 * MB);
        totals(a, 3 * MB, 0, 0);
        take(a, 2 * MB, 0, 0);
        a.reserve(8 * MB);
        totals(a, 3 * MB, 2 * MB, 2 * MB);
        a.release_all();
        totals(a, 0, 0, 2 * MB);
        a.reserve(300); a.reserve(200);
        totals(a, 300, 0, 2 * MB);
        g_live.clear();
        take(a, 200, 0, 0);
        take(a, 200, 1, 0);                            // (the 300-byte block holds one 256-byte allocation)
    }
    {      // the side stream's ring: a handle stays valid until N_EV more events were taken
        SideStream& s = SideStream::get();
        (void)s.take_ring_counts();
        void* h = s.main_event();
        for (unsigned i = 0; i + 1 < SideStream::N_EV; i++) (void)s.mark();
        SideStream::wait_event(h);
        SideStream::RingCounts c = s.take_ring_counts();
        CHECK(c.events_taken == SideStream::N_EV); CHECK(c.recycled_waits == 0);
        h = s.mark();
        for (unsigned i = 0; i < SideStream::N_EV; i++) s.after_main();
        SideStream::wait_event(h);
        c = s.take_ring_counts();
        CHECK(c.events_taken == SideStream::N_EV + 1); CHECK(c.recycled_waits == 1);
    }
    printf(failures ? "runtime_host_check: %d FAILED\n" : "runtime_host_check: OK\n", failures);
    return failures ? 1 : 0;
}
