// The step meter of csrc/device_rt.hpp on the host alone (-DAC_EMU): its intervals, their reuse, what it counts of the launchers and the
// read-backs against numbers worked out from their rules, and that it leaves nothing behind when a step ends early — built under the
// address and undefined-behaviour sanitizers:
//   g++ -std=c++17 -g -O1 -DAC_EMU -fsanitize=address,undefined -I autocycler_amd/csrc tests/c_client/step_meter_check.cpp -o step_meter_check -pthread
// (`make step_meter_check` in autocycler_amd/csrc; tests/test_step_meter_emu.py builds and runs it).  CPU only.
#define AC_EMU_DEFINE_CTX_SWITCH
#include "device_rt.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace ac;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

struct AddOneFunctor { u32* v; void operator()(u64 i) const { v[i] += 1; } };
struct AddOneFullFunctor { u32* v; void operator()(u64 i, bool valid) const { if (valid) v[i] += 1; } };

static const u64 N = 5000;      // more than one scan tile (4096) and more than one sort tile (2048)

static void some_work(DBuf<u32>& v) { launch(N, AddOneFunctor{v.ptr()}); }

int main() {
    DeviceCtx ctx;      // (everything the runtime keeps — the arena, the scan pool — dies with it: the leak check sees the rest)
    set_device_ctx(&ctx);
    {
        DBuf<u32> v(N, true);
        {      // never begun: nothing to read
            StepMeter m;
            CHECK(m.seconds() == 0 && m.seconds(0) == 0 && m.seconds(1) == 0 && m.take() == 0);
            CHECK(m.launches() == 0 && m.read_backs() == 0);
            const StepStats s = m.stats();
            CHECK(s.launches == 0 && s.read_backs == 0 && s.seconds_device == 0);
        }
        {      // two intervals and their sum; a third is refused
            StepMeter m;
            m.begin(); some_work(v); m.end();
            CHECK(m.seconds(1) == 0);      // (not begun yet)
            m.begin(); some_work(v); some_work(v);
            CHECK(m.seconds(1) == 0);      // (begun, not ended)
            m.end();
            const double a = m.seconds(0), b = m.seconds(1);
            CHECK(std::isfinite(a) && std::isfinite(b) && a > 0 && b > 0);
            CHECK(m.seconds() == a + b && m.seconds(0) == a);      // (reading changes nothing)
            CHECK(m.launches() == 3 && m.stats().launches == 3 && m.stats().seconds_device == a + b);
            bool refused = false;
            try { m.begin(); } catch (const DeviceError&) { refused = true; }
            CHECK(refused);
            refused = false;
            try { m.end(); } catch (const DeviceError&) { refused = true; }      // (the second interval has ended already)
            CHECK(refused);
        }
        {      // one interval, reused lap after lap
            StepMeter m;
            double total = 0;
            for (int lap = 0; lap < 10; lap++) {
                m.begin(); some_work(v); m.end();
                const double t = m.take();
                CHECK(std::isfinite(t) && t > 0);
                CHECK(m.seconds() == 0);      // (taken)
                total += t;
            }
            CHECK(total > 0 && m.launches() == 10);
        }
        {      // what the launchers and the read-backs count: literal numbers
            StepMeter m;
            launch(N, AddOneFunctor{v.ptr()});                           // 1
            launch_full(N, AddOneFullFunctor{v.ptr()});                  // 1
            launch(0, AddOneFunctor{v.ptr()});                           // nothing to launch
            launch_full(0, AddOneFullFunctor{v.ptr()});
            CHECK(m.launches() == 2);
            DBuf<u32> sum(N);
            exclusive_scan_u32(v.ptr(), sum.ptr(), N);                   // one launch per scan
            CHECK(m.launches() == 3);
            DBuf<u64> key(N); DBuf<u32> val(N);
            std::vector<u64> hk(N);
            for (u64 i = 0; i < N; i++) hk[i] = (i * 2654435761ULL) & 0xFFFFFFULL;
            copy_h2d(key.ptr(), hk.data(), N * 8);
            sort_pairs_u64_u32(key, val, N, 24);                         // 24 bits: the histogram and three passes
            CHECK(m.launches() == 7);
            sort_pairs_u64_u32(key, val, 1, 24);                         // nothing to sort
            CHECK(m.launches() == 7 && m.read_backs() == 0);
            const std::vector<u64> sorted = to_host(key, N);             // a read-back
            for (u64 i = 1; i < N; i++) CHECK(sorted[i - 1] <= sorted[i]);
            u32 first = 0, last = 0, total = 0;
            copy_d2h(&first, v.ptr(), 0);                                // no bytes: no round trip
            CHECK(m.read_backs() == 1);
            ReadBatch rb;
            rb.run();                                                    // nothing in it
            rb.add(&first, sum.ptr(), 4); rb.add(&last, sum.ptr() + (N - 1), 4); rb.add(&total, v.ptr(), 0);
            rb.run();                                                    // one round trip for both
            CHECK(m.read_backs() == 2 && first == 0 && last == (u32)(N - 1) * to_host(v, 1)[0]);
            CHECK(m.read_backs() == 3);
            m.sync_copies();                                             // the bulk copies' one synchronisation
            CHECK(m.read_backs() == 4 && m.launches() == 7);
            StepMeter later;      // a meter made now has seen none of it
            CHECK(later.launches() == 0 && later.read_backs() == 0);
        }
        {      // destroyed with an interval begun and not ended
            StepMeter m;
            m.begin(); some_work(v); m.end();
            m.begin(); some_work(v);
        }
        {      // an exception between begin() and end()
            bool caught = false;
            try {
                StepMeter m;
                m.begin();
                launch_wave_kernel_sized(+[](u32*) {}, (u64)1 << 30, 64u, 0, v.ptr());      // "grid too large"
                m.end();
                CHECK(false);
            } catch (const DeviceError&) { caught = true; }
            CHECK(caught);
            StepMeter m;      // and the next step measures as usual
            m.begin(); some_work(v); m.end();
            CHECK(m.seconds() > 0 && m.launches() == 1);
        }
    }
    set_device_ctx(nullptr);
    if (failures) { printf("step_meter_check: %d check(s) FAILED\n", failures); return 1; }
    printf("step_meter_check: OK\n");
    return 0;
}
