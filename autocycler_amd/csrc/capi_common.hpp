// What the units of the C ABI share (capi.cpp, capi_shard.cpp, capi_steps.cpp, capi_command.cpp): the handle structs, the error
// convention, the build lock with the device selection behind it, and the input checks.  Private to the library: everything in
// ac::abi has hidden visibility, so none of it reaches the dynamic symbol table.
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/autocycler_hip.h"
#include "graph_build.hpp"
#include "host_io.hpp"
#include "multi_build.hpp"
#include "device_rt.hpp"

struct ac_graph {
    ac::FinalGraph g;
    ac::BuildTimings tm;
    ac::MultiStats multi;      // n_ranks == 0: not built by ac_compress_build_multi
    std::vector<uint16_t> seq_ids;
    std::vector<uint32_t> seq_lens;
    bool positions_built = false;
    bool host_arrays = true;   // false: a rank of a sharded build that did not ask for the unitigs / links
    bool host_paths = true;    // false: ... that did not ask for its paths either
    std::vector<std::string> filenames, headers;   // graphs loaded from a GFA carry them (FN:Z / HD:Z)
};

struct ac_seqs {
    ac::LoadResult lr;
    std::vector<ac_seq_view> views;
    void make_views() {
        views.resize(lr.seqs.size());
        for (size_t i = 0; i < views.size(); i++)
            views[i] = ac_seq_view{(const uint8_t*)lr.seqs[i].forward_seq.data(), lr.seqs[i].length, lr.seqs[i].id};
    }
};

namespace ac {
namespace abi __attribute__((visibility("hidden"))) {

// ---- errors: a call returns 1 and leaves its text for ac_last_error() of the calling thread ----
std::string& last_error();
inline int fail(const char* what) { last_error() = what; return 1; }
// (a call that failed may have left a scan between its ticket take and its kernel: the calling thread's scan state pool starts over)
template <class F> int guarded(F&& f) {
    try { f(); return 0; }
    catch (const std::exception& e) { last_error() = e.what(); scan_pool().invalidate(); return 1; }
    catch (...) { last_error() = "unknown internal error"; scan_pool().invalidate(); return 1; }
}

// ---- one device user at a time (defined in capi.cpp) ----
extern std::mutex g_build_mutex;                // one build at a time per process: the device / pinned arenas are shared
extern int g_live_shards;                       // a live sharded build owns the arenas between its phases: no other build may start
extern std::atomic<int> g_host_side_device;     // ac_set_host_side_device: where ac_seqs_load / ac_seqs_from_raw run the end repair

// The prologue of every call that uses a device, after its own argument checks: takes the build lock for the call's lifetime, refuses
// while a sharded build is live, makes `device` current (capi.cpp select_device: the gfx950 check, the arena's device).
struct DeviceCall {
    enum Kind {
        PLAIN,
        SHARD_PHASE,      // a call of the live sharded build itself (or on its results): not refused
        SHARD_BEGIN,      // refuses as "another sharded build ..."
        ALL_DEVICES,      // ac_compress_build_multi: the rank threads select their devices; only the knobs are refreshed here
    };
    explicit DeviceCall(int device, Kind kind = PLAIN);
    std::lock_guard<std::mutex> lock;
};

// ---- input checks and copies of the build entries ----
void validate(uint32_t k, const ac_seq_view* seqs, uint32_t n_seqs);
// The device entries take the text layout from the caller: check it before any kernel indexes the text with it (the header
// promises errors, not faults).  off[i] = first padded byte of sequence i; every padded sequence is followed by one separator.
void validate_layout(uint32_t k, uint64_t n_text, const uint64_t* off, const uint32_t* len, const uint16_t* d1, const uint16_t* d2,
                     uint32_t n_seqs);
// the caller's views as the builder takes them; their ids and lengths are appended to what a handle keeps
std::vector<SeqView> seq_views(const ac_seq_view* seqs, uint32_t n_seqs, std::vector<uint16_t>* seq_ids, std::vector<uint32_t>* seq_lens);
// the caller's device text and layout arrays into the builder (set_text_device); the ids and lengths for the handle
void set_device_text(GraphBuilder& b, const void* d_text, uint64_t n_text, const uint64_t* seq_off, const uint32_t* seq_len,
                     const uint16_t* ids, const uint16_t* seq_d1, const uint16_t* seq_d2, uint32_t n_seqs,
                     std::vector<uint16_t>* seq_ids, std::vector<uint32_t>* seq_lens);

}  // namespace abi
}  // namespace ac
