// C ABI, everything that touches files: the whole `compress` and `decompress` commands, and the loading of assemblies with the end
// repair of sequences that live in host memory.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <filesystem>
#include <fstream>
#include <map>
#include <memory>
#include <thread>
#include <unistd.h>
#include <zlib.h>

#include "capi_common.hpp"
#include "gfa_writer.hpp"

using namespace ac;
using namespace ac::abi;

// Writes the pieces one behind the other into `path`, each at its own offset by its own thread (pwrite): the GFA of config C is
// 95 MB.  With the S and L lines formatted by several threads too (gfa_chunks) the write stage of the whole command went from 48 to
// 26 ms (profiles/r07l_e2e_configC.log).
static void write_pieces(const std::string& path, const std::vector<std::string>& pieces, int threads) {
    // into a temporary file next to the target, renamed over it when every piece is down: a failed write never leaves a truncated
    // input_assemblies.gfa behind
    const std::string tmp = path + ".tmp." + std::to_string((long)::getpid());
    int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw UserError("failed to write " + path);
    std::vector<uint64_t> at(pieces.size() + 1, 0);
    for (size_t i = 0; i < pieces.size(); i++) at[i + 1] = at[i] + pieces[i].size();
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    auto worker = [&] {
        for (size_t i; (i = next.fetch_add(1)) < pieces.size();) {
            const char* p = pieces[i].data(); uint64_t left = pieces[i].size(), off = at[i];
            while (left) {
                ssize_t w = ::pwrite(fd, p, left, (off_t)off);
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) { bad.store(true); return; }
                p += w; left -= (uint64_t)w; off += (uint64_t)w;
            }
        }
    };
    const int T = std::max(1, std::min<int>({threads, 16, (int)pieces.size()}));
    std::vector<std::thread> pool;
    for (int i = 1; i < T; i++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    const bool closed = ::close(fd) == 0;
    if (!closed || bad.load() || ::rename(tmp.c_str(), path.c_str()) != 0) { ::unlink(tmp.c_str()); throw UserError("failed to write " + path); }
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// What both forms of the compress command begin with: the settings, then the form's own argument check (`refuse`: its text when that
// failed), then the output directory.
static void open_output_dir(const char* assemblies_dir, const char* autocycler_dir, uint32_t k, int threads, const char* refuse = nullptr) {
    check_compress_settings(assemblies_dir, autocycler_dir, k, threads);
    if (refuse) throw DeviceError(refuse);
    std::error_code ec;
    std::filesystem::create_directories(autocycler_dir, ec);
    if (ec) throw UserError(std::string("failed to create directory ") + autocycler_dir + "\n" + ec.message());
}
// ... and end with: input_assemblies.gfa and .yaml of the graph that was built from t0 on.  times[4] = load, repair, graph (hot path), write.
static void write_outputs(const char* autocycler_dir, const LoadResult& lr, const FinalGraph& g, int threads, double t0, double* times) {
    namespace fs = std::filesystem;
    const double t1 = now_s();
    std::vector<SeqMeta> meta(lr.seqs.size());
    for (size_t i = 0; i < meta.size(); i++) meta[i] = SeqMeta{lr.seqs[i].id, lr.seqs[i].length, lr.seqs[i].filename, lr.seqs[i].contig_header};
    write_pieces((fs::path(autocycler_dir) / "input_assemblies.gfa").string(), gfa_chunks(g, meta, threads), threads);
    {
        std::string y = metrics_yaml(lr, g.post.unitigs, g.post.total_length);
        std::ofstream f(fs::path(autocycler_dir) / "input_assemblies.yaml", std::ios::binary);
        f.write(y.data(), (std::streamsize)y.size());
    }
    const double t2 = now_s();
    if (times) { times[0] = lr.load_seconds; times[1] = lr.repair_seconds; times[2] = t1 - t0; times[3] = t2 - t1; }
}

extern "C" {

// The whole `autocycler decompress` command (decompress.rs:27-39): GFA file -> the assemblies it was built from, one file per
// original filename in out_dir (gzip when the name ends in .gz, decompress.rs:83-105) and / or all contigs in one FASTA file
// (headers ">{filename}__{header}", :117-137).  Either of out_dir / out_file may be NULL, not both.
int ac_decompress(const char* in_gfa, const char* out_dir, const char* out_file, int threads) {
    return guarded([&] {
        namespace fs = std::filesystem;
        if (!in_gfa || !fs::is_regular_file(in_gfa)) throw UserError(std::string("file does not exist: ") + (in_gfa ? in_gfa : ""));
        if (!out_dir && !out_file) throw UserError("either --out_dir or --out_file is required");
        if (out_dir && fs::exists(out_dir) && !fs::is_directory(out_dir)) throw UserError(std::string(out_dir) + " exists but is not a directory");
        std::string text;
        {
            std::ifstream f(in_gfa, std::ios::binary);
            text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        }
        ac_graph h;
        std::vector<SeqMeta> meta;
        load_gfa(text.data(), text.size(), &h.g, &meta);
        const size_t S = meta.size();
        std::vector<std::string> seqs(S);
        {   // reconstruct_original_sequences (unitig_graph.rs:362-388), one sequence per task
            std::atomic<size_t> next{0};
            auto worker = [&] { for (size_t i; (i = next.fetch_add(1)) < S;) { seqs[i].resize(meta[i].length); decompress_sequence(h.g, i, seqs[i].data()); } };
            int T = std::max(1, std::min<int>(threads, (int)S));
            std::vector<std::thread> pool;
            for (int t = 1; t < T; t++) pool.emplace_back(worker);
            worker();
            for (auto& t : pool) t.join();
        }
        std::map<std::string, std::vector<size_t>> by_file;      // filenames sorted; contigs in GFA order within a file
        for (size_t i = 0; i < S; i++) by_file[meta[i].filename].push_back(i);
        if (out_dir) {
            std::error_code ec;
            fs::create_directories(out_dir, ec);
            if (ec) throw UserError(std::string("failed to create directory ") + out_dir + "\n" + ec.message());
            for (auto& [fname, idx] : by_file) {
                fs::path path = fs::path(out_dir) / fname;
                std::string body;
                for (size_t i : idx) { body += ">" + meta[i].contig_header + "\n"; body += seqs[i]; body += "\n"; }
                if (path.extension() == ".gz") {
                    gzFile gz = gzopen(path.c_str(), "wb");
                    if (!gz) throw UserError("failed to create " + path.string());
                    size_t o = 0;
                    while (o < body.size()) { int n = gzwrite(gz, body.data() + o, (unsigned)std::min<size_t>(body.size() - o, 1u << 30)); if (n <= 0) { gzclose(gz); throw UserError("failed to write " + path.string()); } o += (size_t)n; }
                    gzclose(gz);
                } else {
                    std::ofstream f(path, std::ios::binary);
                    f.write(body.data(), (std::streamsize)body.size());
                    if (!f) throw UserError("failed to write " + path.string());
                }
            }
        }
        if (out_file) {
            std::ofstream f(out_file, std::ios::binary);
            for (auto& [fname, idx] : by_file) {
                std::string clean = fname;
                std::replace(clean.begin(), clean.end(), ' ', '_');
                for (size_t i : idx) { f << ">" << clean << "__" << meta[i].contig_header << "\n"; f.write(seqs[i].data(), (std::streamsize)seqs[i].size()); f << "\n"; }
            }
            if (!f) throw UserError(std::string("failed to write ") + out_file);
        }
    });
}
// ---- host side: load_sequences / end repair / whole command ---------------------------------------------
// sequence_end_repair (compress.rs:202-270) for sequences that live in host memory (ac_seqs_load, ac_seqs_from_raw, the multi-device
// command): the padded sequences go up as one text, the device kernels repair it in place (neighbours.inc — the only implementation
// the library has), and the k - 1 leading / trailing bytes of every sequence come back.
static void repair_on_device(LoadResult& lr, uint32_t k, int device) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<LoadedSeq>& seqs = lr.seqs;
    const size_t m = (size_t)k - 1;
    if (m == 0 || seqs.empty()) return;
    std::vector<SeqView> v(seqs.size());
    for (size_t i = 0; i < seqs.size(); i++) v[i] = SeqView{(const uint8_t*)seqs[i].forward_seq.data(), seqs[i].length};
    std::vector<uint64_t> off; std::vector<uint32_t> len; std::vector<uint16_t> d1, d2;
    std::vector<uint8_t> text = layout_text(v, k, &off, &len, &d1, &d2);
    {
        DeviceCall call(device);
        RepairTimings rt;
#ifdef AC_EMU
        end_repair_device(k, text.data(), text.size(), off, len, &d1, &d2, &rt);
#else
        void* d_text = nullptr;
        AC_HIP_CHECK(hipMalloc(&d_text, text.size() + 64));
        struct Free { void* p; ~Free() { (void)hipFree(p); } } fr{d_text};
        AC_HIP_CHECK(hipMemcpy(d_text, text.data(), text.size(), hipMemcpyHostToDevice));
        end_repair_device(k, (uint8_t*)d_text, text.size(), off, len, &d1, &d2, &rt);
        // only the two ends of a sequence can have changed: k - 1 bytes from either end of each come back (many short sequences: the whole text)
        if (seqs.size() > 256) AC_HIP_CHECK(hipMemcpy(text.data(), d_text, text.size(), hipMemcpyDeviceToHost));
        else for (size_t i = 0; i < seqs.size(); i++) {
            const size_t plen = seqs[i].forward_seq.size();
            AC_HIP_CHECK(hipMemcpyAsync(&text[off[i]], (const uint8_t*)d_text + off[i], std::min(m, plen), hipMemcpyDeviceToHost, 0));
            if (plen > m) AC_HIP_CHECK(hipMemcpyAsync(&text[off[i] + plen - m], (const uint8_t*)d_text + off[i] + plen - m, m, hipMemcpyDeviceToHost, 0));
        }
        AC_HIP_CHECK(hipStreamSynchronize(0));
#endif
    }
    for (size_t i = 0; i < seqs.size(); i++) {
        std::string& f = seqs[i].forward_seq;
        const size_t plen = f.size(), head = std::min(m, plen);
        memcpy(&f[0], &text[off[i]], head);
        if (plen > m) memcpy(&f[plen - m], &text[off[i] + plen - m], m);
    }
    lr.repair_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
int ac_seqs_load(const char* assemblies_dir, uint32_t k, uint32_t max_contigs, int threads, ac_seqs** out) {
    return guarded([&] {
        auto h = std::make_unique<ac_seqs>();
        h->lr = load_sequences(assemblies_dir, k, max_contigs, threads);
        repair_on_device(h->lr, k, g_host_side_device.load());
        h->make_views();
        *out = h.release();
    });
}
int ac_seqs_from_raw(uint32_t k, uint32_t n, const uint8_t* const* seqs, const uint32_t* lens, const char* const* filenames,
                     const char* const* headers, uint32_t assembly_count, int repair, int threads, ac_seqs** out) {
    return guarded([&] {
        auto h = std::make_unique<ac_seqs>();
        if (n > 32767) throw UserError("no more than 32767 input sequences are allowed");
        for (uint32_t i = 0; i < n; i++) {
            LoadedSeq s;
            s.id = (uint16_t)(i + 1);
            s.filename = filenames ? filenames[i] : ("assembly_" + std::to_string(i) + ".fasta");
            s.contig_header = headers ? headers[i] : ("contig_" + std::to_string(i + 1));
            pad_sequence(&s, std::string((const char*)seqs[i], lens[i]), k);
            h->lr.seqs.push_back(std::move(s));
        }
        h->lr.assembly_count = assembly_count;
        h->lr.total_contigs_seen = n;
        (void)threads;      // (the packers of a later build use their own pool; the repair is a device kernel)
        if (repair) repair_on_device(h->lr, k, g_host_side_device.load());
        h->make_views();
        *out = h.release();
    });
}
uint32_t ac_seqs_count(const ac_seqs* s) { return (uint32_t)s->lr.seqs.size(); }
uint32_t ac_seqs_assembly_count(const ac_seqs* s) { return s->lr.assembly_count; }
const ac_seq_view* ac_seqs_views(const ac_seqs* s) { return s->views.data(); }
int ac_seqs_get(const ac_seqs* s, uint32_t i, ac_seq_view* view, const char** filename, const char** header) {
    if (i >= s->lr.seqs.size()) return fail("sequence index out of range");
    if (view) *view = s->views[i];
    if (filename) *filename = s->lr.seqs[i].filename.c_str();
    if (header) *header = s->lr.seqs[i].contig_header.c_str();
    return 0;
}
double ac_seqs_repair_seconds(const ac_seqs* s) { return s->lr.repair_seconds; }
int ac_seqs_metrics_yaml(const ac_seqs* s, uint32_t unitig_count, uint64_t unitig_total_length, char** out) {
    return guarded([&] {
        std::string y = metrics_yaml(s->lr, unitig_count, unitig_total_length);
        char* p = (char*)malloc(y.size() + 1);
        if (!p) throw DeviceError("out of memory");
        memcpy(p, y.data(), y.size() + 1);
        *out = p;
    });
}
void ac_seqs_free(ac_seqs* s) { delete s; }

int ac_compress_seqs(uint32_t k, const ac_seqs* s, int device, ac_graph** out) {
    return ac_compress_build(k, s->lr.assembly_count, s->views.data(), (uint32_t)s->views.size(), device, out);
}

// compress.rs:32-50: the whole `autocycler compress` command.  times[4] = load, repair, graph (hot path), write.
int ac_compress_dir(const char* assemblies_dir, const char* autocycler_dir, uint32_t k, uint32_t max_contigs, int threads,
                    int device, ac_graph** graph_out, double* times) {
    return guarded([&] {
        namespace fs = std::filesystem;
        open_output_dir(assemblies_dir, autocycler_dir, k, threads);
        // load (host) -> text layout -> H2D -> end repair on the device text -> graph build from the same buffer
        // the HIP context and the code objects come up on another thread while the host reads the FASTA files
        // (with the arena and the upload ring it will need, sized from the files' sizes: a .gz holds about four times its size in bases)
        uint64_t est = 0;
        {
            std::error_code ec2;
            for (auto& e : fs::directory_iterator(assemblies_dir, ec2)) {
                if (!e.is_regular_file(ec2)) continue;
                const uint64_t sz = (uint64_t)e.file_size(ec2);
                est += e.path().extension() == ".gz" ? 4 * sz : sz;
            }
        }
        // (the helper thread also notes which device the arena it reserves lives on — select_device — so that the build's own
        // select_device, after the join below, finds it in place; nothing else runs in this process meanwhile: the CLI's only call)
        std::thread warm([device, k, est] {
            try {
                { DeviceCall call(device); }      // (refused while a sharded build is live: no warm-up then)
                device_warmup(device, k, est + (est >> 4) + (1u << 20));
            } catch (...) {}
        });
        struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{warm};
        ac_seqs s;
        s.lr = load_sequences(assemblies_dir, k, max_contigs, threads);
        s.make_views();
        warm.join();
        double t0 = now_s();
        ac_graph* g = nullptr;
        {
            const uint32_t n = (uint32_t)s.views.size();
            validate(k, s.views.data(), n);
            DeviceCall call(device);
            auto h = std::make_unique<ac_graph>();
            const std::vector<SeqView> v = seq_views(s.views.data(), n, &h->seq_ids, &h->seq_lens);
            // pinned-ring upload of the padded sequences -> end repair in place on the device text -> pack + build from the same buffer
            GraphBuilder b(k);
            b.set_sequences_host(v, /*pack_now=*/false);
            RepairTimings rt;
            b.repair_ends(&rt);
            s.lr.repair_seconds = now_s() - t0;        // upload of the text + the repair itself
            t0 = now_s();
            b.build(s.lr.assembly_count, &h->g);
            h->tm = b.timings();
            g = h.release();
        }
        std::unique_ptr<ac_graph> guard(g);
        write_outputs(autocycler_dir, s.lr, g->g, threads, t0, times);
        if (graph_out) *graph_out = guard.release();
    });
}

// The whole command over several devices: load + end repair on the host (the reference's own order, compress.rs:38-41), then ONE
// ac_compress_build_multi call, then the same writers.
int ac_compress_dir_multi(const char* assemblies_dir, const char* autocycler_dir, uint32_t k, uint32_t max_contigs, int threads,
                          const int* devices, int n_devices, ac_graph** graph_out, double* times) {
    return guarded([&] {
        open_output_dir(assemblies_dir, autocycler_dir, k, threads, !devices || n_devices < 1 ? "ac_compress_dir_multi: no devices" : nullptr);
        ac_seqs s;
        s.lr = load_sequences(assemblies_dir, k, max_contigs, threads);
        repair_on_device(s.lr, k, devices[0]);      // (compress.rs:38-41: load, then repair, then the build — the repair on the first rank's device)
        s.make_views();
        double t0 = now_s();
        ac_graph* g = nullptr;
        if (ac_compress_build_multi(k, s.lr.assembly_count, s.views.data(), (uint32_t)s.views.size(), devices, n_devices, &g) != 0) throw DeviceError(last_error());
        std::unique_ptr<ac_graph> guard(g);
        write_outputs(autocycler_dir, s.lr, g->g, threads, t0, times);
        if (graph_out) *graph_out = guard.release();
    });
}

// ---- `trim` and `resolve` as commands on a cluster directory: the text entries of capi_steps.cpp between a read and write_pieces ----
namespace fs = std::filesystem;
static std::string read_cluster_file(const fs::path& dir, const char* name) {
    if (!fs::is_directory(dir)) throw UserError("directory does not exist: " + dir.string());
    const fs::path p = dir / name;
    std::ifstream f(p, std::ios::binary);
    if (!f) throw UserError("file does not exist: " + p.string());
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
struct OwnedText {
    char* p = nullptr;
    ~OwnedText() { free(p); }
    std::string str() const { return p ? std::string(p) : std::string(); }
};
// trim.rs:36-53
int ac_trim_dir(const char* cluster_dir, double min_identity, uint32_t max_unitigs, double mad, int device) {
    return guarded([&] {
        if (!cluster_dir) throw DeviceError("null pointer: cluster_dir");
        const fs::path dir(cluster_dir);
        const std::string text = read_cluster_file(dir, "1_untrimmed.gfa");
        OwnedText gfa, yaml;
        if (ac_trim_gfa(text.data(), text.size(), min_identity, max_unitigs, mad, device, &gfa.p, nullptr, &yaml.p, nullptr) != 0) throw DeviceError(last_error());
        write_pieces((dir / "2_trimmed.gfa").string(), {gfa.str()}, 1);
        write_pieces((dir / "2_trimmed.yaml").string(), {yaml.str()}, 1);
    });
}
// resolve.rs:41-67 (without --verbose): 2_trimmed.gfa is renumbered, so load_gfa reads it
int ac_resolve_dir(const char* cluster_dir, int device) {
    return guarded([&] {
        if (!cluster_dir) throw DeviceError("null pointer: cluster_dir");
        const fs::path dir(cluster_dir);
        const std::string text = read_cluster_file(dir, "2_trimmed.gfa");
        ac_graph* gp = nullptr;
        if (ac_graph_from_gfa(text.data(), text.size(), &gp) != 0) throw DeviceError(last_error());
        std::unique_ptr<ac_graph> g(gp);
        OwnedText bridged, merged, final_text;
        uint32_t culled = 0;
        if (ac_resolve_graphs(g.get(), device, &bridged.p, &merged.p, &final_text.p, &culled) != 0) throw DeviceError(last_error());
        write_pieces((dir / "3_bridged.gfa").string(), {bridged.str()}, 1);
        write_pieces((dir / "4_merged.gfa").string(), {merged.str()}, 1);
        write_pieces((dir / "5_final.gfa").string(), {final_text.str()}, 1);
    });
}

// ---- `combine` and `gfa2fasta` as commands: the text entries of capi_combine.cpp between reads and write_pieces ----
static std::string read_input_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw UserError(std::string("file does not exist: ") + path);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
// combine.rs:28-54
int ac_combine(const char* autocycler_dir, const char* const* in_gfas, uint32_t n_gfas, const char* const* reads, uint32_t n_reads, uint32_t depth_kmer, int device,
               char** report) {
    return guarded([&] {
        if (report) *report = nullptr;
        if (!autocycler_dir) throw DeviceError("null pointer: autocycler_dir");
        if (n_gfas == 0) throw DeviceError("combine: at least one graph is required");
        if (!in_gfas || (n_reads && !reads)) throw DeviceError("null pointer: in_gfas and reads");
        // check_settings (combine.rs:57-67)
        for (uint32_t i = 0; i < n_gfas; i++) if (!in_gfas[i] || !fs::is_regular_file(in_gfas[i])) throw UserError(std::string("file does not exist: ") + (in_gfas[i] ? in_gfas[i] : "(null)"));
        for (uint32_t i = 0; i < n_reads; i++) if (!reads[i] || !fs::is_regular_file(reads[i])) throw UserError(std::string("file does not exist: ") + (reads[i] ? reads[i] : "(null)"));
        if (n_reads) {
            if (depth_kmer < 11) throw UserError("--depth_kmer cannot be less than 11");
            if (depth_kmer > 31) throw UserError("--depth_kmer cannot be greater than 31");
            if (depth_kmer % 2 == 0) throw UserError("--depth_kmer must be odd");
        }
        std::error_code ec;
        fs::create_directories(autocycler_dir, ec);
        if (ec) throw UserError(std::string("failed to create directory ") + autocycler_dir + "\n" + ec.message());
        std::vector<std::string> texts(n_gfas);
        std::vector<const char*> text_p(n_gfas);
        std::vector<uint64_t> text_n(n_gfas);
        for (uint32_t i = 0; i < n_gfas; i++) { texts[i] = read_input_file(in_gfas[i]); text_p[i] = texts[i].data(); text_n[i] = texts[i].size(); }
        // set_read_depths over all graphs together: one table
        std::vector<std::vector<double>> rd(n_gfas);
        std::vector<std::vector<uint8_t>> has(n_gfas);
        std::vector<const double*> rd_p; std::vector<const uint8_t*> has_p;
        if (n_reads) {
            std::vector<CombineGfa> loaded(n_gfas);
            std::vector<ac_depth_graph> dg(n_gfas);
            for (uint32_t i = 0; i < n_gfas; i++) {
                combine_load_gfa(text_p[i], text_n[i], &loaded[i]);
                const CombineGfa& c = loaded[i];
                dg[i] = ac_depth_graph{(const uint8_t*)text_p[i], c.seq_at.data(), c.len.data(), (uint32_t)c.number.size(), (const ac_link*)c.links.data(), c.links.size()};
            }
            ac_depth* dp = nullptr;
            if (ac_depth_begin(depth_kmer, dg.data(), n_gfas, device, &dp) != 0) throw DeviceError(last_error());
            struct FreeDepth { void operator()(ac_depth* p) const { ac_depth_free(p); } };
            std::unique_ptr<ac_depth, FreeDepth> d(dp);
            for (uint32_t i = 0; i < n_reads; i++) if (ac_depth_add_fastq(d.get(), reads[i]) != 0) throw DeviceError(last_error());
            for (uint32_t i = 0; i < n_gfas; i++) {
                rd[i].assign(loaded[i].number.size() + 1, 0.0); has[i].assign(loaded[i].number.size() + 1, 0);
                if (ac_depth_finish(d.get(), i, rd[i].data(), has[i].data()) != 0) throw DeviceError(last_error());
                rd_p.push_back(rd[i].data()); has_p.push_back(has[i].data());
            }
        }
        OwnedText gfa, fasta, yaml;
        uint64_t gfa_n = 0, fasta_n = 0, yaml_n = 0;
        ac_combined_summary sm;
        memset(&sm, 0, sizeof sm);
        sm.size = (uint32_t)sizeof sm;
        if (ac_combine_gfas(text_p.data(), text_n.data(), n_gfas, n_reads ? rd_p.data() : nullptr, n_reads ? has_p.data() : nullptr, device, &gfa.p, &gfa_n, &fasta.p, &fasta_n,
                            &yaml.p, &yaml_n, &sm) != 0)
            throw DeviceError(last_error());
        const fs::path dir(autocycler_dir);
        write_pieces((dir / "consensus_assembly.gfa").string(), {std::string(gfa.p, gfa_n)}, 1);
        write_pieces((dir / "consensus_assembly.fasta").string(), {std::string(fasta.p, fasta_n)}, 1);
        write_pieces((dir / "consensus_assembly.yaml").string(), {std::string(yaml.p, yaml_n)}, 1);
        if (report) {
            // print_read_depths (combine.rs:94-104) from the FASTA's own headers, then finished_message's verdict
            std::string r;
            if (n_reads) {
                r = "Sequence depths:\n";
                const std::string f(fasta.p, fasta_n);
                size_t a = 0;
                while (a < f.size()) {
                    size_t e = f.find('\n', a);
                    if (e == std::string::npos) e = f.size();
                    if (f[a] == '>') {
                        std::string h = f.substr(a + 1, e - a - 1);
                        const size_t cut = h.find(" circular=");
                        if (cut != std::string::npos) h.resize(cut);
                        r += "  " + h + "\n";
                    }
                    a = e + 1;
                }
            }
            r += sm.fully_resolved ? "Consensus assembly is fully resolved\n" : "One or more clusters failed to fully resolve\n";
            char* p = (char*)malloc(r.size() + 1);
            if (!p) throw DeviceError("out of memory");
            memcpy(p, r.c_str(), r.size() + 1);
            *report = p;
        }
    });
}
// gfa2fasta.rs:25-36
int ac_gfa2fasta(const char* in_gfa, const char* out_fasta, int device, uint64_t* counts) {
    return guarded([&] {
        if (!in_gfa || !out_fasta) throw DeviceError("null pointer: in_gfa and out_fasta are required");
        const std::string text = read_input_file(in_gfa);
        OwnedText fasta;
        uint64_t n = 0;
        if (ac_gfa2fasta_string(text.data(), text.size(), device, &fasta.p, &n, counts) != 0) throw DeviceError(last_error());
        write_pieces(out_fasta, {std::string(fasta.p, n)}, 1);
    });
}

}  // extern "C"
