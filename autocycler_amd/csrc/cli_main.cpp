// autocycler-compress — standalone driver with the flag surface of `autocycler compress` (main.rs:140-160):
//   -i/--assemblies_dir DIR  -a/--autocycler_dir DIR  [--kmer 51] [--max_contigs 25] [-t/--threads 8] [--device 0 | --devices 0,1,..] [--stats]
// (--devices: one job over several GPUs of the node through ac_compress_build_multi; --stats: the graph's connected components and
// topology after the usual lines, ac_graph_components; neither is a flag of the reference)
// Four more commands sit next to it: `decompress`, `clean`, `trim` and `resolve` (below).
// Writes DIR/input_assemblies.gfa and DIR/input_assemblies.yaml (compress.rs:45-46) through the C ABI
// (ac_compress_dir: C++ loader + end repair, HIP graph build, host tail, buffered GFA writer).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#include "../../include/autocycler_hip.h"

static void usage() {
    fprintf(stderr, "Usage: autocycler-compress --assemblies_dir <DIR> --autocycler_dir <DIR> [--kmer 51] [--max_contigs 25] [--threads 8] [--device 0 | --devices 0,1,..] [--stats]\n");
    fprintf(stderr, "       autocycler-compress decompress --in_gfa <GFA> [--out_dir <DIR>] [--out_file <FASTA>]\n");
    fprintf(stderr, "       autocycler-compress clean --in_gfa <GFA> --out_gfa <GFA> [--remove <TIGS>] [--duplicate <TIGS>] [--min_depth <DEPTH>] [--device 0]\n");
    fprintf(stderr, "       autocycler-compress trim --cluster_dir <DIR> [--min_identity 0.75] [--max_unitigs 5000] [--mad 5.0] [--device 0]\n");
    fprintf(stderr, "       autocycler-compress resolve --cluster_dir <DIR> [--device 0]\n");
}

// `autocycler decompress` (main.rs:163-175): -i/--in_gfa FILE  [-o/--out_dir DIR]  [-f/--out_file FASTA]
static int decompress_main(int argc, char** argv) {
    std::string in, dir, file;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        if (a == "-i" || a == "--in_gfa") in = val();
        else if (a == "-o" || a == "--out_dir") dir = val();
        else if (a == "-f" || a == "--out_file") file = val();
        else { fprintf(stderr, "error: unexpected argument '%s'\nUsage: autocycler-compress decompress --in_gfa <GFA> [--out_dir <DIR>] [--out_file <FASTA>]\n", a.c_str()); return 2; }
    }
    fprintf(stderr, "\nStarting autocycler decompress\nSettings:\n  --in_gfa %s\n", in.c_str());
    if (!dir.empty()) fprintf(stderr, "  --out_dir %s\n", dir.c_str());
    if (!file.empty()) fprintf(stderr, "  --out_file %s\n", file.c_str());
    if (ac_decompress(in.c_str(), dir.empty() ? nullptr : dir.c_str(), file.empty() ? nullptr : file.c_str(), 8) != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());
        return 1;
    }
    return 0;
}

// `autocycler clean` (main.rs: Clean): -i/--in_gfa FILE  -o/--out_gfa FILE  [-r/--remove 1,2]  [-d/--duplicate 3]  [-m/--min_depth 1.5]  [--device 0]
static int clean_main(int argc, char** argv) {
    std::string in, out, remove, duplicate, depth;
    bool has_remove = false, has_duplicate = false, has_depth = false;
    int device = 0;
    const char* use = "Usage: autocycler-compress clean --in_gfa <GFA> --out_gfa <GFA> [--remove <TIGS>] [--duplicate <TIGS>] [--min_depth <DEPTH>] [--device 0]\n";
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        if (a == "-i" || a == "--in_gfa") in = val();
        else if (a == "-o" || a == "--out_gfa") out = val();
        else if (a == "-r" || a == "--remove") { remove = val(); has_remove = true; }
        else if (a == "-d" || a == "--duplicate") { duplicate = val(); has_duplicate = true; }
        else if (a == "-m" || a == "--min_depth") { depth = val(); has_depth = true; }
        else if (a == "--device") device = atoi(val());
        else { fprintf(stderr, "error: unexpected argument '%s'\n%s", a.c_str(), use); return 2; }
    }
    if (in.empty() || out.empty()) { fprintf(stderr, "%s", use); return 2; }
    double min_depth = 0;
    if (has_depth) {
        char* end = nullptr;
        min_depth = strtod(depth.c_str(), &end);
        if (depth.empty() || *end) { fprintf(stderr, "error: invalid value '%s' for '--min_depth <MIN_DEPTH>'\n", depth.c_str()); return 2; }
    }
    fprintf(stderr, "\nStarting autocycler clean\nSettings:\n  --in_gfa %s\n  --out_gfa %s\n", in.c_str(), out.c_str());
    if (ac_clean(in.c_str(), out.c_str(), has_remove ? remove.c_str() : nullptr, has_duplicate ? duplicate.c_str() : nullptr, has_depth ? 1 : 0, min_depth, device) != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());
        return 1;
    }
    fprintf(stderr, "\nFinished!\nCleaned graph: %s\n\n", out.c_str());
    return 0;
}

// `autocycler trim` (main.rs: Trim): -c/--cluster_dir DIR  [--min_identity 0.75]  [--max_unitigs 5000]  [--mad 5.0]  [--device 0]
// `autocycler resolve` (main.rs: Resolve): -c/--cluster_dir DIR  [--device 0]   (--verbose is not offered)
static int cluster_dir_main(int argc, char** argv, bool trim) {
    std::string dir;
    double min_identity = 0.75, mad = 5.0;
    unsigned max_unitigs = 5000;
    int device = 0;
    const char* use = trim ? "Usage: autocycler-compress trim --cluster_dir <DIR> [--min_identity 0.75] [--max_unitigs 5000] [--mad 5.0] [--device 0]\n"
                           : "Usage: autocycler-compress resolve --cluster_dir <DIR> [--device 0]\n";
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        auto real = [&](const char* v, double* out) {
            char* end = nullptr;
            *out = strtod(v, &end);
            if (!*v || *end) { fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, a.c_str()); exit(2); }
        };
        if (a == "-c" || a == "--cluster_dir") dir = val();
        else if (trim && a == "--min_identity") real(val(), &min_identity);
        else if (trim && a == "--max_unitigs") max_unitigs = (unsigned)strtoul(val(), nullptr, 10);
        else if (trim && a == "--mad") real(val(), &mad);
        else if (a == "--device") device = atoi(val());
        else { fprintf(stderr, "error: unexpected argument '%s'\n%s", a.c_str(), use); return 2; }
    }
    if (dir.empty()) { fprintf(stderr, "%s", use); return 2; }
    fprintf(stderr, "\nStarting autocycler %s\nSettings:\n  --cluster_dir %s\n", trim ? "trim" : "resolve", dir.c_str());
    if (trim) fprintf(stderr, "  --min_identity %g\n  --max_unitigs %u\n  --mad %g\n", min_identity, max_unitigs, mad);
    const int rc = trim ? ac_trim_dir(dir.c_str(), min_identity, max_unitigs, mad, device) : ac_resolve_dir(dir.c_str(), device);
    if (rc != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());
        return 1;
    }
    if (trim) fprintf(stderr, "\nFinished!\nTrimmed graph: %s/2_trimmed.gfa\n\n", dir.c_str());
    else fprintf(stderr, "\nFinished!\nFinal graph: %s/5_final.gfa\n\n", dir.c_str());
    return 0;
}

// `autocycler combine` (main.rs: Combine): -a/--autocycler_dir DIR  -i/--in_gfas A.gfa [B.gfa ...]  [-r/--reads R.fastq ...]  [--depth_kmer 19]  [--device 0]
static int combine_main(int argc, char** argv) {
    std::string dir;
    std::vector<const char*> gfas, reads;
    unsigned depth_kmer = 19;
    int device = 0;
    const char* use = "Usage: autocycler-compress combine --autocycler_dir <DIR> --in_gfas <GFA>... [--reads <FASTQ>...] [--depth_kmer 19] [--device 0]\n";
    std::vector<const char*>* list = nullptr;      // the option whose values are being read
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        if (a == "-a" || a == "--autocycler_dir") { dir = val(); list = nullptr; }
        else if (a == "-i" || a == "--in_gfas") { gfas.push_back(val()); list = &gfas; }
        else if (a == "-r" || a == "--reads") { reads.push_back(val()); list = &reads; }
        else if (a == "--depth_kmer") { depth_kmer = (unsigned)strtoul(val(), nullptr, 10); list = nullptr; }
        else if (a == "--device") { device = atoi(val()); list = nullptr; }
        else if (list && !a.empty() && a[0] != '-') list->push_back(argv[i]);
        else { fprintf(stderr, "error: unexpected argument '%s'\n%s", a.c_str(), use); return 2; }
    }
    if (dir.empty() || gfas.empty()) { fprintf(stderr, "%s", use); return 2; }
    fprintf(stderr, "\nStarting autocycler combine\nSettings:\n  --autocycler_dir %s\n  --in_gfas %s\n", dir.c_str(), gfas[0]);
    for (size_t i = 1; i < gfas.size(); i++) fprintf(stderr, "            %s\n", gfas[i]);
    if (!reads.empty()) {
        fprintf(stderr, "  --reads %s\n", reads[0]);
        for (size_t i = 1; i < reads.size(); i++) fprintf(stderr, "          %s\n", reads[i]);
        fprintf(stderr, "  --depth_kmer %u\n", depth_kmer);
    }
    char* report = nullptr;
    if (ac_combine(dir.c_str(), gfas.data(), (uint32_t)gfas.size(), reads.empty() ? nullptr : reads.data(), (uint32_t)reads.size(), depth_kmer, device, &report) != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());
        return 1;
    }
    fprintf(stderr, "\n%s", report ? report : "");
    ac_string_free(report);
    fprintf(stderr, "\nFinished!\nCombined graph: %s/consensus_assembly.gfa\nCombined fasta: %s/consensus_assembly.fasta\n\n", dir.c_str(), dir.c_str());
    return 0;
}

// `autocycler gfa2fasta` (main.rs: Gfa2fasta): -i/--in_gfa FILE  -o/--out_fasta FILE  [--device 0]
static int gfa2fasta_main(int argc, char** argv) {
    std::string in, out;
    int device = 0;
    const char* use = "Usage: autocycler-compress gfa2fasta --in_gfa <GFA> --out_fasta <FASTA> [--device 0]\n";
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        if (a == "-i" || a == "--in_gfa") in = val();
        else if (a == "-o" || a == "--out_fasta") out = val();
        else if (a == "--device") device = atoi(val());
        else { fprintf(stderr, "error: unexpected argument '%s'\n%s", a.c_str(), use); return 2; }
    }
    if (in.empty() || out.empty()) { fprintf(stderr, "%s", use); return 2; }
    fprintf(stderr, "\nStarting autocycler gfa2fasta\nSettings:\n  --in_gfa %s\n  --out_fasta %s\n\n", in.c_str(), out.c_str());
    uint64_t counts[3] = {0, 0, 0};
    if (ac_gfa2fasta(in.c_str(), out.c_str(), device, counts) != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());
        return 1;
    }
    const char* what[3] = {"circular", "linear", "other"};
    for (int c = 0; c < 3; c++) fprintf(stderr, "%llu %s sequence%s\n", (unsigned long long)counts[c], what[c], counts[c] == 1 ? "" : "s");
    fprintf(stderr, "\nFinished!\n\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "decompress") == 0) return decompress_main(argc, argv);
    if (argc > 1 && strcmp(argv[1], "combine") == 0) return combine_main(argc, argv);
    if (argc > 1 && strcmp(argv[1], "gfa2fasta") == 0) return gfa2fasta_main(argc, argv);
    if (argc > 1 && strcmp(argv[1], "trim") == 0) return cluster_dir_main(argc, argv, true);
    if (argc > 1 && strcmp(argv[1], "resolve") == 0) return cluster_dir_main(argc, argv, false);
    if (argc > 1 && strcmp(argv[1], "clean") == 0) return clean_main(argc, argv);
    std::string in, out;
    unsigned k = 51, max_contigs = 25;
    int threads = 8, device = 0;
    bool stats = false;
    std::vector<int> devices;
    int i = 1;
    if (argc > 1 && strcmp(argv[1], "compress") == 0) i = 2;
    for (; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", a.c_str()); usage(); exit(2); }
            return argv[++i];
        };
        if (a == "-i" || a == "--assemblies_dir") in = val();
        else if (a == "-a" || a == "--autocycler_dir") out = val();
        else if (a == "--kmer") k = (unsigned)strtoul(val(), nullptr, 10);
        else if (a == "--max_contigs") max_contigs = (unsigned)strtoul(val(), nullptr, 10);
        else if (a == "-t" || a == "--threads") threads = atoi(val());
        else if (a == "--device") device = atoi(val());
        else if (a == "--devices") { const char* v = val(); for (const char* q = v; *q;) { devices.push_back(atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; } }
        else if (a == "--stats") stats = true;
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str()); usage(); return 2; }
    }
    if (in.empty() || out.empty()) { usage(); return 2; }
    auto t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "\nStarting autocycler compress (%s)\n", ac_version());
    fprintf(stderr, "Settings:\n  --assemblies_dir %s\n  --autocycler_dir %s\n  --kmer %u\n  --threads %d\n\n", in.c_str(), out.c_str(), k, threads);
    ac_graph* g = nullptr;
    double times[4] = {0, 0, 0, 0};
    const int rc = devices.size() > 1 ? ac_compress_dir_multi(in.c_str(), out.c_str(), k, max_contigs, threads, devices.data(), (int)devices.size(), &g, times)
                                      : ac_compress_dir(in.c_str(), out.c_str(), k, max_contigs, threads, devices.empty() ? device : devices[0], &g, times);
    if (rc != 0) {
        fprintf(stderr, "\nError: %s\n", ac_last_error());    // quit_with_error, misc.rs:131-137
        return 1;
    }
    ac_stats pre = ac_stats_pre(g), post = ac_stats_post(g);
    fprintf(stderr, "Graph contains %llu k-mers\n\n", (unsigned long long)ac_kmer_count(g));
    fprintf(stderr, "%u unitig%s, %llu link%s\ntotal length: %llu bp\n\n", pre.unitigs, pre.unitigs == 1 ? "" : "s",
            (unsigned long long)pre.links_one_way, pre.links_one_way == 1 ? "" : "s", (unsigned long long)pre.total_length);
    fprintf(stderr, "%u unitig%s, %llu link%s\ntotal length: %llu bp\n\n", post.unitigs, post.unitigs == 1 ? "" : "s",
            (unsigned long long)post.links_one_way, post.links_one_way == 1 ? "" : "s", (unsigned long long)post.total_length);
    if (stats) {
        ac_components* c = nullptr;
        ac_components_summary sm;
        if (ac_graph_components(g, nullptr, devices.empty() ? device : devices[0], &c) != 0) { fprintf(stderr, "\nError: %s\n", ac_last_error()); return 1; }
        ac_components_summary_get_sized(c, &sm, sizeof sm);
        fprintf(stderr, "%u connected component%s (%s)\n\n", sm.components, sm.components == 1 ? "" : "s", ac_topology_name(sm.topology));
        ac_components_free(c);
    }
    ac_free(g);
    double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "Compressed unitig graph: %s/input_assemblies.gfa\nInput assembly stats:    %s/input_assemblies.yaml\n", out.c_str(), out.c_str());
    fprintf(stderr, "Stage times: load %.3fs, end repair %.3fs, graph build (GPU hot path) %.3fs, write %.3fs\n", times[0], times[1], times[2], times[3]);
    unsigned long long us = (unsigned long long)(total * 1e6);
    fprintf(stderr, "Time to run: %llu:%02llu:%02llu.%06llu\n\n", us / 1000000 / 3600, us / 1000000 / 60 % 60, us / 1000000 % 60, us % 1000000);
    // the output files are written and closed: leave without tearing down the HIP runtime, the device arena and the pinned pools
    // (tens of milliseconds of a sub-second command)
    fflush(stdout); fflush(stderr);
    _exit(0);
}
