#!/usr/bin/env python3
"""Times ac_graph_components on the graphs this library builds for the mixed-species workloads (mini-E and E' of autocycler_amd.synth), on one
MI355X, without torch: the graph is built with the library (end repair and compress build on the device), then the analysis runs on the
handle — one warm-up call, then `--repeats` timed calls, the best one reported.

    AC_NO_TORCH=1 python tools/components_bench.py [--workloads configEmini_k51 configEprime_k51] [--full-size] [--repeats 3] [--out FILE]

--full-size adds BASELINE configs[4] itself (25 species x 40 strains x ~5 Mbp, the job of tests/fullsize_e.py: text resident in HBM).

Per workload: unitigs, links (L lines), components, circular loops, topology, launches, read-backs, the device time from the first kernel to
the last (the handle's own two events) and the end-to-end time of the call (upload of the links and lengths, kernels, read-back, totals on
the host).  Writes profiles/components_bench.json, stamped with ac_source_hash.  Not a gate and no speed-up: nothing else on the machine
computes these components to compare with (the plain-Python model of tests/components_util.py is a checker, not a baseline)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("AC_NO_TORCH", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["configEmini_k51", "configEprime_k51"])
    ap.add_argument("--full-size", action="store_true", help="also BASELINE configs[4] at full size (tests/fullsize_e.py: 1000 assemblies, 5 G bp)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job instead of the workloads")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "components_bench.json"))
    a = ap.parse_args()
    from autocycler_amd import _capi, graph_components, synth
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    rows = []
    FULL = "configs[4] at full size"
    for name in (["emu dry run"] if a.emu else a.workloads + ([FULL] if a.full_size else [])):
        t0 = time.perf_counter()
        if name == FULL:      # the text goes to the device by the HIP runtime itself (no torch), end repair and build on the resident text
            sys.path.insert(0, str(ROOT / "tests"))
            import fullsize_e
            hip = C.CDLL("libamdhip64.so.7")
            job = fullsize_e.make_job(25, 40)
            k, bases = job["k"], job["bases"]
            d_text = C.c_void_p()
            assert hip.hipSetDevice(a.device) == 0 and hip.hipMalloc(C.byref(d_text), C.c_size_t(job["n_text"])) == 0
            assert hip.hipMemcpy(d_text, job["text"].ctypes.data_as(C.c_void_p), C.c_size_t(job["n_text"]), C.c_int(1)) == 0
            t1 = time.perf_counter()
            g = fullsize_e.build_device(lib, job, d_text.value, repair=True, builds=1)[0]
            hip.hipFree(d_text)
            del job
            t2 = time.perf_counter()
        elif a.emu:
            k, n_asm, asm = 21, 6, synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5)
        else:
            k, n_asm, gen = synth.WORKLOADS[name]
            asm = gen()
        if name != FULL:
            seqs, fn, hd = synth.flatten(asm)
            bases = sum(len(s) for s in seqs)
            h_seqs = bench.prepare(lib, k, seqs, fn, hd, n_asm, threads=min(16, os.cpu_count() or 1), repair=1)
            del seqs, asm
            t1 = time.perf_counter()
            h = C.c_void_p()
            if lib.ac_compress_seqs(C.c_uint32(k), h_seqs, C.c_int(a.device), C.byref(h)):
                raise RuntimeError(lib.ac_last_error().decode())
            g = _capi.Graph(lib, h, lib.ac_graph_seq_count(h))
            lib.ac_seqs_free(h_seqs)
            t2 = time.perf_counter()
        graph_components(g, device=a.device)      # warm-up: arena growth, code load
        runs = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            c = graph_components(g, device=a.device)
            runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=c.summary["seconds_device"]))      # (end to end: with the copies into numpy arrays)
        best = min(runs, key=lambda r: r["end_to_end_s"])
        sm = c.summary
        assert sm["links_one_way"] == g.stats_post["links"] and sm["total_length"] == g.stats_post["total_length"] and sm["unitigs"] == g.unitig_count
        links = len(g.bulk()["links"])
        row = dict(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), kmer=k, input_bases=bases, unitigs=sm["unitigs"], links=links, links_all=sm["links_all"],
                   links_one_way=sm["links_one_way"], components=sm["components"], circular_loops=int(c.records["circular_loop"].sum()),
                   largest_component=int(c.records["unitigs"].max()), topology=c.topology, launches=sm["launches"], read_backs=sm["read_backs"],
                   seconds_device=best["seconds_device"], end_to_end_s=best["end_to_end_s"], runs=runs, generate_and_repair_s=t1 - t0, build_s=t2 - t1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        g.close()
    out = dict(tool="tools/components_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
