#!/usr/bin/env python3
"""Times ac_graph_subsets, one ac_subsets_merge_plan and one ac_subsets_merged_paths on the graphs this library builds for the mixed-species
workloads (E' and mini-E of autocycler_amd.synth), on one MI355X, without torch: the graph is built with the library, then the sequences
are put into 2, 8 and 50 synthetic clusters — by assembly index modulo C, and by species (one cluster per species: what `cluster` would find)
— one warm-up call, then `--repeats` timed calls, the best one reported.

    AC_NO_TORCH=1 python tools/subsets_bench.py [--workloads configEprime_k51 configEmini_k51] [--repeats 3] [--out FILE]

BASELINE configs[4] at full size (1.21 G path entries) is not among the workloads: the numpy restatement next to it would need the host
memory of the full-size job several times over.

Per workload and labelling: kept entries, (cluster, unitig) pairs, kept links, launches, read-backs, device seconds and end-to-end seconds
of the subsets call; the same for the merge plan and the re-threading of the largest cluster; and the seconds of a plain numpy restatement
of the subsets step in the same process (np.unique over the same (cluster, unitig) keys, a per-unitig bit row per cluster for the links) —
the only comparison offered: nothing else on the machine computes these subsets.  Writes profiles/subsets_bench.json, stamped with
ac_source_hash.  Not a gate."""
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


def numpy_subsets(n, links, entries, off, labels, n_clusters):
    """the subsets step in plain numpy: (pairs, kept links, seconds)"""
    import numpy as np
    t = time.perf_counter()
    label_of_entry = np.repeat(labels.astype(np.int64), np.diff(off.astype(np.int64)))
    keep = label_of_entry > 0
    keys, counts = np.unique((label_of_entry[keep] - 1) * n + (np.abs(entries[keep].astype(np.int64)) - 1), return_counts=True)
    words = (n_clusters + 63) // 64
    bits = np.zeros((n + 1, words), dtype=np.uint64)
    c, u = keys // n, keys % n + 1
    np.bitwise_or.at(bits, (u, c // 64), np.uint64(1) << (c % 64).astype(np.uint64))
    both = bits[np.abs(links["a"])] & bits[np.abs(links["b"])]
    kept = int(sum(int(np.unpackbits(both[:, w].view(np.uint8)).sum()) for w in range(words))) if len(links) else 0
    return len(keys), kept, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["configEprime_k51", "configEmini_k51"])
    ap.add_argument("--clusters", nargs="+", type=int, default=[2, 8, 50])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job instead of the workloads")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "subsets_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, graph_subsets, synth
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    rows = []
    for name in (["emu dry run"] if a.emu else a.workloads):
        t0 = time.perf_counter()
        if a.emu:
            k, n_asm, n_strains, asm = 21, 6, 3, synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5)
        else:
            k, n_asm, gen = synth.WORKLOADS[name]
            n_strains = {"configEprime_k51": 20, "configEmini_k51": 40}.get(name, n_asm)      # assembly i is strain i % n_strains of species i // n_strains
            asm = gen()
        seqs, fn, hd = synth.flatten(asm)
        assembly_of_seq = np.array([int(f[len("assembly_"):len("assembly_") + 4]) for f in fn], dtype=np.int64)
        h_seqs = bench.prepare(lib, k, seqs, fn, hd, n_asm, threads=min(16, os.cpu_count() or 1), repair=1)
        del seqs, asm
        h = C.c_void_p()
        if lib.ac_compress_seqs(C.c_uint32(k), h_seqs, C.c_int(a.device), C.byref(h)):
            raise RuntimeError(lib.ac_last_error().decode())
        g = _capi.Graph(lib, h, lib.ac_graph_seq_count(h))
        lib.ac_seqs_free(h_seqs)
        build_s = time.perf_counter() - t0
        bulk = g.bulk()
        n, n_seqs = g.unitig_count, len(bulk["path_off"]) - 1
        labellings = [(f"assembly index modulo {c}", c, (assembly_of_seq % c + 1).astype(np.uint16)) for c in a.clusters]
        n_species = int(assembly_of_seq.max()) // n_strains + 1
        labellings.append((f"by species ({n_species})", n_species, (assembly_of_seq // n_strains + 1).astype(np.uint16)))
        for label, nc, labels in labellings:
            graph_subsets(g, labels, nc, device=a.device).close()      # warm-up: arena growth, code load
            runs = []
            for rep in range(a.repeats):
                t = time.perf_counter()
                sub = graph_subsets(g, labels, nc, device=a.device)
                runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=sub.summary["seconds_device"]))
                if rep + 1 < a.repeats:
                    sub.close()
            best = min(runs, key=lambda r: r["end_to_end_s"])
            sm = sub.summary
            pairs, kept, numpy_s = numpy_subsets(n, bulk["links"], bulk["path_entries"], bulk["path_off"], labels, nc)
            assert pairs == sm["unitigs"] and kept == sm["links"], (pairs, sm["unitigs"], kept, sm["links"])
            big = int(np.argmax(sub.records["entries"])) + 1
            t = time.perf_counter()
            plan = sub.merge_plan(big, with_sequences=True, device=a.device)
            plan_s = time.perf_counter() - t
            t = time.perf_counter()
            mp = sub.merged_paths(big, plan, device=a.device)
            paths_s = time.perf_counter() - t
            row = dict(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), kmer=k, unitigs=n, links=len(bulk["links"]), sequences=n_seqs,
                       path_entries=len(bulk["path_entries"]), labelling=label, n_clusters=nc, entries_kept=sm["entries_kept"], pairs=sm["unitigs"], links_kept=sm["links"],
                       launches=sm["launches"], read_backs=sm["read_backs"], seconds_device=best["seconds_device"], end_to_end_s=best["end_to_end_s"], runs=runs,
                       numpy_s=numpy_s, build_s=build_s,
                       merge_plan=dict(cluster=big, unitigs=int(sub.records["unitigs"][big - 1]), links=int(sub.records["links"][big - 1]), chains=plan.summary["chains"],
                                       merged_unitigs=plan.summary["merged_unitigs"], bases_copied=plan.summary["bases_copied"], launches=plan.summary["launches"],
                                       read_backs=plan.summary["read_backs"], seconds_device=plan.summary["seconds_device"], end_to_end_s=plan_s),
                       merged_paths=dict(cluster=big, sequences=mp.summary["sequences"], entries_before=mp.summary["entries_before"], entries_after=mp.summary["entries_after"],
                                         launches=mp.summary["launches"], read_backs=mp.summary["read_backs"], seconds_device=mp.summary["seconds_device"], end_to_end_s=paths_s))
            rows.append(row)
            print(json.dumps(row), flush=True)
            plan.close(); sub.close()
        del bulk
        g.close()
    out = dict(tool="tools/subsets_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
