#!/usr/bin/env python3
"""Times Subsets.finish (ac_subsets_finish) on the graphs this library builds for the mixed-species workloads (E' and mini-E of
autocycler_amd.synth) and ac_merge_finish on three synthetic tie shapes, on one MI355X, without torch.

    AC_NO_TORCH=1 python tools/finish_bench.py [--workloads configEprime_k51 configEmini_k51] [--tie-n 16777216] [--repeats 3] [--out FILE]

Workloads: the sequences go into C = 2 and C = 50 clusters by assembly index modulo C; the largest cluster's plan and merged paths are made
once and the cluster is finished with renumber 0 and 1 — one warm-up call, then `--repeats` timed calls, the best one reported.
Tie shapes, `--tie-n` unitigs without links, renumber 1: one-base unitigs over ACGT (huge full ties, all settled by the radix keys);
40-base unitigs that share their first 32 bytes (one tie group of all of them); 24-base unitigs in groups of 64 that are identical but for
the last byte.

Per row: unitigs, bases, links, path entries, tie items, launches, read-backs, device seconds and end-to-end seconds; the sequence gather's
seconds and bytes per second next to a plain device-to-device copy of the same bytes in the same run; and, as the only comparison offered,
the seconds of a plain numpy / sorted() restatement of the renumbering in the same process (nothing else on the machine computes this
order).  Writes profiles/finish_bench.json, stamped with ac_source_hash.  Not a gate."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
os.environ.setdefault("AC_NO_TORCH", "1")


def host_renumber_seconds(fin):
    """renumber_unitigs restated on the host over the library's own records: sorted() by (length descending, sequence, depth descending) from
    the order before the sort; returns (seconds, whether it is the library's order)"""
    import numpy as np
    u = fin.unitigs
    seqs = fin.unitig_sequences()
    first = np.argsort(u["source"], kind="stable").tolist()
    depth = (u["depth"] + 0.0).tolist()
    t = time.perf_counter()
    order = sorted(first, key=lambda i: (-len(seqs[i]), seqs[i], -depth[i]))
    s = time.perf_counter() - t
    return s, order == list(range(len(u)))


def numpy_renumber_seconds(arr, depths):
    """the same for equal-length sequences given as an (n, L) uint8 array: a stable lexsort"""
    import numpy as np
    t = time.perf_counter()
    order = np.lexsort([-(depths + 0.0)] + [arr[:, j] for j in range(arr.shape[1] - 1, -1, -1)])
    return time.perf_counter() - t, order


def summary_row(sm, best, runs, plain_s):
    gather = min(r["seconds_gather"] for r in runs)
    return dict(unitigs=sm["unitigs"], bases=sm["bases"], links=sm["links"], path_entries=sm["path_entries"], tie_items=sm["tie_items"], launches=sm["launches"],
                read_backs=sm["read_backs"], seconds_device=best["seconds_device"], end_to_end_s=best["end_to_end_s"], runs=runs, seconds_gather=gather,
                gather_gbytes_per_s=sm["bases"] / gather / 1e9 if gather else None, plain_d2d_copy_s=plain_s,
                plain_d2d_gbytes_per_s=sm["bases"] / plain_s / 1e9 if plain_s else None)


def tie_shapes(n, rng):
    import numpy as np
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    yield "one-base unitigs over ACGT", rng.choice(acgt, (n, 1))
    shared = np.empty((n, 40), dtype=np.uint8)
    shared[:, :32] = rng.choice(acgt, 32)
    shared[:, 32:] = rng.choice(acgt, (n, 8))
    yield "40 bases, the first 32 shared", shared
    groups = (n + 63) // 64
    body = np.repeat(rng.choice(acgt, (groups, 24)), 64, axis=0)[:n].copy()
    body[:, 23] = rng.choice(acgt, n)
    yield "24 bases, groups of 64 identical but for the last byte", body[rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["configEprime_k51", "configEmini_k51"])
    ap.add_argument("--clusters", nargs="+", type=int, default=[2, 50])
    ap.add_argument("--tie-n", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job and small tie shapes")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "finish_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, graph_subsets, merge_finish, merge_plan_from_links, synth
    import bench
    from merge_bench import plain_copy_seconds
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
        a.tie_n = min(a.tie_n, 3000)
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    hip = None if a.emu else C.CDLL("libamdhip64.so.7")
    rows = []
    for name in (["emu dry run"] if a.emu else a.workloads):
        t0 = time.perf_counter()
        if a.emu:
            k, n_asm, asm = 21, 6, synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5)
        else:
            k, n_asm, gen = synth.WORKLOADS[name]
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
        for nc in a.clusters:
            labels = (assembly_of_seq % nc + 1).astype(np.uint16)
            sub = graph_subsets(g, labels, nc, device=a.device)
            big = int(np.argmax(sub.records["entries"])) + 1
            plan = sub.merge_plan(big, with_sequences=True, device=a.device)
            mp = sub.merged_paths(big, plan, device=a.device, keep=True)
            for renumber in (False, True):
                sub.finish(big, plan, mp, renumber=renumber, device=a.device).close()      # warm-up: arena growth, code load
                runs = []
                for rep in range(a.repeats):
                    t = time.perf_counter()
                    fin = sub.finish(big, plan, mp, renumber=renumber, device=a.device)
                    runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=fin.summary["seconds_device"], seconds_gather=fin.summary["seconds_gather"]))
                    if rep + 1 < a.repeats:
                        fin.close()
                best = min(runs, key=lambda r: r["end_to_end_s"])
                row = dict(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), kmer=k, n_clusters=nc, cluster=big, renumber=int(renumber), chains=plan.summary["chains"],
                           build_s=build_s, **summary_row(fin.summary, best, runs, plain_copy_seconds(hip, fin.summary["bases"]) if hip is not None else 0.0))
                if renumber:
                    row["host_sorted_s"], same = host_renumber_seconds(fin)
                    assert same, "sorted() disagrees with the library's order"
                rows.append(row)
                print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
                fin.close()
            mp.close(); plan.close(); sub.close()
        g.close()
    rng = np.random.default_rng(12)
    for label, arr in (tie_shapes(a.tie_n, rng) if a.tie_n > 0 else ()):
        n, length = arr.shape
        depths = rng.choice(np.array([1.0, 2.5, 40.0]), n)
        lens = np.full(n, length, dtype=np.uint32)
        sequences = (np.ascontiguousarray(arr).reshape(-1), np.arange(n, dtype=np.uint64) * np.uint64(length))
        links = np.zeros((0, 2), dtype=np.int32)
        plan = merge_plan_from_links(n, links, lens, depth=depths, device=a.device, lib_path=lib_path, keep=True)
        call = lambda: merge_finish(plan, n, links, lens, depth=depths, sequences=sequences, renumber=True, device=a.device, lib_path=lib_path)
        call().close()
        runs = []
        for rep in range(a.repeats):
            t = time.perf_counter()
            fin = call()
            runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=fin.summary["seconds_device"], seconds_gather=fin.summary["seconds_gather"]))
            if rep + 1 < a.repeats:
                fin.close()
        best = min(runs, key=lambda r: r["end_to_end_s"])
        numpy_s, order = numpy_renumber_seconds(arr, depths)
        assert np.array_equal(order + 1, fin.unitigs["source"]), "numpy's lexsort disagrees with the library's order"
        row = dict(workload=f"tie shape: {label}", n=n, length=length, renumber=1, numpy_lexsort_s=numpy_s,
                   **summary_row(fin.summary, best, runs, plain_copy_seconds(hip, fin.summary["bases"]) if hip is not None else 0.0))
        rows.append(row)
        print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
        fin.close(); plan.close()
    out = dict(tool="tools/finish_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
