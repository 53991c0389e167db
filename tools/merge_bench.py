#!/usr/bin/env python3
"""Times ac_graph_merge_plan on the graphs this library builds for the mixed-species workloads (mini-E and E' of autocycler_amd.synth), on
one MI355X, without torch: the graph is built with the library (end repair and compress build on the device), then the plan runs on the
handle — with use_paths = 0 (a graph whose sequences were removed: everything mergeable merges; the heavy case) and use_paths = 1, each with
and without the merged sequences; one warm-up call, then `--repeats` timed calls, the best one reported.

    AC_NO_TORCH=1 python tools/merge_bench.py [--workloads configEmini_k51 configEprime_k51] [--full-size] [--repeats 3] [--out FILE]

--full-size adds BASELINE configs[4] itself (25 species x 40 strains x ~5 Mbp, the job of tests/fullsize_e.py: text resident in HBM).

Per workload and variant: chains, merged unitigs, unitigs and links after, bytes copied, launches, read-backs, the device time of all
kernels, the time of the sequence kernel alone and the end-to-end time of the call (uploads, kernels, read-backs, depths and types on the
host, the copies into numpy arrays).  The sequence kernel's bytes per second stand next to a plain device-to-device copy of the same size,
measured in the same run.  Writes profiles/merge_bench.json, stamped with ac_source_hash.  Not a gate and no speed-up: nothing else on the
machine computes this plan to compare with (the plain-Python model of tests/merge_util.py is a checker, not a baseline)."""
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


def plain_copy_seconds(hip, n_bytes, repeats=5):
    """hipMemcpy device to device of n_bytes, the best of `repeats` after one warm-up, by HIP events"""
    if n_bytes == 0:
        return 0.0
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)) == 0 and hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)) == 0
    assert hip.hipMemset(src, 65, C.c_size_t(n_bytes)) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    best = None
    for i in range(repeats + 1):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst, src, C.c_size_t(n_bytes), C.c_int(3), None) == 0
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if i:
            best = ms.value if best is None else min(best, ms.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipFree(src); hip.hipFree(dst)
    return 1e-3 * best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["configEmini_k51", "configEprime_k51"])
    ap.add_argument("--full-size", action="store_true", help="also BASELINE configs[4] at full size (tests/fullsize_e.py: 1000 assemblies, 5 G bp)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job instead of the workloads")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "merge_bench.json"))
    a = ap.parse_args()
    from autocycler_amd import _capi, graph_merge_plan, synth
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    hip = None if a.emu else C.CDLL("libamdhip64.so.7")
    rows = []
    FULL = "configs[4] at full size"
    for name in (["emu dry run"] if a.emu else a.workloads + ([FULL] if a.full_size else [])):
        t0 = time.perf_counter()
        if name == FULL:      # the text goes to the device by the HIP runtime itself (no torch), end repair and build on the resident text
            sys.path.insert(0, str(ROOT / "tests"))
            import fullsize_e
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
        links = len(g.bulk()["links"])
        for use_paths in (0, 1):
            for with_sequences in (0, 1):
                graph_merge_plan(g, use_paths, with_sequences, device=a.device)      # warm-up: arena growth, code load
                runs = []
                for _ in range(a.repeats):
                    t = time.perf_counter()
                    p = graph_merge_plan(g, use_paths, with_sequences, device=a.device)
                    runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=p.summary["seconds_device"], seconds_copy=p.summary["seconds_copy"]))
                best = min(runs, key=lambda r: r["end_to_end_s"])
                sm = p.summary
                row = dict(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), kmer=k, input_bases=bases, unitigs=g.unitig_count, links=links, use_paths=use_paths,
                           with_sequences=with_sequences, chains=sm["chains"], merged_unitigs=sm["merged_unitigs"], unitigs_after=sm["unitigs_after"],
                           links_after=sm["links_after"], bases_copied=sm["bases_copied"], longest_chain=int(p.chains["members"].max()) if sm["chains"] else 0,
                           launches=sm["launches"], read_backs=sm["read_backs"], seconds_device=best["seconds_device"], seconds_copy=best["seconds_copy"],
                           end_to_end_s=best["end_to_end_s"], runs=runs, generate_and_repair_s=t1 - t0, build_s=t2 - t1)
                if with_sequences and sm["bases_copied"] and hip is not None:
                    del p
                    copy_s = min(r["seconds_copy"] for r in runs)
                    plain_s = plain_copy_seconds(hip, sm["bases_copied"])
                    row.update(copy_gbytes_per_s=sm["bases_copied"] / copy_s / 1e9 if copy_s else None, plain_d2d_copy_s=plain_s,
                               plain_d2d_gbytes_per_s=sm["bases_copied"] / plain_s / 1e9 if plain_s else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
        g.close()
    # The graphs above are compress's own: their unitigs are maximal already, so little merges.  What a graph looks like after its sequences
    # were removed — long chains — is synthetic here: chains of `members` unitigs in a random order on random strands.
    import numpy as np
    from autocycler_amd import merge_plan_from_links
    for label, n, members, max_len in ([("synthetic emu", 5000, 100, 9)] if a.emu else
                                       [("synthetic: 16 Mi unitigs of 1 base, chains of 4096", 1 << 24, 4096, 1),
                                        ("synthetic: 4 Mi unitigs of 1-255 bases, chains of 4096", 1 << 22, 4096, 255),
                                        ("synthetic: 64 Ki unitigs of 1-32767 bases, chains of 16", 1 << 16, 16, 32767)]):
        rng = np.random.default_rng(3)
        s = (rng.permutation(n) + 1).astype(np.int64)
        s[rng.random(n) < 0.5] *= -1
        keep = (np.arange(1, n) % members) != 0      # no link across a chain boundary
        links = np.empty((2 * int(keep.sum()), 2), dtype=np.int32)
        links[0::2, 0] = s[:-1][keep]; links[0::2, 1] = s[1:][keep]
        links[1::2, 0] = -s[1:][keep]; links[1::2, 1] = -s[:-1][keep]
        lens = rng.integers(1, max_len + 1, n).astype(np.uint32)
        begin = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.uint64))).astype(np.uint64)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(lens.sum(dtype=np.uint64)))]
        call = lambda: merge_plan_from_links(n, links, lens, depth=np.ones(n), sequences=(seq, begin), device=a.device, lib_path=lib_path)
        call()
        runs = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            p = call()
            runs.append(dict(end_to_end_s=time.perf_counter() - t, seconds_device=p.summary["seconds_device"], seconds_copy=p.summary["seconds_copy"]))
        sm = p.summary
        assert sm["chains"] == (n + members - 1) // members - (1 if n % members == 1 else 0) and sm["bases_copied"] == len(seq) and sm["links_after"] == 0
        del p
        best = min(runs, key=lambda r: r["end_to_end_s"])
        copy_s = min(r["seconds_copy"] for r in runs)
        plain_s = plain_copy_seconds(hip, sm["bases_copied"]) if hip is not None else 0.0
        row = dict(workload=label, unitigs=n, links=len(links), use_paths=0, with_sequences=1, chains=sm["chains"], merged_unitigs=sm["merged_unitigs"],
                   unitigs_after=sm["unitigs_after"], links_after=sm["links_after"], bases_copied=sm["bases_copied"], longest_chain=members, launches=sm["launches"],
                   read_backs=sm["read_backs"], seconds_device=best["seconds_device"], seconds_copy=copy_s, end_to_end_s=best["end_to_end_s"], runs=runs,
                   copy_gbytes_per_s=sm["bases_copied"] / copy_s / 1e9 if copy_s else None, plain_d2d_copy_s=plain_s,
                   plain_d2d_gbytes_per_s=sm["bases_copied"] / plain_s / 1e9 if plain_s else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(tool="tools/merge_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
