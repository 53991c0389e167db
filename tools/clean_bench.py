#!/usr/bin/env python3
"""Times `autocycler clean`'s edit (ac_graph_clean / ac_clean_graph) on the graph this library builds for the mixed-species workload mini-E
and on a synthetic chain with low-depth stretches, on one MI355X, without torch.

    AC_NO_TORCH=1 python tools/clean_bench.py [--workloads configEmini_k51] [--chain-unitigs 4194304] [--stretch 32] [--repeats 3] [--out FILE]

mini-E: built with the library, then cleaned with min_depth = 1 (every unitig only one sequence visits is a candidate), a few of the highest
numbers removed and one tig duplicated where one can be.  Chain: 1 - 2 - ... - n in a row, every second stretch of `--stretch` unitigs low: as
many rounds as a stretch is long.  One warm-up call, then `--repeats` timed calls, the best one reported: device and end-to-end seconds, rounds,
launches and read-backs.  As the only comparison offered, the seconds of a plain numpy restatement of the removal-and-filter step (the alive
mask after remove, the links whose two ends are alive) in the same process: nothing else on the machine computes this edit, and the low-depth
rounds have no counterpart there.  No speed-up is claimed and no time is a pass condition.
Writes profiles/clean_bench.json, stamped with ac_source_hash.  Not a gate."""
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

KEYS = ("rounds", "launches", "read_backs", "seconds_device")


def best_of(call, repeats):
    """one warm-up call, then `repeats` timed ones -> (the last result's summary, the best run, all runs)"""
    call().close()
    runs, sm = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        res = call()
        runs.append(dict(end_to_end_s=time.perf_counter() - t, **{k: res.summary[k] for k in KEYS}))
        sm = res.summary
        res.close()
    return sm, min(runs, key=lambda r: r["end_to_end_s"]), runs


def numpy_remove_and_filter_seconds(np, n, links, remove):
    """the removal and the link filter restated with numpy: the alive mask, then the entries whose two ends are alive"""
    t = time.perf_counter()
    alive = np.ones(n + 1, dtype=bool)
    alive[0] = False
    alive[np.asarray(remove, dtype=np.int64)] = False
    keep = alive[np.abs(links[:, 0])] & alive[np.abs(links[:, 1])]
    kept = links[keep]
    return time.perf_counter() - t, len(kept)


def duplicable(np, n, links, limit=1):
    """numbers with exactly two non-self links (entries that leave either strand), the first `limit` of them"""
    a, b = np.abs(links[:, 0].astype(np.int64)), np.abs(links[:, 1].astype(np.int64))
    out = np.bincount(a[a != b], minlength=n + 1)
    return [int(u) for u in np.flatnonzero(out == 2)[:limit]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["configEmini_k51"])
    ap.add_argument("--chain-unitigs", type=int, default=1 << 22)
    ap.add_argument("--stretch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job and a short chain")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clean_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, clean_graph, synth
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
        a.chain_unitigs = min(a.chain_unitigs, 5000)
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    rows = []
    for name in (["emu dry run"] if a.emu else a.workloads):
        t0 = time.perf_counter()
        if a.emu:
            k, n_asm, asm = 21, 6, synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5)
        else:
            k, n_asm, gen = synth.WORKLOADS[name]
            asm = gen()
        seqs, fn, hd = synth.flatten(asm)
        bases = sum(len(s) for s in seqs)
        h_seqs = bench.prepare(lib, k, seqs, fn, hd, n_asm, threads=min(16, os.cpu_count() or 1), repair=1)
        del seqs, asm
        h = C.c_void_p()
        if lib.ac_compress_seqs(C.c_uint32(k), h_seqs, C.c_int(a.device), C.byref(h)):
            raise RuntimeError(lib.ac_last_error().decode())
        g = _capi.Graph(lib, h, lib.ac_graph_seq_count(h))
        lib.ac_seqs_free(h_seqs)
        build_s = time.perf_counter() - t0
        bulk = g.bulk()
        n = g.unitig_count
        links = np.ascontiguousarray(np.stack([bulk["links"]["a"], bulk["links"]["b"]], axis=1))
        remove = list(range(max(1, n - 7), n + 1))
        dup = [u for u in duplicable(np, n, links) if u not in remove]
        for label, options in (("min_depth 1", dict(min_depth=1.0)), ("remove 8, duplicate, min_depth 1", dict(remove=remove, duplicate=dup, min_depth=1.0)),
                               ("remove 8 alone", dict(remove=remove))):
            sm, best, runs = best_of(lambda: g.clean(device=a.device, **options), a.repeats)
            numpy_s, numpy_kept = numpy_remove_and_filter_seconds(np, n, links, options.get("remove", []))
            if "duplicate" not in options and "min_depth" not in options:
                assert numpy_kept == sm["links_out"]
            row = dict(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), options=label, kmer=k, input_bases=bases, unitigs=n, links_in=sm["links_in"],
                       links_out=sm["links_out"], removed=sm["removed"], duplicated=sm["duplicated"], low_depth=sm["low_depth"], kept_dead_end=sm["kept_dead_end"],
                       rounds_per_batch=sm["rounds_per_batch"], best=best, runs=runs, numpy_remove_and_filter_s=numpy_s, build_s=build_s)
            rows.append(row)
            print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
        g.close()
    # ---- a chain with low stretches: the rounds follow the stretch, not the chain ----
    n, stretch = a.chain_unitigs, a.stretch
    u = np.arange(1, n, dtype=np.int32)
    links = np.empty((2 * (n - 1), 2), dtype=np.int32)      # L-line order: u -> u + 1, then -u -> -(u - 1)
    fwd = np.stack([u, u + 1], axis=1)
    rev = np.stack([-(u + 1), -u], axis=1)
    order = np.argsort(np.concatenate([2 * (u.astype(np.int64) - 1), 2 * u.astype(np.int64) + 1]), kind="stable")
    links[:] = np.concatenate([fwd, rev])[order]
    depth = np.where((np.arange(n) // stretch) % 2 == 1, 0.5, 5.0)
    lens = np.full(n, 3, dtype=np.uint32)
    sm, best, runs = best_of(lambda: clean_graph(n, links, lens, depth=depth, min_depth=1.0, device=a.device, lib_path=lib_path), a.repeats)
    assert n < 2 * stretch or sm["rounds"] == stretch, sm      # a stretch of adjacent candidates is decided one per round, all stretches side by side
    numpy_s, _ = numpy_remove_and_filter_seconds(np, n, links, [])
    row = dict(workload=f"synthetic chain: {n} unitigs, every second stretch of {stretch} low", unitigs=n, links_in=sm["links_in"], links_out=sm["links_out"],
               low_depth=sm["low_depth"], kept_dead_end=sm["kept_dead_end"], rounds_per_batch=sm["rounds_per_batch"], best=best, runs=runs, numpy_remove_and_filter_s=numpy_s)
    rows.append(row)
    print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
    out = dict(tool="tools/clean_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(),
               note="device and end-to-end seconds of the edit; the numpy figure restates the removal-and-filter step alone; no speed-up is claimed", results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
