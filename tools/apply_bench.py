#!/usr/bin/env python3
"""Times resolve's graph edit (ac_graph_resolve_apply, ac_applied_merge_plan, ac_applied_finish) on config C's chromosome — one genome, 96
assemblies, so that anchors exist — and ac_apply_bridges on synthetic rings of anchors with planted bridges, on one MI355X, without torch.

    AC_NO_TORCH=1 python tools/apply_bench.py [--assemblies 96] [--genome 5000000] [--ring-bridges 1000000] [--repeats 3] [--out FILE]

Config C (BASELINE.json configs[2]'s model without the plasmid contigs: the chromosome's cluster, which is what `resolve` is run on): built, resolved (ac_resolve_bridges), applied (both passes), planned and finished with renumbering — one warm-up call, then
`--repeats` timed calls per stage, the best one reported: device and end-to-end seconds, launches and read-backs per stage.
Rings: A anchors on a ring, the bridge from each to the next over m member unitigs of its own, for member sizes of 1 base (m = 8),
128 bytes (m = 2) and 16 KB (m = 1; fewer bridges, so that the bytes stay below 1 GB): the copy kernel's seconds and bytes per second next to a
plain device-to-device copy of the same bytes in the same run; and, as the only comparison offered, the seconds of a plain numpy
restatement of the link edit and the depths in the same process (nothing else on the machine computes this edit).
Writes profiles/apply_bench.json, stamped with ac_source_hash.  Not a gate."""
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


def best_of(call, repeats, keys):
    """one warm-up call, then `repeats` timed ones -> (the last result, the best run, all runs)"""
    call().close()
    runs, res = [], None
    for rep in range(repeats):
        if res is not None:
            res.close()
        t = time.perf_counter()
        res = call()
        runs.append(dict(end_to_end_s=time.perf_counter() - t, **{k: res.summary[k] for k in keys}))
    return res, min(runs, key=lambda r: r["end_to_end_s"]), runs


def ring(np, n_bridges, members, size):
    """the arrays of a ring: anchors 1 .. A, bridge i from anchor i to the next over `members` unitigs of `size` bases that are its own"""
    A, m = n_bridges, members
    n = A + A * m
    first = A + 1 + np.arange(A, dtype=np.int64) * m                       # the first member of bridge i
    chain = first[:, None] + np.arange(m, dtype=np.int64)[None, :]        # (A, m)
    nodes = np.concatenate([np.arange(1, A + 1, dtype=np.int64)[:, None], chain, np.roll(np.arange(1, A + 1, dtype=np.int64), -1)[:, None]], axis=1)
    fwd = np.stack([nodes[:, :-1].reshape(-1), nodes[:, 1:].reshape(-1)], axis=1)
    links = np.ascontiguousarray(np.concatenate([fwd, -fwd[:, ::-1]]).astype(np.int32))
    lens = np.concatenate([np.full(A, 3, dtype=np.uint32), np.full(A * m, size, dtype=np.uint32)])
    depth = np.concatenate([np.full(A, 4.0), np.full(A * m, 2.0)])
    begin = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(3).integers(0, 4, int(lens.sum(dtype=np.uint64)) + 1)]
    bdt = np.dtype([("start", "<i4"), ("end", "<i4"), ("depth", "<u4"), ("n_distinct", "<u4"), ("best_off", "<u8"), ("best_total", "<u8"), ("first_distinct", "<u8"),
                    ("best_len", "<u4"), ("status", "<u4"), ("conflicting", "<u4"), ("culled", "<u4"), ("cull_rank", "<u4"), ("reserved", "<u4")])
    br = np.zeros(A, dtype=bdt)
    br["start"], br["end"] = np.arange(1, A + 1), np.roll(np.arange(1, A + 1), -1)
    br["depth"] = br["n_distinct"] = 1
    br["best_off"] = br["first_distinct"] = 0
    br["best_off"] = np.arange(A, dtype=np.uint64) * m
    br["first_distinct"] = np.arange(A, dtype=np.uint64)
    br["best_len"] = m
    best = np.ascontiguousarray(chain.reshape(-1).astype(np.int32))
    off = (np.arange(A + 1, dtype=np.uint64) * m).astype(np.uint64)
    return dict(n=n, links=links, lens=lens, depth=depth, anchors=np.arange(1, A + 1, dtype=np.uint32), seq=np.ascontiguousarray(seq), begin=begin, bridges=br, best=best,
                dist=best, off=off, mult=np.ones(A, dtype=np.uint32), apply=np.ones(A, dtype=np.uint8))


def numpy_edit_seconds(np, r):
    """the link edit and the depths restated with numpy: which entries survive, the created ones, the visit counts and the clamp"""
    t = time.perf_counter()
    a, b = r["links"][:, 0], r["links"][:, 1]
    s, e = r["bridges"]["start"], r["bridges"]["end"]
    keep = ~np.isin(a, np.concatenate([s, -e])) & ~np.isin(b, np.concatenate([e, -s]))
    new = r["n"] + 1 + np.arange(len(s), dtype=np.int32)
    created = np.stack([np.stack([s, new], 1), np.stack([new, e], 1), np.stack([-new, -s], 1), np.stack([-e, -new], 1)], 1).reshape(-1, 2)
    edited = np.concatenate([r["links"][keep], created])
    visits = np.bincount(np.abs(r["dist"]) - 1, minlength=r["n"])
    depth = np.where(visits == 0, r["depth"], np.maximum(r["depth"] - visits, 0.0))
    return time.perf_counter() - t, len(edited), float(depth.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assemblies", type=int, default=96)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--ring-bridges", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small job and small rings")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "apply_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, synth
    import bench
    from merge_bench import plain_copy_seconds
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
        a.ring_bridges = min(a.ring_bridges, 2000)
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    hip = None if a.emu else C.CDLL("libamdhip64.so.7")
    rows = []
    # ---- config C's chromosome cluster: one genome, 96 assemblies, no plasmid contigs (with them no unitig is in every sequence: no anchors) ----
    t0 = time.perf_counter()
    if a.emu:
        name, k, n_asm, asm = "emu dry run", 21, 6, synth.make_assemblies(6, genome=20_000, plasmid=0, sub=1e-3, indel=1e-4, seed=5)
    else:
        name, k, n_asm = f"config C, chromosome cluster ({a.assemblies} x {a.genome} bp)", 51, a.assemblies
        asm = synth.make_assemblies(a.assemblies, genome=a.genome, plasmid=0, sub=1e-4, indel=1e-5, seed=51_000)
    seqs, fn, hd = synth.flatten(asm)
    h_seqs = bench.prepare(lib, k, seqs, fn, hd, n_asm, threads=min(16, os.cpu_count() or 1), repair=1)
    del seqs, asm
    h = C.c_void_p()
    if lib.ac_compress_seqs(C.c_uint32(k), h_seqs, C.c_int(a.device), C.byref(h)):
        raise RuntimeError(lib.ac_last_error().decode())
    g = _capi.Graph(lib, h, lib.ac_graph_seq_count(h))
    lib.ac_seqs_free(h_seqs)
    build_s = time.perf_counter() - t0
    t = time.perf_counter()
    anchors, bridges, rsm = g.resolve_bridges(device=a.device)
    resolve_s = time.perf_counter() - t
    row = dict(workload=name, kmer=k, unitigs=g.unitig_count, anchors=len(anchors), bridges=len(bridges),
               conflicting=sum(b["conflicting"] for b in bridges), culled=sum(b["culled"] for b in bridges), build_s=build_s, resolve_end_to_end_s=resolve_s,
               resolve_seconds_device=rsm["seconds_device"], stages={})
    keys = ("launches", "read_backs", "seconds_device")
    rh = C.c_void_p()      # the bridges once, as a handle: the timed calls apply them
    if lib.ac_resolve_bridges(g._h, a.device, C.byref(rh)):
        raise RuntimeError(lib.ac_last_error().decode())

    def apply_handle(which):
        out = C.c_void_p()
        if lib.ac_graph_resolve_apply(g._h, rh, _capi.Applied.UNIQUE if which == "unique" else _capi.Applied.KEPT, a.device, C.byref(out)):
            raise RuntimeError(lib.ac_last_error().decode())
        return _capi.Applied(lib, out)
    for which in ("unique", "kept"):
        ap_, best, runs = best_of(lambda: apply_handle(which), a.repeats, keys + ("launches_components", "seconds_copy", "seconds_components"))
        row["stages"][f"apply {which}"] = dict(best, runs=runs, **{k_: ap_.summary[k_] for k_ in ("bridges_applied", "direct_links", "removed_no_anchor", "removed_zero_depth",
                                                                                                  "links_in", "links_out", "bases_copied")})
        plan, best, runs = best_of(lambda: ap_.merge_plan(device=a.device), a.repeats, keys + ("seconds_copy",))
        row["stages"][f"plan {which}"] = dict(best, runs=runs, chains=plan.summary["chains"], unitigs_after=plan.summary["unitigs_after"])
        fin, best, runs = best_of(lambda: ap_.finish(plan, renumber=True, device=a.device), a.repeats, keys + ("seconds_gather",))
        row["stages"][f"finish {which}"] = dict(best, runs=runs, unitigs=fin.summary["unitigs"], links=fin.summary["links"], bases=fin.summary["bases"])
        fin.close(); plan.close(); ap_.close()
    t = time.perf_counter()
    texts = g.resolve_graphs(device=a.device)
    row["resolve_graphs_end_to_end_s"], row["text_bytes"], row["cull_count"] = time.perf_counter() - t, [len(x) for x in texts[:3]], texts[3]
    rows.append(row)
    print(json.dumps({k_: v for k_, v in row.items() if k_ != "stages"}), flush=True)
    lib.ac_resolve_free(rh)
    g.close()
    # ---- rings of anchors with planted bridges ----
    lib.ac_apply_bridges.restype = C.c_int
    for label, members, size, n_bridges in (("1-base members", 8, 1, a.ring_bridges), ("128-byte members", 2, 128, a.ring_bridges),
                                            ("16 KB members", 1, 16384, max(1, min(a.ring_bridges, 32768) // (64 if a.emu else 1)))):
        r = ring(np, n_bridges, members, size)
        p = lambda x: x.ctypes.data

        class Result:
            def __init__(self, handle):
                self.h = handle
                sm = _capi.AppliedSummary()
                lib.ac_applied_summary_get_sized(handle, C.byref(sm), C.sizeof(sm))
                self.summary = sm.as_dict()

            def close(self):
                lib.ac_applied_free(self.h)

        def call():
            out = C.c_void_p()
            rc = lib.ac_apply_bridges(r["n"], p(r["links"]), len(r["links"]), p(r["lens"]), None, p(r["depth"]), p(r["anchors"]), len(r["anchors"]), p(r["seq"]), p(r["begin"]),
                                      p(r["bridges"]), len(r["bridges"]), p(r["best"]), len(r["best"]), p(r["dist"]), p(r["off"]), p(r["mult"]), len(r["mult"]), p(r["apply"]),
                                      96.0, a.device, C.byref(out))
            if rc:
                raise RuntimeError(lib.ac_last_error().decode())
            return Result(out)
        res, best, runs = best_of(call, a.repeats, ("launches", "launches_components", "read_backs", "seconds_device", "seconds_copy", "seconds_components"))
        sm = res.summary
        assert sm["bridges_applied"] == n_bridges and sm["bases_copied"] == n_bridges * members * size
        numpy_s, n_edited, _ = numpy_edit_seconds(np, r)
        assert n_edited == 4 * n_bridges + 2 * (members - 1) * n_bridges      # the created links, and the old ones between two members
        plain = plain_copy_seconds(hip, sm["bases_copied"]) if hip is not None else 0.0
        row = dict(workload=f"ring: {label}", bridges=n_bridges, members_per_bridge=members, member_bytes=size, unitigs=r["n"], links_in=sm["links_in"], links_out=sm["links_out"],
                   bases_copied=sm["bases_copied"], removed_no_anchor=sm["removed_no_anchor"], best=best, runs=runs,
                   copy_gbytes_per_s=sm["bases_copied"] / best["seconds_copy"] / 1e9 if best["seconds_copy"] else None, plain_d2d_copy_s=plain,
                   plain_d2d_gbytes_per_s=sm["bases_copied"] / plain / 1e9 if plain else None, numpy_edit_s=numpy_s)
        rows.append(row)
        print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
        res.close()
    out = dict(tool="tools/apply_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(), results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
