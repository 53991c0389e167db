#!/usr/bin/env python3
"""Times `autocycler combine`'s device stage (ac_combine_graphs) on one MI355X, without torch.

    AC_NO_TORCH=1 python tools/combine_bench.py [--workload configEmini_k51] [--parts 50 5000] [--pairs 3] [--out FILE]

Inputs:
  resolved shape of config C   two one-unitig circular graphs of 5 Mbp and 100 kbp, given in reverse size order: what compress -> cluster -> trim ->
                               resolve leaves of config C (one chromosome, one plasmid).  Lengths only: the chain itself is not run here, and the
                               stage never sees the bases.  A call this small is all fixed cost: launches and two read-backs.
  many graphs                  the unitigs and links of the graph this library builds for the mixed-species workload mini-E, cut into P graphs of
                               consecutive unitigs (links that cross a cut dropped, numbers and link entries made local), P = 50 and 5 000: the
                               concatenated passes and the link sort have something to do.
Per input: device seconds by events, end-to-end seconds of the C call, launches and read-backs.  As the only comparison offered, a numpy
restatement of the ordering, the offsets and the link reorder (stable argsorts and a cumulative sum) in the same process; its links must equal
the library's.  One warm-up of each, then `--pairs` alternated pairs, the best of each reported.  No time is a pass condition.
Writes profiles/combine_bench.json, stamped with ac_source_hash.  Not a gate."""
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


def numpy_combine(np, uoff, loff, number, lens, links):
    """load_clusters' order, combine_clusters' offsets and get_links_for_gfa's order for all graphs at once -> (order, offsets in rank order, links out)"""
    G = len(uoff) - 1
    prefix = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)])
    total = prefix[uoff[1:]] - prefix[uoff[:-1]]
    order = np.argsort(-total.astype(np.int64), kind="stable")
    graph_of = np.repeat(np.arange(G), np.diff(uoff).astype(np.int64))
    maxima = np.zeros(G, dtype=np.uint64)
    np.maximum.at(maxima, graph_of, number.astype(np.uint64))
    offset_ranked = np.concatenate([[0], np.cumsum(maxima[order])[:-1]]).astype(np.uint64)
    base_ranked = np.concatenate([[0], np.cumsum(np.diff(uoff)[order])[:-1]]).astype(np.uint64)
    offset_of, base_of = np.empty(G, dtype=np.uint64), np.empty(G, dtype=np.uint64)
    offset_of[order], base_of[order] = offset_ranked, base_ranked
    link_graph = np.repeat(np.arange(G), np.diff(loff).astype(np.int64))
    a, b = links[:, 0].astype(np.int64), links[:, 1].astype(np.int64)
    key = (base_of[link_graph].astype(np.int64) + np.abs(a) - 1) * 2 + (a < 0)
    by = np.argsort(key, kind="stable")
    first = uoff[link_graph].astype(np.int64)
    pa = number[first + np.abs(a) - 1].astype(np.int64) + offset_of[link_graph].astype(np.int64)
    pb = number[first + np.abs(b) - 1].astype(np.int64) + offset_of[link_graph].astype(np.int64)
    out = np.stack([np.where(a > 0, pa, -pa), np.where(b > 0, pb, -pb)], axis=1)[by].astype(np.int32)
    return order, offset_ranked, out


def cut_into_graphs(np, n, links, parts):
    """consecutive unitig ranges; the links inside one range, local -> (unitig_off, link_off, number, links)"""
    uoff = (np.arange(parts + 1, dtype=np.uint64) * n) // parts
    part_of = np.searchsorted(uoff, np.arange(1, n + 1, dtype=np.uint64), side="left") - 1      # of unitig numbers 1 .. n
    pa, pb = part_of[np.abs(links[:, 0]) - 1], part_of[np.abs(links[:, 1]) - 1]
    kept = links[pa == pb]
    g = pa[pa == pb]
    first = uoff[g].astype(np.int64)
    local = np.stack([np.sign(kept[:, 0]) * (np.abs(kept[:, 0].astype(np.int64)) - first), np.sign(kept[:, 1]) * (np.abs(kept[:, 1].astype(np.int64)) - first)], axis=1).astype(np.int32)
    loff = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=parts))]).astype(np.uint64)      # (the links are sorted by their first unitig: by graph already)
    number = (np.arange(n, dtype=np.int64) - uoff[part_of].astype(np.int64) + 1).astype(np.uint32)
    return uoff, loff, number, np.ascontiguousarray(local)


def measure(np, lib, _capi, label, uoff, loff, number, lens, links, pairs, device):
    G = len(uoff) - 1
    uoff, loff = np.ascontiguousarray(uoff, dtype=np.uint64), np.ascontiguousarray(loff, dtype=np.uint64)
    number, lens = np.ascontiguousarray(number, dtype=np.uint32), np.ascontiguousarray(lens, dtype=np.uint32)
    links = np.ascontiguousarray(links, dtype=np.int32).reshape(-1, 2)
    links_arg = links if len(links) else np.zeros((1, 2), dtype=np.int32)

    def library():
        h = C.c_void_p()
        t = time.perf_counter()
        rc = lib.ac_combine_graphs(G, uoff.ctypes.data, loff.ctypes.data, number.ctypes.data, lens.ctypes.data, None, None, links_arg.ctypes.data, None, None, None, None, device,
                                   C.byref(h))
        s = time.perf_counter() - t
        if rc:
            raise RuntimeError(lib.ac_last_error().decode())
        return s, _capi.Combined(lib, h)

    def restated():
        t = time.perf_counter()
        res = numpy_combine(np, uoff, loff, number, lens, links)
        return time.perf_counter() - t, res
    _, c = library()
    _, (order, offsets, out) = restated()
    assert c.clusters["input_index"].tolist() == order.tolist() and c.clusters["offset"].tolist() == offsets.tolist() and np.array_equal(c.links, out), label
    c.close()
    runs = []
    for _ in range(pairs):
        s, c = library()
        runs.append(dict(end_to_end_s=s, seconds_device=c.summary["seconds_device"], launches=c.summary["launches"], read_backs=c.summary["read_backs"], numpy_s=restated()[0]))
        c.close()
    row = dict(input=label, graphs=G, unitigs=int(uoff[-1]), links=int(loff[-1]), best_end_to_end_s=min(r["end_to_end_s"] for r in runs),
               best_seconds_device=min(r["seconds_device"] for r in runs), best_numpy_s=min(r["numpy_s"] for r in runs), launches=runs[-1]["launches"],
               read_backs=runs[-1]["read_backs"], runs=runs)
    print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="configEmini_k51")
    ap.add_argument("--parts", type=int, nargs="*", default=[50, 5000])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): a small mixed-species job")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "combine_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, synth
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]
    rows = []
    # the resolved shape of config C, smallest first: the sort has something to do
    rows.append(measure(np, lib, _capi, "resolved shape of config C: one-unitig circular graphs of 100 kbp and 5 Mbp", [0, 1, 2], [0, 2, 4], [1, 1], [100_000, 5_000_000],
                        [[1, 1], [-1, -1], [1, 1], [-1, -1]], a.pairs, a.device))
    t0 = time.perf_counter()
    if a.emu:
        name, (k, n_asm, asm) = "emu dry run", (21, 6, synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5))
    else:
        name = a.workload
        k, n_asm, gen = synth.WORKLOADS[name]
        asm = gen()
    seqs, fn, hd = synth.flatten(asm)
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
    lens = np.ascontiguousarray(bulk["seq_len"], dtype=np.uint32)
    g.close()
    for parts in ([3, 40] if a.emu else a.parts):
        uoff, loff, number, local = cut_into_graphs(np, n, links, parts)
        row = measure(np, lib, _capi, f"{name} cut into {parts} graphs", uoff, loff, number, lens, local, a.pairs, a.device)
        row.update(workload=name, note=synth.WORKLOAD_NOTES.get(name, ""), kmer=k, build_s=build_s, links_dropped_at_cuts=int(len(links) - len(local)))
        rows.append(row)
    out = dict(tool="tools/combine_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(),
               note="device and end-to-end seconds of ac_combine_graphs (no bases, no texts); numpy_s restates the ordering, the offsets and the link reorder alone, without the "
                    "end tests, the duplicate check or the records; no speed-up is claimed", results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
