#!/usr/bin/env python3
"""Times trim's edit (ac_graph_trim_apply / ac_trim_apply, then ac_trimmed_finish) on config C's chromosome cluster and on the largest cluster
of the mixed-species workload mini-E, on one MI355X, without torch.

    AC_NO_TORCH=1 python tools/trim_apply_bench.py [--assemblies 96] [--genome 5000000] [--workloads configEmini_k51] [--repeats 3] [--out FILE]

Config C's chromosome cluster: one genome, 96 assemblies, no plasmid contigs; the handle of the compressed graph is the cluster.  mini-E: the
40 chromosomes of the first species over the whole compressed graph of both (the cluster as `cluster` finds it, before save_cluster_gfa's
merge: the other species' unitigs die in the edit), on plain arrays.  The alignments run once (ac_trim_paths / ac_trim_path_slices, reported
on their own); their table is what the timed calls apply, with the default --mad.
Two routes, in the same process, alternated run by run, one warm-up each and then `--repeats` timed pairs, the best of each reported:
  new    the library's edit: the slices go to the device once, are checked, excluded by length and handed to the subset stages there
  glue   what a caller had to write before: slice the paths on the host, compute the allowed range, then ac_subsets_from_paths
both followed by the same merge plan, merged paths and finish with renumbering.  Per route: seconds of the edit (device, by events, and end to
end), launches and read-backs of the edit, seconds to the finished graph, entries and unitigs.  No ratio is a pass condition.
Writes profiles/trim_apply_bench.json, stamped with ac_source_hash.  Not a gate."""
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


def allowed_range(lengths, mad):
    """exclude_outliers_in_length's range as the glue computes it (tests/chain_util.py: allowed_length_range)"""
    import math

    def median(v):
        v = sorted(v)
        n = len(v)
        return (v[n // 2 - 1] + v[n // 2]) // 2 if n % 2 == 0 else v[n // 2]
    m = median(lengths)
    dev = median([abs(x - m) for x in lengths])
    rnd = lambda x: max(0, int(math.floor(x + 0.5)))
    return rnd(float(m) - float(dev) * mad), rnd(float(m) + float(dev) * mad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assemblies", type=int, default=96)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--workloads", nargs="*", default=["configEmini_k51"])
    ap.add_argument("--min-identity", type=float, default=0.75)
    ap.add_argument("--max-unitigs", type=int, default=5000)
    ap.add_argument("--mad", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu): two small jobs")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trim_apply_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, subsets_from_paths, synth, trim_apply, trim_path_slices
    import bench
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_seqs_free.argtypes = [C.c_void_p]

    def build(k, n_asm, asm):
        seqs, fn, hd = synth.flatten(asm)
        h_seqs = bench.prepare(lib, k, seqs, fn, hd, n_asm, threads=min(16, os.cpu_count() or 1), repair=1)
        h = C.c_void_p()
        if lib.ac_compress_seqs(C.c_uint32(k), h_seqs, C.c_int(a.device), C.byref(h)):
            raise RuntimeError(lib.ac_last_error().decode())
        lib.ac_seqs_free(h_seqs)
        return _capi.Graph(lib, h, lib.ac_graph_seq_count(h)), fn, hd, [len(s) for s in seqs]

    jobs = []
    if a.emu:
        jobs.append(("emu dry run: one genome", 21, 6, lambda: synth.make_assemblies(6, genome=20_000, plasmid=0, sub=1e-3, indel=1e-4, seed=5), None))
        jobs.append(("emu dry run: two species", 21, 6, lambda: synth.make_mixed_species(2, 3, genome=20_000, plasmid=1_500, seed=5), 3))
    else:
        jobs.append((f"config C, chromosome cluster ({a.assemblies} x {a.genome} bp)", 51, a.assemblies,
                     lambda: synth.make_assemblies(a.assemblies, genome=a.genome, plasmid=0, sub=1e-4, indel=1e-5, seed=51_000), None))
        for name in a.workloads:
            k, n_asm, gen = synth.WORKLOADS[name]
            jobs.append((f"{name}: the chromosomes of the first species ({synth.WORKLOAD_NOTES.get(name, '')})", k, n_asm, gen, n_asm // 2))
    rows = []
    for name, k, n_asm, gen, first_species in jobs:
        t0 = time.perf_counter()
        g, fn, hd, seq_len = build(k, n_asm, gen())
        build_s = time.perf_counter() - t0
        b = g.bulk()
        n = g.unitig_count
        links = np.ascontiguousarray(np.stack([b["links"]["a"], b["links"]["b"]], axis=1).astype(np.int32)) if len(b["links"]) else np.zeros((0, 2), dtype=np.int32)
        lens = np.ascontiguousarray(b["seq_len"], dtype=np.uint32)
        entries, off = np.ascontiguousarray(b["path_entries"], dtype=np.int32), np.ascontiguousarray(b["path_off"], dtype=np.uint64)
        sequences = (np.append(np.array(b["seq_bytes"], dtype=np.uint8), np.uint8(0)), np.array(b["seq_begin"], dtype=np.uint64))
        if first_species is None:      # the whole handle is the cluster
            members = list(range(len(seq_len)))
        else:                          # assemblies 0 .. first_species - 1, their first contig
            members = [s for s in range(len(seq_len)) if int(fn[s][9:13]) < first_species and hd[s].startswith("contig_1 ")]
        lengths = [seq_len[s] for s in members]
        if first_species is not None:      # a cluster of its own arrays: the members' paths back to back
            entries = np.ascontiguousarray(np.concatenate([entries[int(off[s]):int(off[s + 1])] for s in members]))
            off = np.concatenate([[0], np.cumsum([int(off[s + 1] - off[s]) for s in members])]).astype(np.uint64)
        t = time.perf_counter()
        if first_species is None:
            results, align = g.trim_paths(a.min_identity, a.max_unitigs, device=a.device)
        else:
            results, align = trim_path_slices([entries[int(off[i]):int(off[i + 1])] for i in range(len(members))], lens, a.min_identity, a.max_unitigs,
                                              device=a.device, lib_path=lib_path)
        align_s = time.perf_counter() - t

        def new_route():
            t = time.perf_counter()
            tr = g.trim_apply(results, mad=a.mad, device=a.device) if first_species is None else \
                trim_apply(n, links, lens, (entries, off), lengths, results, mad=a.mad, device=a.device, lib_path=lib_path)
            edit_s = time.perf_counter() - t
            fin = tr.finish(sequences=None if first_species is None else sequences, device=a.device)
            total_s = time.perf_counter() - t
            out = dict(edit_end_to_end_s=edit_s, finished_end_to_end_s=total_s, edit_seconds_device=tr.summary["seconds_device"], launches=tr.summary["launches"],
                       read_backs=tr.summary["read_backs"], entries_kept=tr.summary["entries_kept"], unitigs_alive=tr.summary["unitigs_alive"],
                       excluded=tr.summary["excluded"], trimmed=tr.summary["trimmed"], chosen=tr.summary["chosen"], unitigs_after=fin.summary["unitigs"])
            text = fin.unitigs.tobytes() + fin.links.tobytes() + fin.path_entries.tobytes()
            fin.close(); tr.close()
            return out, text

        def glue_route():
            t = time.perf_counter()
            kind = None if align["chosen"] == 0 else "start_end" if align["chosen"] == 1 else "hairpin"
            parts, new_len = [], []
            for i, r in enumerate(results):
                lo, hi = int(off[i]), int(off[i + 1])
                if kind is not None and r[kind]["status"] == 1:
                    parts.append(entries[lo + r[kind]["begin"]:lo + r[kind]["end"]]); new_len.append(r[kind]["trimmed_length"])
                else:
                    parts.append(entries[lo:hi]); new_len.append(lengths[i])
            ent = np.ascontiguousarray(np.concatenate(parts))
            off2 = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
            lo, hi = allowed_range(new_len, a.mad)
            keep = [1 if lo <= x <= hi else 0 for x in new_len]
            sub = subsets_from_paths(n, links, lens, (ent, off2), keep, 1, device=a.device, lib_path=lib_path)
            edit_s = time.perf_counter() - t
            plan = sub.merge_plan(1, sequences=sequences, device=a.device)
            mp = sub.merged_paths(1, plan, device=a.device, keep=True)
            fin = sub.finish(1, plan, mp, renumber=True, sequences=sequences, device=a.device)
            total_s = time.perf_counter() - t
            out = dict(edit_end_to_end_s=edit_s, finished_end_to_end_s=total_s, edit_seconds_device=sub.summary["seconds_device"], launches=sub.summary["launches"],
                       read_backs=sub.summary["read_backs"], entries_kept=sub.summary["entries_kept"], unitigs_alive=sub.summary["unitigs"],
                       excluded=keep.count(0), unitigs_after=fin.summary["unitigs"])
            text = fin.unitigs.tobytes() + fin.links.tobytes() + fin.path_entries.tobytes()
            fin.close(); mp.close(); plan.close(); sub.close()
            return out, text

        _, want = new_route()
        _, got = glue_route()      # (the warm-ups: arena growth, code load)
        assert want == got, "the two routes give different finished graphs"
        runs = dict(new=[], glue=[])
        for _ in range(a.repeats):
            runs["new"].append(new_route()[0])
            runs["glue"].append(glue_route()[0])
        row = dict(workload=name, kmer=k, sequences=len(members), unitigs=n, links=int(links.shape[0]), path_entries=int(off[-1]), build_s=build_s,
                   alignment=dict(end_to_end_s=align_s, seconds_device=align["seconds_device"], launches=align["launches"], cells=align["cells"], c_se=align["c_se"],
                                  c_hp=align["c_hp"]),
                   best={r: min(v, key=lambda x: x["edit_end_to_end_s"]) for r, v in runs.items()}, runs=runs)
        rows.append(row)
        print(json.dumps({k_: v for k_, v in row.items() if k_ != "runs"}), flush=True)
        g.close()
    out = dict(tool="tools/trim_apply_bench.py", source_hash=lib.ac_source_hash().decode(), version=lib.ac_version().decode(),
               note="the edit of `trim` by two routes in one process, alternated; both end in the same finished graph (asserted); no ratio is claimed", results=rows)
    if not a.emu:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
