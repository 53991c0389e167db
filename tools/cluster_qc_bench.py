#!/usr/bin/env python3
"""Times ac_cluster_generate (cut + refine_auto_clusters + the final qc_clusters) on one MI355X, without torch, against the same refinement
driven through the entry points a caller had before it: ac_cluster_cut, then per alternative ac_cluster_assign and ac_cluster_containment
(the O(S^2) host loop), with the verdict chain and the scores on the host (numpy and plain floats, in the library's order of operations).

    AC_NO_TORCH=1 python tools/cluster_qc_bench.py [--sizes 2000 8000] [--replicons 40] [--repeats 3] [--out profiles/cluster_qc_bench.json]

Input: a synthetic block matrix.  `replicons` replicons, S / replicons files; most replicons have one sequence per file, every fifth has two
copies per file (its first cut has balance 0: refinement splits it), every seventh is asymmetric towards its neighbour (contained).  Distances
are dyadic: k / 1024 inside a copy, 1/16 + k / 1024 between the copies of a replicon, 1/2 + k / 1024 between replicons.  The tree is built
once (ac_cluster_tree_from_distances) and is not part of either timing.  Before anything is timed the baseline's clusters, verdicts and
scores are checked to be identical to generate's.  One warm call, then the best of `repeats`; the baseline is run once more than it is
checked only when it is short (it is the slow side).  Writes one JSON document stamped with ac_source_hash."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("AC_NO_TORCH", "1")


def make_input(np, S, replicons, seed=1):
    rs = np.random.RandomState(seed)
    files = max(2, S // replicons)
    rep, copy, file_of = [], [], []
    r = 0
    while len(rep) < S:
        copies = 2 if r % 5 == 4 else 1
        for c in range(copies):
            for f in range(files):
                rep.append(r); copy.append(c); file_of.append(f)
        r += 1
    rep, copy, file_of = (np.array(x[:S]) for x in (rep, copy, file_of))
    same_rep = rep[:, None] == rep[None, :]
    same_copy = same_rep & (copy[:, None] == copy[None, :])
    noise = np.triu(rs.randint(1, 17, (S, S)), 1)
    noise = (noise + noise.T) / 1024.0
    m = np.where(same_copy, noise, np.where(same_rep, 0.0625 + noise, 0.5 + noise))
    inner = (rep % 7 == 6)[:, None] & (rep[None, :] == rep[:, None] - 1)      # d(a, b) small for a in replicon r, b in replicon r - 1
    m = np.where(inner, 0.03125, m)
    np.fill_diagonal(m, 0.0)
    first = {}
    assembly = np.array([first.setdefault(f, len(first)) for f in file_of.tolist()], dtype=np.uint32)
    seq_len = (5_000_000 // (1 + rep) + rs.randint(0, 50, S)).astype(np.uint64)
    return np.ascontiguousarray(m, dtype=np.float64), seq_len, assembly, np.ones(S, dtype=np.uint32), np.zeros(S, dtype=np.uint8)


class Baseline:
    """refine_auto_clusters with every alternative scored from scratch through ac_cluster_assign + ac_cluster_containment"""

    def __init__(self, np, lib, tree, asym, seq_len, assembly, weight, trusted, cutoff, min_assemblies):
        self.np, self.lib, self.h, self.asym, self.cutoff, self.min_assemblies = np, lib, tree._h, asym, cutoff, min_assemblies
        self.seq_len, self.assembly, self.weight, self.trusted = seq_len, assembly.astype(np.int64), weight.astype(np.int64), trusted.astype(bool)
        self.S, self.F = len(seq_len), int(assembly.max()) + 1
        nodes = tree.nodes
        self.children = {n[0]: (nodes[n[1]][0], nodes[n[2]][0]) for n in nodes if n[1] >= 0}
        self.of_seq = np.zeros(self.S, dtype=np.uint16)
        self.calls = 0

    def qc(self, clusters):
        np, lib, n = self.np, self.lib, len(clusters)
        cn = np.array(clusters, dtype=np.uint16)
        dist = np.zeros(n, dtype=np.float64)
        top = C.c_uint32()
        assert lib.ac_cluster_assign(self.h, cn.ctypes.data, n, self.seq_len.ctypes.data, self.of_seq.ctypes.data, dist.ctypes.data, C.byref(top)) == 0, lib.ac_last_error()
        top = top.value
        cc, tc = np.zeros((top, top), dtype=np.uint64), np.zeros((top, top), dtype=np.uint64)
        assert lib.ac_cluster_containment(self.asym.ctypes.data, self.S, self.of_seq.ctypes.data, top, self.cutoff, cc.ctypes.data, tc.ctypes.data) == 0, lib.ac_last_error()
        self.calls += 1
        c0 = self.of_seq.astype(np.int64) - 1
        size = np.bincount(c0, minlength=top)
        per_file = np.zeros((top, self.F), dtype=np.int64)
        np.add.at(per_file, (c0, self.assembly), 1)
        best = np.zeros((top, self.F), dtype=np.int64)
        np.maximum.at(best, (c0, self.assembly), self.weight)
        ones = (per_file == 1).sum(axis=1)
        trusted = np.bincount(c0, weights=self.trusted, minlength=top) > 0
        fail = np.where((best.sum(axis=1) < self.min_assemblies) & ~trusted, 2, 0)
        inside = 2 * cc > tc
        for c in range(top):
            row = inside[c] & (fail == 0)
            row[c] = False
            if row.any() and not trusted[c]:
                fail[c] |= 4
        acc = tight = 0.0
        pass_size = 0
        for c in range(top):
            acc += (float(ones[c]) / float(self.F)) * float(size[c])
            if fail[c] == 0:
                tight += (1.0 - math.sqrt(dist[c])) * float(size[c]); pass_size += int(size[c])
        balance = acc / float(self.S)
        tightness = tight / float(pass_size) if pass_size else 0.0
        return (balance + tightness) / 2.0, fail.tolist()

    def split_clusters(self, clusters):
        return sorted(sorted([o for o in clusters if o != c] + list(self.children[c])) for c in clusters if c in self.children)

    def generate(self, start):
        best = list(start)
        best_score, _ = self.qc(best)
        scores, improved = [], True
        while improved:
            improved = False
            for alt in self.split_clusters(best):
                score, _ = self.qc(alt)
                scores.append(score)
                if score > best_score + 1e-12:
                    best, best_score, improved = alt, score, True
        return best, self.qc(best)[1], scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 8000])
    ap.add_argument("--replicons", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cutoff", type=float, default=0.2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emu", action="store_true", help="dry run of this script on the CPU emulation (tests/_emu), small sizes only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cluster_qc_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import _capi, cluster_min_assemblies, cluster_tree
    lib_path = None
    if a.emu:
        sys.path.insert(0, str(ROOT / "tests"))
        import emu_lib
        lib_path = emu_lib.emu_path()
    lib = _capi.load_library(lib_path)
    lib.ac_cluster_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    rows = []
    for S in a.sizes:
        asym, seq_len, assembly, weight, trusted = make_input(np, S, a.replicons)
        mn = cluster_min_assemblies(assembly.tolist(), lib_path=lib_path)
        tree = cluster_tree(asym, range(1, S + 1), normalise=True, device=a.device, lib_path=lib_path)
        args = (asym, seq_len.tolist(), assembly.tolist(), weight.tolist(), trusted.tolist(), a.cutoff, mn)
        got = tree.generate(*args, device=a.device)      # warm: code objects, arena growth
        base = Baseline(np, lib, tree, asym, seq_len, assembly, weight, trusted, a.cutoff, mn)
        t0 = time.perf_counter()
        b_clusters, b_fail, b_scores = base.generate(tree.cut(a.cutoff))
        baseline_s = [time.perf_counter() - t0]
        scores = [s for r in got.trace for s in r["scores"]]
        assert b_clusters == got.clusters and b_fail == [r["fail"] for r in got.records], "the baseline's clusters or verdicts differ"
        assert [s.hex() for s in b_scores] == [s.hex() for s in scores], "the baseline's scores differ"
        if baseline_s[0] < 20.0:
            t0 = time.perf_counter()
            base.generate(tree.cut(a.cutoff))
            baseline_s.append(time.perf_counter() - t0)
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            q = tree.generate(*args, device=a.device)
            runs.append(dict(wall_s=time.perf_counter() - t0, device_s=q.summary["seconds"]))
        best = min(runs, key=lambda r: r["wall_s"])
        sm = got.summary
        row = dict(n_seqs=S, replicons=a.replicons, assemblies=int(assembly.max()) + 1, min_assemblies=mn, cutoff=a.cutoff, start_clusters=len(tree.cut(a.cutoff)),
                   final_clusters=len(got.clusters), fail_clusters=got.metrics["fail_cluster_count"], rounds=sm["rounds"], evaluations=sm["evaluations"],
                   alternatives=sm["alternatives"], node_pairs=sm["node_pairs"], launches=sm["launches"], readbacks=sm["readbacks"],
                   bytes_read_back=sm["bytes_read_back"], generate_runs=runs, generate_wall_s=best["wall_s"], generate_device_s=best["device_s"],
                   baseline_runs_s=baseline_s, baseline_wall_s=min(baseline_s), baseline_containment_calls=base.calls // len(baseline_s),
                   baseline_identical=True)
        rows.append(row)
        print(json.dumps(row), flush=True)
        tree.close()
    out = dict(tool="tools/cluster_qc_bench.py", source_hash=lib.ac_source_hash().decode(), emulation=bool(a.emu),
               input="synthetic block matrix: dyadic distances, every fifth replicon in two copies per file, every seventh contained in its neighbour",
               baseline="ac_cluster_cut + per alternative ac_cluster_assign and ac_cluster_containment, chain and scores on the host", results=rows)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
