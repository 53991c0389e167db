#!/usr/bin/env python3
"""Times ac_cluster_tree_from_distances on random symmetric matrices (S = 64, 1024, 4096): per size one warm-up call, then `--repeats`
timed calls; the median wall time of a call, the median of the merge loop alone (the library's device events) and their difference (upload,
setup kernels, read-back, the tree on the host), with the launches, rescans and compares of the last call.  Writes
profiles/cluster_time.json, stamped with ac_source_hash.  Not a gate: nothing else computes this tree to compare with."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cluster_time.json"))
    a = ap.parse_args()
    import numpy as np
    from autocycler_amd import cluster_tree, load_library
    lib = load_library()
    rows = []
    for n in a.sizes:
        rng = np.random.default_rng(n)
        m = np.triu(rng.random((n, n)), 1)
        m = np.ascontiguousarray(m + m.T)
        ids = range(1, n + 1)
        cluster_tree(m, ids, device=a.device).close()      # warm-up: arena growth, code load
        wall, loop = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            t = cluster_tree(m, ids, device=a.device)
            wall.append(time.perf_counter() - t0)
            sm = t.summary
            loop.append(sm["seconds"])
            t.close()
        row = dict(n_seqs=n, repeats=a.repeats, wall_s_median=statistics.median(wall), loop_s_median=statistics.median(loop),
                   outside_loop_s_median=statistics.median(w - l for w, l in zip(wall, loop)), wall_s_min=min(wall), wall_s_max=max(wall),
                   launches=sm["launches"], rescans=sm["rescans"], compares=sm["compares"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(tool="tools/cluster_time.py", source_hash=lib.ac_source_hash().decode(), input="uniform random symmetric f64, zero diagonal", results=rows)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
