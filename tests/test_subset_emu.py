"""ac_graph_subsets / ac_subsets_from_paths, the two composed entries and ac_subsets_merged_paths on the CPU emulation of the shipped kernels
(kernels_subset.inc) against the literal Python model of subset_util.py — drop sequences, rebuild positions, recalculate_depth,
remove_zero_depth_unitigs, merge_linear_paths, and the P lines after the merge by the reference's position walk.  Every comparison is
equality.  The same checks run on the device in test_subset_gpu.py."""
import random

import numpy as np
import pytest

import emu_lib
import merge_util as M
import parity_util
import seqgen
import subset_util as S
from autocycler_amd import AutocyclerError, Subsets, components_from_links, graph_from_gfa, graph_merge_plan, graph_subsets, merge_plan_from_links, subsets_from_paths, \
    trim_path_slices
from autocycler_amd import _capi
from test_merge_emu import TILE_SIZES

NEW_SYMBOLS = ("ac_graph_subsets", "ac_subsets_from_paths", "ac_subsets_records", "ac_subsets_unitigs", "ac_subsets_links", "ac_subsets_seqs", "ac_subsets_path_ends",
               "ac_subsets_dense", "ac_subsets_summary_get_sized", "ac_subsets_free", "ac_subsets_components", "ac_subsets_merge_plan", "ac_subsets_merged_paths",
               "ac_merged_paths_get", "ac_merged_paths_summary_get_sized", "ac_merged_paths_free")


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_subsets(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


def test_host_functions_stand_alone(tmp_path):
    """subset_host.cpp without the library (tests/c_client/subset_host_check.cpp), under the address and undefined-behaviour sanitizers: labels,
    offsets, the sequence lists and path ends, the records, densify, locate, the refusals and their texts"""
    import subprocess
    root = emu_lib.ROOT
    exe = tmp_path / "subset_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           str(root / "autocycler_amd" / "csrc"), str(root / "tests" / "c_client" / "subset_host_check.cpp"),
                           str(root / "autocycler_amd" / "csrc" / "subset_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "subset_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


# ---- through the library ----------------------------------------------------------------------------------------------------------------------
def seq_arrays(seqs):
    """unitig sequences as ac_subsets_merge_plan takes them: (all bytes, the first byte of every unitig)"""
    begin = np.zeros(len(seqs), dtype=np.uint64)
    begin[1:] = np.cumsum([len(s) for s in seqs[:-1]], dtype=np.uint64) if len(seqs) > 1 else []
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8), begin


def run_raw(lib_path, n, links, lens, paths, labels, n_clusters, alive=None, device=0):
    sub = subsets_from_paths(n, links, lens, paths, labels, n_clusters, alive=alive, device=device, lib_path=lib_path)
    assert isinstance(sub, Subsets) and sub.n_clusters == n_clusters
    return sub


COVERAGE = ("shared_unitig", "link_dropped", "revisited", "both_strands", "empty_cluster", "dropped_sequence", "chain", "chain_backwards", "merged_loop", "shorter_path")


def check_clusters(sub, n, links, lens, alive, paths, labels, n_clusters, seqs=None, gfa_order=False, handle_seqs=False, what="", device=0):
    """every cluster of `sub` against the model, through the merge plan and the re-threaded paths; returns what it met, by the names of COVERAGE"""
    met = dict.fromkeys(COVERAGE, 0)
    met["dropped_sequence"] = int(any(l == 0 for l in labels))
    alive_in = {}
    sequences = seq_arrays(seqs) if seqs is not None and not handle_seqs and n else None
    for c in range(1, n_clusters + 1):
        m = S.model_cluster(n, links, lens, alive, paths, labels, c, gfa_order)
        S.assert_cluster_same(S.library_cluster(sub, c), m, f"{what} cluster {c}")
        for u in m["unitigs"]:
            alive_in[u] = alive_in.get(u, 0) + 1
        present = set(m["unitigs"])
        met["link_dropped"] |= any((abs(a) in present) != (abs(b) in present) for a, b in links)
        met["revisited"] |= any(x > 1 for x in m["fwd"])
        signed = {e for p in m["paths"].values() for e in p}
        met["both_strands"] |= any(-e in signed for e in signed)
        met["empty_cluster"] |= not m["seqs"]
        # the merge plan of this cluster and the paths over it
        exp = S.model_merge(m, seqs)
        plan = sub.merge_plan(c, sequences=sequences, with_sequences=seqs is not None, device=device)
        M.assert_same(M.library_result(plan), exp, f"{what} cluster {c} plan")
        want = S.model_merged_paths(m, exp)
        got = sub.merged_paths(c, plan, device=device)
        assert got.paths() == want and got.seq_index.tolist() == m["seqs"], (what, c, got.paths(), want)
        assert got.summary["entries_before"] == m["entries"] and got.summary["entries_after"] == sum(len(p) for p in want.values())
        for s, p in want.items():
            assert S.path_length(p, lens, exp) == S.path_length(m["paths"][s], lens, exp), (what, c, s)
        plan.close()
        numbers = set(exp["numbers"])
        met["chain"] |= bool(exp["chains"])
        met["chain_backwards"] |= any(-e in numbers for p in want.values() for e in p)
        met["merged_loop"] |= any(exp["loops"])
        met["shorter_path"] |= any(len(want[s]) < len(m["paths"][s]) for s in want)
    met["shared_unitig"] = int(any(v >= 2 for v in alive_in.values()))
    return {k: int(v) for k, v in met.items()}


# ---- named cases: the committed GFA that has paths ---------------------------------------------------------------------------------------------
def check_named_cases(lib_path, device=0):
    g = S.gfa_14()
    n_seqs = len(g["paths"])
    assert n_seqs >= 2
    kw = dict(n=g["n"], links=g["links"], lens=g["lens"], alive=g["alive"], paths=g["paths"])
    subsets = [[int(s == keep) for s in range(n_seqs)] for keep in range(n_seqs)] + [[int(s != out) for s in range(n_seqs)] for out in range(n_seqs)]
    for labels in subsets:
        sub = run_raw(lib_path, g["n"], g["links"], g["lens"], g["paths"], labels, 1, g["alive"], device)
        check_clusters(sub, labels=labels, n_clusters=1, seqs=g["seqs"], what=f"test_gfa_14 {labels}", device=device, **kw)
    # all sequences in one cluster: the graph's own merge plan
    ones = [1] * n_seqs
    sub = run_raw(lib_path, g["n"], g["links"], g["lens"], g["paths"], ones, 1, g["alive"], device)
    check_clusters(sub, labels=ones, n_clusters=1, seqs=g["seqs"], what="test_gfa_14 all", device=device, **kw)
    a = g["merge_args"]
    whole = merge_plan_from_links(a["n"], a["links"], a["lens"], a["alive"], a["path_ends"], a["depths"], a["fwd"], a["rev"], None, a["seqs"], device=device, lib_path=lib_path)
    plan = sub.merge_plan(1, sequences=seq_arrays(g["seqs"]), device=device)
    for k in ("chains", "members_per_chain", "lengths", "member_off", "seq_off", "types", "loops", "unitigs_after", "merged_unitigs", "seqs"):
        assert M.library_result(plan)[k] == M.library_result(whole)[k], k
    assert plan.links.tolist() == whole.links.tolist() and plan.fixed.tolist() == whole.fixed.tolist()
    # every label 0: nothing is alive anywhere, and no device is asked for
    sub = run_raw(lib_path, g["n"], g["links"], g["lens"], g["paths"], [0] * n_seqs, 2, g["alive"], device)
    assert sub.records.tolist() == [(0, 0, 0, 0, 0)] * 2 and sub.summary["launches"] == 0 and not sub.dense(1)["alive"].any()
    assert sub.merge_plan(2, with_sequences=False, device=device).chain_members() == []
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


def check_handle_reproduces_graph_merge_plan(lib_path, device=0):
    """a loadable GFA with paths, all sequences in one cluster: graph_merge_plan(use_paths=True) exactly, wherever no path walks a chain's first
    member on the other strand (there the handle's per-strand histogram counts fewer positions than create_sequence_and_positions makes)"""
    n, links, lens, seqs, paths = 6, M.closed_set([(1, 2), (2, 3), (3, 4), (3, 5), (5, 6)]), [9, 8, 7, 3, 2, 1], None, [[1, 2, 3, 4], [1, 2, 3, 5, 6], [2, 3, 5, 6]]
    seqs = [bytes(random.Random(7).choice(b"ACGT") for _ in range(l)) for l in lens]
    g, _, _ = graph_from_gfa(S.hand_gfa_text(n, links, seqs, paths), lib_path=lib_path)
    sub = graph_subsets(g, [1, 1, 1], device=device)
    whole = graph_merge_plan(g, use_paths=True, device=device)
    plan = sub.merge_plan(1, device=device)
    assert whole.chain_members() == [[2, 3], [5, 6]] and M.result_bytes(plan) == M.result_bytes(whole)
    assert sub.merged_paths(1, plan, device=device).paths() == {0: [1, 7, 4], 1: [1, 7, 8], 2: [7, 8]}
    return True


def test_handle_reproduces_graph_merge_plan(emu):
    assert check_handle_reproduces_graph_merge_plan(emu)


# ---- random sweep -----------------------------------------------------------------------------------------------------------------------------
def check_sweep(lib_path, seed, cases, device=0):
    rng = random.Random(seed)
    met = dict.fromkeys(COVERAGE, 0)
    for i in range(cases):
        what = f"seed {seed} case {i}"
        if i % 10 == 9:      # a small compress build at k = 5 ... 11
            k = rng.choice((5, 7, 9, 11))
            seqs_in, fn, hd = seqgen.make_case(rng.randrange(10 ** 6), k)
            g, _, _ = parity_util.check_case(k, seqs_in, fn, hd, lib_path=lib_path, repair=False, device=device)
            n = g.unitig_count
            links = [(a if fa else -a, b if fb else -b) for a, fa, b, fb in g.links()]
            useq = [bytes(g.unitig(u)[0]) for u in range(n)]
            paths = [[int(e) for e in g.path(s)] for s in range(len(seqs_in))]
            labels, nc = S.random_labels(rng, len(paths))
            sub = graph_subsets(g, labels, nc, device=device)
            got = check_clusters(sub, n, links, [len(s) for s in useq], None, paths, labels, nc, useq, gfa_order=True, handle_seqs=True, what=what, device=device)
        else:
            n, links, lens, useq, paths = S.hand_graph(rng)
            labels, nc = S.random_labels(rng, len(paths))
            if i % 2 and all(paths):      # as a handle, through ac_graph_from_gfa (the loader takes no empty path)
                g, _, _ = graph_from_gfa(S.hand_gfa_text(n, links, useq, paths), lib_path=lib_path)
                links = [(a if fa else -a, b if fb else -b) for a, fa, b, fb in g.links()]
                sub = graph_subsets(g, labels, nc, device=device)
                got = check_clusters(sub, n, links, lens, None, paths, labels, nc, useq, gfa_order=True, handle_seqs=True, what=what, device=device)
            else:
                sub = run_raw(lib_path, n, links, lens, paths, labels, nc, None, device)
                got = check_clusters(sub, n, links, lens, None, paths, labels, nc, useq, what=what, device=device)
        for k_ in COVERAGE:
            met[k_] += got[k_]
    return met


def assert_sweep_coverage(results, least=20):
    total = {k: sum(r[k] for r in results) for k in COVERAGE}
    assert all(v >= least for v in total.values()), total


def test_random_sweep(emu):
    assert_sweep_coverage([check_sweep(emu, 11000 + seed, 150) for seed in range(4)])      # 600 graphs


# ---- boundary table: expected by construction, in numpy ----------------------------------------------------------------------------------------
ENTRY_COUNTS = (63, 64, 65, 255, 256, 257) + TILE_SIZES
CLUSTER_COUNTS = (1, 2, 63, 64, 65, 300)


def boundary_case(size, n_clusters, seed):
    """`size` kept entries (the last sequence is dropped and does not count) and `size` links over 97 unitigs, labels over all clusters"""
    rng = np.random.default_rng(seed)
    n = 97
    n_seqs = min(size, max(2, n_clusters + 3))
    cuts = np.sort(rng.choice(np.arange(1, size), n_seqs - 1, replace=False)) if n_seqs > 1 else np.zeros(0, dtype=np.int64)
    off = np.concatenate([[0], cuts, [size, size + 9]]).astype(np.uint64)
    entries = (rng.integers(1, n + 1, size + 9) * rng.choice((-1, 1), size + 9)).astype(np.int32)
    labels = np.concatenate([rng.permutation(n_seqs) % n_clusters + 1, [0]]).astype(np.uint16)
    links = (rng.integers(1, n + 1, (size, 2)) * rng.choice((-1, 1), (size, 2))).astype(np.int32)
    lens = rng.integers(1, 50, n).astype(np.uint32)
    return n, links, lens, entries, off, labels


def special_cases():
    one = np.array([[1, 1]], dtype=np.int32)
    yield "one sequence of one entry", (3, one, [4, 5, 6], np.array([-1], dtype=np.int32), np.array([0, 1], dtype=np.uint64), [1]), 1
    yield "one unitig 1000 times", (3, np.array([[2, 2], [-2, -2], [2, 1]], dtype=np.int32), [4, 5, 6], np.full(1000, 2, dtype=np.int32), np.array([0, 1000], dtype=np.uint64), [1]), 1
    yield "one unitig in all 300 clusters", (5, np.array([[3, 3], [3, 1], [-3, -3]], dtype=np.int32), [1, 2, 3, 4, 5], np.full(300, -3, dtype=np.int32),
                                             np.arange(301, dtype=np.uint64), list(range(1, 301))), 300
    yield "no unitigs", (0, np.zeros((0, 2), dtype=np.int32), [], np.zeros(0, dtype=np.int32), np.array([0, 0, 0], dtype=np.uint64), [1, 2]), 2
    yield "empty paths only", (2, one, [1, 1], np.zeros(0, dtype=np.int32), np.array([0, 0, 0], dtype=np.uint64), [1, 0]), 3


def check_boundary_table(lib_path, device=0):
    for size in ENTRY_COUNTS:
        for nc in CLUSTER_COUNTS:
            n, links, lens, entries, off, labels = boundary_case(size, nc, seed=size * 1000 + nc)
            sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc, device=device, lib_path=lib_path)
            S.assert_numpy_same(sub, S.expected_by_numpy(n, links, lens, entries, off, labels, nc), f"{size} entries, {nc} clusters")
            assert sub.summary["entries_kept"] == size and sub.summary["read_backs"] == 2
    for name, (n, links, lens, entries, off, labels), nc in special_cases():
        sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc, device=device, lib_path=lib_path)
        S.assert_numpy_same(sub, S.expected_by_numpy(n, links, lens, entries, off, labels, nc), name)
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


# ---- independence ------------------------------------------------------------------------------------------------------------------------------
def independence_case(seed=5):
    rng = random.Random(seed)
    graphs = [S.hand_graph(rng) for _ in range(12)]      # twelve hand graphs side by side
    n, links, lens, paths, base = 0, [], [], [], 0
    for gn, gl, glens, _, gp in graphs:
        shift = lambda e: e + base if e > 0 else e - base
        links += [(shift(a), shift(b)) for a, b in gl]
        paths += [[shift(e) for e in p] for p in gp]
        lens += glens
        base += gn
    n = base
    labels = [rng.randint(0, 5) for _ in paths]
    return n, links, lens, paths, labels, 6


def check_independence(lib_path, device=0):
    n, links, lens, paths, labels, nc = independence_case()
    first = run_raw(lib_path, n, links, lens, paths, labels, nc, None, device)
    for c in range(1, nc + 1):
        S.assert_cluster_same(S.library_cluster(first, c), S.model_cluster(n, links, lens, None, paths, labels, c), f"independence cluster {c}")
    want = S.subsets_bytes(first)
    assert S.subsets_bytes(run_raw(lib_path, n, links, lens, paths, labels, nc, None, device)) == want
    # relabelled clusters: the same products under the inverse permutation
    perm = [0, 4, 6, 1, 3, 2, 5]
    moved = run_raw(lib_path, n, links, lens, paths, [perm[l] for l in labels], nc, None, device)
    for c in range(1, nc + 1):
        assert S.library_cluster(moved, perm[c]) == S.library_cluster(first, c), c
    # shuffled links: everything the same but the links' own order, which follows the input
    shuffled = list(links)
    random.Random(1).shuffle(shuffled)
    other = run_raw(lib_path, n, shuffled, lens, paths, labels, nc, None, device)
    for c in range(1, nc + 1):
        a, b = S.library_cluster(first, c), S.library_cluster(other, c)
        present = set(a["unitigs"])
        assert b["links"] == [l for l in shuffled if abs(l[0]) in present and abs(l[1]) in present] and sorted(a["links"]) == sorted(b["links"])
        assert {k: v for k, v in a.items() if k != "links"} == {k: v for k, v in b.items() if k != "links"}
    return True


@pytest.mark.parametrize("order", [0, 1, 2])
def test_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))      # the emulation's launch order: ascending, descending, pseudo-random
    assert check_independence(emu)


def test_launch_orders_give_identical_bytes(emu, monkeypatch):
    n, links, lens, paths, labels, nc = independence_case()
    seen = set()
    for order in (0, 1, 2):
        monkeypatch.setenv("AC_EMU_ORDER", str(order))
        sub = run_raw(emu, n, links, lens, paths, labels, nc)
        plan = sub.merge_plan(2, with_sequences=False)
        mp = sub.merged_paths(2, plan)
        seen.add(S.subsets_bytes(sub) + M.result_bytes(plan) + mp.entries.tobytes() + mp.path_off.tobytes())
    assert len(seen) == 1


def check_counts(lib_path, device=0):
    """launches and read-backs: the same for 2 clusters and 300 at equal key width (16 bits: 2 x 20 000 and 300 x 200 unitigs), and for all
    sequences in one cluster or spread evenly"""
    rng = np.random.default_rng(3)
    counts = []
    for nc, n in ((2, 20000), (300, 200)):
        entries = rng.integers(1, n + 1, 6000).astype(np.int32)
        off = np.arange(0, 6001, 10, dtype=np.uint64)
        links = rng.integers(1, n + 1, (3000, 2)).astype(np.int32)
        labels = (np.arange(600) % nc + 1).astype(np.uint16)
        sub = subsets_from_paths(n, links, np.ones(n, dtype=np.uint32), (entries, off), labels, nc, device=device, lib_path=lib_path)
        S.assert_numpy_same(sub, S.expected_by_numpy(n, links, np.ones(n), entries, off, labels, nc), f"{nc} clusters")
        assert sub.summary["links"] > 1
        counts.append((sub.summary["launches"], sub.summary["read_backs"]))
        if nc == 300:
            together = subsets_from_paths(n, links, np.ones(n, dtype=np.uint32), (entries, off), np.ones(600, dtype=np.uint16), nc, device=device, lib_path=lib_path)
            counts.append((together.summary["launches"], together.summary["read_backs"]))
    assert counts[0] == counts[1] == counts[2] and counts[0][1] == 2 and counts[0][0] > 0, counts
    return True


def test_counts_do_not_follow_the_clusters(emu):
    assert check_counts(emu)


# ---- composition --------------------------------------------------------------------------------------------------------------------------------
def check_composition(lib_path, device=0):
    n, links, lens, paths, labels, nc = independence_case(seed=8)
    sub = run_raw(lib_path, n, links, lens, paths, labels, nc, None, device)
    marked = [u % 3 == 0 for u in range(n)]
    for c in range(1, nc + 1):
        d = sub.dense(c)
        by_hand = components_from_links(n, links, lens, alive=d["alive"], marked=marked, device=device, lib_path=lib_path)
        got = sub.components(c, marked=marked, device=device)
        for k in ("records", "component_of", "member_off", "members", "flags"):
            assert getattr(got, k).tobytes() == getattr(by_hand, k).tobytes(), (c, k)
        assert got.topology == by_hand.topology
        plan_by_hand = merge_plan_from_links(n, links, lens, alive=d["alive"], path_ends=sub.path_ends(c), depth=d["depth"], fwd_positions=d["fwd_positions"],
                                             rev_positions=d["rev_positions"], device=device, lib_path=lib_path)
        assert M.result_bytes(sub.merge_plan(c, with_sequences=False, device=device)) == M.result_bytes(plan_by_hand), c
    return True


def test_composition(emu):
    assert check_composition(emu)


# ---- trim: the slices as paths, an excluded sequence as label 0 -------------------------------------------------------------------------------
def check_trim(lib_path, device=0):
    """clean_up_graph (trim.rs:260-269) after trim_start_end_overlap and exclude_outliers_in_length: the trimmed sequences walk their slices, the
    excluded one is removed from the graph, then recalculate_depths, remove_zero_depth_unitigs and merge_linear_paths"""
    rng = random.Random(4)
    n = 14
    lens = [rng.randint(2, 9) for _ in range(n)]
    useq = [bytes(rng.choice(b"ACGT") for _ in range(l)) for l in lens]
    core = [1, 2, 3, -4, 5, 6, 7, 8]
    paths = [core + core[:3], core[2:] + core[:4], core + [9, 10], [11, 12, 13, 14, 3, 11, 12]]      # overlaps of 3, 2 (from the third on), none; the last is excluded and leaves links at 3 dangling
    links = M.closed_set([(a, b) for p in paths for a, b in zip(p, p[1:])])
    res, _ = trim_path_slices(paths, lens, 0.75, 5000, device=device, lib_path=lib_path)
    sliced = [p[r["start_end"]["begin"]:r["start_end"]["end"]] if r["start_end"]["status"] == 1 else p for p, r in zip(paths, res)]
    assert sum(r["start_end"]["status"] == 1 for r in res) >= 2 and sliced[0] == core
    labels = [1, 1, 1, 0]
    sub = run_raw(lib_path, n, links, lens, sliced, labels, 1, None, device)
    met = check_clusters(sub, n, links, lens, None, sliced, labels, 1, useq, what="trim", device=device)
    assert met["chain"] and met["link_dropped"] and met["dropped_sequence"]
    assert sub.unitigs(1).tolist() == list(range(1, 11))
    return True


def test_trim_slices(emu):
    assert check_trim(emu)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, torch_device, device=0):
    import ctypes as C
    lib = _capi.load_library(lib_path)
    n, links, lens, paths = 4, [(1, 2), (-2, -1), (2, 3), (-3, -2)], [3, 4, 5, 6], [[1, 2, 3], [-3, -2], []]
    call = lambda **kw: run_raw(lib_path, **dict(dict(n=n, links=links, lens=lens, paths=paths, labels=[1, 2, 1], n_clusters=2, device=device), **kw))

    def works():      # a call after a failed one works
        sub = call()
        plan = sub.merge_plan(1, with_sequences=False, device=device)
        return sub.unitigs(2).tolist() == [2, 3] and plan.chain_members() == [[1, 2, 3]] and sub.merged_paths(1, plan, device=device).paths() == {0: [5], 2: []}
    assert works()
    with pytest.raises(AutocyclerError, match=r"sequence 1 has label 3, above n_clusters = 2"):
        call(labels=[1, 3, 1])
    for bad in (0, 65536):
        with pytest.raises(AutocyclerError, match=r"n_clusters is \d+: it must be between 1 and 65535"):
            call(n_clusters=bad, labels=[0, 0, 0])
    for entry in (0, 5, -5, -2147483648):
        with pytest.raises(AutocyclerError, match=rf"entry 1 of the path of sequence 1 \({entry}\) names no unitig: unitig numbers run from 1 to 4"):
            call(paths=[[1, 2, 3], [-3, entry], []])
        assert works()
    assert call(paths=[[1, 2, 3], [-3, 7], []], labels=[1, 0, 1]).unitigs(1).tolist() == [1, 2, 3]      # (a dropped path is not looked at)
    with pytest.raises(AutocyclerError, match=r"entry 2 of the path of sequence 0 \(3\) enters a unitig that is not alive in the input"):
        call(alive=[1, 1, 0, 1])
    assert works()
    with pytest.raises(AutocyclerError, match=r"link 2 \(2 -> 5\) names no unitig"):
        call(links=links[:2] + [(2, 5)] + links[2:])
    assert works()
    with pytest.raises(AutocyclerError, match=r"entry 0 of the path of sequence 0 \(1\) names no unitig"):
        call(n=0, links=[], lens=[])
    ent, off = np.array([1, 2, 3, -3, -2], dtype=np.int32), np.array([0, 3, 5, 4], dtype=np.uint64)
    with pytest.raises(AutocyclerError, match=r"path_off decreases at sequence 2 \(5 then 4\)"):
        call(paths=(ent, off))
    # the null pointers, on the raw entry
    la = (_capi.Link * 4)(*[_capi.Link(a, b) for a, b in links])
    ln, lab = (C.c_uint32 * 4)(*lens), (C.c_uint16 * 3)(1, 2, 1)
    pe, po = (C.c_int32 * 5)(1, 2, 3, -3, -2), (C.c_uint64 * 4)(0, 3, 5, 5)
    h = C.c_void_p()
    raw = lambda links_, ln_, pe_, po_, lab_, out: lib.ac_subsets_from_paths(4, links_, 4, ln_, None, pe_, po_, 3, lab_, 2, device, out)
    assert raw(la, ln, pe, po, None, C.byref(h)) != 0 and b"cluster_of_seq" in lib.ac_last_error() and not h.value
    assert raw(la, ln, pe, None, lab, C.byref(h)) != 0 and b"path_off" in lib.ac_last_error() and not h.value
    assert raw(la, None, pe, po, lab, C.byref(h)) != 0 and b"unitig_len" in lib.ac_last_error() and not h.value
    assert raw(la, ln, pe, po, lab, None) != 0 and b"null pointer: out" in lib.ac_last_error()
    assert raw(None, ln, pe, po, lab, C.byref(h)) != 0 and b"without links" in lib.ac_last_error() and not h.value
    assert raw(la, ln, None, po, lab, C.byref(h)) != 0 and b"path_entries" in lib.ac_last_error() and not h.value
    assert raw(la, ln, pe, po, lab, C.byref(h)) == 0 and h.value
    assert Subsets(lib, h, 4, None).unitigs(1).tolist() == [1, 2, 3]
    # a cluster that does not exist
    sub = call()
    for c in (0, 3):
        with pytest.raises(AutocyclerError, match=rf"cluster {c} does not exist"):
            sub.merge_plan(c, device=device)
        assert lib.ac_subsets_dense(sub._h, c, None, None, None, None) != 0 and b"does not exist" in lib.ac_last_error()
    # a handle without host arrays or paths
    from test_components_emu import handle_without_host_arrays
    with pytest.raises(AutocyclerError, match="kept no host arrays"):
        bare = handle_without_host_arrays(lib_path, torch_device)
        graph_subsets(bare, [1] * lib.ac_graph_seq_count(bare._h), 1, device=device)
    # plans that were not made from these paths
    plan1, plan2 = sub.merge_plan(1, with_sequences=False, device=device), sub.merge_plan(2, with_sequences=False, device=device)
    with pytest.raises(AutocyclerError, match="the plan was made for cluster 2, not for cluster 1"):
        sub.merged_paths(1, plan2, device=device)
    by_hand, out = C.c_void_p(), C.c_void_p()
    assert lib.ac_merge_plan_from_links(4, la, 4, ln, None, None, 0, None, None, None, None, None, None, device, C.byref(by_hand)) == 0
    assert lib.ac_subsets_merged_paths(sub._h, 1, by_hand, device, C.byref(out)) != 0 and b"the plan was not made by ac_subsets_merge_plan" in lib.ac_last_error()
    assert not out.value
    lib.ac_merge_free(by_hand)
    wider = call(n=5, lens=lens + [1])
    with pytest.raises(AutocyclerError, match="the plan is over 4 unitigs, the subsets over 5"):
        wider.merged_paths(1, plan1, device=device)
    assert works()
    # a kept path that begins or ends strictly inside a chain, or changes its length: only a plan of other paths (here: of a second object over
    # the same unitigs, for the same cluster number) can do it
    inside = call(paths=[[2, 3], [-3, -2], []])
    plan = inside.merge_plan(1, with_sequences=False, device=device)
    assert plan.chain_members() == [[2, 3]] and inside.merged_paths(1, plan, device=device).paths() == {0: [5], 2: []}
    for other_paths, text in (([[3], [-3, -2], []], r"the path of sequence 0 begins strictly inside chain 5 \(entry 3\)"),
                              ([[1], [-3, -2], [1, 2]], r"the path of sequence 2 ends strictly inside chain 5 \(entry 2\)"),
                              ([[-3], [-3, -2], []], r"the path of sequence 0 ends strictly inside chain 5 \(entry -3\)"),
                              ([[1], [-3, -2], [2, 2, 3]], r"the path of sequence 2 changes its length over the merged unitigs")):
        with pytest.raises(AutocyclerError, match=text):
            call(paths=other_paths).merged_paths(1, plan, device=device)
        assert works()
    return True


def test_errors(emu):
    import torch
    assert check_errors(emu, torch.device("cpu"))
