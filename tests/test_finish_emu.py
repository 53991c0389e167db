"""ac_merge_finish / ac_subsets_finish and the Finished object on the CPU emulation of the shipped kernels (kernels_finish.inc) against the
literal Python model of finish_util.py: the S order after merge_path, renumber_unitigs by sorted() with the reference's comparator, the L
lines by a literal get_links_for_gfa over the model's lists, the P lines by the position walk, the text by a literal save_gfa.  Every
comparison is equality.  The same checks run on the device in test_finish_gpu.py."""
import json
import random

import numpy as np
import pytest

import emu_lib
import finish_util as F
import merge_util as M
import subset_util as S
from autocycler_amd import AutocyclerError, Finished, graph_from_gfa, graph_subsets, merge_finish, merge_plan_from_links, subsets_from_paths
from autocycler_amd import _capi
from test_merge_emu import TILE_SIZES
from test_subset_emu import seq_arrays

NEW_SYMBOLS = ("ac_merge_finish", "ac_subsets_finish", "ac_finished_unitigs", "ac_finished_sequences", "ac_finished_new_of_old", "ac_finished_links", "ac_finished_paths",
               "ac_finished_summary_get_sized", "ac_finished_free", "ac_finished_gfa_string", "ac_finished_to_graph")


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_finish(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


# ---- through the library ----------------------------------------------------------------------------------------------------------------------
def plan_of(case, lib_path, device=0):
    return merge_plan_from_links(case["n"], case["links"], case["lens"], case["alive"], case["path_ends"], case["depths"], case["fwd"], case["rev"], case["types"],
                                 case["seqs"], device=device, lib_path=lib_path, keep=True)


def finish_of(case, plan, renumber, lib_path, device=0):
    fin = merge_finish(plan, case["n"], case["links"], case["lens"], case["alive"], case["depths"], case["types"], case["seqs"], renumber=renumber, device=device,
                       lib_path=lib_path)
    assert isinstance(fin, Finished) and fin.summary["renumbered"] == int(renumber)
    return fin


def check_merge_case(case, lib_path, device=0, what=""):
    """one graph as keyword arguments of merge_util.model_expected, renumber 0 and 1: records, new_of_old, links and the whole text"""
    graph, mpaths = F.model_graph(**case)
    met = dict.fromkeys(F.COVERAGE, 0)
    met["chain_from_minus"] = int(any(not p[0][1] for p in mpaths))
    plan = plan_of(case, lib_path, device)
    assert plan.chain_members() == [[num if st else -num for num, st in p] for p in mpaths], what
    for renumber in (False, True):
        exp, got_met = F.finish_model(graph, case["n"], renumber)
        fin = finish_of(case, plan, renumber, lib_path, device)
        F.assert_model_same(F.library_model(fin, False), exp, f"{what} renumber {int(renumber)}")
        for colour in (False, True):
            assert fin.gfa(7, use_other_colour=colour) == F.save_gfa(exp, 7, use_other_colour=colour), f"{what} renumber {int(renumber)} text"
        for k in got_met:
            met[k] |= got_met[k]
        fin.close()
    plan.close()
    return met


def check_cluster_case(n, links, lens, useq, paths, labels, nc, lib_path, device=0, what="", sub=None, handle_seqs=False):
    """every cluster of a graph with paths through Subsets.finish, renumber 0 and 1, as whole GFA text with its P lines"""
    met = dict.fromkeys(F.COVERAGE, 0)
    if sub is None:
        sub = subsets_from_paths(n, links, lens, paths, labels, nc, device=device, lib_path=lib_path)
    sequences = None if handle_seqs else seq_arrays(useq)
    for c in range(1, nc + 1):
        m = S.model_cluster(n, links, lens, None, paths, labels, c)
        exp_plan = S.model_merge(m, useq)
        want = S.model_merged_paths(m, exp_plan)
        graph, mpaths = F.model_graph(m["n"], m["links"], m["lens"], m["alive"], m["path_ends"], m["depth"], m["fwd"], m["rev"], None, useq)
        met["chain_from_minus"] |= int(any(not p[0][1] for p in mpaths))
        plan = sub.merge_plan(c, sequences=sequences, device=device)
        mp = sub.merged_paths(c, plan, device=device, keep=True)
        metas = [(s, s + 1, S.path_length(m["paths"][s], lens, exp_plan), f"hand_{s % 3}.fasta", f"contig_{s}", c) for s in m["seqs"]]
        for renumber in (False, True):
            exp, got_met = F.finish_model(graph, n, renumber, want)
            fin = sub.finish(c, plan, mp, renumber=renumber, sequences=sequences, device=device)
            F.assert_model_same(F.library_model(fin, True), exp, f"{what} cluster {c} renumber {int(renumber)}")
            assert fin.path_seq.tolist() == m["seqs"]
            text = fin.gfa(5, [x[1] for x in metas], [x[2] for x in metas], [x[3] for x in metas], [x[4] for x in metas], [x[5] for x in metas])
            assert text == F.save_gfa(exp, 5, metas), f"{what} cluster {c} renumber {int(renumber)} text"
            for k in got_met:
                met[k] |= got_met[k]
            fin.close()
        mp.close(); plan.close()
    return met


# ---- named cases: the committed GFA that has paths ---------------------------------------------------------------------------------------------
def check_named_cases(lib_path, device=0):
    g = S.gfa_14()
    n_seqs = len(g["paths"])
    subsets = [[int(s == keep) for s in range(n_seqs)] for keep in range(n_seqs)] + [[int(s != out) for s in range(n_seqs)] for out in range(n_seqs)]
    for labels in subsets:
        sub = subsets_from_paths(g["n"], g["links"], g["lens"], g["paths"], labels, 1, alive=g["alive"], device=device, lib_path=lib_path)
        m = S.model_cluster(g["n"], g["links"], g["lens"], g["alive"], g["paths"], labels, 1)
        exp_plan = S.model_merge(m, g["seqs"])
        want = S.model_merged_paths(m, exp_plan)
        graph, _ = F.model_graph(m["n"], m["links"], m["lens"], m["alive"], m["path_ends"], m["depth"], m["fwd"], m["rev"], None, g["seqs"])
        plan = sub.merge_plan(1, sequences=seq_arrays(g["seqs"]), device=device)
        mp = sub.merged_paths(1, plan, device=device, keep=True)
        metas = [(s, s + 1, S.path_length(m["paths"][s], g["lens"], exp_plan), f"assembly_{s}.fasta", f"contig_{s} of test_gfa_14", 1) for s in m["seqs"]]
        for renumber in (False, True):
            exp, _ = F.finish_model(graph, g["n"], renumber, want)
            fin = sub.finish(1, plan, mp, renumber=renumber, sequences=seq_arrays(g["seqs"]), device=device)
            text = fin.gfa(9, [x[1] for x in metas], [x[2] for x in metas], [x[3] for x in metas], [x[4] for x in metas], [x[5] for x in metas], use_other_colour=True)
            assert text == F.save_gfa(exp, 9, metas, use_other_colour=True), (labels, renumber)
            F.assert_model_same(F.library_model(fin, True), exp, f"test_gfa_14 {labels} renumber {int(renumber)}")
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


def check_kats(lib_path, device=0):
    """what the unit tests of graph_simplification.rs state about a graph after merge_linear_paths (tests/golden/finish_kats.json: data only)"""
    for kat in json.loads((M.GOLDEN / "finish_kats.json").read_text()):
        g = M.gfa_graph(kat["gfa"])
        case = dict(n=g["n"], links=g["links"], lens=g["lens"], alive=g["alive"], path_ends=g["path_ends"], depths=g["depths"], fwd=g["fwd"], rev=g["rev"], types=None,
                    seqs=g["seqs"])
        plan = plan_of(case, lib_path, device)
        fin = finish_of(case, plan, False, lib_path, device)
        by_number = dict(zip(fin.unitigs["number"].tolist(), (s.decode() for s in fin.unitig_sequences())))
        assert len(by_number) == kat["unitigs"], kat["name"]
        for number, seq in kat["sequences"].items():      # (the reference's tests name the merged unitigs by number)
            assert by_number[int(number)] == seq, (kat["name"], number)
        if kat["links"] is not None:      # (... and state the links as a sorted set)
            assert sorted(tuple(l) for l in fin.links.tolist()) == sorted(tuple(l) for l in kat["links"]), (kat["name"], fin.links.tolist())
        plan.close()
        check_merge_case(case, lib_path, device, kat["name"])
    return True


def test_known_answers(emu):
    assert check_kats(emu)


# ---- random sweep -----------------------------------------------------------------------------------------------------------------------------
def planted_case(rng):
    """merge_util.random_case with what random links rarely give planted on top: a stretch whose lowest member sits inside it on the reverse
    strand (the chain is found from a - strand), a stretch closed into a loop beside a fixed neighbour, a flip at a stretch's start or end,
    two stretches linked end to start; short equal sequences with equal and unequal depths for the ties"""
    case = M.random_case(rng)
    n = case["n"]
    if n < 8:
        return case
    case["alive"] = None
    order = list(range(1, n + 1))
    rng.shuffle(order)
    a, b = [x if rng.random() < 0.5 else -x for x in order[:3]], [x if rng.random() < 0.5 else -x for x in order[3:6]]
    used = {abs(x) for x in a + b}
    links = [(p, q) for p, q in case["links"] if abs(p) not in used and abs(q) not in used]
    links += list(zip(a, a[1:])) + list(zip(b, b[1:]))
    spare = order[6]
    kind_a, kind_b = rng.choice(("loop", "start_flip", "end_flip", "plain")), rng.choice(("linked", "start_flip", "end_flip", "plain"))
    for chain, kind in ((a, kind_a), (b, kind_b)):
        if kind == "loop":
            links += [(chain[-1], chain[0]), (spare, chain[0])]           # a loop with a second way in: the chain's own link + -> +
        elif kind == "start_flip":
            links += [(-chain[0], chain[0]), (-chain[0], spare)]          # a start flip beside another target
        elif kind == "end_flip":
            links += [(chain[-1], -chain[-1]), (chain[-1], spare)]        # an end flip beside another target
        elif kind == "linked":
            links.append((a[-1], b[0]))                                   # two chains linked to each other, kept apart by a path end
            case["path_ends"] = list(case["path_ends"]) + [(b[0], b[-1])]
        else:
            links.append((chain[-1], spare))
    case["links"] = M.closed_set(links)
    rng.shuffle(case["links"])
    seqs, depths = list(case["seqs"]), list(case["depths"])
    for u in order[6:]:
        if rng.random() < 0.5:
            seqs[u - 1] = rng.choice((b"ACGTACGTACG", b"ACGTACGTACT", b"ACGTACGTAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAC"))
            depths[u - 1] = rng.choice((1.0, 1.0, 2.0, -0.0, 0.0))
    case["seqs"], case["depths"], case["lens"] = seqs, depths, [len(s) for s in seqs]
    return case


def check_sweep(lib_path, seed, cases, device=0):
    rng = random.Random(seed)
    total = dict.fromkeys(F.COVERAGE, 0)
    for i in range(cases):
        what = f"seed {seed} case {i}"
        if i % 3 == 0:
            n, links, lens, useq, paths = S.hand_graph(rng)
            labels, nc = S.random_labels(rng, len(paths))
            got = check_cluster_case(n, links, lens, useq, paths, labels, nc, lib_path, device, what)
        elif i % 6 == 1:
            got = check_merge_case(M.random_case(rng), lib_path, device, what)
        else:
            got = check_merge_case(planted_case(rng), lib_path, device, what)
        for k in F.COVERAGE:
            total[k] += got[k]
    return total


def assert_sweep_coverage(results, least=20):
    total = {k: sum(r[k] for r in results) for k in F.COVERAGE}
    assert all(v >= least for v in total.values()), total


def test_random_sweep(emu):
    assert_sweep_coverage([check_sweep(emu, 12000 + seed, 150) for seed in range(4)])      # 600 graphs


# ---- renumbering alone: unlinked unitigs against sorted() and numpy ------------------------------------------------------------------------------
def renumber_only(seqs, depths, lib_path, device=0):
    """unitigs without links: (old numbers in new order, the Finished)"""
    n = len(seqs)
    case = dict(n=n, links=[], lens=[len(s) for s in seqs], alive=None, path_ends=[], depths=list(depths), fwd=None, rev=None, types=None, seqs=list(seqs))
    plan = plan_of(case, lib_path, device)
    fin = finish_of(case, plan, True, lib_path, device)
    plan.close()
    assert fin.unitigs["number"].tolist() == list(range(1, n + 1)) and sorted(fin.unitigs["source"].tolist()) == list(range(1, n + 1))
    assert fin.unitig_sequences() == [seqs[s - 1] for s in fin.unitigs["source"].tolist()]
    assert fin.new_of_old[fin.unitigs["source"].astype(np.int64) - 1].tolist() == list(range(1, n + 1))
    return fin.unitigs["source"].tolist(), fin


GROUP_SIZES = (1, 2, 63, 64, 65)


def boundary_unitigs(n, group, seed):
    """n unitigs: groups of `group` share length 21 and their first 12 bytes (a tie group each, beyond the 8 bytes of the radix key) and differ
    behind them or not at all; the rest are 1-3 bases long.  Depths from three values, -0.0 among them."""
    rng = np.random.default_rng(seed)
    seqs, depths = [], []
    n_groups = max(1, min(n // group, 6))
    for g in range(n_groups):
        head = bytes(rng.choice(list(b"ACGT"), 12).tolist())
        for _ in range(group):
            seqs.append(head + bytes(rng.choice(list(b"AC"), 9, p=(0.9, 0.1)).tolist()))
    while len(seqs) < n:
        seqs.append(bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 4))).tolist()))
    seqs = seqs[:n]
    order = rng.permutation(n)
    seqs = [seqs[i] for i in order]
    depths = rng.choice((2.0, 0.0, -0.0, 7.5), n).tolist()
    return seqs, depths


def check_boundary_table(lib_path, device=0):
    sizes = sorted(set(GROUP_SIZES + TILE_SIZES + (255, 256, 257)))
    for n in sizes:
        for group in GROUP_SIZES:
            if group > n:
                continue
            seqs, depths = boundary_unitigs(n, group, seed=n * 100 + group)
            got, fin = renumber_only(seqs, depths, lib_path, device)
            assert got == F.expected_order(seqs, depths), (n, group)
            assert fin.summary["read_backs"] == 3      # the tie header, the results' header, the results
    # equal lengths throughout: numpy's lexsort says the same
    rng = np.random.default_rng(3)
    for n, length in ((65, 1), (300, 9), (257, 33)):
        arr = rng.choice(np.frombuffer(b"AC", dtype=np.uint8), (n, length))
        depths = rng.choice((1.0, 2.0, -0.0, 0.0), n)
        got, _ = renumber_only([bytes(r) for r in arr], depths.tolist(), lib_path, device)
        assert got == F.expected_order_numpy(arr, depths) == F.expected_order([bytes(r) for r in arr], depths.tolist()), (n, length)
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


# ---- independence ------------------------------------------------------------------------------------------------------------------------------
def check_independence(lib_path, device=0, orders=(None,)):
    """the same bytes run after run (and, on the emulation, for its three launch orders)"""
    import os
    rng = random.Random(77)
    cases = [planted_case(rng) for _ in range(6)]
    seqs, depths = boundary_unitigs(300, 65, seed=9)
    want = None
    before = os.environ.get("AC_EMU_ORDER")
    try:
        for order in orders:
            if order is not None:
                os.environ["AC_EMU_ORDER"] = str(order)
            got = []
            for case in cases:
                plan = plan_of(case, lib_path, device)
                got += [F.finished_bytes(finish_of(case, plan, r, lib_path, device)) for r in (False, True)]
                plan.close()
            got.append(F.finished_bytes(renumber_only(seqs, depths, lib_path, device)[1]))
            want = want or got
            assert got == want, order
    finally:
        if before is None:
            os.environ.pop("AC_EMU_ORDER", None)
        else:
            os.environ["AC_EMU_ORDER"] = before
    return True


def test_independent_of_launch_order(emu):
    assert check_independence(emu, orders=(0, 1, 2, 0))


# ---- independent of the model: through a graph handle ---------------------------------------------------------------------------------------------
def check_round_trip(lib_path, device=0, cases=12):
    """a hand graph as a handle; every cluster finished with renumber = 1 and turned into a handle again: every kept sequence decompresses to the
    bytes it decompresses to from the original handle, and the text loads"""
    rng = random.Random(31)
    done = 0
    while done < cases:
        n, links, lens, useq, paths = S.hand_graph(rng)
        if not all(paths):
            continue
        g, fns, hds = graph_from_gfa(S.hand_gfa_text(n, links, useq, paths), lib_path=lib_path)
        labels, nc = S.random_labels(rng, len(paths))
        sub = graph_subsets(g, labels, nc, device=device)
        for c in range(1, nc + 1):
            kept = sub.seqs(c).tolist()
            plan = sub.merge_plan(c, device=device)
            mp = sub.merged_paths(c, plan, device=device, keep=True)
            fin = sub.finish(c, plan, mp, renumber=True, device=device)
            originals = [g.decompress(s) for s in kept]
            meta = ([s + 1 for s in kept], [len(x) for x in originals], [fns[s] for s in kept], [hds[s] for s in kept])
            g2 = fin.to_graph(5, *meta)
            assert [g2.decompress(i) for i in range(len(kept))] == originals, (done, c)
            g3, fns3, hds3 = graph_from_gfa(fin.gfa(5, *meta, cluster_tags=[c] * len(kept)), lib_path=lib_path)      # (the loader passes over CL:i)
            assert [g3.decompress(i) for i in range(len(kept))] == originals and fns3 == meta[2] and hds3 == meta[3]
            assert g2.unitig_count == fin.summary["unitigs"] == g3.unitig_count
            with pytest.raises(AutocyclerError, match="renumber = 1"):
                sub.finish(c, plan, mp, renumber=False, device=device).to_graph(5, *meta)
            mp.close(); plan.close()
        done += 1
    return True


def test_round_trip_through_a_handle(emu):
    assert check_round_trip(emu)


# ---- the shapes that cross the tie-group paths ---------------------------------------------------------------------------------------------------
def one_base_unitigs(n, seed=1):
    rng = np.random.default_rng(seed)
    return [bytes([b]) for b in rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tolist()], rng.choice((1.0, 2.5, 40.0), n).tolist()


def shared_prefix_unitigs(n, seed=2):
    """40 bases, the first 32 shared, the first difference at byte 32 + i % 8"""
    rng = np.random.default_rng(seed)
    head = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 32).tolist())
    seqs = []
    for i in range(n):
        tail = bytearray(b"A" * 8)
        for j in range(i % 8, 8):
            tail[j] = int(rng.choice(np.frombuffer(b"CGT" if j == i % 8 else b"ACGT", dtype=np.uint8)))
        seqs.append(head + bytes(tail))
    return seqs, rng.choice((1.0, 2.5, 40.0), n).tolist()


def check_one_base_unitigs(lib_path, n, device=0):
    """n one-base unitigs over ACGT with three depth values: four groups of full sequence ties, a third of each a full tie down to the depth"""
    seqs, depths = one_base_unitigs(n)
    got, fin = renumber_only(seqs, depths, lib_path, device)
    assert got == F.expected_order(seqs, depths)
    assert fin.summary["tie_items"] == 0      # (up to 8 bases the radix keys are exact)
    return True


def check_shared_prefix(lib_path, n, device=0):
    """n unitigs of 40 bases that share 32: one tie group of all of them behind the radix keys"""
    seqs, depths = shared_prefix_unitigs(n)
    got, fin = renumber_only(seqs, depths, lib_path, device)
    assert got == F.expected_order(seqs, depths)
    assert fin.summary["tie_items"] == n
    return True


def check_last_byte(lib_path, length, device=0):
    """130 unitigs of `length` bases, identical but for the last byte, two of them fully identical with different depths"""
    rng = np.random.default_rng(3)
    body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), length - 1).tolist())
    seqs = [body + bytes([60 + int(x)]) for x in rng.permutation(129)]      # 129 different last bytes
    depths = rng.choice((1.0, 2.0), 129).tolist()
    seqs.append(seqs[5])      # unitig 130 = unitig 6, and the deeper of the two: depth, not order, must decide
    depths[5] = 3.0
    depths.append(9.0)
    got, fin = renumber_only(seqs, depths, lib_path, device)
    want = F.expected_order(seqs, depths)
    assert got == want and want.index(130) + 1 == want.index(6)
    assert fin.summary["tie_items"] == 130
    return True


def check_length_classes(lib_path, longest, device=0):
    """lengths 1 ... longest mixed, three unitigs of every length, two of them equal"""
    rng = np.random.default_rng(4)
    seqs = []
    for length in range(1, longest + 1):
        s = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), length).tolist())
        seqs += [s, s, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), length).tolist())]
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    depths = rng.choice((1.0, 2.0, 0.0, -0.0), len(seqs)).tolist()
    got, _ = renumber_only(seqs, depths, lib_path, device)
    assert got == F.expected_order(seqs, depths)
    return True


def check_launch_counts(lib_path, n, device=0):
    """the first two shapes at the same n: the same launches and read-backs, whether the radix keys leave nothing open or everything"""
    _, ones = renumber_only(*one_base_unitigs(n), lib_path, device)
    _, shared = renumber_only(*shared_prefix_unitigs(n), lib_path, device)
    assert ones.summary["tie_items"] == 0 and shared.summary["tie_items"] == n
    assert (ones.summary["launches"], ones.summary["read_backs"]) == (shared.summary["launches"], shared.summary["read_backs"])
    return True


def ring_case(n, n_paths, path_len, n_clusters, seed):
    links, entries, off = S.ring_with_chords(n, n_paths, path_len, seed)
    labels = (np.random.default_rng(seed + 1).permutation(n_paths) % n_clusters + 1).astype(np.uint16)
    return links, entries, off, labels


def check_ring(lib_path, n, path_len, least_unitigs, device=0):
    """subset_util.ring_with_chords: n one-base unitigs on a ring with chords, 64 walks of path_len entries, 8 clusters, cluster 3 finished with
    renumber = 1.  The order is sorted()'s over the library's own records; the links are the plan's set under the printed numbers, grouped as
    get_links_for_gfa groups them; every path keeps its length."""
    nc, c = 8, 3
    links, entries, off, labels = ring_case(n, 64, path_len, nc, seed=21)
    lens = np.ones(n, dtype=np.uint32)
    seq_bytes = np.random.default_rng(8).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n + 1)
    sequences = (seq_bytes, np.arange(n, dtype=np.uint64))
    sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc, device=device, lib_path=lib_path)
    plan = sub.merge_plan(c, sequences=sequences, device=device)
    mp = sub.merged_paths(c, plan, device=device, keep=True)
    fin = sub.finish(c, plan, mp, renumber=True, sequences=sequences, device=device)
    u = fin.unitigs
    assert len(u) == plan.summary["unitigs_after"] > least_unitigs and u["number"].tolist() == list(range(1, len(u) + 1))
    seqs = fin.unitig_sequences()
    first = np.argsort(u["source"], kind="stable").tolist()      # graph.unitigs before the sort: ascending source
    want = sorted(first, key=lambda i: (-len(seqs[i]), seqs[i], -float(u["depth"][i])))
    assert want == list(range(len(u)))
    # sources: what is alive and unmerged keeps its base; a chain its merged sequence
    merged = u["source"] > n
    assert np.array_equal(u["length"][~merged], np.ones((~merged).sum(), dtype=np.uint64))
    assert [seqs[i] for i in np.flatnonzero(merged)[:50].tolist()] == [plan.chain_sequences()[int(s) - n - 1] for s in u["source"][merged][:50].tolist()]
    # links: the plan's set under the printed numbers
    new = np.concatenate([[0], fin.new_of_old.astype(np.int64)])
    relabelled = np.sign(plan.links.astype(np.int64)) * new[np.abs(plan.links.astype(np.int64))]
    assert sorted(map(tuple, relabelled.tolist())) == sorted(map(tuple, fin.links.tolist()))
    src = fin.links[:, 0].astype(np.int64)
    group = 2 * np.abs(src) + (src < 0)
    assert (np.diff(group) >= 0).all()      # per unitig in S order: forward_next, then reverse_next
    # paths: the merged paths under the printed numbers
    assert np.array_equal(np.sign(mp.entries) * new[np.abs(mp.entries.astype(np.int64))], fin.path_entries) and fin.path_seq.tolist() == sub.seqs(c).tolist()
    length_of = np.zeros(len(u) + 1, dtype=np.int64)
    length_of[u["number"]] = u["length"]
    assert np.add.reduceat(length_of[np.abs(fin.path_entries)], fin.path_off[:-1].astype(np.int64)).tolist() == [path_len] * 8
    return True


def check_ring_against_the_model(lib_path, device=0):
    n, nc = 2000, 8
    links, entries, off, labels = ring_case(n, 64, 300, nc, seed=22)
    lens = [1] * n
    useq = [bytes([b]) for b in np.random.default_rng(9).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tolist()]
    paths = [entries[int(off[s]):int(off[s + 1])].tolist() for s in range(64)]
    sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc, device=device, lib_path=lib_path)
    met = check_cluster_case(n, [tuple(l) for l in links.tolist()], lens, useq, paths, labels.tolist(), nc, lib_path, device, what="ring of 2000", sub=sub)
    assert met["chains_linked"] and met["merged_before_unmerged"] and met["tie_by_order"]
    return True


def test_tie_group_shapes_small(emu):
    """the device's shapes (test_finish_gpu.py) at sizes the emulation takes"""
    assert check_one_base_unitigs(emu, 2049) and check_shared_prefix(emu, 131) and check_last_byte(emu, 2050) and check_length_classes(emu, 40)
    assert check_launch_counts(emu, 131)


def test_ring_small(emu):
    assert check_ring(emu, 3001, 300, 100) and check_ring_against_the_model(emu)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, device=0):
    rng = random.Random(5)
    case = planted_case(rng)
    while case["n"] < 8 or case["alive"] is not None:
        case = planted_case(rng)
    n = case["n"]
    plan = plan_of(case, lib_path, device)

    def works():
        exp, _ = F.finish_model(F.model_graph(**case)[0], n, True)
        F.assert_model_same(F.library_model(finish_of(case, plan, True, lib_path, device), False), exp, "after an error")

    def refused(pattern, **change):
        kw = dict(case, **change)
        with pytest.raises(AutocyclerError, match=pattern):
            merge_finish(plan, kw["n"], kw["links"], kw["lens"], kw["alive"], kw["depths"], kw["types"], kw["seqs"], renumber=kw.get("renumber", True), device=device,
                         lib_path=lib_path)
        works()
    refused(rf"the plan is over {n} unitigs, the call over {n + 1}", n=n + 1, lens=case["lens"] + [1], depths=case["depths"] + [0.0], types=case["types"] + [0],
            seqs=case["seqs"] + [b"A"])
    refused(rf"the plan was made from {len(case['links'])} links, the call gives {len(case['links']) + 1}", links=case["links"] + [(1, 1)])
    survivor = next(u for u in range(1, n + 1) if plan.chain_of[u - 1] == M.NOT_MERGED)
    depths = list(case["depths"])
    depths[survivor - 1] = float("nan")
    refused(rf"the depth of unitig {survivor} is NaN", depths=depths)
    fin = merge_finish(plan, n, case["links"], case["lens"], None, depths, case["types"], case["seqs"], renumber=False, device=device, lib_path=lib_path)      # (no comparator: no error)
    assert np.isnan(fin.unitigs["depth"]).sum() == 1
    refused("missing sequences: seq_bytes and seq_begin are needed", seqs=None)
    dead = [1] * n
    dead[survivor - 1] = 0
    refused("it was made from another alive mask", alive=dead)
    no_seq_plan = merge_plan_from_links(n, case["links"], case["lens"], None, case["path_ends"], case["depths"], case["fwd"], case["rev"], case["types"], None, device=device,
                                        lib_path=lib_path, keep=True)
    if len(no_seq_plan.chains):
        with pytest.raises(AutocyclerError, match="missing sequences: the plan was made without them"):
            merge_finish(no_seq_plan, n, case["links"], case["lens"], None, case["depths"], case["types"], case["seqs"], device=device, lib_path=lib_path)
        works()
    lib = _capi.load_library(lib_path)
    h = _capi.C.c_void_p()
    assert lib.ac_merge_finish(None, 0, None, 0, None, None, None, None, None, None, None, 0, device, _capi.C.byref(h)) == 1 and b"null pointer: plan" in lib.ac_last_error()
    assert lib.ac_merge_finish(plan._h, 0, None, 0, None, None, None, None, None, None, None, 0, device, None) == 1 and b"null pointer: out" in lib.ac_last_error()
    works()
    # shuffled links of the same set: still the plan's links, another list order — a valid call whose L lines follow the new order
    shuffled = list(case["links"])
    random.Random(2).shuffle(shuffled)
    other = dict(case, links=shuffled)
    exp, _ = F.finish_model(F.model_graph(**other)[0], n, True)
    F.assert_model_same(F.library_model(finish_of(other, plan, True, lib_path, device), False), exp, "shuffled links")
    plan.close()
    with pytest.raises(AutocyclerError, match="handle must be open"):
        finish_of(case, plan, True, lib_path, device)
    return True


def test_errors(emu):
    assert check_errors(emu)
