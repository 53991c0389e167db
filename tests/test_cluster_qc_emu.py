"""ac_cluster_generate / ac_cluster_qc_nodes and their helpers on the CPU emulation of the shipped kernels (kernels_cluster_qc.inc under the
lockstep emulation of wave_rt.hpp), against the reference's known answers (golden/cluster_qc_kats.json) and the plain-Python model of
cluster_qc_util.py.  Everything is compared bit for bit with the model's "fixed" form, and with its "literal" form under three shuffles of
the balance sum wherever the number of file names is a power of two.  The same checks run on the device in test_cluster_qc_gpu.py."""
import random

import pytest

import cluster_qc_util as Q
import cluster_util as U
import emu_lib
import parity_util
import seqgen
from autocycler_amd import AutocyclerError, ClusterTree, cluster_min_assemblies, cluster_tree, graph_from_gfa


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = Q.load_kats()
_cache = {}


def cached(key, fn):
    if key is None:
        return fn()
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def power_of_two(x):
    return x > 0 and x & (x - 1) == 0


def check_summary(got, manual=False, default_batches=True):
    """the schedule DESIGN.md 9f states: one launch for the bits, then per evaluation its pair batches and one chain launch, and one
    read-back; an evaluation = the start clustering, or a round that has an alternative.  Nothing with manual clusters."""
    sm, trace = got.summary, got.trace
    evaluations = 0 if manual else 1 + sum(1 for r in trace if r["scores"])
    assert sm["rounds"] == len(trace) and sm["evaluations"] == evaluations and sm["readbacks"] == evaluations
    assert sm["launches"] == (1 + sm["pair_batches"] + evaluations if evaluations else 0)
    assert sm["pair_batches"] >= evaluations and (not default_batches or sm["pair_batches"] == evaluations)
    assert sm["alternatives"] == (0 if manual else 1 + sum(len(r["scores"]) for r in trace))
    assert sm["n_clusters"] == len(got.records) and sm["n_seqs"] == len(got.cluster_of_seq) and sm["seconds"] >= 0
    return True


def compare_generate(t, asym, inp, cutoff, min_assemblies, manual=(), device=0, key=None, default_batches=True):
    """generate on the library's tree handle against both forms of the model -> (library result, model result)"""
    model = U.Tree(t.nodes, t.root)
    exp = cached(key and (key, "fixed"), lambda: Q.generate_clusters(model, asym, inp, cutoff, min_assemblies, manual, "fixed"))
    got = t.generate(asym, *inp.args(), cutoff, min_assemblies, manual, device=device)
    assert Q.same_result(got, exp)
    if power_of_two(inp.n_assemblies):
        for seed in (1, 2, 3):
            lit = cached(key and (key, "literal", seed), lambda: Q.generate_clusters(model, asym, inp, cutoff, min_assemblies, manual, "literal", random.Random(seed)))
            assert Q.same_result(got, lit)
    assert check_summary(got, bool(manual), default_batches)
    return got, exp


def compare_qc(t, nodes, asym, inp, cutoff, min_assemblies, manual=(), device=0):
    model = U.Tree(t.nodes, t.root)
    exp = Q.qc_clusters(model, asym, inp, nodes, list(manual), cutoff, min_assemblies, "fixed")
    got = t.qc(nodes, asym, *inp.args(), cutoff, min_assemblies, manual, device=device)
    assert got.clusters == list(nodes) and got.trace == []
    assert Q.same_result(got, exp, ("cluster_of_seq", "records", "metrics"))
    assert got.summary["start_score"].hex() == exp["metrics"]["overall_clustering_score"].hex()
    if power_of_two(inp.n_assemblies):
        for seed in (1, 2, 3):
            assert Q.same_result(got, Q.qc_clusters(model, asym, inp, nodes, list(manual), cutoff, min_assemblies, "literal", random.Random(seed)),
                                 ("cluster_of_seq", "records", "metrics"))
    assert check_summary(got, bool(manual))
    return got


def two_files(n):
    return [i % 2 for i in range(n)]


# ---- 1. the known answers -------------------------------------------------------------------------------------------------------------
def test_models_reproduce_kats():
    trees = {k: U.Tree([tuple(n) for n in v["nodes"]], v["root"]) for k, v in KATS["trees"].items()}
    for c in KATS["split_clusters"]:
        assert Q.split_clusters(trees[c["tree"]], c["clusters"]) == c["expected"]
    for c in KATS["cluster_assembly_count"]:
        seqs = c["sequences"]
        assembly = Q.number_assemblies([s["filename"] for s in seqs])
        weights = [Q.cluster_weight(s["header"]) for s in seqs]
        for cl, exp in c["expected"].items():
            assert Q.cluster_assembly_count([s["cluster"] for s in seqs], int(cl), assembly, weights) == exp, c["test"]
    c = KATS["set_minpts"]
    for user in c["explicit"]:
        assert Q.set_min_assemblies(len(set(c["filenames"])), user) == user
    for step in c["automatic"]:
        assert Q.set_min_assemblies(len(set(c["filenames"][:step["sequences"]]))) == step["expected"]
    c = KATS["calculate_balance"]
    for rng in (None, random.Random(1), random.Random(2)):      # (either form: the order of the sum only moves the last bits)
        scores = []
        for case in c["cases"]:
            order = sorted(case)
            if rng:
                rng.shuffle(order)
            scores.append(Q.calculate_balance(case, order))
        assert abs(scores[0] - c["first"]) < c["tolerance"] and all(a > b for a, b in zip(scores, scores[1:]))
    c = KATS["calculate_tightness"]
    assert abs(Q.calculate_tightness([tuple(x) for x in c["combined"]]) - Q.calculate_tightness([tuple(x) for x in c["split"]])) < c["tolerance"]


def check_kats(lib_path, device=0):
    c = KATS["set_minpts"]
    for step in c["automatic"]:
        assert cluster_min_assemblies(Q.number_assemblies(c["filenames"][:step["sequences"]]), lib_path=lib_path) == step["expected"]
    # cluster_assembly_count: the reference's clusters as groups of a tree, read from the records
    for c in KATS["cluster_assembly_count"]:
        seqs = sorted(c["sequences"], key=lambda s: s["cluster"])
        sizes = [sum(1 for s in seqs if s["cluster"] == cl) for cl in sorted(set(s["cluster"] for s in seqs))]
        nodes, groups = Q.grouped_tree(sizes)
        t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
        inp = Q.inputs_from_headers([10 - s["cluster"] for s in seqs], [s["filename"] for s in seqs], [s["header"] for s in seqs])
        got = compare_qc(t, groups, Q.contain_matrix(sizes, {}), inp, 0.2, 2, device=device)
        assert [r["assembly_count"] for r in got.records] == [c["expected"][str(cl)] for cl in sorted(int(x) for x in c["expected"])], c["test"]
    # calculate_balance: the six cases as clusterings (3 and 6 file names: the fixed order is what is compared)
    c = KATS["calculate_balance"]
    scores = []
    for case in c["cases"]:
        files = [f for cl in sorted(case) for f in case[cl]]
        sizes = [len(case[cl]) for cl in sorted(case)]
        nodes, groups = Q.grouped_tree(sizes)
        t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
        lengths = [100 - g for g, s in enumerate(sizes) for _ in range(s)]
        inp = Q.Inputs(lengths, Q.number_assemblies(files), [1] * len(files), [0] * len(files))
        got = compare_qc(t, groups, Q.contain_matrix(sizes, {}), inp, 0.2, 1, device=device)
        assert got.metrics["cluster_balance_score"].hex() == Q.calculate_balance({int(k): v for k, v in case.items()}).hex()
        scores.append(got.metrics["cluster_balance_score"])
    assert abs(scores[0] - c["first"]) < c["tolerance"] and all(a > b for a, b in zip(scores, scores[1:]))
    # calculate_tightness: one cluster of 4 at distance 0 and one of 8 at 0.25, whole and with the first split into single sequences
    c = KATS["calculate_tightness"]
    nodes, groups = Q.grouped_tree([4, 8], inner=0.0, group=0.0, step=0.25)
    top = [n[0] for n in nodes].index(groups[1])
    nodes[top] = (nodes[top][0], nodes[top][1], nodes[top][2], 0.125)      # the top of the second group: max_pairwise_distance 0.25
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    inp = Q.Inputs([9] * 4 + [5] * 8, two_files(12), [1] * 12, [0] * 12)
    m = Q.contain_matrix([4, 8], {})
    whole = compare_qc(t, groups, m, inp, 0.2, 0, device=device)
    split = compare_qc(t, [1, 2, 3, 4, groups[1]], m, inp, 0.2, 0, device=device)
    assert whole.metrics["cluster_tightness_score"].hex() == Q.calculate_tightness([tuple(x) for x in c["combined"]]).hex()
    assert abs(whole.metrics["cluster_tightness_score"] - split.metrics["cluster_tightness_score"]) < c["tolerance"]
    return True


def test_kats(emu):
    assert check_kats(emu)


# ---- 2. the smallest shapes --------------------------------------------------------------------------------------------------------------
def check_smallest(lib_path, device=0):
    one = Q.Inputs([7], [0], [1], [0])
    t = cluster_tree([[0.0]], [9], normalise=False, device=device, lib_path=lib_path)
    assert cluster_min_assemblies(one.assembly, lib_path=lib_path) == 1
    got, _ = compare_generate(t, [[0.0]], one, 0.2, 1, device=device)
    assert got.clusters == [9] and got.cluster_of_seq == [1] and got.trace == [{"scores": [], "accepted": []}] and got.records[0]["fail"] == 0
    assert got.summary["launches"] == 3 and got.summary["node_pairs"] == 0
    asym = [[0.0, 0.25], [0.25, 0.0]]
    t = cluster_tree(asym, [3, 8], normalise=False, device=device, lib_path=lib_path)
    for inp in (Q.Inputs([5, 6], [0, 1], [1, 1], [0, 0]), Q.Inputs([5, 6], [0, 0], [1, 1], [0, 0])):      # two assemblies; ONE assembly
        mn = cluster_min_assemblies(inp.assembly, lib_path=lib_path)
        assert mn == Q.set_min_assemblies(inp.n_assemblies) == (2 if inp.n_assemblies == 2 else 1)
        got, _ = compare_generate(t, asym, inp, 0.5, mn, device=device)      # the cut is the root: one alternative
        assert [len(r["scores"]) for r in got.trace][0] == 1
        got, _ = compare_generate(t, asym, inp, 0.1, mn, device=device)      # the cut is the tips: none
        assert got.clusters == [3, 8] and got.trace == [{"scores": [], "accepted": []}]
    return True


def test_smallest(emu):
    assert check_smallest(emu)


# ---- 3. splitting helps, twice in a row -------------------------------------------------------------------------------------------------
def check_split_twice(lib_path, device=0):
    """two replicons, two copies of each per file, two files: the first cut (the root) has balance 0, splitting it into the replicons
    raises the tightness, splitting a replicon into its copies raises the balance"""
    of = [(r, copy) for r in range(2) for copy in range(2) for _ in range(2)]      # sequences 0..7; the two of a (replicon, copy) are one per file
    d = lambda x, y: 0.0 if x == y else (0.0625 if of[x] == of[y] else (0.125 if of[x][0] == of[y][0] else 0.5))
    asym = [[d(i, j) for j in range(8)] for i in range(8)]
    inp = Q.Inputs([4000 - 1000 * of[i][0] - 10 * i for i in range(8)], two_files(8), [1] * 8, [0] * 8)
    t = cluster_tree(asym, range(1, 9), normalise=False, device=device, lib_path=lib_path)
    got, exp = compare_generate(t, asym, inp, 2.0, 2, device=device)
    accepted_rounds = [any(r["accepted"]) for r in got.trace]
    assert accepted_rounds.count(True) >= 2 and accepted_rounds[-1] is False and accepted_rounds[:-1] == [True] * (len(accepted_rounds) - 1)
    assert len(got.clusters) == 4 and got.metrics["cluster_balance_score"] == 1.0 and got.summary["start_score"] < got.metrics["overall_clustering_score"]
    start = compare_qc(t, t.cut(2.0), asym, inp, 2.0, 2, device=device)
    assert start.metrics["cluster_balance_score"] == 0.0 and len(start.records) == 1
    return True


def test_split_twice(emu):
    assert check_split_twice(emu)


# ---- 4. the running best -----------------------------------------------------------------------------------------------------------------
def running_best_tree(dx, dy):
    """X = (X1, X2) and Y = (Y1, Y2), each X1 .. Y2 two sequences from two files: alternatives [9, 10, 14] (split X) < [11, 12, 13] (split Y)"""
    return [(i, -1, -1, 0.0) for i in range(1, 9)] + [(9, 0, 1, 0.0), (10, 2, 3, 0.0), (11, 4, 5, 0.0), (12, 6, 7, 0.0),
                                                       (13, 8, 9, dx / 2.0), (14, 10, 11, dy / 2.0), (15, 12, 13, 0.45)]


def check_running_best(lib_path, device=0):
    asym = Q.contain_matrix([4, 4], {})
    inp = Q.Inputs([900 - i for i in range(8)], two_files(8), [1] * 8, [0] * 8)
    for (dx, dy), accepted, winner in (((0.0625, 0.5625), [True, True], [11, 12, 13]),      # both beat the start, the later is better
                                       ((0.5625, 0.0625), [True, False], [9, 10, 14]),     # the earlier is better
                                       ((0.25, 0.25), [True, False], [9, 10, 14])):        # equal scores: a tie is not > best + 1e-12
        t = ClusterTree.from_nodes(running_best_tree(dx, dy), 14, lib_path=lib_path)
        assert t.cut(0.6) == [13, 14]
        got, exp = compare_generate(t, asym, inp, 0.6, 2, device=device)
        first = got.trace[0]
        assert first["accepted"] == accepted and all(s > got.summary["start_score"] + 1e-12 for s in first["scores"])
        assert (first["scores"][1] > first["scores"][0]) == (accepted == [True, True]) and ((dx == dy) == (first["scores"][0] == first["scores"][1]))
        # the winner of the round is the LAST accepted alternative, and the next round starts from it
        second = Q.split_clusters(U.Tree(t.nodes, t.root), winner)
        assert len(got.trace[1]["scores"]) == len(second)
    return True


def test_running_best(emu):
    assert check_running_best(emu)


# ---- 5. reorder_clusters -------------------------------------------------------------------------------------------------------------------
def check_reorder(lib_path, device=0):
    t = ClusterTree.from_nodes(running_best_tree(0.5625, 0.0625), 14, lib_path=lib_path)
    asym = Q.contain_matrix([4, 4], {})
    # X: lengths 100, 101, 900, 903 -> median (101 + 900) / 2 = 500 (integer division); Y: 500 four times.  Equal medians: the earlier
    # old number is cluster 1, whichever node id it has.
    tie = Q.Inputs([100, 101, 900, 903, 500, 500, 500, 500], two_files(8), [1] * 8, [0] * 8)
    start = compare_qc(t, [13, 14], asym, tie, 0.6, 2, device=device)
    assert [r["median_length"] for r in start.records] == [500, 500] and [r["node"] for r in start.records] == [13, 14]
    swapped = compare_qc(t, [14, 13], asym, tie, 0.6, 2, device=device)
    assert [r["node"] for r in swapped.records] == [14, 13] and swapped.cluster_of_seq == [2] * 4 + [1] * 4
    compare_generate(t, asym, tie, 0.6, 2, device=device)
    # Y at 600: Y is cluster 1 and X cluster 2.  With X split, X2 (901) is 1, the unrelated Y becomes 2, X1 (100) is 3.
    inp = Q.Inputs([100, 101, 900, 903, 600, 600, 600, 600], two_files(8), [1] * 8, [0] * 8)
    assert compare_qc(t, [13, 14], asym, inp, 0.6, 2, device=device).cluster_of_seq == [2] * 4 + [1] * 4
    split = compare_qc(t, [9, 10, 14], asym, inp, 0.6, 2, device=device)
    assert [r["node"] for r in split.records] == [10, 14, 9] and [r["median_length"] for r in split.records] == [901, 600, 100]
    assert split.cluster_of_seq == [3, 3, 1, 1, 2, 2, 2, 2]
    got, _ = compare_generate(t, asym, inp, 0.6, 2, device=device)
    assert got.trace[0]["accepted"][0] and got.trace[0]["scores"][0].hex() == split.metrics["overall_clustering_score"].hex()
    odd = Q.Inputs([5, 1, 9, 7, 3, 8, 2, 2], two_files(8), [1] * 8, [0] * 8)      # medians of 4: (5 + 7) / 2 = 6 and (2 + 3) / 2 = 2
    assert [r["median_length"] for r in compare_qc(t, [13, 14], asym, odd, 0.6, 2, device=device).records] == [6, 2]
    return True


def test_reorder(emu):
    assert check_reorder(emu)


# ---- 6. the chain's order dependence --------------------------------------------------------------------------------------------------
def chain_case(lib_path, sizes, lengths, inside, min_assemblies=2, trusted=(), weights=None, files=None, device=0):
    nodes, groups = Q.grouped_tree(sizes)
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    n = sum(sizes)
    of = [g for g, s in enumerate(sizes) for _ in range(s)]
    inp = Q.Inputs([lengths[g] for g in of], files or two_files(n), weights or [1] * n, [1 if of[i] in trusted else 0 for i in range(n)])
    got = compare_qc(t, groups, Q.contain_matrix(sizes, inside), inp, 0.2, min_assemblies, device=device)
    by_group = {r["node"]: (r["fail"], r["container"]) for r in got.records}
    return [by_group[g] for g in groups]


def check_chain(lib_path, device=0):
    kw = dict(device=device)
    nested = {(2, 1): 4, (1, 0): 4}      # group 2 in group 1, group 1 in group 0
    # numbered 1, 2, 3: 2 fails in 1; when 3 is tested its container has failed, so it passes
    assert chain_case(lib_path, [2, 2, 2], [300, 200, 100], nested, **kw) == [(0, 0), (4, 1), (0, 0)]
    # numbered 3, 2, 1: the innermost is tested first, while its container still counts as passing
    assert chain_case(lib_path, [2, 2, 2], [100, 200, 300], nested, **kw) == [(0, 0), (4, 3), (4, 2)]
    # the container failed for too few assemblies (and is itself contained): fail 2 | 4, and what it contains passes
    assert chain_case(lib_path, [2, 1, 2], [300, 200, 100], {(2, 1): 2, (1, 0): 2}, **kw) == [(0, 0), (6, 1), (0, 0)]
    # a trusted cluster that would fail both tests passes, and goes on containing
    assert chain_case(lib_path, [2, 1, 2], [300, 200, 100], {(2, 1): 2, (1, 0): 2}, trusted=(1,), **kw) == [(0, 0), (0, 0), (4, 2)]
    # two possible containers: the smaller number is named
    assert chain_case(lib_path, [2, 2, 2], [300, 200, 100], {(2, 0): 4, (2, 1): 4}, **kw) == [(0, 0), (0, 0), (4, 1)]
    assert chain_case(lib_path, [2, 2, 2], [200, 300, 100], {(2, 0): 4, (2, 1): 4}, **kw) == [(0, 0), (0, 0), (4, 1)]
    # exactly half of the pairs: not contained; one more: contained
    assert chain_case(lib_path, [2, 2], [300, 200], {(1, 0): 2}, **kw) == [(0, 0), (0, 0)]
    assert chain_case(lib_path, [2, 2], [300, 200], {(1, 0): 3}, **kw) == [(0, 0), (4, 1)]
    assert chain_case(lib_path, [3, 2], [300, 200], {(0, 1): 3}, **kw) == [(0, 0), (0, 0)]
    assert chain_case(lib_path, [3, 2], [300, 200], {(0, 1): 4}, **kw) == [(4, 2), (0, 0)]
    # weights: the largest per file, summed.  min_assemblies 3: one sequence of weight 3; files 0 / 1 with 1 + 2; one file with 3 and 1;
    # one file with 1 and 1 (fails); weight 0 twice (fails even min_assemblies 1)
    got = chain_case(lib_path, [1, 2, 2, 2], [500, 400, 300, 200], {}, min_assemblies=3, weights=[3, 1, 2, 3, 1, 1, 1], files=[0, 0, 1, 0, 0, 1, 1], **kw)
    assert got == [(0, 0), (0, 0), (0, 0), (2, 0)]
    assert chain_case(lib_path, [2, 2], [300, 200], {}, min_assemblies=1, weights=[0, 0, 1, 0], files=[0, 1, 0, 1], **kw) == [(2, 0), (0, 0)]
    assert chain_case(lib_path, [2, 2], [300, 200], {}, min_assemblies=0, weights=[0, 0, 1, 0], files=[0, 1, 0, 1], **kw) == [(0, 0), (0, 0)]
    return True


def test_chain(emu):
    assert check_chain(emu)


# ---- 7. word boundaries ---------------------------------------------------------------------------------------------------------------
BOUNDARY_SIZES = {63: [31, 32], 64: [1, 31, 32], 65: [1, 63, 1], 129: [63, 2, 64], 130: [1, 62, 1, 2, 63, 1]}


def boundary_case(S):
    """Groups whose sequences all come from different files (32 or 64 of them), so that peeling a sequence off a group lowers the balance
    and refinement ends after a round or two; between two groups every sequence pair is asymmetric, one way or the other with a
    probability per group pair, so that the counts lie on both sides of half."""
    rng = random.Random(1300 + S)
    sizes = BOUNDARY_SIZES[S]
    F = 32 if S <= 64 else 64
    of = [g for g, s in enumerate(sizes) for _ in range(s)]
    lean = {(x, y): rng.choice((0.3, 0.5, 0.7)) for x in range(len(sizes)) for y in range(x + 1, len(sizes))}
    asym = [[0.0] * S for _ in range(S)]
    for a in range(S):
        for b in range(a + 1, S):
            if of[a] == of[b]:
                asym[a][b] = asym[b][a] = 0.0625
            else:
                asym[a][b], asym[b][a] = (0.125, 0.25) if rng.random() < lean[(of[a], of[b])] else (0.25, 0.125)
    files, at = [], 0
    for s in sizes:
        files += [F - 1] if s == 1 else list(range(s))
    assert len(set(files)) == F
    inp = Q.Inputs([rng.choice((1000, 2000, 2001, 5)) for _ in range(S)], files, [1] * S, [rng.random() < 0.05 for _ in range(S)])
    return sizes, asym, inp


def check_word_boundaries(lib_path, S, device=0):
    """clusters whose depth-first tip ranges begin and end inside, on and across the 64-bit words of the contain bits; refinement then peels
    the groups one tip at a time, which moves the ranges' ends across the boundaries"""
    sizes, asym, inp = boundary_case(S)
    nodes, groups = Q.grouped_tree(sizes, inner=2.0 ** -4)
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    assert t.cut(0.15) == sorted(groups)
    got, exp = compare_generate(t, asym, inp, 0.15, 2, device=device, key=("boundary", S))
    assert len(got.trace[0]["scores"]) == sum(1 for s in sizes if s > 1)
    model = U.Tree(t.nodes, t.root)
    for nid in (n[0] for n in nodes[len(nodes) - len(sizes) + 1:]):      # coarser clusterings: ranges that join groups
        rest = [g for g in groups if not set(model.get_tips(g)) <= set(model.get_tips(nid))]
        compare_qc(t, sorted(rest + [nid]), asym, inp, 0.15, 2, device=device)
    return True


@pytest.mark.parametrize("S", sorted(BOUNDARY_SIZES))
def test_word_boundaries(emu, S):
    assert check_word_boundaries(emu, S)


# ---- 8. more alternatives than a wavefront has lanes; the schedule ---------------------------------------------------------------------
def pairs_case(n_pairs):
    """n_pairs clusters of two sequences (one per file); splitting one leaves two single sequences that fail for too few assemblies, so
    the one round accepts nothing"""
    rng = random.Random(70 + n_pairs)
    sizes = [2] * n_pairs
    inside = {(x, y): 3 for x in range(n_pairs) for y in range(n_pairs) if x != y and rng.random() < 0.05}
    asym = Q.contain_matrix(sizes, inside)
    inp = Q.Inputs([1000 + 7 * (i // 2 % 5) for i in range(2 * n_pairs)], two_files(2 * n_pairs), [1] * (2 * n_pairs), [0] * (2 * n_pairs))
    return sizes, asym, inp


def check_many_alternatives(lib_path, n_pairs=70, device=0, default_batches=True):
    sizes, asym, inp = pairs_case(n_pairs)
    nodes, groups = Q.grouped_tree(sizes)
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    got, exp = compare_generate(t, asym, inp, 0.15, 2, device=device, key=("pairs", n_pairs), default_batches=default_batches)
    assert [len(r["scores"]) for r in got.trace] == [n_pairs] and not any(got.trace[0]["accepted"]) and got.clusters == sorted(groups)
    assert n_pairs < 70 or any(r["fail"] & 4 for r in got.records)
    return got.summary


def check_schedule(lib_path, device=0):
    """launches and read-backs depend on the number of evaluations (and pair batches) only: 3 and 70 alternatives, one round each"""
    few, many = check_many_alternatives(lib_path, 3, device), check_many_alternatives(lib_path, 70, device)
    for sm in (few, many):
        assert (sm["rounds"], sm["evaluations"], sm["pair_batches"], sm["launches"], sm["readbacks"]) == (1, 2, 2, 5, 2)
    assert few["alternatives"] == 4 and many["alternatives"] == 71
    # per evaluation one word per cluster and alternative, and one word for the device's flag
    assert few["bytes_read_back"] == 4 * ((1 + 1 * 4) + (1 + 3 * 4)) and many["bytes_read_back"] == 4 * ((1 + 1 * 71) + (1 + 70 * 71))
    assert many["node_pairs"] == 70 * 69 + (70 * 69 + 70 * (4 * 69 + 2))
    return True


def test_many_alternatives(emu):
    assert check_many_alternatives(emu)


def test_many_alternatives_batched(emu, monkeypatch):
    monkeypatch.setenv("AC_CLUSTER_QC_PAIR_BATCH", "8000")      # 70 * 70 + 70 * 282 = 24640 pair entries: four launches for the round
    sm = check_many_alternatives(emu, default_batches=False)
    assert sm["pair_batches"] == 1 + 4 and sm["launches"] == 1 + 5 + 2 and sm["readbacks"] == 2


def test_schedule(emu):
    assert check_schedule(emu)


# ---- 9. the random sweep -----------------------------------------------------------------------------------------------------------------
def check_sweep(lib_path, seed, device=0):
    asym, ids, inp, cutoffs = Q.sweep_case(seed)
    t = cluster_tree(asym, ids, normalise=True, device=device, lib_path=lib_path)
    mn = cluster_min_assemblies(inp.assembly, lib_path=lib_path)
    assert mn == Q.set_min_assemblies(inp.n_assemblies)
    counts = []
    for cutoff in cutoffs:
        got, exp = compare_generate(t, asym, inp, cutoff, mn, device=device, key=("sweep", seed, cutoff))
        counts.append(len(t.cut(cutoff)))
    assert counts[0] == 1 and counts[2] == len(ids) and 1 <= counts[1] <= len(ids)      # the first cut at the root, in the middle, at the tips
    return True


@pytest.mark.parametrize("block", range(6))
def test_sweep(emu, block):
    for seed in range(10 * block, 10 * block + 10):
        assert check_sweep(emu, seed)


def test_sweep_is_not_trivial():
    """the sweep's cases between them accept splits, fail clusters for both reasons, trust some, and renumber"""
    seen = set()
    for seed in range(0, 60, 3):
        asym, ids, inp, cutoffs = Q.sweep_case(seed)
        assert 3 <= len(ids) <= 40
        model = U.Tree(U.build_nodes(ids, U.upgma_recurrence(U.symmetrical(asym)), True))
        for cutoff in cutoffs:
            exp = cached((("sweep", seed, cutoff), "fixed"), lambda: Q.generate_clusters(model, asym, inp, cutoff, Q.set_min_assemblies(inp.n_assemblies)))
            seen |= {("fail", r["fail"]) for r in exp["records"]} | {("trusted", r["trusted"]) for r in exp["records"]}
            seen |= {("accepted", any(r["accepted"])) for r in exp["trace"]} | {("rounds>2", len(exp["trace"]) > 2)}
    assert {("fail", 0), ("fail", 2), ("fail", 4), ("trusted", 1), ("accepted", True), ("accepted", False), ("rounds>2", True)} <= seen, seen


# ---- 10. manual clusters -----------------------------------------------------------------------------------------------------------------
def check_manual(lib_path, device=0):
    sizes, asym, inp = boundary_case(65)
    inp.trusted = [1] * 65      # trust rescues nothing here
    nodes, groups = Q.grouped_tree(sizes, inner=2.0 ** -4)
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    model = U.Tree(t.nodes, t.root)
    inner = nodes[65 + 30][0]      # a node inside the middle group
    for manual in ([groups[1]], [groups[0], groups[2]], [inner], [inner, groups[2]]):
        got, exp = compare_generate(t, asym, inp, 0.15, 2, manual, device=device)
        assert got.clusters == model.cut(0.15, manual) and got.trace == [] and got.summary["launches"] == 0
        assert [r["fail"] for r in got.records] == [0 if r["node"] in manual else 1 for r in got.records] and any(r["fail"] for r in got.records)
        compare_qc(t, got.clusters, asym, inp, 0.15, 2, manual, device=device)
    for manual in ([groups[1], inner], [nodes[-1][0], groups[0]]):
        with pytest.raises(AutocyclerError, match="manual clusters cannot be nested"):
            t.generate(asym, *inp.args(), 0.15, 2, manual, device=device)
        with pytest.raises(AutocyclerError, match="manual clusters cannot be nested"):
            t.qc(groups, asym, *inp.args(), 0.15, 2, manual, device=device)
    return True


def test_manual(emu):
    assert check_manual(emu)


# ---- 11. from a graph handle -------------------------------------------------------------------------------------------------------------
def qc_assemblies(seed):
    """four assemblies of two replicons; headers that carry the trusted mark and cluster weights in mixed case"""
    r = random.Random(seed)
    common = seqgen.rand_seq(r, 150)
    reps = [seqgen.rand_seq(r, 420) + common + seqgen.rand_seq(r, 260), seqgen.rand_seq(r, 230) + common]
    marks = {(0, 0): " Autocycler_cluster_weight=3 other stuff", (1, 1): " other AUTOCYCLER_TRUSTED", (2, 0): " aUtOcYcLeR_cluster_weight=0",
             (2, 1): " autocycler_cluster_weight=x2 Autocycler_Cluster_Weight=+2", (3, 1): " xAutocycler_trustedx autocycler_cluster_weight=7"}
    seqs, fn, hd = [], [], []
    for a in range(4):
        for c, rep in enumerate(reps):
            s = list(rep)
            for _ in range(3):
                s[r.randrange(len(s))] = r.choice("ACGT")
            s = "".join(s)
            seqs.append(seqgen.rc(s) if (a + c) % 3 == 2 else s)
            fn.append(f"assembly_{a}.fasta"); hd.append(f"contig_{c} circular=true" + marks.get((a, c), ""))
    return seqs, fn, hd


def check_graph(lib_path, seed, k, device=0):
    seqs, fn, hd = qc_assemblies(seed)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    g2, fns, hds = graph_from_gfa(gfa, lib_path=lib_path)
    assert fns == fn and hds == hd
    ci = g2.cluster_inputs()
    inp = Q.inputs_from_headers([len(s) for s in seqs], fn, hd)
    assert (ci["seq_len"], ci["assembly"], ci["cluster_weight"], ci["trusted"], ci["n_assemblies"]) == (*inp.args(), 4)
    assert ci["cluster_weight"] == [3, 1, 1, 1, 0, 2, 1, 7] and ci["trusted"] == [0, 0, 0, 1, 0, 0, 0, 1]
    with pytest.raises(AutocyclerError, match="no file names"):
        g.cluster_inputs()
    t, asym = g2.cluster_tree(device=device, want_distances=True)
    mn = cluster_min_assemblies(ci["assembly"], lib_path=lib_path)
    assert mn == 2
    results = []
    for cutoff in (0.2, 2.0):
        on_handle, _ = compare_generate(t, asym, inp, cutoff, mn, device=device)
        ids = [x[0] for x in t.nodes[:len(asym)]]
        on_matrix, _ = compare_generate(cluster_tree(asym, ids, normalise=True, device=device, lib_path=lib_path), asym, inp, cutoff, mn, device=device)
        for name in ("clusters", "cluster_of_seq", "records", "metrics", "trace"):
            assert Q._key(getattr(on_handle, name)) == Q._key(getattr(on_matrix, name))
        results.append(on_handle)
    assert any(0 < d < 1 for row in asym for d in row)
    return True


@pytest.mark.parametrize("seed,k", [(4, 21)])
def test_graph_built_and_reloaded(emu, seed, k):
    assert check_graph(emu, seed, k)


# ---- 12. argument checks ---------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib_path, device=0):
    sizes = [2, 2, 2]
    nodes, groups = Q.grouped_tree(sizes)
    t = ClusterTree.from_nodes(nodes, len(nodes) - 1, lib_path=lib_path)
    asym = Q.contain_matrix(sizes, {})
    inp = Q.Inputs([300, 300, 200, 200, 100, 100], two_files(6), [1] * 6, [0] * 6)
    ok = lambda: t.generate(asym, *inp.args(), 0.15, 2, device=device).clusters == sorted(groups)
    assert ok()
    five = [row[:5] for row in asym[:5]]
    bad_calls = [
        (lambda: t.generate(five, [1] * 5, [0, 1, 0, 1, 0], [1] * 5, [0] * 5, 0.15, 2, device=device), "6 tips"),
        (lambda: t.qc(groups[:2] + [999], asym, *inp.args(), 0.15, 2, device=device), "does not contain a node with id 999"),
        (lambda: t.qc(groups[:2], asym, *inp.args(), 0.15, 2, device=device), "cover 4 of 6"),
        (lambda: t.qc(groups + [1], asym, *inp.args(), 0.15, 2, device=device), "overlap"),
        (lambda: t.qc(groups + [groups[0]], asym, *inp.args(), 0.15, 2, device=device), "overlap"),
        (lambda: t.qc([nodes[-1][0], groups[2]], asym, *inp.args(), 0.15, 2, device=device), "overlap"),
        (lambda: t.generate(asym, *inp.args(), 0.15, 2, [nodes[-1][0], groups[0]], device=device), "manual clusters cannot be nested"),
        (lambda: t.generate(asym, inp.seq_len, [0, 2, 0, 2, 0, 2], inp.cluster_weight, inp.trusted, 0.15, 2, device=device), "not dense"),
        (lambda: t.generate(asym, inp.seq_len, [1, 1, 1, 1, 1, 1], inp.cluster_weight, inp.trusted, 0.15, 2, device=device), "not dense"),
        (lambda: t.generate(asym, inp.seq_len, [0, 1, 0, 1, 0, 7], inp.cluster_weight, inp.trusted, 0.15, 2, device=device), "not dense"),
        (lambda: cluster_min_assemblies([0, 2], lib_path=lib_path), "not dense"),
        (lambda: cluster_min_assemblies([], lib_path=lib_path), "no sequences"),
    ]
    for bad, (row, col, value) in enumerate(((0, 1, float("nan")), (5, 0, float("inf")), (2, 3, -0.25))):      # as the tree entry reports them
        m = [list(r) for r in asym]
        m[row][col] = value
        bad_calls.append((lambda m=m: t.generate(m, *inp.args(), 0.15, 2, device=device), "NaN, an infinite or a negative"))
        bad_calls.append((lambda m=m: t.qc(groups, m, *inp.args(), 0.15, 2, device=device), "NaN, an infinite or a negative"))
    for call, what in bad_calls:
        with pytest.raises(AutocyclerError, match=what):
            call()
        assert ok()      # a later valid call still succeeds
    assert t.generate(asym, *inp.args(), 0.15, 0, device=device).metrics["fail_cluster_count"] == 0      # min_assemblies 0 fails nothing
    assert t.generate(asym, *inp.args(), 0.15, 3, device=device).metrics["fail_cluster_count"] == 3
    return True


def test_argument_errors(emu):
    assert check_argument_errors(emu)


# ---- 13. the host side alone; the emulation's lane orders -----------------------------------------------------------------------------
def test_host_functions_stand_alone(tmp_path):
    """cluster_qc_host.cpp (+ cluster_host.cpp) without the library, a plain loop in place of the device
    (tests/c_client/cluster_qc_host_check.cpp; the same program is what a sanitizer build runs)"""
    import subprocess
    root = emu_lib.ROOT
    csrc = root / "autocycler_amd" / "csrc"
    exe = tmp_path / "cluster_qc_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", str(csrc), str(root / "tests" / "c_client" / "cluster_qc_host_check.cpp"),
                           str(csrc / "cluster_qc_host.cpp"), str(csrc / "cluster_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "cluster_qc_host_check: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("order", [1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))
    assert check_word_boundaries(emu, 65) and check_chain(emu) and check_many_alternatives(emu, 3)
