"""ac_cluster_tree_* and the host functions on the tree, on the CPU emulation of the shipped kernels (kernels_cluster.inc under the lockstep
emulation of wave_rt.hpp), against the reference's known answers (golden/cluster_kats.json) and the two plain-Python models of
cluster_util.py.  Merges and nodes are compared bit for bit with `upgma_recurrence` everywhere, and with the literal `upgma_reference`
wherever that algorithm does not depend on its summation order.  The same checks run on the device in test_cluster_gpu.py."""
import random

import pytest

import cluster_util as U
import emu_lib
import parity_util
import seqgen
from autocycler_amd import AutocyclerError, ClusterTree, cluster_containment, cluster_tree, graph_from_gfa
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = U.load_kats()
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def ids_for(n, first=1):
    return list(range(first, first + n))


def run_tree(lib_path, asym, ids, normalise=False, device=0):
    t = cluster_tree(asym, ids, normalise=normalise, device=device, lib_path=lib_path)
    return t, t.merges, t.nodes


def check_exact(lib_path, asym, ids=None, normalise=False, device=0, reference=True, key=None):
    """the library's merges and nodes equal upgma_recurrence (and, with reference, upgma_reference in sorted and in shuffled order) bit
    for bit"""
    ids = ids or ids_for(len(asym))
    sym = U.symmetrical(asym)
    rec = cached(("rec", key), lambda: U.upgma_recurrence(sym)) if key else U.upgma_recurrence(sym)
    t, merges, nodes = run_tree(lib_path, asym, ids, normalise, device)
    assert U.same_bits(merges, U.id_merges(ids, rec))
    assert U.same_bits(nodes, U.build_nodes(ids, rec, normalise)) and t.root == len(nodes) - 1
    if reference:
        ref = cached(("ref", key), lambda: (U.upgma_reference(sym), U.upgma_reference(sym, random.Random(5)))) if key else \
            (U.upgma_reference(sym), U.upgma_reference(sym, random.Random(5)))
        assert U.same_bits(ref[0], rec) and U.same_bits(ref[1], rec)
    sm = t.summary
    assert sm["n_seqs"] == len(ids) and sm["launches"] == 3 + 3 * (len(ids) - 1) and sm["seconds"] >= 0
    return t


# ---- 1. the models reproduce the known answers -----------------------------------------------------------------------------------------
def test_models_reproduce_kats():
    for c in KATS["upgma"]:
        sym = U.symmetrical(c["distances"])
        for merges in (U.upgma_reference(sym), U.upgma_reference(sym, random.Random(1)), U.upgma_recurrence(sym), U.upgma_recurrence_numpy(sym)):
            raw = U.build_nodes(c["ids"], merges, False)
            assert raw[-1][3] == c["root_distance"]
            tree = U.Tree(U.build_nodes(c["ids"], merges, c["normalise"]))
            assert tree.newick(c["names"]) == c["newick"], c["test"]
            assert abs(U.build_nodes(c["ids"], merges, True)[-1][3] - c["normalised_root_distance"]) < 1e-8
    trees = {k: U.Tree([tuple(n) for n in v["nodes"]], v["root"]) for k, v in KATS["trees"].items()}
    for c in KATS["automatic_clustering"]:
        assert trees[c["tree"]].cut(c["cutoff"]) == c["expected"]
    for c in KATS["manual_clustering"]:
        assert trees[c["tree"]].cut(c["cutoff"], c["manual"]) == c["expected"]
    c = KATS["has_manual_child"]
    t = trees[c["tree"]]
    assert not t.has_manual_child(t.root, [])
    assert all(t.has_manual_child(t.root, [n]) for n in c["true_for"]) and not any(t.has_manual_child(t.root, [n]) for n in c["false_for"])
    c = KATS["check_consistency"]
    for m in c["consistent"]:
        trees[c["tree"]].check_consistency(trees[c["tree"]].root, m)
    for m in c["nested"]:
        with pytest.raises(ValueError):
            trees[c["tree"]].check_consistency(trees[c["tree"]].root, m)
    c = KATS["max_pairwise_distance"]
    for n, exp in c["expected"].items():
        assert abs(trees[c["tree"]].max_pairwise_distance(int(n)) - exp) < c["tolerance"]
    c = KATS["get_tips"]
    for n, exp in c["expected"].items():
        assert trees[c["tree"]].get_tips(int(n)) == exp
    for c in KATS["format_f64"]:
        assert U.format_f64(eval_expr(c["expr"])) == c["expected"]


def eval_expr(expr):
    parts = expr.split()
    if len(parts) == 1:
        return float(parts[0])
    a, op, b = parts
    return float(a) - float(b) if op == "-" else float(a) + float(b)


def test_model_numpy_equals_plain():
    for seed in range(30):
        n = 2 + seed
        for m in (U.uniform_matrix(n, 100 + seed), U.grid_matrix(n, 4, 200 + seed)):
            assert U.same_bits(U.upgma_recurrence_numpy(m), U.upgma_recurrence(m))


def test_models_agree_on_dyadic_inputs():
    for seed in range(20):
        n = random.Random(seed).randint(2, 40)
        for steps in (4, 65536):
            m = U.grid_matrix(n, steps, 300 + seed)
            rec = U.upgma_recurrence(m)
            assert U.same_bits(U.upgma_reference(m), rec) and U.same_bits(U.upgma_reference(m, random.Random(seed)), rec)


# ---- 2. the known answers through the library ------------------------------------------------------------------------------------------
REORDER_TREE = [(1, -1, -1, 0.0), (2, -1, -1, 0.0), (3, -1, -1, 0.0), (4, -1, -1, 0.0), (5, -1, -1, 0.0), (6, -1, -1, 0.0),
                (7, 0, 3, 0.1), (8, 1, 4, 0.1), (9, 2, 5, 0.1), (10, 6, 7, 0.3), (11, 9, 8, 0.5)]


def check_kats(lib_path, device=0):
    for c in KATS["upgma"]:
        t = cluster_tree(c["distances"], c["ids"], normalise=c["normalise"], device=device, lib_path=lib_path)
        assert t.newick(c["names"]) == c["newick"], c["test"]
        assert t.nodes[t.root][3] == c["root_distance"]
        assert len(t.merges) == len(c["ids"]) - 1
    trees = {k: ClusterTree.from_nodes([tuple(n) for n in v["nodes"]], v["root"], lib_path=lib_path) for k, v in KATS["trees"].items()}
    for c in KATS["automatic_clustering"]:
        assert trees[c["tree"]].cut(c["cutoff"]) == c["expected"]
    for c in KATS["manual_clustering"]:
        assert trees[c["tree"]].cut(c["cutoff"], c["manual"]) == c["expected"]
    c = KATS["has_manual_child"]      # (a manual cluster that is in the tree is always one of the clusters; one that is not changes nothing)
    for n in c["true_for"]:
        assert n in trees[c["tree"]].cut(2.0, [n])
    for n in c["false_for"]:
        assert trees[c["tree"]].cut(2.0, [n]) == [9]
    c = KATS["check_consistency"]
    for m in c["consistent"]:
        assert trees[c["tree"]].cut(0.5, m) == m
    for m in c["nested"]:
        with pytest.raises(AutocyclerError, match="manual clusters cannot be nested"):
            trees[c["tree"]].cut(0.5, m)
    assert trees[c["tree"]].cut(0.5) == [1, 2, 7]      # (the handle is as good as before)
    c, g = KATS["max_pairwise_distance"], KATS["get_tips"]
    t = trees[c["tree"]]
    for n, exp in c["expected"].items():
        if exp < 0:
            with pytest.raises(AutocyclerError, match="does not contain a node with id"):
                t.assign([int(n)], [1] * 5)
            continue
        of_seq, dist = t.assign([int(n)], [1] * 5)
        assert abs(dist[0] - exp) < c["tolerance"] and len(dist) == 1
        assert [i + 1 for i, x in enumerate(of_seq) if x == 1] == g["expected"][n] and set(of_seq) <= {0, 1}
    c = KATS["reorder_clusters"]
    t = ClusterTree.from_nodes(REORDER_TREE, 10, lib_path=lib_path)
    assert U.Tree(REORDER_TREE, 10).assign([7, 8, 9], [1] * 6)[0] == c["clusters"]      # (the clusters the reference's test starts from)
    assert t.assign([7, 8, 9], c["lengths"])[0] == c["expected"]
    for name, v in KATS["trees"].items():
        m = U.Tree([tuple(n) for n in v["nodes"]], v["root"])
        names = [f"s{n[0]}" for n in v["nodes"] if n[1] < 0]
        assert trees[name].newick(names) == m.newick(names) and trees[name].newick(names, file_form=True) == m.newick(names) + ";\n"
        assert trees[name].newick() == m.newick([n[1:] for n in names]) and trees[name].merges == []
    return True


def test_kats(emu):
    assert check_kats(emu)


def test_from_nodes_rejects_what_is_no_tree(emu):
    for nodes, root in (([], 0), ([(1, -1, -1, 0.0)], 1), ([(1, -1, -1, 0.0), (2, 0, -1, 0.1)], 1), ([(1, -1, -1, 0.0), (2, 0, 0, 0.1)], 1),
                        ([(1, -1, -1, 0.0), (1, -1, -1, 0.0), (3, 0, 1, 0.1)], 2), ([(1, -1, -1, 0.0), (2, -1, -1, 0.0), (3, 0, 1, 0.1)], 0),
                        ([(1, -1, -1, 0.0), (2, 0, 2, 0.1), (3, 0, 1, 0.1)], 2), ([(1, -1, -1, 0.0), (2, 0, 5, 0.1)], 1)):
        with pytest.raises(AutocyclerError):
            ClusterTree.from_nodes(nodes, root, lib_path=emu)
    assert ClusterTree.from_nodes([(7, -1, -1, 0.0)], 0, lib_path=emu).cut(0.2) == [7]


# ---- 3. the smallest shapes --------------------------------------------------------------------------------------------------------------
def check_smallest(lib_path, device=0):
    t = check_exact(lib_path, [[0.0]], [9], device=device)
    assert t.nodes == [(9, -1, -1, 0.0)] and t.merges == [] and t.root == 0 and t.cut(0.2) == [9] and t.newick() == "9"
    t = check_exact(lib_path, [[0.0, 0.3], [0.3, 0.0]], [3, 8], device=device)
    assert t.merges == [(3, 8, 0.3)] and t.nodes[2] == (9, 0, 1, 0.15)
    check_exact(lib_path, [[0.0, 0.5, 0.25], [0.5, 0.0, 0.75], [0.25, 0.75, 0.0]], [1, 2, 40], device=device)
    return True


def test_smallest(emu):
    assert check_smallest(emu)


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------------------
def check_ties_small(lib_path, device=0):
    t = check_exact(lib_path, [[0.0] * 7 for _ in range(7)], device=device)
    assert t.merges == [(1, b, 0.0) for b in range(2, 8)]
    t = check_exact(lib_path, U.block_matrix([3, 1, 4, 2]), device=device)
    assert [m[2] for m in t.merges] == [0.0] * 6 + [0.5] * 3
    return True


TIE_SIZES = (5, 33, 64, 65, 130)


def check_quarter_grid(lib_path, n, device=0):
    check_exact(lib_path, U.grid_matrix(n, 4, 400 + n), device=device, key=("quarter", n))
    return True


def test_ties_small(emu):
    assert check_ties_small(emu)


@pytest.mark.parametrize("n", TIE_SIZES)
def test_quarter_grid(emu, n):
    assert check_quarter_grid(emu, n)


# ---- 5. exact sums -----------------------------------------------------------------------------------------------------------------------
EXACT_SIZES = (63, 64, 65, 257)


def check_exact_sums(lib_path, n, device=0):
    check_exact(lib_path, U.grid_matrix(n, 65536, 500 + n), ids_for(n, 3), device=device, key=("dyadic", n))
    return True


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_sums(emu, n):
    assert check_exact_sums(emu, n)


# ---- 6. shapes that drive each branch of the refresh ------------------------------------------------------------------------------------
def check_refresh_branches(lib_path, device=0):
    n = 130
    t = check_exact(lib_path, U.formula_matrix(n, lambda i, j: max(i, j) * 2.0 ** -10), device=device, key="swallow")
    assert t.summary["rescans"] >= n - 2
    assert [m[:2] for m in t.merges] == [(1, b) for b in range(2, n + 1)]
    t = check_exact(lib_path, U.formula_matrix(n, lambda i, j: (n + 1 - min(i, j)) * 2.0 ** -10), device=device, key="high")
    assert t.summary["compares"] > 0
    return True


def test_refresh_branches(emu):
    assert check_refresh_branches(emu)


# ---- 7. generic inputs -------------------------------------------------------------------------------------------------------------------
def generic_case(seed):
    n = 300 if seed == "large" else random.Random(7000 + seed).randint(2, 40)
    return U.uniform_matrix(n, 7100 + (999 if seed == "large" else seed))


def check_generic(lib_path, seed, device=0):
    """bit equal to upgma_recurrence; the merge pairs of upgma_reference, its distances within 2 n 2^-53 relative (n = the member pairs of
    the merge: the bound on two orderings of an n-term sum of non-negative terms, each within n 2^-53 of the true sum).  That the pairs
    must agree is checked on the reference model alone first: at every merge the runner-up lies beyond the minimum by more than the bound
    of the LARGEST sum there can be (S^2 terms), on either side."""
    m = generic_case(seed)
    n = len(m)
    ref, margins = cached(("generic-ref", seed), lambda: U.upgma_reference(m, want_runner_up=True))
    wide = 2.0 * n * n * U.EPS
    for (a, b, d), (runner, pairs) in zip(ref, margins):
        assert runner * (1.0 - wide) > d * (1.0 + wide), (seed, a, b)
    t = check_exact(lib_path, m, device=device, reference=False, key=("generic", seed))
    got = t.merges
    assert [(a, b) for a, b, _ in got] == [(a + 1, b + 1) for a, b, _ in ref]
    for (_, _, d), (_, _, e), (_, pairs) in zip(got, ref, margins):
        assert abs(d - e) <= 2.0 * pairs * U.EPS * e
    return True


@pytest.mark.parametrize("block", range(6))
def test_generic_small(emu, block):
    for seed in range(10 * block, 10 * block + 10):
        assert check_generic(emu, seed)


def test_generic_300(emu):
    assert check_generic(emu, "large")


# ---- 8. asymmetric input -----------------------------------------------------------------------------------------------------------------
def check_asymmetric(lib_path, device=0):
    rng = random.Random(81)
    n = 37
    asym = [[0.0 if i == j else rng.randint(0, 1024) / 1024 for j in range(n)] for i in range(n)]
    assert any(asym[i][j] != asym[j][i] for i in range(n) for j in range(n))
    t = check_exact(lib_path, asym, ids_for(n, 100), normalise=True, device=device)
    assert U.same_bits(t.nodes, U.build_nodes(ids_for(n, 100), U.upgma_recurrence(U.symmetrical(asym)), True))
    return True


def test_asymmetric(emu):
    assert check_asymmetric(emu)


# ---- 9. on a graph handle ----------------------------------------------------------------------------------------------------------------
def cluster_assemblies(seed, k):
    """three assemblies of two replicons each (one shared stretch between the replicons), with a few substitutions per copy"""
    r = random.Random(seed)
    common = seqgen.rand_seq(r, 200)
    reps = [seqgen.rand_seq(r, 500) + common + seqgen.rand_seq(r, 300), seqgen.rand_seq(r, 250) + common]
    seqs, fn, hd = [], [], []
    for a in range(3):
        for c, rep in enumerate(reps):
            s = list(rep)
            for _ in range(3):
                s[r.randrange(len(s))] = r.choice("ACGT")
            s = "".join(s)
            seqs.append(seqgen.rc(s) if (a + c) % 3 == 2 else s)
            fn.append(f"assembly_{a}.fasta"); hd.append(f"contig_{c} circular=true")
    return seqs, fn, hd


def check_graph(lib_path, seed, k, device=0):
    seqs, fn, hd = cluster_assemblies(seed, k)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    g2, fns, hds = graph_from_gfa(gfa, lib_path=lib_path)      # what `autocycler cluster` itself starts from
    results = []
    for graph in (g, g2):
        asym = graph.pairwise_distances(device=device)
        t, got = graph.cluster_tree(device=device, want_distances=True)
        assert U.same_bits(got, asym)
        n = len(asym)
        ids = [x[0] for x in t.nodes[:n]]
        rec = U.upgma_recurrence(U.symmetrical(asym))
        assert U.same_bits(t.merges, U.id_merges(ids, rec)) and U.same_bits(t.nodes, U.build_nodes(ids, rec, True))
        raw = graph.cluster_tree(normalise=False, device=device)
        assert U.same_bits(raw.nodes, U.build_nodes(ids, rec, False)) and raw.summary["launches"] == 6 + 3 * (n - 1)
        assert any(0 < d < 1 for row in asym for d in row) and len(set(m[2] for m in rec)) > 2      # (or the case tests nothing)
        results.append((t.merges, t.nodes, ids))
    assert results[0] == results[1]
    assert fns == fn and hds == hd
    names = [U.default_name(i, f, h, len(s)) for i, f, h, s in zip(results[1][2], fn, hd, seqs)]
    assert g2.default_tip_names() == names and all("__contig_" in x and " " not in x for x in names)
    t2 = g2.cluster_tree(device=device)
    model = U.Tree(t2.nodes)
    assert t2.newick() == model.newick(names) and t2.newick(file_form=True) == model.newick_file(names)
    assert g.cluster_tree(device=device).newick() == model.newick([U.default_name(i, "", "", len(s)) for i, s in zip(results[0][2], seqs)])
    return True


@pytest.mark.parametrize("seed,k", [(4, 21)])
def test_graph_built_and_reloaded(emu, seed, k):
    assert check_graph(emu, seed, k)


# ---- 10. the host functions ------------------------------------------------------------------------------------------------------------
def check_host_functions(lib_path, device=0):
    rng = random.Random(10)
    for seed, n, normalise in ((1, 12, False), (2, 29, True), (3, 40, True)):
        m = U.grid_matrix(n, 16, 600 + seed) if seed != 3 else U.uniform_matrix(n, 600)
        ids = sorted(rng.sample(range(1, 200), n))
        t = cluster_tree(m, ids, normalise=normalise, device=device, lib_path=lib_path)
        nodes = t.nodes
        model = U.Tree(nodes)
        # cutoffs ON node distances (distance <= cutoff / 2 is inclusive), next to them, and beyond both ends
        dists = sorted(set(x[3] for x in nodes))
        cutoffs = [-1.0, 0.0, 3.0] + [2.0 * d for d in dists] + [2.0 * d * (1 - 2.0 ** -52) for d in dists[1:]]
        seen = set()
        for c in cutoffs:
            got = t.cut(c)
            assert got == model.cut(c)
            seen.add(len(got))
        assert 0 in seen and 1 in seen and len(seen) > 3      # (below every tip; the root; several levels between)
        internal = [x[0] for x in nodes if x[1] >= 0]
        for trial in range(30):
            manual = rng.sample(internal + ids, rng.randint(1, 3))
            c = rng.choice(cutoffs)
            try:
                exp = model.cut(c, manual)
            except ValueError:
                with pytest.raises(AutocyclerError, match="nested"):
                    t.cut(c, manual)
                continue
            assert t.cut(c, manual) == exp
        # assign: equal medians, even counts, lengths in any order; clusters from a cut, from a partial list, and overlapping ones
        for trial in range(20):
            lengths = [rng.choice((1000, 1000, 2000, 2001, 2002, 5)) for _ in range(n)]
            which = t.cut(rng.choice(cutoffs)) if trial % 2 == 0 else rng.sample(internal + ids, rng.randint(1, 4))
            assert t.assign(which, lengths) == model.assign(which, lengths)
        # containment on random labels
        asym = [[0.0 if i == j else rng.randint(0, 8) / 8 for j in range(n)] for i in range(n)]
        for n_clusters in (1, 2, 5):
            labels = [rng.randint(0, n_clusters) for _ in range(n)]
            for cutoff in (0.2, 0.5, 1.5):
                assert cluster_containment(asym, labels, n_clusters, cutoff, lib_path=lib_path) == U.containment(asym, labels, n_clusters, cutoff)
        with pytest.raises(AutocyclerError, match="carries cluster"):
            cluster_containment(asym, [3] * n, 2, 0.2, lib_path=lib_path)
        names = [f"{i}__f__c__{i}_bp" for i in ids]
        assert t.newick(names) == model.newick(names) and t.newick(names, file_form=True) == model.newick_file(names)
    # the file form with a root below, at and above 0.5
    for root_distance, line in ((0.2, "((a:0.2,b:0.2)3:0.3);\n"), (0.5, "(a:0.5,b:0.5)3;\n"), (8.5, "(a:8.5,b:8.5)3;\n"), (0.05, "((a:0.05,b:0.05)3:0.45);\n")):
        t = ClusterTree.from_nodes([(1, -1, -1, 0.0), (2, -1, -1, 0.0), (3, 0, 1, root_distance)], 2, lib_path=lib_path)
        assert t.newick(["a", "b"], file_form=True) == line == U.Tree(t.nodes).newick_file(["a", "b"])
    # the float list, as branch lengths
    for c in KATS["format_f64"]:
        x = eval_expr(c["expr"])
        t = ClusterTree.from_nodes([(1, -1, -1, 0.0), (2, -1, -1, 0.0), (3, 0, 1, x)], 2, lib_path=lib_path)
        assert t.newick(["a", "b"]) == f"(a:{c['expected']},b:{c['expected']})3" and U.format_f64(x) == c["expected"]
    for x in (1.0 / 3.0, 123456789.125, 5e-324, 1.7976931348623157e308, 2.0 ** -30, 0.1 * 3):
        t = ClusterTree.from_nodes([(1, -1, -1, 0.0), (2, -1, -1, 0.0), (3, 0, 1, x)], 2, lib_path=lib_path)
        assert t.newick(["a", "b"]) == f"(a:{U.format_f64(x)},b:{U.format_f64(x)})3"
    return True


def test_host_functions(emu):
    assert check_host_functions(emu)


def test_host_functions_stand_alone(tmp_path):
    """cluster_host.cpp without the library, a CPU stub for the merge loop (tests/c_client/cluster_host_check.cpp; the same program is what a
    sanitizer build runs)"""
    import subprocess
    root = emu_lib.ROOT
    exe = tmp_path / "cluster_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", str(root / "autocycler_amd" / "csrc"),
                           str(root / "tests" / "c_client" / "cluster_host_check.cpp"), str(root / "autocycler_amd" / "csrc" / "cluster_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "cluster_host_check: OK" in out.stdout, out.stdout[-2000:]


# ---- 11. argument checks ---------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib_path, device=0):
    ok = [[0.0, 0.5], [0.5, 0.0]]
    kw = dict(device=device, lib_path=lib_path)
    bad_calls = [
        (([], []), "no sequences"),
        ((ok, [2, 1]), "ascend"),
        ((ok, [4, 4]), "ascend"),
        ((ok, [65000, 65535]), "65535"),
        (([[0.0, float("nan")], [0.5, 0.0]], [1, 2]), "NaN"),
        (([[0.0, 0.5], [float("inf"), 0.0]], [1, 2]), "infinite"),
        (([[0.0, -0.25], [0.5, 0.0]], [1, 2]), "negative"),
        (([[float("nan")]], [1]), "NaN"),
    ]
    for (m, ids), what in bad_calls:
        with pytest.raises(AutocyclerError, match=what):
            cluster_tree(m, ids, **kw)
        assert cluster_tree(ok, [1, 2], **kw).merges == [(1, 2, 0.5)]      # a later valid call still succeeds
    assert cluster_tree([[0.0]], [65535], **kw).nodes == [(65535, -1, -1, 0.0)]      # max id + n - 1 == 65535 exactly
    assert cluster_tree(ok, [65533, 65534], **kw).nodes[2][0] == 65535
    # above ac_cluster_max_seqs: refused before anything is read (the matrix is never touched)
    limit = _capi.max_cluster_seqs(lib_path)
    assert limit >= 4096
    lib = _capi.load_library(lib_path)
    import ctypes as C
    n = limit + 1
    h = C.c_void_p()
    one = (C.c_double * 1)()
    assert lib.ac_cluster_tree_from_distances(one, (C.c_uint16 * n)(*range(1, n + 1)), n, 0, device, C.byref(h)) == 1 and not h.value
    assert b"ac_cluster_max_seqs" in lib.ac_last_error()
    assert cluster_tree(ok, [1, 2], **kw).merges == [(1, 2, 0.5)]
    return True


def test_argument_errors(emu):
    assert check_argument_errors(emu)


# ---- 13. the emulation's lane orders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))
    assert check_quarter_grid(emu, 65) and check_ties_small(emu)
