"""Plain-Python model of `autocycler cluster` after the tree (cluster.rs:497-661, 692-723, 852-903; metrics.rs:123-187), the generators and
the shared helpers of test_cluster_qc_emu.py / test_cluster_qc_gpu.py.  Built on cluster_util.Tree and cluster_util.containment; no numpy and
nothing shared with the library.

Two forms of one model (`form`):
  "literal"  the reference as written.  Every clustering is scored from scratch: a full qc_clusters (assign + reorder, the two failure
             loops, cluster_is_contained_in_another over the matrix with the quotient contain / total > 0.5 in floating point) and
             clustering_metrics with calculate_balance / calculate_tightness.  The reference sums the balance terms in HashMap order; here
             they are summed in an order shuffled by the caller's RNG (or ascending without one).
  "fixed"    the library's arithmetic: 2 * contain > total in integers, balance over c ascending.
The two agree bit for bit wherever every balance term is exact (F a power of two).  Where several passing clusters contain a cluster the
reference names whichever its HashMap yields first; both forms name the smallest number, as the library does.

Sequences are rows of the matrix = tips of the tree in tip order; `inp` is an Inputs."""
import json
import math
import random
from pathlib import Path

import cluster_util as U

FAIL_MANUAL, FAIL_ASSEMBLIES, FAIL_CONTAINED = 1, 2, 4
REASON = {FAIL_MANUAL: "not included in manual clusters", FAIL_ASSEMBLIES: "present in too few assemblies", FAIL_CONTAINED: "contained within cluster"}
METRIC_FIELDS = ("pass_cluster_count", "fail_cluster_count", "pass_contig_count", "fail_contig_count", "pass_contig_fraction",
                 "fail_contig_fraction", "cluster_balance_score", "cluster_tightness_score", "overall_clustering_score")


def load_kats():
    return json.loads((Path(__file__).parent / "golden" / "cluster_qc_kats.json").read_text())


class Inputs:
    def __init__(self, seq_len, assembly, cluster_weight, trusted):
        self.seq_len, self.assembly, self.cluster_weight, self.trusted = list(seq_len), list(assembly), list(cluster_weight), [int(bool(t)) for t in trusted]
        self.n_assemblies = len(set(self.assembly))

    def args(self):
        return self.seq_len, self.assembly, self.cluster_weight, self.trusted


# ---- Sequence::is_trusted / cluster_weight (sequence.rs:89-102), get_assembly_count, set_min_assemblies ------------------------------
def is_trusted(header):
    return "autocycler_trusted" in header.lower()


def cluster_weight(header):
    prefix = "autocycler_cluster_weight="
    for token in header.lower().split():
        if token.startswith(prefix):
            digits = token[len(prefix):]
            if digits.startswith("+"):
                digits = digits[1:]
            if digits and all(ch in "0123456789" for ch in digits) and int(digits) < 2 ** 64:
                return int(digits)
    return 1


def number_assemblies(filenames):
    first = {}
    return [first.setdefault(f, len(first)) for f in filenames]


def inputs_from_headers(lengths, filenames, headers):
    return Inputs(lengths, number_assemblies(filenames), [cluster_weight(h) for h in headers], [is_trusted(h) for h in headers])


def set_min_assemblies(assembly_count, user=None):
    """cluster.rs:645-661 with usize_division_rounded (misc.rs:388-394)"""
    if user is not None:
        return user
    if assembly_count == 1:
        return 1
    return max(2, (assembly_count + 4 // 2) // 4)


# ---- pieces of qc_clusters ---------------------------------------------------------------------------------------------------------------
def cluster_assembly_count(cluster, c, assembly, weights):
    """cluster.rs:573-585: per file name the largest weight among the cluster's sequences, summed"""
    best = {}
    for i, ci in enumerate(cluster):
        if ci == c:
            w = weights[i]
            if assembly[i] not in best or w > best[assembly[i]]:
                best[assembly[i]] = w
    return sum(best.values())


def cluster_is_trusted(cluster, c, trusted):
    return any(ci == c and t for ci, t in zip(cluster, trusted))


def split_clusters(tree, clusters):
    """cluster.rs:311-335"""
    result = []
    for c in clusters:
        _, left, right, _ = tree.nodes[tree.find(c)]
        if left >= 0:
            new = [o for o in clusters if o != c] + [tree.nodes[left][0], tree.nodes[right][0]]
            result.append(sorted(new))
    return sorted(result)


def check_complete_coverage(tree, clusters):
    """cluster.rs:297-309 (the reference panics)"""
    all_tips = set(tree.get_tips(tree.nodes[tree.root][0]))
    covered = set()
    for c in clusters:
        for tip in tree.get_tips(c):
            if tip in covered:
                raise ValueError("overlap detected")
            covered.add(tip)
    if covered != all_tips:
        raise ValueError("incomplete coverage")


def median_usize(values):
    v = sorted(values)
    if not v:
        return 0
    return (v[len(v) // 2 - 1] + v[len(v) // 2]) // 2 if len(v) % 2 == 0 else v[len(v) // 2]


# ---- metrics.rs:123-187 --------------------------------------------------------------------------------------------------------------------
def calculate_balance(cluster_filenames, order=None):
    """cluster_filenames: {cluster: [file name per sequence]}; order: the clusters in the order their terms are summed"""
    all_files = set(f for fs in cluster_filenames.values() for f in fs)
    total_weight = 0.0
    acc = 0.0
    for c in (sorted(cluster_filenames) if order is None else order):
        fs = cluster_filenames[c]
        ones = sum(1 for f in all_files if fs.count(f) == 1)
        cluster_score = float(ones) / float(len(all_files))
        acc += cluster_score * float(len(fs))
        total_weight += float(len(fs))
    return acc / total_weight


def calculate_tightness(pass_cluster_stats):
    if not pass_cluster_stats:
        return 0.0
    sum_scores, total_weight = 0.0, 0.0
    for distance, size in pass_cluster_stats:
        sum_scores += (1.0 - math.sqrt(distance)) * float(size)
        total_weight += float(size)
    return sum_scores / total_weight


def clustering_metrics(cluster, fails, dist, assembly, rng=None):
    """cluster.rs:852-879 on the reordered cluster numbers, fails[c] = failure bits, dist[c - 1] = cluster_dist"""
    top = max(cluster)
    m = dict.fromkeys(METRIC_FIELDS, 0)
    files = {}
    for ci, f in zip(cluster, assembly):
        files.setdefault(ci, []).append(f)
        m["pass_contig_count" if not fails[ci] else "fail_contig_count"] += 1
    stats = []
    for c in range(1, top + 1):
        if not fails[c]:
            m["pass_cluster_count"] += 1
            stats.append((dist[c - 1], len(files.get(c, []))))
        else:
            m["fail_cluster_count"] += 1
    total = m["pass_contig_count"] + m["fail_contig_count"]
    m["pass_contig_fraction"] = float(m["pass_contig_count"]) / float(total) if total else 0.0
    m["fail_contig_fraction"] = float(m["fail_contig_count"]) / float(total) if total else 0.0
    order = sorted(files)
    if rng is not None:
        rng.shuffle(order)
    m["cluster_balance_score"] = calculate_balance(files, order)
    m["cluster_tightness_score"] = calculate_tightness(stats)
    m["overall_clustering_score"] = (m["cluster_balance_score"] + m["cluster_tightness_score"]) / 2.0
    return m


_counts = {}


def containment_counts(asym, cluster, top, cutoff):
    """cluster_util.containment, remembered by its arguments' values: the two forms of the model and the three shuffles ask for the same
    counts, and the pair-by-pair loop is what the model's time goes into"""
    key = (hash(tuple(map(tuple, asym))), len(asym), tuple(cluster), top, cutoff)
    if key not in _counts:
        if len(_counts) > 4096:
            _counts.clear()
        _counts[key] = U.containment(asym, cluster, top, cutoff)
    return _counts[key]


# ---- qc_clusters (cluster.rs:511-570) ---------------------------------------------------------------------------------------------------
def qc_clusters(tree, asym, inp, cluster_nodes, manual, cutoff, min_assemblies, form="fixed", rng=None):
    """-> {"cluster_of_seq", "records", "metrics"}; a full pass from scratch"""
    cluster, dist = tree.assign(cluster_nodes, inp.seq_len)
    top = max(cluster)
    tip_ids = [tree.nodes[v][0] for v in tree.tips]
    node_of = {}
    for nid in cluster_nodes:
        node_of[cluster[tip_ids.index(tree.get_tips(nid)[0])]] = nid
    fails = {c: 0 for c in range(1, top + 1)}
    container = {c: 0 for c in range(1, top + 1)}
    if manual:
        for c in fails:
            if node_of[c] not in manual:
                fails[c] |= FAIL_MANUAL
    else:
        for c in range(1, top + 1):
            if cluster_assembly_count(cluster, c, inp.assembly, inp.cluster_weight) < min_assemblies and not cluster_is_trusted(cluster, c, inp.trusted):
                fails[c] |= FAIL_ASSEMBLIES
        cc, tc = containment_counts(asym, cluster, top, cutoff)
        for c in range(1, top + 1):
            found = 0
            for p in range(1, top + 1):      # cluster_is_contained_in_another over the clusters that pass so far
                if p == c or fails[p]:
                    continue
                inside = (float(cc[(c, p)]) / float(tc[(c, p)]) > 0.5) if form == "literal" else (2 * cc[(c, p)] > tc[(c, p)])
                if inside:
                    found = p
                    break
            if found and not cluster_is_trusted(cluster, c, inp.trusted):
                fails[c] |= FAIL_CONTAINED
                container[c] = found
    records = []
    for c in range(1, top + 1):
        members = [i for i, ci in enumerate(cluster) if ci == c]
        records.append({"node": node_of[c], "container": container[c], "size": len(members),
                        "assembly_count": cluster_assembly_count(cluster, c, inp.assembly, inp.cluster_weight), "fail": fails[c],
                        "trusted": int(cluster_is_trusted(cluster, c, inp.trusted)), "median_length": median_usize([inp.seq_len[i] for i in members]),
                        "cluster_dist": dist[c - 1]})
    metrics = clustering_metrics(cluster, fails, dist, inp.assembly, rng if form == "literal" else None)
    return {"cluster_of_seq": cluster, "records": records, "metrics": metrics}


def refine_auto_clusters(tree, score, clusters):
    """cluster.rs:607-630 -> (clusters, start score, trace)"""
    best = list(clusters)
    best_score = start = score(best)
    trace = []
    improved = True
    while improved:
        improved = False
        rnd = {"scores": [], "accepted": []}
        for alt in split_clusters(tree, best):
            alt_score = score(alt)
            accept = alt_score > best_score + 1e-12
            rnd["scores"].append(alt_score); rnd["accepted"].append(accept)
            if accept:
                best, best_score, improved = alt, alt_score, True
        trace.append(rnd)
    return best, start, trace


def generate_clusters(tree, asym, inp, cutoff, min_assemblies, manual=(), form="fixed", rng=None):
    """cluster.rs:497-508 -> {"clusters", "cluster_of_seq", "records", "metrics", "trace", "start_score"}"""
    manual = list(manual)
    trace, start = [], None
    if manual:
        clusters = tree.cut(cutoff, manual)
    else:
        score = lambda nodes: qc_clusters(tree, asym, inp, nodes, [], cutoff, min_assemblies, form, rng)["metrics"]["overall_clustering_score"]
        clusters, start, trace = refine_auto_clusters(tree, score, tree.cut(cutoff))
    check_complete_coverage(tree, clusters)
    out = qc_clusters(tree, asym, inp, clusters, manual, cutoff, min_assemblies, form, rng)
    out.update(clusters=clusters, trace=trace, start_score=start)
    return out


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def _key(x):
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {k: _key(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_key(v) for v in x]
    return x


def same_result(got, exp, what=("clusters", "cluster_of_seq", "records", "metrics", "trace")):
    """a library result (ClusterQC) against a model result, floats by their bit patterns; raises with the first field that differs"""
    for name in what:
        g, e = _key(getattr(got, name)), _key(exp[name])
        assert g == e, (name, getattr(got, name), exp[name])
    if exp.get("start_score") is not None:
        assert got.summary["start_score"].hex() == exp["start_score"].hex()
    return True


# ---- generators ---------------------------------------------------------------------------------------------------------------------------
def grouped_tree(sizes, inner=2.0 ** -6, group=2.0 ** -4, step=2.0 ** -5, first_id=1):
    """A tree for ClusterTree.from_nodes whose tips 1 .. S fall into consecutive groups of the given sizes: every group is a left-leaning
    chain ((t1, t2), t3) ... (internal distances inner * 1, 2, ... capped at `group`, the group's top at `group`), the groups are joined
    the same way (distances group + step, group + 2 step, ...).  Left-first depth-first order is tip order.  -> (nodes, group node ids)"""
    S = sum(sizes)
    nodes = [(first_id + i, -1, -1, 0.0) for i in range(S)]
    next_id = first_id + S
    tops, at = [], 0
    for size in sizes:
        top = at
        for j in range(1, size):
            d = group if j == size - 1 else min(inner * j, group)
            nodes.append((next_id, top, at + j, d)); top = len(nodes) - 1; next_id += 1
        tops.append(top); at += size
    root = tops[0]
    for g in range(1, len(tops)):
        nodes.append((next_id, root, tops[g], group + step * g)); root = len(nodes) - 1; next_id += 1
    return nodes, [nodes[t][0] for t in tops]


def contain_matrix(sizes, inside, far=0.5, low=0.125, high=0.25, within=0.0625):
    """Symmetric `within` inside a group and `far` between groups, except: inside = {(x, y): count} makes the first `count` sequence pairs
    (a in group x, b in group y, row-major) asymmetric, d(a,b) = low < d(b,a) = high."""
    of = [g for g, s in enumerate(sizes) for _ in range(s)]
    n = len(of)
    m = [[0.0 if i == j else (within if of[i] == of[j] else far) for j in range(n)] for i in range(n)]
    members = [[i for i in range(n) if of[i] == g] for g in range(len(sizes))]
    for (x, y), count in inside.items():
        for a, b in [(a, b) for a in members[x] for b in members[y]][:count]:
            m[a][b], m[b][a] = low, high
    return m


def sweep_case(seed):
    """The random sweep: F in {2, 4, 8} files, a few replicons, one to three sequences per file and replicon; distances on a dyadic grid
    (0 inside a replicon, 0.5 between, plus k / 64, k = 1 .. 9) with asymmetric blocks that create containment; random lengths, trusted flags and
    weights.  -> (asym, ids, Inputs, cutoffs)"""
    rng = random.Random(9000 + seed)
    F = (2, 4, 8)[seed % 3]
    R = {2: rng.randint(2, 5), 4: rng.randint(1, 3), 8: 1}[F]
    of_rep, files = [], []
    for r in range(R):
        for f in range(F):
            for _ in range(rng.randint(1, 3)):
                of_rep.append(r); files.append(f)
    order = list(range(len(of_rep)))
    rng.shuffle(order)
    order = order[:40]
    of_rep, files = [of_rep[i] for i in order], [files[i] for i in order]
    S = len(of_rep)
    noise = U.grid_matrix(S, 8, 9100 + seed)
    block = U.block_matrix([1] * S)
    asym = [[0.0 if i == j else (block[i][j] if of_rep[i] != of_rep[j] else 0.0) + noise[i][j] / 8.0 + 0.015625 for j in range(S)] for i in range(S)]
    for _ in range(rng.randint(0, 3)):      # sequences of one replicon (or half of it) "contained" in another replicon
        x, y = rng.randrange(R), rng.randrange(R)
        for a in range(S):
            for b in range(S):
                if a != b and of_rep[a] == x and of_rep[b] == y and rng.random() < 0.8 and (x != y or a < b):
                    asym[a][b] = rng.choice((0.03125, 0.0625)); asym[b][a] = max(asym[b][a], 0.125)
    lengths = [rng.choice((1000, 1000, 2000, 2001, 2002, 5)) * (1 + of_rep[i]) for i in range(S)]
    inp = Inputs(lengths, number_assemblies(files), [rng.choice((1, 1, 1, 0, 2, 3)) for _ in range(S)], [rng.random() < 0.1 for _ in range(S)])
    return asym, list(range(1, S + 1)), inp, (3.0, 0.3, 0.0)
