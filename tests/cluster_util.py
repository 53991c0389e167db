"""Plain-Python models of `autocycler cluster`'s tree (cluster.rs:177-546, 692-723), the generators and the shared checks of
test_cluster_emu.py / test_cluster_gpu.py.

Two models of upgma.  `upgma_reference` is the reference's algorithm as written: after every merge the distance from the new cluster to
every other one is summed again over the ORIGINAL distances of all member pairs and divided by their count.  The reference walks the members
in HashSet order, which changes from process to process; here they are walked in sorted order, or in an order shuffled by the caller's RNG.
`upgma_recurrence` is the arithmetic the library fixes: a running sum per cluster pair, sum(a, X) = sum(a, X) + sum(b, X), compared as
sum / float(size(a u b) * size(X)).  Wherever every sum is exact (distances on a dyadic grid, small S) the two agree bit for bit whatever
the order; on generic inputs they agree in topology and differ in the last bits of the distances.

Matrices are lists of lists indexed by ROW (sequences in ascending id order); merges are (row a, row b, distance) inside the models and
(id a, id b, distance) where they meet the library.  No numpy, except `upgma_recurrence_numpy`."""
import json
import random
from decimal import Decimal
from pathlib import Path

INF = float("inf")
EPS = 2.0 ** -53


def load_kats():
    return json.loads((Path(__file__).parent / "golden" / "cluster_kats.json").read_text())


def symmetrical(asym):
    """make_symmetrical_distances (cluster.rs:177-192)"""
    n = len(asym)
    sym = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            sym[i][j] = sym[j][i] = max(asym[i][j], asym[j][i])
    return sym


def _closest_pair(cd, act, want_runner_up=False):
    """get_closest_pair (cluster.rs:461-480) over the live rows `act` (ascending): all pairs a < b in order, the first strictly smaller
    distance is kept.  With want_runner_up also the smallest distance among all the OTHER pairs (inf when there is none)."""
    best, pair = INF, (0, 0)
    others = []
    for i, a in enumerate(act[:-1]):
        row = cd[a]
        rest = act[i + 1:]
        vals = [row[b] for b in rest]
        m = min(vals)
        if want_runner_up:
            others.append((m, a, vals))
        if m < best:
            best, pair = m, (a, rest[vals.index(m)])
    if not want_runner_up:
        return pair[0], pair[1], best
    runner = INF
    for m, a, vals in others:
        if a != pair[0]:
            runner = min(runner, m)
        else:
            v = list(vals)
            v.remove(best)
            runner = min([runner] + v)
    return pair[0], pair[1], best, runner


def upgma_reference(sym, rng=None, want_runner_up=False):
    """upgma (cluster.rs:395-458) -> merges [(row a, row b, distance)]; with want_runner_up also, per merge, (the smallest distance among
    the pairs that were not chosen, the number of member pairs behind the chosen distance)"""
    n = len(sym)
    members = {i: [i] for i in range(n)}
    cd = [list(r) for r in sym]
    merges, margins = [], []
    while len(members) > 1:
        act = sorted(members)
        if want_runner_up:
            a, b, d, runner = _closest_pair(cd, act, True)
            margins.append((runner, len(members[a]) * len(members[b])))
        else:
            a, b, d = _closest_pair(cd, act)
        new = members[a] + members.pop(b)
        members[a] = new
        merges.append((a, b, d))
        for other in members:
            if other == a:
                continue
            m1, m2 = list(new), list(members[other])
            if rng is not None:
                rng.shuffle(m1); rng.shuffle(m2)
            else:
                m1.sort(); m2.sort()
            avg, count = 0.0, 0
            for i1 in m1:
                r = sym[i1]
                for i2 in m2:
                    avg += r[i2]
                    count += 1
            avg /= float(count)
            cd[a][other] = cd[other][a] = avg
    return (merges, margins) if want_runner_up else merges


def upgma_recurrence(sym):
    """the library's arithmetic -> merges [(row a, row b, distance)]"""
    n = len(sym)
    sums = [list(r) for r in sym]
    avg = [list(r) for r in sym]
    size = [1] * n
    act = list(range(n))
    merges = []
    while len(act) > 1:
        a, b, d = _closest_pair(avg, act)
        merges.append((a, b, d))
        act.remove(b)
        size[a] += size[b]
        for x in act:
            if x == a:
                continue
            s = sums[a][x] + sums[b][x]
            sums[a][x] = sums[x][a] = s
            avg[a][x] = avg[x][a] = s / float(size[a] * size[x])
    return merges


def upgma_recurrence_numpy(sym):
    """upgma_recurrence with the closest pair found by one argmin over a masked copy (row-major: the first minimum is the lexicographically
    smallest pair)"""
    import numpy as np
    sums = np.array(sym, dtype=np.float64)
    n = sums.shape[0]
    work = sums.copy()                      # avg on the live pairs a < b, inf elsewhere
    work[np.tril_indices(n)] = np.inf
    size = np.ones(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    merges = []
    for _ in range(n - 1):
        at = int(np.argmin(work))
        a, b = divmod(at, n)
        merges.append((a, b, float(work[a, b])))
        live[b] = False
        size[a] += size[b]
        s = sums[a, :] + sums[b, :]
        sums[a, :] = s
        sums[:, a] = s
        v = s / (size[a] * size).astype(np.float64)
        work[b, :] = np.inf
        work[:, b] = np.inf
        lo = live.copy(); lo[a:] = False    # rows below a: column a
        hi = live.copy(); hi[:a + 1] = False
        work[lo, a] = v[lo]
        work[a, hi] = v[hi]
    return merges


# ---- the tree ------------------------------------------------------------------------------------------------------------------------
def build_nodes(ids, merges, normalise):
    """upgma's tree in the library's layout: [(id, left, right, distance)], tips first; then normalise_tree (cluster.rs:483-494)"""
    nodes = [(i, -1, -1, 0.0) for i in ids]
    node_of = list(range(len(ids)))
    internal = max(ids)
    for a, b, d in merges:
        internal += 1
        nodes.append((internal, node_of[a], node_of[b], d / 2.0))
        node_of[a] = len(nodes) - 1
    root = nodes[-1]
    if normalise and root[3] > 0.5:
        factor = 0.5 / root[3]
        nodes = [(i, l, r, d * factor) for i, l, r, d in nodes]
    return nodes


def id_merges(ids, merges):
    return [(ids[a], ids[b], d) for a, b, d in merges]


def format_f64(x):
    """an f64 as Rust's `{}` prints it: the shortest digits that round-trip (Python's repr finds the same digits), never an exponent"""
    s = format(Decimal(repr(float(x))), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def default_name(seq_id, filename, header, length):
    """Sequence::string_for_newick (sequence.rs:77-87)"""
    return f"{seq_id}__{filename}__{header.split(' ')[0]}__{length}_bp"


class Tree:
    """TreeNode's methods (cluster.rs:203-348, 363-392) on the library's node layout"""

    def __init__(self, nodes, root=None):
        self.nodes = nodes
        self.root = len(nodes) - 1 if root is None else root
        self.tips = [i for i, n in enumerate(nodes) if n[1] < 0]

    def has_manual_child(self, v, manual):
        nid, l, r, _ = self.nodes[v]
        if nid in manual:
            return True
        return l >= 0 and (self.has_manual_child(l, manual) or self.has_manual_child(r, manual))

    def check_consistency(self, v, manual):
        nid, l, r, _ = self.nodes[v]
        if l >= 0:
            if nid in manual and (self.has_manual_child(l, manual) or self.has_manual_child(r, manual)):
                raise ValueError("manual clusters cannot be nested")
            self.check_consistency(l, manual); self.check_consistency(r, manual)

    def _collect(self, v, cutoff, manual, out):
        nid, l, r, d = self.nodes[v]
        if nid in manual or (d <= cutoff and not self.has_manual_child(v, manual)):
            out.append(nid)
        elif l >= 0:
            self._collect(l, cutoff, manual, out); self._collect(r, cutoff, manual, out)

    def cut(self, cutoff, manual=()):
        out = []
        if manual:
            self.check_consistency(self.root, manual)
        self._collect(self.root, cutoff / 2.0, manual, out)
        return sorted(out)

    def find(self, nid):
        for v, n in enumerate(self.nodes):
            if n[0] == nid:
                return v
        return None

    def get_tips(self, nid):
        v = self.find(nid)
        if v is None:
            return []
        out, stack = [], [v]
        while stack:
            x = stack.pop()
            _, l, r, _ = self.nodes[x]
            if l < 0:
                out.append(self.nodes[x][0])
            else:
                stack.append(r); stack.append(l)
        return out

    def max_pairwise_distance(self, nid):
        v = self.find(nid)
        return -1.0 if v is None else self.nodes[v][3] * 2.0

    def assign(self, cluster_nodes, lengths):
        """the first half of qc_clusters (cluster.rs:522-546) with reorder_clusters (:882-903) -> (cluster per tip, cluster_dist)"""
        tip_ids = [self.nodes[v][0] for v in self.tips]
        cluster = [0] * len(tip_ids)
        dist_old = []
        for k, nid in enumerate(cluster_nodes):
            if self.find(nid) is None:
                raise ValueError(f"clustering tree does not contain a node with id {nid}")
            under = set(self.get_tips(nid))
            for i, t in enumerate(tip_ids):
                if t in under:
                    cluster[i] = k + 1
            dist_old.append(self.max_pairwise_distance(nid))
        top = max(cluster)
        med = {}
        for c in range(1, top + 1):
            ls = sorted(lengths[i] for i in range(len(cluster)) if cluster[i] == c)
            med[c] = 0 if not ls else ((ls[len(ls) // 2 - 1] + ls[len(ls) // 2]) // 2 if len(ls) % 2 == 0 else ls[len(ls) // 2])
        order = sorted(med, key=lambda c: (-med[c], c))
        old_to_new = {c: i + 1 for i, c in enumerate(order)}
        dist = [0.0] * top
        for c in range(1, top + 1):
            dist[old_to_new[c] - 1] = dist_old[c - 1]
        return [old_to_new[c] if c else 0 for c in cluster], dist

    def newick(self, names, v=None):
        v = self.root if v is None else v
        nid, l, r, d = self.nodes[v]
        if l < 0:
            return names[self.tips.index(v)]
        return f"({self.newick(names, l)}:{format_f64(d - self.nodes[l][3])},{self.newick(names, r)}:{format_f64(d - self.nodes[r][3])}){nid}"

    def newick_file(self, names):
        d = self.nodes[self.root][3]
        if d < 0.5:
            return f"({self.newick(names)}:{format_f64(0.5 - d)});\n"
        return f"{self.newick(names)};\n"


def containment(asym, cluster, n_clusters, cutoff):
    """the counts of cluster_is_contained_in_another (cluster.rs:705-717) for every ordered pair of different clusters"""
    cc = {(x, y): 0 for x in range(1, n_clusters + 1) for y in range(1, n_clusters + 1) if x != y}
    tc = dict(cc)
    for a, ca in enumerate(cluster):
        for b, cb in enumerate(cluster):
            if ca and cb and ca != cb:
                tc[(ca, cb)] += 1
                if asym[a][b] < asym[b][a] and asym[a][b] < cutoff:
                    cc[(ca, cb)] += 1
    return cc, tc


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def grid_matrix(n, steps, seed):
    """symmetric, entries k / steps with k uniform in 0 .. steps, zero diagonal"""
    rng = random.Random(seed)
    m = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            m[i][j] = m[j][i] = rng.randint(0, steps) / steps
    return m


def uniform_matrix(n, seed):
    rng = random.Random(seed)
    m = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            m[i][j] = m[j][i] = rng.random()
    return m


def formula_matrix(n, f):
    """d(i, j) = f(i, j) for the 1-based i != j, zero diagonal"""
    return [[0.0 if i == j else f(i + 1, j + 1) for j in range(n)] for i in range(n)]


def block_matrix(sizes):
    """blocks of identical sequences: 0 inside a block, 0.5 between blocks"""
    of = [b for b, s in enumerate(sizes) for _ in range(s)]
    return [[0.0 if of[i] == of[j] else 0.5 for j in range(len(of))] for i in range(len(of))]


def bits(x):
    return float(x).hex()


def same_bits(got, exp):
    """equality of two lists of tuples, floats compared by their bit patterns"""
    key = lambda rows: [tuple(bits(v) if isinstance(v, float) else v for v in r) for r in rows]
    return key(got) == key(exp)
