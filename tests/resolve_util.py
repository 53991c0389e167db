"""Test-side model of ac_resolve_bridges / ac_path_distances, written from resolve.rs (and sequence.rs:104-109), not from the library:
plain Python over lists of signed unitig numbers.  The model does what the reference does, path by path and pair by pair (it does not merge
equal paths); the only shortcut is a memo of distances by path content.  `w` maps |unitig| -> length (a dict, or a sequence indexed by
number - 1).  Also the generators of random cases."""
import json
from collections import Counter
from pathlib import Path

import numpy as np

U32_MAX = 0xFFFFFFFF
KATS = Path(__file__).resolve().parent / "golden" / "resolve_kats.json"


def load_kats():
    k = json.loads(KATS.read_text())
    for group in ("bridge_unitig_nums", "determine_ambiguity", "best_path", "global_alignment_distance"):
        for c in k[group]:
            c["weights"] = {int(u): x for u, x in c["weights"].items()}
    return k


def weight_of(w, u):
    return w[abs(u)] if isinstance(w, dict) else w[abs(u) - 1]


def reverse_path(p):
    return [-u for u in reversed(p)]


def consensus_weight(header):
    """sequence.rs:104-109"""
    for token in header.lower().split():
        if token.startswith("autocycler_consensus_weight="):
            v = token[len("autocycler_consensus_weight="):]
            digits = v[1:] if v.startswith("+") else v
            if digits and all(c in "0123456789" for c in digits) and int(digits) < 2 ** 64:
                return int(digits)
    return 1


def global_alignment_distance(a, b, w):
    """resolve.rs:387-418, as written there"""
    n, m = len(a), len(b)
    prev = [0] * (m + 1)
    curr = [0] * (m + 1)
    for j in range(1, m + 1):
        prev[j] = prev[j - 1] + weight_of(w, b[j - 1])
    for i in range(1, n + 1):
        wi = weight_of(w, a[i - 1])
        curr[0] = prev[0] + wi
        for j in range(1, m + 1):
            wj = weight_of(w, b[j - 1])
            sub = 0 if a[i - 1] == b[j - 1] else max(wi, wj)
            curr[j] = min(prev[j - 1] + sub, prev[j] + wi, curr[j - 1] + wj)
        prev, curr = curr, prev
    return prev[m]


def global_alignment_distance_numpy(a, b, w):
    """The same row by row in int64: curr[j] = min(t[j], curr[j-1] + w_j) with t[j] = min(prev[j-1] + sub, prev[j] + w_i) unrolls to
    W[j] + min over k <= j of (t[k] - W[k]), W the prefix sums of w(b) (t[0] = curr[0])."""
    bv = np.array(b, dtype=np.int64)
    wb = np.array([weight_of(w, x) for x in b], dtype=np.int64)
    W = np.concatenate(([0], np.cumsum(wb)))
    prev = W.copy()
    for x in a:
        wi = weight_of(w, x)
        t = np.empty_like(prev)
        t[0] = prev[0] + wi
        t[1:] = np.minimum(prev[:-1] + np.where(bv == x, 0, np.maximum(wb, wi)), prev[1:] + wi)
        prev = np.minimum.accumulate(t - W) + W
    return int(prev[-1])


def find_anchors(paths, n_unitigs):
    """resolve.rs:134-163 for sequences with distinct ids: once, on either strand, in every sequence's path"""
    counts = [Counter(abs(u) for u in p) for p in paths]
    return [u for u in range(1, n_unitigs + 1) if all(c[u] == 1 for c in counts)]


def get_anchor_to_anchor_paths(sequence_paths, anchor_set):
    """resolve.rs:344-365"""
    out = []
    for path in sequence_paths:
        last = None
        for i, v in enumerate(path):
            if abs(v) in anchor_set:
                if last is not None:
                    fwd = list(path[last:i + 1])
                    rev = reverse_path(fwd)
                    out.append(fwd if fwd > rev else rev)
                last = i
    return out


def group_paths_by_start_end(paths):
    """resolve.rs:368-377 (a dict: the library's order comes from bridge_key)"""
    grouped = {}
    for p in paths:
        if p:
            grouped.setdefault((p[0], p[-1]), []).append(p)
    return grouped


def bridge_key(start, end):
    """Bridge::cmp (resolve.rs:506-514) without the best path: (start, end) is unique per bridge"""
    return (abs(start), -start, abs(end), -end)


def new_bridge(start, end, all_paths, w, dist=global_alignment_distance):
    """Bridge::new (resolve.rs:430-462) -> dict.  status 2: some pair's weights add up to 2^32 or more, or a total reaches u32::MAX (the
    reference's u32 arithmetic would overflow)."""
    trimmed = [list(p[1:-1]) for p in all_paths]
    sums = [sum(weight_of(w, u) for u in p) for p in trimmed]
    br = dict(start=start, end=end, depth=len(trimmed), status=0, best_path=None, best_total=None,
              distinct_paths=sorted(Counter(tuple(p) for p in trimmed).items()), conflicting=0, culled=0, cull_rank=0)
    br["distinct_paths"] = [(list(p), c) for p, c in br["distinct_paths"]]
    distinct_sums = sorted({tuple(p): s for p, s in zip(trimmed, sums)}.values())
    if len(distinct_sums) >= 2 and distinct_sums[-1] + distinct_sums[-2] >= 2 ** 32:
        br["status"] = 2
        return br
    memo = {}
    best_path, best_total = [], U32_MAX
    for i, pi in enumerate(trimmed):
        total = 0
        for j, pj in enumerate(trimmed):
            if i == j:
                continue
            key = (tuple(pi), tuple(pj))
            if key not in memo:
                memo[key] = dist(pi, pj, w)
            total += memo[key]
        if total >= U32_MAX:
            br["status"] = 2
        if total < best_total or (total == best_total and pi < best_path):
            best_total, best_path = total, list(pi)
    if br["status"] == 0:
        br["best_path"], br["best_total"] = best_path, best_total
    return br


def determine_ambiguity(bridges):
    """resolve.rs:193-220; sets b["_c"]"""
    sc, ec = Counter(), Counter()
    for b in bridges:
        sc[b["start"]] += 1; sc[-b["end"]] += 1
        ec[b["end"]] += 1; ec[-b["start"]] += 1
    for b in bridges:
        b["_c"] = int(sc[b["start"]] > 1 or sc[-b["end"]] > 1 or ec[b["end"]] > 1 or ec[-b["start"]] > 1)


def cull_ambiguity(bridges):
    """resolve.rs:285-313; sets culled / cull_rank on the bridges it removes"""
    left = list(bridges)
    rank = 0
    while True:
        ambi = sorted((b for b in left if b["_c"]), key=lambda b: (b["depth"], bridge_key(b["start"], b["end"])))
        if not ambi:
            return
        rank += 1
        ambi[0]["culled"], ambi[0]["cull_rank"] = 1, rank
        left.remove(ambi[0])
        determine_ambiguity(left)


def resolve_expected(paths, w, n_unitigs, consensus_weights=None, dist=global_alignment_distance):
    """resolve.rs:44-57 without the graph edits -> (anchors, bridges): what the library reports, minus the summary."""
    anchors = find_anchors(paths, n_unitigs)
    cw = consensus_weights if consensus_weights is not None else [1] * len(paths)
    sequence_paths = [p for p, c in zip(paths, cw) for _ in range(c)]
    grouped = group_paths_by_start_end(get_anchor_to_anchor_paths(sequence_paths, set(anchors)))
    bridges = [new_bridge(s, e, ps, w, dist) for (s, e), ps in grouped.items()]
    bridges.sort(key=lambda b: bridge_key(b["start"], b["end"]))
    determine_ambiguity(bridges)
    for b in bridges:
        b["conflicting"] = b["_c"]
    cull_ambiguity(bridges)
    for b in bridges:
        del b["_c"]
    return anchors, bridges


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def random_case(rng):
    """2-12 sequences over 5-40 unitigs (weights 1-5000): a common circular order, mutated per sequence (substitutions, insertions,
    deletions, inversions), started anywhere, some reverse-complemented; consensus weights 0-3.  -> (paths, weights, consensus weights)"""
    U = rng.randint(5, 40)
    w = [rng.randint(1, 5000) for _ in range(U)]
    core = [rng.choice((-1, 1)) * u for u in rng.sample(range(1, U + 1), rng.randint(3, U))]
    paths = []
    for _ in range(rng.randint(2, 12)):
        p = list(core)
        for _ in range(rng.choice((0, 0, 1, 1, 2, 4))):
            kind = rng.random()
            i = rng.randrange(len(p)) if p else 0
            if kind < 0.3 and p:
                p[i] = rng.choice((-1, 1)) * rng.randint(1, U)
            elif kind < 0.55:
                p.insert(i, rng.choice((-1, 1)) * rng.randint(1, U))
            elif kind < 0.8 and len(p) > 2:
                del p[i]
            elif p:
                j = min(len(p), i + rng.randint(1, 4))
                p[i:j] = reverse_path(p[i:j])
        if p:
            r = rng.randrange(len(p))
            p = p[r:] + p[:r]
        if rng.random() < 0.3:
            p = reverse_path(p)
        paths.append(p)
    cw = [rng.choice((0, 1, 1, 1, 1, 2, 3)) for _ in paths]
    return paths, w, cw


def random_path(rng, n, n_unitigs):
    return [rng.choice((-1, 1)) * rng.randint(1, n_unitigs) for _ in range(n)]


def edited_copy(rng, p, rate, n_unitigs):
    """a copy of p with about `rate` of its entries substituted, deleted or preceded by an insertion"""
    out = []
    for u in p:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice((-1, 1)) * rng.randint(1, n_unitigs))
        elif x < 2 * rate / 3:
            continue
        elif x < rate:
            out.extend((rng.choice((-1, 1)) * rng.randint(1, n_unitigs), u))
        else:
            out.append(u)
    return out
