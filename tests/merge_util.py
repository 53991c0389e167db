"""The model the merge-plan tests hold the library to: merge_linear_paths with get_fixed_unitig_starts_and_ends, fix_circular_loops,
get_exclusive_inputs / outputs, merge_path, merge_unitig_seqs, get_merge_path_depth (graph_simplification.rs:190-526) and
delete_dangling_links (unitig_graph.rs:547-564), restated line by line in plain Python over components_util's graph class extended with
sequences, depths, types and position counts — the sequential loop with its already_used set, the list pushes of merge_path and the
dangling deletion included.  Plus the generators of the random sweep and the boundary shapes, whose expected values are built by
construction.  It shares no code with kernels_merge.inc or merge_host.cpp."""
import json

import numpy as np

import components_util as U

GOLDEN = U.GOLDEN
FORWARD, REVERSE = True, False
OTHER, ANCHOR, CONSENTIG, BRIDGE = 0, 1, 2, 3
FIXED_START, FIXED_END = 1, 2
NOT_MERGED = 0xFFFFFFFF
COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("G"): ord("C"), ord("C"): ord("G"), ord("."): ord(".")}


def load_kats():
    return json.loads((GOLDEN / "merge_kats.json").read_text())


def reverse_complement(seq):
    """misc.rs:358-376"""
    return bytes(COMPLEMENT.get(b, ord("N")) for b in reversed(seq))


def gfa_graph(name):
    """a golden GFA whose segment numbers may have gaps: (n_unitigs = the highest number, links, lens, alive or None, seqs, depths,
    path_ends [(first, last)], fwd position counts, rev position counts)"""
    seqs, depths, links, paths = {}, {}, [], []
    for line in (GOLDEN / name).read_text().splitlines():
        p = line.split("\t")
        if p[0] == "S":
            seqs[int(p[1])] = p[2].encode()
            depths[int(p[1])] = float([t for t in p[3:] if t.startswith("DP:f:")][0][5:])
        elif p[0] == "L":
            links.append((int(p[1]) * (1 if p[2] == "+" else -1), int(p[3]) * (1 if p[4] == "+" else -1)))
        elif p[0] == "P":
            paths.append([int(e[:-1]) * (1 if e[-1] == "+" else -1) for e in p[2].split(",")])
    n = max(seqs)
    alive = [int(u in seqs) for u in range(1, n + 1)]
    fwd, rev = [0] * n, [0] * n
    for path in paths:      # create_sequence_and_positions (unitig_graph.rs:151-174): one position per path entry, on the entry's strand
        for e in path:
            (fwd if e > 0 else rev)[abs(e) - 1] += 1
    return dict(n=n, links=links, lens=[len(seqs.get(u, b"")) for u in range(1, n + 1)], alive=None if all(alive) else alive,
                seqs=[seqs.get(u, b"") for u in range(1, n + 1)], depths=[depths.get(u, 0.0) for u in range(1, n + 1)],
                path_ends=[(p[0], p[-1]) for p in paths if p], fwd=fwd, rev=rev)


# ---- the reference, literally ---------------------------------------------------------------------------------------------------------------
class MergeGraph(U.UnitigGraph):
    """components_util.UnitigGraph with what merge_path reads: per unitig the forward sequence, depth, type and the number of positions per
    strand.  List entries are (number, strand); `objects` finds a unitig by number whether it is still in the graph or not, as the
    reference's weak references do."""

    def __init__(self, n_unitigs, links, alive=None, seqs=None, lens=None, depths=None, types=None, fwd=None, rev=None):
        super().__init__(n_unitigs, links, alive)
        self.n_unitigs = n_unitigs
        for u in self.unitigs:
            i = u.number - 1
            u.forward_seq = bytes(seqs[i]) if seqs is not None else b"N" * int(lens[i])
            u.depth = float(depths[i]) if depths is not None else 0.0
            u.unitig_type = int(types[i]) if types is not None else OTHER
            u.forward_positions = int(fwd[i]) if fwd is not None else 0      # (only their number is read)
            u.reverse_positions = int(rev[i]) if rev is not None else 0
        self.objects = dict(self.unitig_index)

    def link_exists(self, a_num, a_strand, b_num, b_strand):
        a = self.unitig_index.get(a_num)
        return a is not None and any(nx == (b_num, b_strand) for nx in (a.forward_next if a_strand else a.reverse_next))


def strand_seq(unitig, strand):
    return unitig.forward_seq if strand else reverse_complement(unitig.forward_seq)


# :190-230
def get_fixed_unitig_starts_and_ends(graph, path_ends):
    fixed_starts, fixed_ends = set(), set()
    for (first, last) in path_ends:
        first_unitig, first_strand = abs(first), first > 0
        (fixed_starts if first_strand else fixed_ends).add(first_unitig)
        last_unitig, last_strand = abs(last), last > 0
        (fixed_ends if last_strand else fixed_starts).add(last_unitig)
    fixed_starts_copy, fixed_ends_copy = set(fixed_starts), set(fixed_ends)
    for u in fixed_starts_copy:
        for upstream in graph.unitig_index[u].forward_prev:
            (fixed_ends if upstream[1] else fixed_starts).add(upstream[0])
    for u in fixed_ends_copy:
        for downstream in graph.unitig_index[u].forward_next:
            (fixed_starts if downstream[1] else fixed_ends).add(downstream[0])
    return fixed_starts, fixed_ends


# :374-384
def fix_circular_loops(graph, fixed_starts):
    for component in graph.connected_components():
        if graph.component_is_circular_loop(component):
            fixed_starts.add(component[0])


# :233-255
def get_exclusive_inputs(graph, unitig):
    inputs = []
    for prev in unitig.forward_prev:
        prev_u = graph.objects[prev[0]]
        nxt = prev_u.forward_next if prev[1] else prev_u.reverse_next
        if not (len(nxt) == 1 and nxt[0][1] and nxt[0][0] == unitig.number):
            return []
        inputs.append(prev)
    if any(inp[0] == unitig.number for inp in inputs):
        return []
    return inputs


# :258-280
def get_exclusive_outputs(graph, unitig):
    outputs = []
    for nxt in unitig.forward_next:
        next_u = graph.objects[nxt[0]]
        prevs = next_u.forward_prev if nxt[1] else next_u.reverse_prev
        if not (len(prevs) == 1 and prevs[0][1] and prevs[0][0] == unitig.number):
            return []
        outputs.append(nxt)
    if any(o[0] == unitig.number for o in outputs):
        return []
    return outputs


def cannot_merge_start(number, strand, fixed_starts, fixed_ends):
    return (strand and number in fixed_starts) or (not strand and number in fixed_ends)


def cannot_merge_end(number, strand, fixed_starts, fixed_ends):
    return (strand and number in fixed_ends) or (not strand and number in fixed_starts)


def has_single_exclusive_input(graph, unitig, strand):
    return len(get_exclusive_inputs(graph, unitig) if strand else get_exclusive_outputs(graph, unitig)) == 1


# :315-361, up to the list of paths
def find_merge_paths(graph, fixed_starts, fixed_ends):
    already_used, merge_paths = set(), []
    for unitig in graph.unitigs:
        number = unitig.number
        for strand in (FORWARD, REVERSE):
            if number in already_used:
                continue
            if has_single_exclusive_input(graph, unitig, strand) and not cannot_merge_start(number, strand, fixed_starts, fixed_ends):
                continue
            current_path = [(number, strand)]
            already_used.add(number)
            while True:
                num, st = current_path[-1]
                if cannot_merge_end(num, st, fixed_starts, fixed_ends):
                    break
                outputs = get_exclusive_outputs(graph, graph.objects[num]) if st else get_exclusive_inputs(graph, graph.objects[num])
                if len(outputs) != 1:
                    break
                output = outputs[0]
                if not st:
                    output = (output[0], not output[1])
                if output[0] in already_used:
                    break
                if cannot_merge_start(output[0], output[1], fixed_starts, fixed_ends):
                    break
                current_path.append(output)
                already_used.add(output[0])
            if len(current_path) > 1:
                merge_paths.append(list(current_path))
    return merge_paths


# :501-526
def get_merge_path_depth(graph, path, forward_positions):
    if forward_positions:
        return float(forward_positions), 1
    for num, _ in path:
        if graph.objects[num].unitig_type == ANCHOR:
            return graph.objects[num].depth, 2
    total_length = float(sum(len(graph.objects[num].forward_seq) for num, _ in path))
    depth_sum = 0.0
    for num, _ in path:
        depth_sum += graph.objects[num].depth * float(len(graph.objects[num].forward_seq))
    return depth_sum / total_length, 3


# :410-485
def merge_path(graph, path, new_number):
    merged_seq = b"".join(strand_seq(graph.objects[num], st) for num, st in path)
    (first_num, first_strand), (last_num, last_strand) = path[0], path[-1]
    first, last = graph.objects[first_num], graph.objects[last_num]
    forward_positions = first.forward_positions if first_strand else first.reverse_positions
    reverse_positions = last.reverse_positions if last_strand else last.forward_positions
    end_to_start_link = graph.link_exists(last_num, last_strand, first_num, first_strand)
    start_flip_link = graph.link_exists(first_num, not first_strand, first_num, first_strand)
    end_flip_link = graph.link_exists(last_num, last_strand, last_num, not last_strand)
    unitig = U.Unitig(new_number)
    unitig.forward_prev = list(first.forward_prev if first_strand else first.reverse_prev)
    unitig.reverse_next = list(first.reverse_next if first_strand else first.forward_next)
    unitig.forward_next = list(last.forward_next if last_strand else last.reverse_next)
    unitig.reverse_prev = list(last.reverse_prev if last_strand else last.forward_prev)
    unitig.forward_seq = merged_seq
    unitig.depth, unitig.depth_rule = get_merge_path_depth(graph, path, forward_positions)
    unitig.forward_positions, unitig.reverse_positions = forward_positions, reverse_positions
    unitig.unitig_type = CONSENTIG if any(graph.objects[num].unitig_type in (ANCHOR, CONSENTIG) for num, _ in path) else OTHER
    unitig.loop = int(end_to_start_link)
    graph.unitigs.append(unitig)
    graph.objects[new_number] = unitig
    for u in unitig.forward_next:
        (graph.objects[u[0]].forward_prev if u[1] else graph.objects[u[0]].reverse_prev).append((new_number, FORWARD))
    for u in unitig.forward_prev:
        (graph.objects[u[0]].forward_next if u[1] else graph.objects[u[0]].reverse_next).append((new_number, FORWARD))
    for u in unitig.reverse_next:
        (graph.objects[u[0]].forward_prev if u[1] else graph.objects[u[0]].reverse_prev).append((new_number, REVERSE))
    for u in unitig.reverse_prev:
        (graph.objects[u[0]].forward_next if u[1] else graph.objects[u[0]].reverse_next).append((new_number, REVERSE))
    if end_to_start_link:
        unitig.forward_next.append((new_number, FORWARD)); unitig.forward_prev.append((new_number, FORWARD))
        unitig.reverse_next.append((new_number, REVERSE)); unitig.reverse_prev.append((new_number, REVERSE))
    if start_flip_link:
        unitig.reverse_next.append((new_number, FORWARD)); unitig.forward_prev.append((new_number, REVERSE))
    if end_flip_link:
        unitig.forward_next.append((new_number, REVERSE)); unitig.reverse_prev.append((new_number, FORWARD))
    path_numbers = {num for num, _ in path}
    graph.unitigs = [u for u in graph.unitigs if u.number not in path_numbers]


# unitig_graph.rs:547-564
def delete_dangling_links(graph):
    numbers = {u.number for u in graph.unitigs}
    for u in graph.unitigs:
        for name in ("forward_next", "forward_prev", "reverse_next", "reverse_prev"):
            setattr(u, name, [e for e in getattr(u, name) if e[0] in numbers])


def model_expected(n, links, lens, alive=None, path_ends=(), depths=None, fwd=None, rev=None, types=None, seqs=None):
    """merge_linear_paths on the graph, and what is left: one form for the model, the shapes and the library.  New numbers start behind
    n (the highest number, alive or not)."""
    graph = MergeGraph(n, [(int(a), int(b)) for a, b in links], alive, seqs, lens, depths, types, fwd, rev)
    before = len(graph.unitigs)
    fixed_starts, fixed_ends = get_fixed_unitig_starts_and_ends(graph, path_ends)
    fix_circular_loops(graph, fixed_starts)
    paths = find_merge_paths(graph, fixed_starts, fixed_ends)
    new_number = n
    for path in paths:
        new_number += 1
        merge_path(graph, path, new_number)
    delete_dangling_links(graph)
    graph.unitig_index = {u.number: u for u in graph.unitigs}
    link_set = set()
    for u in graph.unitigs:
        for nx in u.forward_next:
            link_set.add((u.number, nx[0] if nx[1] else -nx[0]))
        for nx in u.reverse_next:
            link_set.add((-u.number, nx[0] if nx[1] else -nx[0]))
    assert all((-b, -a) in link_set for a, b in link_set)      # check_links: the merge keeps the set closed
    merged = [graph.unitig_index[n + 1 + i] for i in range(len(paths))]
    fixed = [FIXED_START * (u in fixed_starts) + FIXED_END * (u in fixed_ends) for u in range(1, n + 1)]
    assert len(graph.unitigs) == before - sum(len(p) for p in paths) + len(paths)
    return make_result(n, [[num if st else -num for num, st in p] for p in paths], [len(m.forward_seq) for m in merged], [m.depth for m in merged],
                       [m.unitig_type for m in merged], [m.loop for m in merged], fixed, sorted(link_set), [m.forward_seq for m in merged] if seqs is not None else None,
                       len(graph.unitigs), depth_rules=[m.depth_rule for m in merged])


def make_result(n, chains, lengths, depths, types, loops, fixed, links, seqs, unitigs_after, depth_rules=None):
    chain_of = np.full(n, NOT_MERGED, dtype=np.uint32)
    for c, members in enumerate(chains):
        chain_of[np.abs(np.asarray(members, dtype=np.int64)) - 1] = c
    counts = [len(c) for c in chains]
    return dict(chains=[list(map(int, c)) for c in chains], numbers=[n + 1 + i for i in range(len(chains))], members_per_chain=counts,
                lengths=[int(x) for x in lengths], member_off=[int(x) for x in np.concatenate(([0], np.cumsum(counts)))[:-1]],
                seq_off=[int(x) for x in np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.uint64))))[:-1]],
                depths=np.asarray(depths, dtype=np.float64), types=[int(t) for t in types], loops=[int(x) for x in loops], chain_of=chain_of,
                fixed=np.asarray(fixed, dtype=np.uint8), links=np.asarray(links, dtype=np.int32).reshape(-1, 2), seqs=seqs, unitigs_after=int(unitigs_after),
                merged_unitigs=int(sum(counts)), depth_rules=depth_rules)


def library_result(p):
    """an autocycler_amd.MergePlan in the same form"""
    d = p.chain_dicts()
    sm = p.summary
    assert sm["chains"] == len(d) and sm["links_after"] == len(p.links) and sm["bases_copied"] == len(p.sequences)
    return dict(chains=p.chain_members(), numbers=[c["number"] for c in d], members_per_chain=[c["members"] for c in d], lengths=[c["length"] for c in d],
                member_off=[c["member_off"] for c in d], seq_off=[c["seq_off"] for c in d], depths=p.chains["depth"].astype(np.float64), types=[c["type"] for c in d],
                loops=[c["loop"] for c in d], chain_of=p.chain_of, fixed=p.fixed, links=p.links, seqs=p.chain_sequences() if len(p.sequences) else None,
                unitigs_after=sm["unitigs_after"], merged_unitigs=sm["merged_unitigs"])


def assert_same(got, exp, what="", sequences=True):
    for k in ("chains", "numbers", "members_per_chain", "lengths", "member_off", "seq_off", "types", "loops", "unitigs_after", "merged_unitigs"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    assert got["depths"].tobytes() == exp["depths"].tobytes(), (what, "depths", got["depths"], exp["depths"])      # bit for bit
    for k in ("chain_of", "fixed", "links"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (what, k, got[k], exp[k])
    if sequences and exp["seqs"] is not None:
        want = exp["seqs"] if sum(len(s) for s in exp["seqs"]) else None      # (no merged byte: the library hands out no sequences)
        assert got["seqs"] == want, (what, "seqs")


def result_bytes(p):
    """every accessor's output as bytes (scheduling independence: identical, not merely equal as values)"""
    return b"|".join([p.chains.tobytes(), p.members.tobytes(), p.chain_of.tobytes(), p.fixed.tobytes(), p.sequences.tobytes(), p.links.tobytes(),
                      repr(sorted((k, v) for k, v in p.summary.items() if k not in ("launches", "read_backs", "seconds_device", "seconds_copy"))).encode()])


# ---- the random sweep ------------------------------------------------------------------------------------------------------------------------
def closed_set(links):
    """the links and their reverse complements, once each, in a fixed order"""
    seen, out = set(), []
    for l in links:
        for x in (l, U.rc(l)):
            if x not in seen:
                seen.add(x); out.append(x)
    return out


def random_case(rng):
    """One graph of the sweep as keyword arguments of model_expected.  A third are components_util.random_case's graphs (planted rings and
    hairpins, dense random links), the rest 1-60 unitigs with 0-1.3 n random links (dense links make no chains) and, half of the time, a
    few planted linear stretches; all made a duplicate-free closed set, shuffled.  Half get an alive mask; 0-3 path-end pairs among the
    alive unitigs; depths, types, position counts and sequences are drawn so that all three depth rules occur: a third of the graphs have
    positions (a third of their unitigs none), a fifth of the unitigs are anchors in half of the graphs."""
    if rng.random() < 1 / 3:
        n, links, _, alive, _ = U.random_case(rng)
    else:
        n = rng.randint(1, 60)
        signed = lambda: rng.choice((1, -1)) * rng.randint(1, n)
        links = [(signed(), signed()) for _ in range(rng.randint(0, int(1.3 * n)))]
        if rng.random() < 0.5:
            order = list(range(1, n + 1))
            rng.shuffle(order)
            at = 0
            while at < n:
                size = min(n - at, rng.randint(1, 8))
                s = [u if rng.random() < 0.5 else -u for u in order[at:at + size]]
                links += list(zip(s[:-1], s[1:]))
                if rng.random() < 0.3 and size > 1:
                    links.append((s[-1], s[0]))
                at += size + rng.randint(0, 3)
        alive = [int(rng.random() < 0.85) for _ in range(n)] if rng.random() < 0.5 else None
    links = closed_set(links)
    rng.shuffle(links)
    living = [u for u in range(1, n + 1) if alive is None or alive[u - 1]]
    path_ends = [(rng.choice((1, -1)) * rng.choice(living), rng.choice((1, -1)) * rng.choice(living)) for _ in range(rng.randint(0, 3))] if living else []
    seqs = [bytes(rng.choice(b"ACGTACGTACGTACGTN.") for _ in range(rng.choice((1, 1, 2, 3, 4, 5, 9, 17, 33, rng.randint(1, 80))))) for _ in range(n)]
    depths = [rng.choice((0.0, 1.0, 2.5, rng.random() * 40, rng.random() * 1e-3, 1e6 * rng.random())) for _ in range(n)]
    with_positions, with_anchors = rng.random() < 1 / 3, rng.random() < 0.5
    fwd = [0 if rng.random() < 1 / 3 else rng.randint(1, 9) for _ in range(n)] if with_positions else None
    rev = [0 if rng.random() < 1 / 3 else rng.randint(1, 9) for _ in range(n)] if with_positions else None
    types = [rng.choice((ANCHOR, OTHER, OTHER, CONSENTIG, BRIDGE)) if with_anchors else rng.choice((OTHER, OTHER, OTHER, CONSENTIG, BRIDGE)) for _ in range(n)]
    return dict(n=n, links=links, lens=[len(s) for s in seqs], alive=alive, path_ends=path_ends, depths=depths, fwd=fwd, rev=rev, types=types, seqs=seqs)


# ---- the boundary shapes: keyword arguments of the library call, and the expected result by construction --------------------------------------
def _seq_of(u, length):
    """the forward sequence of unitig u: a pattern that tells unitigs, offsets and strands apart"""
    return bytes(b"ACGT"[(u * 7 + i * (1 + u % 3) + (i >> 3)) & 3] for i in range(length))


def shape_lengths(n, pattern=(1, 3, 4, 5, 31, 32, 33)):
    return [pattern[(u * 5 + u // 7) % len(pattern)] for u in range(n)]


def shape_chain(n, order, strands, lens=None, with_seqs=True):
    """order[0] -> order[1] -> ... on the given strands (True = +), closed under reverse complement: one chain through every unitig"""
    order, strands = [int(x) for x in order], [bool(st) for st in strands]
    lens = list(lens) if lens is not None else shape_lengths(n)
    s = [u if st else -u for u, st in zip(order, strands)]
    links = closed_set(list(zip(s[:-1], s[1:])))
    seqs = [_seq_of(u, lens[u]) for u in range(n)] if with_seqs else None
    depths = [float(1 + u % 5) for u in range(n)]
    # both ends are literal heads: emitted from the end whose unitig has the lower number, which the reference meets first
    if len(order) > 1 and order[-1] < order[0]:
        s = [-x for x in reversed(s)]
    if len(s) < 2:
        exp = make_result(n, [], [], [], [], [], [0] * n, [], None, n)
    else:
        total, wsum = sum(lens[abs(x) - 1] for x in s), 0.0
        for x in s:
            wsum += depths[abs(x) - 1] * float(lens[abs(x) - 1])
        merged_seq = b"".join(seqs[abs(x) - 1] if x > 0 else reverse_complement(seqs[abs(x) - 1]) for x in s) if with_seqs else None
        exp = make_result(n, [s], [total], [wsum / float(total)], [OTHER], [0], [0] * n, [], [merged_seq] if with_seqs else None, n - len(s) + 1)
    return dict(n=n, links=links, lens=lens, path_ends=[], depths=depths, seqs=seqs), exp


def shape_straight(n, **kw):
    return shape_chain(n, range(1, n + 1), [True] * n, **kw)


def shape_permuted(n, seed=5, **kw):
    rng = np.random.default_rng(seed)
    return shape_chain(n, rng.permutation(n) + 1, rng.random(n) < 0.5, **kw)


def shape_ring(n, seed=9):
    """one ring through 1 .. n with mixed strands: a circular loop, so unitig 1's start is fixed and the chain runs from (1, +) all round"""
    assert n >= 2
    st = np.random.default_rng(seed).random(n) < 0.5
    s = [u if f else -u for u, f in zip(range(1, n + 1), st)]
    links = closed_set(list(zip(s, s[1:] + s[:1])))
    if s[0] < 0:      # from (1, +) the ring runs the other way
        s = [-s[0]] + [-x for x in reversed(s[1:])]
    lens = shape_lengths(n)
    seqs = [_seq_of(u, lens[u]) for u in range(n)]
    depths = [float(1 + u % 5) for u in range(n)]
    total, wsum = sum(lens), 0.0
    for x in s:
        wsum += depths[abs(x) - 1] * float(lens[abs(x) - 1])
    merged_seq = b"".join(seqs[abs(x) - 1] if x > 0 else reverse_complement(seqs[abs(x) - 1]) for x in s)
    fixed = [FIXED_START] + [0] * (n - 1)
    exp = make_result(n, [s], [total], [wsum / float(total)], [OTHER], [1], fixed, [(-(n + 1), -(n + 1)), (n + 1, n + 1)], [merged_seq], 1)
    return dict(n=n, links=links, lens=lens, path_ends=[], depths=depths, seqs=seqs), exp


def shape_pairs(n):
    """unitig 1 alone, then (2, 3), (4, 5), ...: (n - 1) / 2 chains of two, every second one through the reverse strand of its second member"""
    assert n % 2 == 1 and n >= 3
    lens = shape_lengths(n)
    seqs = [_seq_of(u, lens[u]) for u in range(n)]
    depths = [float(1 + u % 5) for u in range(n)]
    chains = [[a, (a + 1) if (a // 2) % 2 else -(a + 1)] for a in range(2, n, 2)]
    links = closed_set([tuple(c) for c in chains])
    lengths = [lens[abs(a) - 1] + lens[abs(b) - 1] for a, b in chains]
    dp = [(0.0 + depths[abs(a) - 1] * float(lens[abs(a) - 1]) + depths[abs(b) - 1] * float(lens[abs(b) - 1])) / float(l) for (a, b), l in zip(chains, lengths)]
    merged = [seqs[a - 1] + (seqs[abs(b) - 1] if b > 0 else reverse_complement(seqs[abs(b) - 1])) for a, b in chains]
    k = len(chains)
    exp = make_result(n, chains, lengths, dp, [OTHER] * k, [0] * k, [0] * n, [], merged, 1 + k)
    return dict(n=n, links=links, lens=lens, path_ends=[], depths=depths, seqs=seqs), exp


def shape_singletons(n):
    lens = shape_lengths(n)
    exp = make_result(n, [], [], [], [], [], [0] * n, [], None, n)
    return dict(n=n, links=[], lens=lens, path_ends=[], depths=None, seqs=None), exp
