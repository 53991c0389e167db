"""The model the sequence-subset tests hold the library to: what save_cluster_gfa (cluster.rs:794-806) and clean_up_graph (trim.rs:260-269) do
to a graph for one cluster of sequences, restated step by step in plain Python, in the reference's order:
  1. the paths of the cluster's sequences (label == c; 0 = dropped)
  2. positions as create_sequence_and_positions builds them (unitig_graph.rs:151-174): the forward path and the reversed path, one Position each
  3. recalculate_depth (unitig.rs:260-262): forward_positions.len() as f64
  4. remove_zero_depth_unitigs (:582-586) with delete_dangling_links (:547-564)
  5. the links in get_links_for_gfa order (:333-350)
  6. merge_util.model_expected on that graph (merge_linear_paths)
  7. the P lines after the merge by the reference's position walk (find_starting_unitig / get_next_unitig, :407-465) over the merged unitigs'
     positions (merge_path, graph_simplification.rs:414-415) — not by collapsing runs of the old path
plus the generators of the random sweep and of the boundary table.  It shares no code with kernels_subset.inc."""
import numpy as np

import components_util as U
import merge_util as M

FORWARD, REVERSE = True, False


# ---- the reference, literally ---------------------------------------------------------------------------------------------------------------
def add_positions_from_path(positions, lens, path, path_strand, seq_id):
    """unitig_graph.rs:160-174; positions[(number, unitig strand)] is a list of (seq_id, strand, pos)"""
    pos = 0
    for unitig_num, unitig_strand in path:
        if (unitig_num, FORWARD) not in positions:
            raise KeyError(f"unitig {unitig_num} not found in unitig index")
        positions[(unitig_num, unitig_strand)].append((seq_id, path_strand, pos))
        pos += lens[unitig_num - 1]
    return pos


def model_cluster(n, links, lens, alive, paths, labels, c, gfa_order=False):
    """steps 1-5 for cluster c.  links: the input's entries in their order; gfa_order: they are a handle's (get_links_for_gfa order), so the
    filtered list must be what get_links_for_gfa gives for the edited graph"""
    numbers = [u for u in range(1, n + 1) if alive is None or alive[u - 1]]
    positions = {(u, s): [] for u in numbers for s in (FORWARD, REVERSE)}
    kept = [s for s, label in enumerate(labels) if label == c]
    for s in kept:
        forward_path = [(abs(e), e > 0) for e in paths[s]]
        reverse_path = [(num, not strand) for num, strand in reversed(forward_path)]
        length = add_positions_from_path(positions, lens, forward_path, FORWARD, s)
        assert add_positions_from_path(positions, lens, reverse_path, REVERSE, s) == length
    depth = {u: float(len(positions[(u, FORWARD)])) for u in numbers}
    still = [u for u in numbers if depth[u] > 0.0]
    alive_c = [int(u in set(still)) for u in range(1, n + 1)]
    graph = U.UnitigGraph(n, links, alive_c)      # build_links_from_gfa, then delete_dangling_links: entries that touch a removed unitig are gone
    gfa_links = []
    for a in graph.unitigs:
        gfa_links += [(a.number, b if st else -b) for b, st in a.forward_next]
        gfa_links += [(-a.number, b if st else -b) for b, st in a.reverse_next]
    present = set(still)
    filtered = [(int(a), int(b)) for a, b in links if abs(a) in present and abs(b) in present]
    assert sorted(filtered) == sorted(gfa_links)
    if gfa_order:
        assert filtered == gfa_links
    return dict(n=n, lens=list(lens), seqs=kept, entries=sum(len(paths[s]) for s in kept), unitigs=still, alive=alive_c,
                fwd=[len(positions[(u, FORWARD)]) if u in present else 0 for u in range(1, n + 1)],
                rev=[len(positions[(u, REVERSE)]) if u in present else 0 for u in range(1, n + 1)],
                depth=[depth[u] if u in present else 0.0 for u in range(1, n + 1)], links=filtered,
                path_ends=[(paths[s][0], paths[s][-1]) for s in kept if len(paths[s])], length=sum(lens[u - 1] for u in still),
                positions=positions, paths={s: [int(e) for e in paths[s]] for s in kept})


def model_merge(m, seqs=None):
    """step 6: merge_linear_paths on the cluster's graph — every type Other, depth = the position count"""
    return M.model_expected(m["n"], m["links"], m["lens"], m["alive"], m["path_ends"], m["depth"], m["fwd"], m["rev"], None, seqs)


def model_merged_paths(m, exp):
    """step 7: get_unitig_path_for_sequence for every kept sequence on the graph after the merge"""
    n, lens = m["n"], m["lens"]
    merged = {abs(x) for chain in exp["chains"] for x in chain}
    length, positions = {}, {}
    for u in m["unitigs"]:
        if u not in merged:
            length[u] = lens[u - 1]
            positions[(u, FORWARD)], positions[(u, REVERSE)] = m["positions"][(u, FORWARD)], m["positions"][(u, REVERSE)]
    for number, chain, total in zip(exp["numbers"], exp["chains"], exp["lengths"]):
        first, last = chain[0], chain[-1]
        length[number] = total
        positions[(number, FORWARD)] = m["positions"][(abs(first), first > 0)]      # merge_path :414
        positions[(number, REVERSE)] = m["positions"][(abs(last), not last > 0)]      # :415: the last member's reverse, seen from its strand
    nxt = {}
    for a, b in exp["links"].tolist():
        nxt.setdefault((abs(a), a > 0), []).append((abs(b), b > 0))
    out = {}
    for s in m["seqs"]:
        if not m["paths"][s]:
            out[s] = []
            continue
        starting = [key for key in sorted(positions) if any(p == (s, FORWARD, 0) for p in positions[key])]      # find_starting_unitig
        assert len(starting) == 1, (s, starting)
        u, pos, path = starting[0], 0, []
        while True:
            path.append(u[0] if u[1] else -u[0])
            next_pos = pos + length[u[0]]
            for cand in nxt.get(u, []):      # get_next_unitig
                if any(p == (s, FORWARD, next_pos) for p in positions[cand]):
                    u, pos = cand, next_pos
                    break
            else:
                break
            assert len(path) <= len(m["paths"][s])
        out[s] = path
    return out


def path_length(path, lens, exp):
    chain_len = dict(zip(exp["numbers"], exp["lengths"]))
    return sum(chain_len[abs(e)] if abs(e) in chain_len else lens[abs(e) - 1] for e in path)


# ---- the library's results in the model's form ------------------------------------------------------------------------------------------------
def library_cluster(sub, c):
    fwd, rev = sub.positions(c)
    rec = sub.records[c - 1]
    d = sub.dense(c)
    got = dict(seqs=sub.seqs(c).tolist(), entries=int(rec["entries"]), unitigs=sub.unitigs(c).tolist(), alive=d["alive"].tolist(), fwd=d["fwd_positions"].tolist(),
               rev=d["rev_positions"].tolist(), depth=d["depth"].tolist(), links=[tuple(l) for l in sub.links(c).tolist()],
               path_ends=[tuple(e) for e in sub.path_ends(c).tolist()], length=int(rec["length"]))
    assert (int(rec["seqs"]), int(rec["unitigs"]), int(rec["links"])) == (len(got["seqs"]), len(got["unitigs"]), len(got["links"]))
    assert fwd.tolist() == [got["fwd"][u - 1] for u in got["unitigs"]] and rev.tolist() == [got["rev"][u - 1] for u in got["unitigs"]]
    return got


CLUSTER_KEYS = ("seqs", "entries", "unitigs", "alive", "fwd", "rev", "depth", "links", "path_ends", "length")


def assert_cluster_same(got, exp, what=""):
    for k in CLUSTER_KEYS:
        assert got[k] == exp[k], (what, k, got[k], exp[k])


def subsets_bytes(sub):
    """every product as bytes (scheduling independence: identical, not merely equal as values)"""
    parts = [sub.records.tobytes(), sub.unitig_off.tobytes(), sub.link_off.tobytes(), sub.seq_off.tobytes(), sub.ends_off.tobytes()]
    for c in range(1, sub.n_clusters + 1):
        parts += [sub.unitigs(c).tobytes(), sub.positions(c)[0].tobytes(), sub.positions(c)[1].tobytes(), sub.links(c).tobytes(), sub.seqs(c).tobytes(),
                  sub.path_ends(c).tobytes()]
    parts.append(repr(sorted((k, v) for k, v in sub.summary.items() if k not in ("launches", "read_backs", "seconds_device"))).encode())
    return b"|".join(parts)


# ---- graphs with paths -------------------------------------------------------------------------------------------------------------------------
def gfa_14():
    """tests/golden/test_gfa_14.gfa — the committed GFA that has paths; its numbers have gaps, so it goes through the arrays with an alive mask"""
    g = M.gfa_graph("test_gfa_14.gfa")
    paths = []
    for line in (M.GOLDEN / "test_gfa_14.gfa").read_text().splitlines():
        p = line.split("\t")
        if p[0] == "P":
            paths.append([int(e[:-1]) * (1 if e[-1] == "+" else -1) for e in p[2].split(",")])
    return dict(n=g["n"], links=g["links"], lens=g["lens"], alive=g["alive"], paths=paths, seqs=g["seqs"], merge_args=g)


def hand_graph(rng):
    """A small graph with paths that are walks over it, made of blocks: the unitigs are cut into blocks of 1-5 signed unitigs, a path strings
    whole blocks together (forwards, or backwards on the other strands; sometimes the same block for several laps), and the links are exactly
    the steps the paths take with their reverse complements.  Blocks that are always walked whole become chains; a block walked lap after
    lap a merged loop; sequences of other clusters that leave a block half way cut the chains of the whole graph but not of the cluster.
    Returns (n, links, lens, unitig sequences, paths)."""
    n = rng.randint(1, 24)
    order = list(range(1, n + 1))
    rng.shuffle(order)
    blocks, at = [], 0
    while at < n:
        size = min(n - at, rng.choice((1, 1, 2, 3, 3, 4, 5)))
        blocks.append([u if rng.random() < 0.6 else -u for u in order[at:at + size]])
        at += size
    paths = []
    for _ in range(rng.randint(1, 6)):
        kind, p = rng.random(), []
        if kind < 0.12:
            b = rng.choice(blocks)
            p = b * rng.randint(2, 3)      # laps of one block
        elif kind < 0.2:
            b = rng.choice(blocks)
            p = b[rng.randrange(len(b)):]      # enters a block half way
        else:
            for _ in range(rng.randint(1, 5)):
                b = rng.choice(blocks)
                p += b if rng.random() < 0.6 else [-x for x in reversed(b)]
        if rng.random() < 0.25:
            p = [-x for x in reversed(p)]
        paths.append(p)
    if rng.random() < 0.1:
        paths.append([])
    links = M.closed_set([(a, b) for p in paths for a, b in zip(p, p[1:])])
    rng.shuffle(links)
    lens = sorted((rng.choice((1, 1, 2, 3, 5, 8, 13)) for _ in range(n)), reverse=True)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(l)) for l in lens]
    return n, links, lens, seqs, paths


def hand_gfa_text(n, links, seqs, paths, k=5):
    """the same as a compress-written GFA (one S line per unitig with its depth, the L lines, one P line per non-empty path)"""
    depth = [sum(abs(e) == u for p in paths for e in p) for u in range(1, n + 1)]
    sg = lambda v: f"{abs(v)}\t{'+' if v > 0 else '-'}"
    out = [f"H\tVN:Z:1.0\tKM:i:{k}"]
    out += [f"S\t{u}\t{seqs[u - 1].decode()}\tDP:f:{depth[u - 1]:.2f}" for u in range(1, n + 1)]
    out += [f"L\t{sg(a)}\t{sg(b)}\t0M" for a, b in links]
    for i, p in enumerate(paths):
        total = sum(len(seqs[abs(e) - 1]) for e in p)
        out.append(f"P\t{i + 1}\t" + ",".join(f"{abs(e)}{'+' if e > 0 else '-'}" for e in p) + f"\t*\tLN:i:{total}\tFN:Z:hand_{i % 3}.fasta\tHD:Z:contig_{i}")
    return "\n".join(out) + "\n"


def random_labels(rng, n_seqs):
    """(labels, n_clusters): 1-4 clusters, sometimes one more than any label reaches (an empty cluster), a fifth of the sequences dropped"""
    used = rng.randint(1, 4)
    labels = [0 if rng.random() < 0.2 else rng.randint(1, used) for _ in range(n_seqs)]
    return labels, used + (rng.random() < 0.3)


# ---- the boundary table: expected by construction, in numpy -------------------------------------------------------------------------------------
def expected_by_numpy(n, links, lens, entries, off, labels, n_clusters):
    """the subsets of every cluster from np.unique over (cluster, unitig) keys: a list of dicts (unitigs, counts, links, seqs, entries, length)"""
    entries, off, labels = np.asarray(entries, dtype=np.int64), np.asarray(off, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    links, lens = np.asarray(links, dtype=np.int64).reshape(-1, 2), np.asarray(lens, dtype=np.int64)
    seq_of_entry = np.repeat(np.arange(len(labels)), np.diff(off))
    label_of_entry = labels[seq_of_entry]
    keep = label_of_entry > 0
    keys, counts = np.unique((label_of_entry[keep] - 1) * n + (np.abs(entries[keep]) - 1), return_counts=True)
    out = []
    for c in range(1, n_clusters + 1):
        mine = (keys // n) == c - 1 if n else np.zeros(0, dtype=bool)
        units = keys[mine] % n + 1 if n else np.zeros(0, dtype=np.int64)
        alive = np.zeros(n + 1, dtype=bool)
        alive[units] = True
        kept_links = links[alive[np.abs(links[:, 0])] & alive[np.abs(links[:, 1])]] if len(links) else links
        seqs = np.flatnonzero(labels == c)
        out.append(dict(unitigs=units, counts=counts[mine], links=kept_links.reshape(-1, 2), seqs=seqs, entries=int(np.diff(off)[seqs].sum()),
                        length=int(lens[units - 1].sum()),
                        path_ends=np.array([(entries[off[s]], entries[off[s + 1] - 1]) for s in seqs if off[s + 1] > off[s]], dtype=np.int64).reshape(-1, 2)))
    return out


def assert_numpy_same(sub, exp, what=""):
    same = lambda got, want: np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64))
    assert sub.n_clusters == len(exp), what
    for c, e in enumerate(exp, start=1):
        fwd, rev = sub.positions(c)
        rec = sub.records[c - 1]
        assert same(sub.unitigs(c), e["unitigs"]), (what, c, "unitigs")
        assert same(fwd, e["counts"]) and same(rev, e["counts"]), (what, c, "positions")
        assert same(sub.links(c), e["links"]), (what, c, "links")
        assert same(sub.seqs(c), e["seqs"]), (what, c, "seqs")
        assert same(sub.path_ends(c), e["path_ends"]), (what, c, "path_ends")
        assert (int(rec["seqs"]), int(rec["unitigs"]), int(rec["entries"]), int(rec["links"]), int(rec["length"])) == \
            (len(e["seqs"]), len(e["unitigs"]), e["entries"], len(e["links"]), e["length"]), (what, c, "record")


def ring_with_chords(n, n_paths, path_len, seed):
    """n unitigs of one base on a ring (u -> u + 1, n -> 1) with a chord u -> u + 7 from every unitig; n_paths forward random walks of
    path_len entries that take the chord three times in ten.  Returns (links (m, 2) int32 closed under reverse complement, entries int32,
    off uint64)."""
    rng = np.random.default_rng(seed)
    u = np.arange(1, n + 1, dtype=np.int64)
    fwd = np.concatenate([np.stack([u, u % n + 1], axis=1), np.stack([u, (u + 6) % n + 1], axis=1)])
    links = np.concatenate([fwd, np.stack([-fwd[:, 1], -fwd[:, 0]], axis=1)]).astype(np.int32)
    steps = np.where(rng.random((n_paths, path_len)) < 0.3, 7, 1)
    steps[:, 0] = rng.integers(0, n, n_paths)      # where the walk starts
    entries = (np.cumsum(steps, axis=1) % n + 1).astype(np.int32).reshape(-1)
    off = (np.arange(n_paths + 1, dtype=np.uint64) * np.uint64(path_len))
    return links, entries, off
