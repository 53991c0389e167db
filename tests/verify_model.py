"""ac_verify_graph restated in plain Python: sequential loops over ints, lists and dicts, written from the contract in
include/autocycler_hip.h (the ac_verify_report comment block) and the reference lines it cites — check_links (unitig_graph.rs:752-793),
renumber_unitigs (:295-315), get_links_for_gfa / create_links (:333-350, :234-287), the walk's break cases (:192-223), the positions
from_gfa_lines rebuilds (:151-174) and expand_repeats with its candidate test and clamps (graph_simplification.rs:43-280).  It is the
reference the mutation sweeps of verify_cases.py hold the device verifier's WHOLE report to; it shares no code with kernels_verify.inc.

A graph is a dict of plain values:
    block, block_size   the unitig sequences one behind the other (bytes) and the size of the block the handle holds them in (None: not
                        known — a built handle keeps them in a pooled block with slack behind them — and then no range is judged)
    begin, len, depth   per unitig: offset into the block, length, depth
    links               [(a, b)] signed unitig numbers in L-line order
    path, path_off      signed path entries of all sequences, and where each sequence's entries begin (n_seqs + 1 offsets)
    stats               post_unitigs, post_links, post_total_length, pre_unitigs, pre_total_length, kmer_count (0: not recorded)
    link_rank           None: a graph without seed numbers (reloaded from a GFA) — only the seed-free part of the L-line order is decided.
                        Else {link: rank}: the seed numbers of a built graph, given as the one correct order of its links (the ABI does
                        not expose the numbers themselves; with them the order is total, so the unmutated array IS that order).
`seqs` are the job's unpadded sequences (bytes), k the k-mer size.

Where the header leaves a detail open the model states its choice:
  * a link that stands again further down the array is the duplicate (so the first of three equal links is the smallest);
  * links with an endpoint out of range are reported as that and left out of the order check; the others are checked in array order;
  * a unitig whose length or range is invalid is not compared with its successor, and its bytes are not compared with its predecessor's;
    a unitig LONGER than its predecessor is out of order whatever its range (the lengths alone decide);
  * a junction with more than five sources is not evaluated (a k-mer has at most five successors, kmer_graph.rs:136-150: the link order
    check refuses the sixth link of a list);
  * path offsets that do not ascend from 0 to the number of entries end the run at once (failed = 128, the first such sequence, nothing
    else filled in): every other check indexes the entries through them.
"""
NONE = (1 << 64) - 1
F_UNITIG, F_ORDER, F_LINK_RANGE, F_LINK_DUP, F_LINK_MIRROR, F_PATH_RANGE, F_PATH_STEP, F_PATH_LEN, F_SPELL, F_DEPTH, F_STATS, F_LINK_ORDER, \
    F_MAXIMAL, F_EXPAND = (1 << i for i in range(14))
C_LINK_ORDER, C_LINK_ORDER_SEEDS, C_MAXIMAL, C_EXPAND = 1, 2, 4, 8
FIELDS = ("failed", "checks", "first_bad_unitig", "first_bad_link", "first_bad_path_entry", "first_bad_sequence", "first_bad_base",
          "first_bad_junction", "unitigs", "links", "path_entries", "bases_checked", "self_mirror_links")
_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def revcomp(q):
    return bytes(_COMP.get(c, ord("N")) for c in reversed(q))      # (misc.rs:358-367)


def verify(G, seqs, k, detail=None):
    """-> the report as a dict of FIELDS.  detail (a dict, optional) receives order_pair: the first out-of-order adjacent pair of links
    (or None), and link_min_other: the smallest first_bad_link of the classes other than the L-line order (NONE: none)."""
    U, links, path, off = len(G["len"]), G["links"], G["path"], G["path_off"]
    n_seqs, n_links, n_ent = len(seqs), len(links), len(path)
    block, begin, length, depth = G["block"], G["begin"], G["len"], G["depth"]
    rep = dict(failed=0, checks=0, first_bad_unitig=NONE, first_bad_link=NONE, first_bad_path_entry=NONE, first_bad_sequence=NONE,
               first_bad_base=NONE, first_bad_junction=NONE, unitigs=0, links=0, path_entries=0, bases_checked=0, self_mirror_links=0)
    if detail is not None:
        detail["order_pair"], detail["link_min_other"] = None, NONE

    def fail(flag, slot, index):
        rep["failed"] |= flag
        rep[slot] = min(rep[slot], index)

    # ---- the path offsets themselves
    bad = [s for s in range(n_seqs) if off[s + 1] < off[s]]
    if off[0] != 0: bad.append(0)
    if off[n_seqs] != n_ent: bad.append(n_seqs - 1)
    if bad:
        fail(F_PATH_LEN, "first_bad_sequence", min(bad))
        return rep
    rep.update(unitigs=U, links=n_links, path_entries=n_ent)

    # ---- unitigs: lengths and ranges, renumber_unitigs order (length descending, sequence ascending, depth descending)
    valid = []
    for i in range(U):
        valid.append(length[i] > 0 and (G["block_size"] is None or begin[i] + length[i] <= G["block_size"]))
        if not valid[i]: fail(F_UNITIG, "first_bad_unitig", i)
    useq = lambda i: block[begin[i]:begin[i] + length[i]]
    for i in range(U - 1):
        if not valid[i]: continue
        if length[i + 1] > length[i]: fail(F_ORDER, "first_bad_unitig", i)      # (the lengths alone decide: no byte of i + 1 is read)
        elif length[i + 1] == length[i] and valid[i + 1]:
            x, y = useq(i), useq(i + 1)
            if y < x or (y == x and depth[i + 1] > depth[i]): fail(F_ORDER, "first_bad_unitig", i)

    # ---- the link set: range, duplicates, mirrors (check_links)
    in_range = [1 <= abs(a) <= U and 1 <= abs(b) <= U for a, b in links]
    last_at, self_mirror = {}, 0
    for i in range(n_links):
        if not in_range[i]: fail(F_LINK_RANGE, "first_bad_link", i)
        else:
            last_at[links[i]] = i
            if links[i][0] == -links[i][1]: self_mirror += 1
    for i in range(n_links):
        if not in_range[i]: continue
        a, b = links[i]
        if last_at[(a, b)] != i: fail(F_LINK_DUP, "first_bad_link", i)
        if (-b, -a) not in last_at: fail(F_LINK_MIRROR, "first_bad_link", i)
    link_set_ok = not rep["failed"] & (F_LINK_RANGE | F_LINK_DUP | F_LINK_MIRROR)
    rep["self_mirror_links"] = self_mirror
    succ, pred = {}, {}
    for i in range(n_links):
        if in_range[i]:
            succ.setdefault(links[i][0], []).append(links[i][1])
            pred.setdefault(links[i][1], []).append(links[i][0])

    # ---- paths: range, steps, lengths; depth = occurrences
    occ, elen = [0] * U, []
    for j in range(n_ent):
        p = path[j]
        if p == 0 or abs(p) > U:
            fail(F_PATH_RANGE, "first_bad_path_entry", j); elen.append(0)
        else:
            elen.append(length[abs(p) - 1]); occ[abs(p) - 1] += 1
    for s in range(n_seqs):
        for j in range(off[s], off[s + 1] - 1):
            if path[j] != 0 and path[j + 1] != 0 and (path[j], path[j + 1]) not in last_at: fail(F_PATH_STEP, "first_bad_path_entry", j)
        if sum(elen[off[s]:off[s + 1]]) != len(seqs[s]): fail(F_PATH_LEN, "first_bad_sequence", s)
    for i in range(U):
        if depth[i] != float(occ[i]): fail(F_DEPTH, "first_bad_unitig", i)
    paths_ok = not rep["failed"] & (F_PATH_LEN | F_PATH_RANGE | F_UNITIG)

    # ---- the strands a sequence strand begins / ends with (the reverse strand of a sequence walks the flipped path backwards)
    strand_starts, strand_ends = set(), set()
    for s in range(n_seqs):
        if off[s] == off[s + 1]: continue
        first, last = path[off[s]], path[off[s + 1] - 1]
        if first != 0 and abs(first) <= U: strand_starts.add(first); strand_ends.add(-first)
        if last != 0 and abs(last) <= U: strand_ends.add(last); strand_starts.add(-last)

    # ---- L-line order
    order_bad = []
    prev, run = None, []
    seen_plus = minus_after_plus = False
    for j in range(n_links):
        if not in_range[j]: continue
        a, b = links[j]
        grp = (abs(a), 0 if a > 0 else 1)
        if prev is None or (abs(links[prev][0]), 0 if links[prev][0] > 0 else 1) != grp:
            if prev is not None and (abs(links[prev][0]), 0 if links[prev][0] > 0 else 1) > grp: order_bad.append((prev, j))
            run = [j]
            seen_plus, minus_after_plus = (a < 0 and b > 0), False
        else:
            run.append(j)
            if len(run) == 6: order_bad.append((prev, j))
            if G["link_rank"] is not None:
                if G["link_rank"][links[prev]] >= G["link_rank"][links[j]]: order_bad.append((prev, j))
            elif a > 0:
                if b > 0 and links[prev][1] < 0: order_bad.append((prev, j))      # forward_next: the b+ before the b-
            elif b > 0:
                if minus_after_plus: order_bad.append((prev, j))                     # reverse_next: a'-, b+, a'- and no b+ after that
                seen_plus = True
            elif seen_plus: minus_after_plus = True
        prev = j
    if detail is not None: detail["link_min_other"] = rep["first_bad_link"]
    if order_bad:
        first = min(order_bad, key=lambda pr: pr[1])
        fail(F_LINK_ORDER, "first_bad_link", first[1])
        if detail is not None: detail["order_pair"] = first
    rep["checks"] = C_LINK_ORDER | (C_LINK_ORDER_SEEDS if G["link_rank"] is not None else 0)

    # ---- maximality: a sole link between two unitigs must be one of the walk's break cases
    if link_set_ok:
        rep["checks"] |= C_MAXIMAL
        for i in range(n_links):
            a, b = links[i]
            if len(succ[a]) != 1 or len(pred[b]) != 1 or b == a or b == -a: continue
            if a not in strand_ends and b not in strand_starts:
                fail(F_MAXIMAL, "first_bad_link", i)
                if detail is not None: detail["link_min_other"] = min(detail["link_min_other"], i)

    # ---- expand_repeats at its fixed point
    if link_set_ok and paths_ok:
        rep["checks"] |= C_EXPAND
        fpos, rpos = [[] for _ in range(U)], [[] for _ in range(U)]
        for s in range(n_seqs):
            o, L = 0, len(seqs[s])
            for j in range(off[s], off[s + 1]):
                p = path[j]; u = abs(p) - 1
                (fpos if p > 0 else rpos)[u].append(o)                       # the forward path
                (rpos if p > 0 else fpos)[u].append(L - o - length[u])        # the reverse path
                o += length[u]
        starts0, ends0 = {x for x in strand_starts if x > 0}, {x for x in strand_ends if x > 0}
        fixed_starts, fixed_ends = set(starts0), set(ends0)
        for u in starts0:
            for up in pred.get(u, []): (fixed_ends if up > 0 else fixed_starts).add(abs(up))
        for u in ends0:
            for dn in succ.get(u, []): (fixed_starts if dn > 0 else fixed_ends).add(abs(dn))
        sseq = lambda v: useq(v - 1) if v > 0 else revcomp(useq(-v - 1))
        for u in range(1, U + 1):
            inputs = list(pred.get(u, []))
            if any(succ[p] != [u] for p in inputs) or any(abs(p) == u for p in inputs): inputs = []
            if 2 <= len(inputs) <= 5 and u not in fixed_starts and not any((p > 0 and p in fixed_ends) or (p < 0 and -p in fixed_starts) for p in inputs):
                common = sseq(inputs[0])
                for p in inputs:
                    while not sseq(p).endswith(common): common = common[1:]
                dup = 2 if len({abs(p) for p in inputs}) != len(inputs) else 1
                while common and min(length[abs(p) - 1] for p in inputs) <= len(common) * dup: common = common[1:]
                while common and any(pos <= len(common) for pos in fpos[u - 1]): common = common[1:]
                if common: fail(F_EXPAND, "first_bad_junction", 2 * (u - 1))
            outputs = list(succ.get(u, []))
            if any(pred[q] != [u] for q in outputs) or any(abs(q) == u for q in outputs): outputs = []
            if 2 <= len(outputs) <= 5 and u not in fixed_ends and not any((q > 0 and q in fixed_starts) or (q < 0 and -q in fixed_ends) for q in outputs):
                common = sseq(outputs[0])
                for q in outputs:
                    while not sseq(q).startswith(common): common = common[:-1]
                dup = 2 if len({abs(q) for q in outputs}) != len(outputs) else 1
                while common and min(length[abs(q) - 1] for q in outputs) <= len(common) * dup: common = common[:-1]
                while common and any(pos <= len(common) for pos in rpos[u - 1]): common = common[:-1]
                if common: fail(F_EXPAND, "first_bad_junction", 2 * (u - 1) + 1)

    # ---- every path spells its sequence
    if paths_ok:
        spelled = b"".join(useq(p - 1) if p > 0 else revcomp(useq(-p - 1)) for p in path)
        want = b"".join(seqs)
        rep["bases_checked"] = len(want)
        for g in range(len(want)):
            if spelled[g] != want[g]:
                fail(F_SPELL, "first_bad_base", g)
                break

    # ---- the statistics the handle carries
    st = G["stats"]
    if st["post_total_length"] != sum(length) or st["post_unitigs"] != U or st["pre_unitigs"] != U or \
            st["post_links"] != (n_links + self_mirror) // 2 or (st["kmer_count"] and st["kmer_count"] != 2 * st["pre_total_length"]):
        rep["failed"] |= F_STATS
    return rep


def from_handle(g, b, block_size, link_rank):
    """The graph a handle holds NOW: b = its bulk() views (taken before any mutation, so that the views' sizes are the clean graph's)."""
    post, pre = g.stats_post, g.stats_pre
    return dict(block=bytes(b["seq_bytes"]), block_size=block_size, begin=[int(x) for x in b["seq_begin"]], len=[int(x) for x in b["seq_len"]],
                depth=[float(x) for x in b["depth"]], links=[(int(l["a"]), int(l["b"])) for l in b["links"]],
                path=[int(x) for x in b["path_entries"]], path_off=[int(x) for x in b["path_off"]], link_rank=link_rank,
                stats=dict(post_unitigs=post["unitigs"], post_links=post["links"], post_total_length=post["total_length"],
                           pre_unitigs=pre["unitigs"], pre_total_length=pre["total_length"], kmer_count=g.kmer_count))


def from_gfa(e):
    """The graph ac_graph_from_gfa makes of an edited GFA (verify_cases._Gfa): segments one behind the other, the L lines gathered per
    unitig strand in file order (save_gfa walks forward_next, then reverse_next), the statistics counted from the file, no seed numbers."""
    block, begin, length, depth = b"", [], [], []
    for q, tags in e.segs:
        begin.append(len(block)); length.append(len(q)); block += q.encode()
        depth.append(float(next(t for t in tags if t.startswith("DP:f:"))[5:]))
    links = sorted(e.links, key=lambda l: (abs(l[0]), 0 if l[0] > 0 else 1))      # (stable)
    path, off = [], [0]
    for _, ents, _ in e.paths:
        path += ents; off.append(len(path))
    sm = sum(1 for a, b in links if a == -b)
    st = dict(post_unitigs=len(length), post_links=(len(links) + sm) // 2, post_total_length=len(block), pre_unitigs=len(length),
              pre_total_length=len(block), kmer_count=0)
    return dict(block=block, block_size=len(block), begin=begin, len=length, depth=depth, links=links, path=path, path_off=off, link_rank=None, stats=st)
