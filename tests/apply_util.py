"""The model the apply-bridges tests hold the library to: resolve.rs:223-282 restated literally on a graph that keeps its four lists per unitig.
  apply_bridges      the loop over the bridges in the given (Bridge::cmp) order; per bridge that is not skipped delete_outgoing_links,
                     delete_incoming_links (unitig_graph.rs:795-865, list by list, by value), then create_link (:867-893, pushes at the end
                     of the lists) — directly, or through a new Bridge unitig numbered max + 1 with reduce_depths (one visit at a time,
                     unitig.rs:269-274)
  after the loop     components_util's unitigs_not_connected_to_anchor, the retain(depth > 0.0), delete_dangling_links
  then               merge_util (through finish_util.model_graph), finish_util.finish_model and finish_util.save_gfa, unedited, for the
                     merged and final texts; resolve_util.resolve_expected for the bridges of the two-pass flow (resolve.rs:44-67)
It shares no code with kernels_apply.inc or apply_host.cpp, and no rule about which links survive or where the created ones land is stated
here: both are read off the lists."""
import components_util as U
import finish_util as F
import merge_util as M
import resolve_util as R

COVERAGE = ("bridge_unitig", "direct_link", "skipped_bridge", "reverse_member", "depth_clamped", "depth_reduced_above_zero", "anchorless_removed", "zero_depth_removed",
            "zero_depth_was_tie", "dangling_link_removed", "link_deleted", "link_survived", "culled", "passes_differ", "merged_chain", "nothing_applied")


def signed(entry):
    return entry[0] if entry[1] else -entry[0]


def entry_of(num):
    return (abs(num), num > 0)


# ---- unitig_graph.rs:795-893, literally ------------------------------------------------------------------------------------------------------
def delete_link_one_way(graph, start_num, end_num):
    start, end = graph.unitig_index[abs(start_num)], graph.unitig_index[abs(end_num)]
    nxt = start.forward_next if start_num > 0 else start.reverse_next
    for i in reversed([i for i, c in enumerate(nxt) if c == entry_of(end_num)]):
        del nxt[i]
    prev = end.forward_prev if end_num > 0 else end.reverse_prev
    for i in reversed([i for i, c in enumerate(prev) if c == entry_of(start_num)]):
        del prev[i]


def delete_link(graph, start_num, end_num):
    delete_link_one_way(graph, start_num, end_num)
    delete_link_one_way(graph, -end_num, -start_num)


def delete_outgoing_links(graph, signed_num):
    unitig = graph.unitig_index[abs(signed_num)]
    next_numbers = [signed(c) for c in (unitig.forward_next if signed_num > 0 else unitig.reverse_next)]
    for next_num in next_numbers:
        delete_link(graph, signed_num, next_num)
    return len(next_numbers)


def delete_incoming_links(graph, signed_num):
    unitig = graph.unitig_index[abs(signed_num)]
    prev_numbers = [signed(c) for c in (unitig.forward_prev if signed_num > 0 else unitig.reverse_prev)]
    for prev_num in prev_numbers:
        delete_link(graph, prev_num, signed_num)
    return len(prev_numbers)


def create_link_one_way(graph, start_num, end_num):
    start, end = graph.unitig_index[abs(start_num)], graph.unitig_index[abs(end_num)]
    (start.forward_next if start_num > 0 else start.reverse_next).append(entry_of(end_num))
    (end.forward_prev if end_num > 0 else end.reverse_prev).append(entry_of(start_num))


def create_link(graph, start_num, end_num):
    create_link_one_way(graph, start_num, end_num)
    if start_num != -end_num:
        create_link_one_way(graph, -end_num, -start_num)


def reduce_depth_by_one(unitig):
    unitig.depth -= 1.0
    if unitig.depth < 0.0:
        unitig.depth = 0.0


def get_links_for_gfa(graph):
    links = []
    for a in graph.unitigs:
        links += [(a.number, signed(b)) for b in a.forward_next]
        links += [(-a.number, signed(b)) for b in a.reverse_next]
    return links


# ---- resolve.rs:223-282 --------------------------------------------------------------------------------------------------------------------
def apply_model(n, links, lens, anchors, bridges, applied, bridge_depth, alive=None, depths=None, seqs=None):
    """bridges: dicts with start, end, best_path, distinct_paths [(path, multiplicity)] in Bridge::cmp order; applied: one truth value per
    bridge (the reference's `!conflicting`).  New numbers start behind n (the highest number, alive or not), as in merge_util.
    -> dict(n_total, len, alive, depth, type, bridge_of, links, bridge_seqs, graph) and the coverage met"""
    met = dict.fromkeys(COVERAGE, 0)
    types = [M.ANCHOR if u in set(anchors) else M.OTHER for u in range(1, n + 1)]
    graph = M.MergeGraph(n, [(int(a), int(b)) for a, b in links], alive, seqs, lens, depths, types)
    depth_in = [float(depths[u]) if depths is not None else 0.0 for u in range(n)]
    before = set(get_links_for_gfa(graph))
    bridge_of, bridge_units = [], []
    met["nothing_applied"] = int(not any(applied))
    for index, (bridge, on) in enumerate(zip(bridges, applied)):
        if not on:
            met["skipped_bridge"] = 1
            continue
        start, end = bridge["start"], bridge["end"]
        delete_outgoing_links(graph, start)
        delete_incoming_links(graph, end)
        if not bridge["best_path"]:
            create_link(graph, start, end)
            met["direct_link"] = 1
        else:
            bridge_seq = b"".join(M.strand_seq(graph.unitig_index[abs(e)], e > 0) for e in bridge["best_path"])
            met["reverse_member"] |= int(any(e < 0 for e in bridge["best_path"]))
            bridge_num = max([n] + [u.number for u in graph.unitigs]) + 1
            unitig = U.Unitig(bridge_num)
            unitig.forward_seq, unitig.depth, unitig.unitig_type, unitig.forward_positions, unitig.reverse_positions = bridge_seq, float(bridge_depth), M.BRIDGE, 0, 0
            graph.unitigs.append(unitig)
            graph.unitig_index[bridge_num] = unitig
            graph.objects[bridge_num] = unitig
            for path, copies in bridge["distinct_paths"]:      # all_paths: every copy of every distinct path
                for _ in range(copies):
                    for e in path:
                        u = graph.unitig_index[abs(e)]
                        had = u.depth
                        reduce_depth_by_one(u)
                        met["depth_clamped"] |= int(had < 1.0)
                        met["depth_reduced_above_zero"] |= int(u.depth > 0.0)
            create_link(graph, start, bridge_num)
            create_link(graph, bridge_num, end)
            bridge_of.append(index); bridge_units.append(unitig)
            met["bridge_unitig"] = 1
    after_edit = set(get_links_for_gfa(graph))
    met["link_deleted"], met["link_survived"] = int(bool(before - after_edit)), int(bool(before & after_edit))
    everyone = dict(graph.unitig_index)
    # delete_unitigs_not_connected_to_anchor
    gone = graph.unitigs_not_connected_to_anchor(set(anchors))
    met["anchorless_removed"] = int(bool(gone))
    graph.unitigs = [u for u in graph.unitigs if u.number not in gone]
    M.delete_dangling_links(graph)
    graph.unitig_index = {u.number: u for u in graph.unitigs}
    # remove_zero_depth_unitigs
    n_before, l_before = len(graph.unitigs), len(get_links_for_gfa(graph))
    graph.unitigs = [u for u in graph.unitigs if u.depth > 0.0]
    M.delete_dangling_links(graph)
    graph.unitig_index = {u.number: u for u in graph.unitigs}
    met["zero_depth_removed"] = int(len(graph.unitigs) < n_before)
    met["dangling_link_removed"] = int(len(get_links_for_gfa(graph)) < l_before)
    met["zero_depth_was_tie"] = int(bool(graph.unitigs_not_connected_to_anchor(set(anchors))))      # something hung on an anchor through a zero-depth unitig only
    n_total = n + len(bridge_units)
    assert [u.number for u in bridge_units] == list(range(n + 1, n_total + 1))
    alive_out = [int(u in graph.unitig_index) for u in range(1, n_total + 1)]
    depth_out = [everyone[u].depth if u in everyone else depth_in[u - 1] for u in range(1, n_total + 1)]
    out = dict(n_total=n_total, len=[int(x) for x in lens] + [len(u.forward_seq) for u in bridge_units], alive=alive_out, depth=depth_out,
               type=types + [M.BRIDGE] * len(bridge_units), bridge_of=bridge_of, links=get_links_for_gfa(graph), bridge_seqs=[u.forward_seq for u in bridge_units],
               graph=graph, seqs=[everyone[u].forward_seq if u in everyone else b"" for u in range(1, n_total + 1)])
    return out, met


def bridged_text(applied, k, use_other_colour=False):
    """3_bridged.gfa: save_gfa of the graph as apply_bridges leaves it"""
    unitigs = [(u.number, u.number, u.forward_seq, u.depth, u.unitig_type) for u in applied["graph"].unitigs]
    return F.save_gfa(dict(unitigs=unitigs, links=applied["links"]), k, (), use_other_colour)


def merged_model(applied):
    """merge_after_bridging: merge_linear_paths(graph, &vec![]) with cleared positions, then renumber_unitigs -> (finish_model's dict, plan members, met)"""
    a = applied
    graph, mpaths = F.model_graph(a["n_total"], a["links"], a["len"], a["alive"], (), a["depth"], None, None, a["type"], a["seqs"])
    exp, met = F.finish_model(graph, a["n_total"], True)
    return exp, [[num if st else -num for num, st in p] for p in mpaths], met


def resolve_model(n, links, lens, depths, seqs, paths, consensus_weights, k):
    """resolve.rs:44-67 -> dict(bridged, merged, final: the three texts; cull_count; unique, kept: the two apply_model results) and the coverage"""
    anchors, bridges = R.resolve_expected(paths, lens, n, consensus_weights)
    assert all(b["status"] == 0 for b in bridges)
    bridge_depth = float(len(paths))
    unique, met = apply_model(n, links, lens, anchors, bridges, [not b["conflicting"] for b in bridges], bridge_depth, None, depths, seqs)
    exp_merged, members, _ = merged_model(unique)
    met["merged_chain"] = int(bool(members))
    cull_count = sum(b["culled"] for b in bridges)
    met["culled"] = int(cull_count > 0)
    kept, exp_final = unique, exp_merged
    if cull_count > 0:
        kept, met2 = apply_model(n, links, lens, anchors, bridges, [not b["culled"] for b in bridges], bridge_depth, None, depths, seqs)
        exp_final, _, _ = merged_model(kept)
        met["passes_differ"] = int(kept["links"] != unique["links"] or kept["alive"] != unique["alive"])
        for key in met2:
            if key not in ("culled", "passes_differ", "merged_chain", "nothing_applied"):
                met[key] |= met2[key]
    return dict(anchors=anchors, bridges=bridges, bridged=bridged_text(unique, k), merged=F.save_gfa(exp_merged, k, (), False), final=F.save_gfa(exp_final, k, (), True),
                cull_count=cull_count, unique=unique, kept=kept), met


# ---- the library's result in the model's form --------------------------------------------------------------------------------------------------
def library_result(ap):
    sm = ap.summary
    assert sm["links_out"] == len(ap.links) and sm["bases_copied"] == len(ap.bridge_sequences)
    return dict(n_total=ap.n_total, len=ap.len.tolist(), alive=ap.alive.tolist(), depth=ap.depth.tobytes(), type=ap.type.tolist(), bridge_of=ap.bridge_of.tolist(),
                links=[tuple(l) for l in ap.links.tolist()], bridge_seqs=ap.bridge_unitig_sequences())


def assert_same(ap, exp, what="", sequences=True):
    import numpy as np
    got = library_result(ap)
    for key in ("n_total", "len", "alive", "type", "bridge_of", "links"):
        assert got[key] == exp[key], (what, key, got[key], exp[key])
    assert got["depth"] == np.asarray(exp["depth"], dtype=np.float64).tobytes(), (what, "depth", ap.depth.tolist(), exp["depth"])      # bit for bit
    if sequences:
        assert got["bridge_seqs"] == [s for s in exp["bridge_seqs"]] or (not got["bridge_seqs"] and not any(exp["bridge_seqs"])), (what, "bridge_seqs")
    sm = ap.summary
    assert sm["bridges_applied"] - sm["direct_links"] == len(exp["bridge_of"]), what


def applied_bytes(ap):
    """every product as bytes (two runs: identical, not merely equal as values)"""
    return b"|".join([ap.len.tobytes(), ap.alive.tobytes(), ap.depth.tobytes(), ap.type.tobytes(), ap.bridge_of.tobytes(), ap.links.tobytes(), ap.bridge_sequences.tobytes(),
                      ap.bridge_seq_off.tobytes(),
                      repr(sorted((k, v) for k, v in ap.summary.items() if k not in ("launches", "launches_components", "read_backs", "seconds_device", "seconds_copy", "seconds_components"))).encode()])


# ---- generators --------------------------------------------------------------------------------------------------------------------------------
def links_of_paths(paths):
    """the links a graph built from these paths holds: every adjacency and its mirror image, in first-seen order"""
    seen, links = set(), []
    for p in paths:
        for a, b in zip(p, p[1:]):
            for l in ((a, b), (-b, -a)):
                if l not in seen:
                    seen.add(l); links.append(l)
    return links


def random_case(rng):
    """a planted graph: resolve_util's random sequence paths over unitigs with short random sequences; the links are the paths' adjacencies
    plus a few strays; depths are the visit counts, some replaced.  -> dict(n, links, lens, depths, seqs, paths, cw)"""
    paths, w, cw = R.random_case(rng)
    n = len(w)
    if rng.random() < 0.5:      # circular sequences: close every path
        paths = [p + p[:1] if len(p) > 1 else p for p in paths]
    lens = [rng.choice((1, 2, 3, 5, 8, 13, 16, 17)) for _ in range(n)]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(l)) for l in lens]
    links = links_of_paths(paths)
    for _ in range(rng.choice((0, 0, 1, 3))):      # unitigs no path visits, hanging off the graph or on their own
        a, b = rng.choice((-1, 1)) * rng.randint(1, n), rng.choice((-1, 1)) * rng.randint(1, n)
        for l in ((a, b), (-b, -a)):
            if l not in links:
                links.append(l)
    visits = [0] * n
    for p in paths:
        for e in p:
            visits[abs(e) - 1] += 1
    depths = [float(v) for v in visits]
    for u in range(n):
        x = rng.random()
        if x < 0.08:
            depths[u] = 0.0
        elif x < 0.16:
            depths[u] = visits[u] + 0.5
        elif x < 0.2:
            depths[u] = 1.0
    return dict(n=n, links=links, lens=lens, depths=depths, seqs=seqs, paths=paths, cw=cw)
