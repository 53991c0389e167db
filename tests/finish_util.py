"""The model the finished-graph tests hold the library to: the graph the reference holds after merge_linear_paths, kept WITH its lists — the
pushes of merge_path (graph_simplification.rs:410-485) and delete_dangling_links (unitig_graph.rs:547-564) as merge_util restates them — and
then, literally:
  the S order   graph.unitigs as merge_path's push and retain leave it
  renumber      renumber_unitigs (unitig_graph.rs:295-315): Python's stable sorted() with the reference's comparator
  the L lines   get_links_for_gfa (:333-350): per unitig in graph.unitigs order its forward_next, then its reverse_next
  the P lines   subset_util.model_merged_paths' position walk, relabelled
  the text      save_gfa (:317-360) with gfa_segment_line and colour_tag (unitig.rs:168-182)
The order of the lists is read off the lists; no rule about it is restated here.  It shares no code with kernels_finish.inc or finish_host.cpp;
merge_util and subset_util are imported, not edited."""
import functools

import numpy as np

import merge_util as M
import subset_util as S

COLOURS = {M.CONSENTIG: "steelblue", M.ANCHOR: "forestgreen", M.BRIDGE: "pink", M.OTHER: "orangered"}


def model_graph(n, links, lens, alive=None, path_ends=(), depths=None, fwd=None, rev=None, types=None, seqs=None):
    """merge_linear_paths exactly as merge_util.model_expected runs it, but the graph is kept: (graph, merge paths)"""
    graph = M.MergeGraph(n, [(int(a), int(b)) for a, b in links], alive, seqs, lens, depths, types, fwd, rev)
    fixed_starts, fixed_ends = M.get_fixed_unitig_starts_and_ends(graph, path_ends)
    M.fix_circular_loops(graph, fixed_starts)
    paths = M.find_merge_paths(graph, fixed_starts, fixed_ends)
    new_number = n
    for path in paths:
        new_number += 1
        M.merge_path(graph, path, new_number)
    M.delete_dangling_links(graph)
    graph.unitig_index = {u.number: u for u in graph.unitigs}
    return graph, paths


def reference_cmp(a, b):
    """the comparator of renumber_unitigs, clause for clause"""
    if len(a.forward_seq) != len(b.forward_seq):      # a.length().cmp(&b.length()).reverse()
        return -1 if len(a.forward_seq) > len(b.forward_seq) else 1
    if a.forward_seq != b.forward_seq:                # a.forward_seq.cmp(&b.forward_seq): bytewise
        return -1 if a.forward_seq < b.forward_seq else 1
    if a.depth > b.depth:                             # a.depth.partial_cmp(&b.depth).unwrap_or(Equal).reverse()
        return -1
    if a.depth < b.depth:
        return 1
    return 0


def finish_model(graph, n, renumber, merged_paths=None):
    """What is printed: dict(unitigs [(number, source, seq, depth, type)], new_of_old, links [(a, b)], paths {seq: [entries]}) and the
    coverage of the case.  merged_paths: {sequence: path over the numbers after the merge} or None"""
    order = list(graph.unitigs)      # after push and retain
    sources = [u.number for u in order]
    met = dict.fromkeys(COVERAGE, 0)
    merged = {u.number for u in order if u.number > n}
    for u in order:
        if u.number > n:
            met["merged_loop"] |= (u.number, M.FORWARD) in u.forward_next and (u.number, M.REVERSE) in u.reverse_next
            met["start_flip"] |= (u.number, M.FORWARD) in u.reverse_next
            met["end_flip"] |= (u.number, M.REVERSE) in u.forward_next
            met["chains_linked"] |= any(t in merged and t != u.number for t, _ in u.forward_next + u.reverse_next)
    if renumber:
        order = sorted(order, key=functools.cmp_to_key(reference_cmp))      # (stable, as sort_by is)
        for a, b in zip(order, order[1:]):
            if a.forward_seq == b.forward_seq:
                met["tie_by_depth" if a.depth != b.depth else "tie_by_order"] = 1
        seen_merged = False
        for u in order:
            met["merged_before_unmerged"] |= seen_merged and u.number <= n
            seen_merged |= u.number > n
    printed = {u.number: (i + 1 if renumber else u.number) for i, u in enumerate(order)}
    chains = max([n] + sources) - n      # (the chain numbers are n + 1 ... without gaps)
    new_of_old = [printed.get(s, 0) for s in range(1, n + chains + 1)]
    signed = lambda num, strand: printed[num] if strand else -printed[num]
    links = []      # get_links_for_gfa
    for a in order:
        for b in a.forward_next:
            links.append((printed[a.number], signed(*b)))
        for b in a.reverse_next:
            links.append((-printed[a.number], signed(*b)))
    paths = None
    if merged_paths is not None:
        paths = {s: [signed(abs(e), e > 0) for e in p] for s, p in merged_paths.items()}
    unitigs = [(printed[u.number], u.number, u.forward_seq, u.depth, u.unitig_type) for u in order]
    return dict(unitigs=unitigs, new_of_old=new_of_old, links=links, paths=paths), {k: int(v) for k, v in met.items()}


COVERAGE = ("merged_loop", "start_flip", "end_flip", "chain_from_minus", "chains_linked", "tie_by_depth", "tie_by_order", "merged_before_unmerged")


def save_gfa(model, k, metas=(), use_other_colour=False):
    """save_gfa's text.  metas: per P line (sequence index, id, length, filename, header, cluster tag), in the order of the lines"""
    out = [f"H\tVN:Z:1.0\tKM:i:{k}"]
    for number, _, seq, depth, utype in model["unitigs"]:
        tag = f"\tCL:Z:{COLOURS[utype]}" if utype != M.OTHER or use_other_colour else ""
        out.append(f"S\t{number}\t{seq.decode()}\tDP:f:{depth:.2f}{tag}")
    sg = lambda v: f"{abs(v)}\t{'+' if v > 0 else '-'}"
    out += [f"L\t{sg(a)}\t{sg(b)}\t0M" for a, b in model["links"]]
    for s, seq_id, length, filename, header, cluster in metas:
        path = ",".join(f"{abs(e)}{'+' if e > 0 else '-'}" for e in model["paths"][s])
        tag = f"\tCL:i:{cluster}" if cluster > 0 else ""
        out.append(f"P\t{seq_id}\t{path}\t*\tLN:i:{length}\tFN:Z:{filename}\tHD:Z:{header}{tag}")
    return ("\n".join(out) + "\n").encode()


# ---- the library's result in the model's form --------------------------------------------------------------------------------------------------
def library_model(fin, with_paths):
    seqs = fin.unitig_sequences()
    unitigs = [(int(u["number"]), int(u["source"]), seqs[i], float(u["depth"]), int(u["type"])) for i, u in enumerate(fin.unitigs)]
    sm = fin.summary
    assert sm["unitigs"] == len(unitigs) and sm["links"] == len(fin.links) and sm["bases"] == len(fin.sequences) and sm["path_entries"] == len(fin.path_entries)
    return dict(unitigs=unitigs, new_of_old=fin.new_of_old.tolist(), links=[tuple(l) for l in fin.links.tolist()], paths=fin.paths() if with_paths else None)


def assert_model_same(got, exp, what=""):
    for k in ("unitigs", "new_of_old", "links", "paths"):
        if k == "unitigs":      # depths bit for bit (0.0 and -0.0 apart, as the text would tell them)
            assert [(a, b, c, np.float64(d).tobytes(), e) for a, b, c, d, e in got[k]] == [(a, b, c, np.float64(d).tobytes(), e) for a, b, c, d, e in exp[k]], (what, k, got[k], exp[k])
        else:
            assert got[k] == exp[k], (what, k, got[k], exp[k])


def finished_bytes(fin):
    """every product as bytes (scheduling independence: identical, not merely equal as values)"""
    return b"|".join([fin.unitigs.tobytes(), fin.sequences.tobytes(), fin.new_of_old.tobytes(), fin.links.tobytes(), fin.path_seq.tobytes(), fin.path_off.tobytes(),
                      fin.path_entries.tobytes(),
                      repr(sorted((k, v) for k, v in fin.summary.items() if k not in ("launches", "read_backs", "seconds_device", "seconds_gather"))).encode()])


# ---- renumbering alone: unitigs without links, expected by sorted() -----------------------------------------------------------------------------
def expected_order(seqs, depths):
    """the places of unlinked unitigs 1..n after renumber_unitigs: a list of old numbers in new order"""
    class U:
        pass
    us = []
    for i, (s, d) in enumerate(zip(seqs, depths)):
        u = U()
        u.number, u.forward_seq, u.depth = i + 1, bytes(s), float(d)
        us.append(u)
    return [u.number for u in sorted(us, key=functools.cmp_to_key(reference_cmp))]


def expected_order_numpy(seqs, depths):
    """the same by numpy for equal-length byte strings given as an (n, L) uint8 array: lexsort is stable"""
    seqs = np.asarray(seqs, dtype=np.uint8)
    depths = np.asarray(depths, dtype=np.float64) + 0.0      # (-0.0 + 0.0 = 0.0)
    keys = [-depths] + [seqs[:, j] for j in range(seqs.shape[1] - 1, -1, -1)]
    return (np.lexsort(keys) + 1).tolist()
