"""The model the clean tests hold the library to: `autocycler clean` (clean.rs:23-45) restated literally on a graph that keeps its four lists
per unitig (merge_util.MergeGraph).
  parse_tig_numbers            clean.rs:142-149
  check_tig_numbers_are_valid  :129-139
  remove_unitigs_by_number     unitig_graph.rs:588-592: retain, delete_dangling_links
  duplicate_unitig_by_number   :594-668 with check_if_unitig_can_be_duplicated, create_link's pushes at the end of the lists and both loops
                               over the target's own lists; new numbers start behind n (the highest number, alive or not), as in merge_util
  remove_low_depth_unitigs     :670-721: the reverse walk over `unitigs`, each decision against the lists as the deletions before it left them
  then                         merge_util (through finish_util.model_graph), finish_util.finish_model and finish_util.save_gfa, unedited
It shares no code with kernels_clean.inc or clean_host.cpp, and states no rule about rounds, neighbourhoods or where created links land: all of
that is read off the lists."""
import json
import math

import finish_util as F
import merge_util as M
from apply_util import create_link, get_links_for_gfa, signed

GOLDEN = M.GOLDEN
KEPT, REMOVED, DUPLICATED, LOW_DEPTH, KEPT_DEAD_END, ABSENT = range(6)
COLOUR_TYPES = {"steelblue": M.CONSENTIG, "forestgreen": M.ANCHOR, "pink": M.BRIDGE}


class CleanError(Exception):
    """quit_with_error, or a panic of the reference that the library reports as an error"""


def load_kats():
    return json.loads((GOLDEN / "clean_kats.json").read_text())


def parse_tig_numbers(text):
    if text is None:
        return []
    out = []
    for s in text.replace(" ", "").split(","):
        digits = s[1:] if s[:1] == "+" else s      # str::parse::<u32>
        if not digits or not all(c in "0123456789" for c in digits) or int(digits) > 0xFFFFFFFF:
            raise CleanError(f"failed to parse '{s}' as a node number")
        out.append(int(digits))
    return sorted(out)


def l_line_order(links):
    """the entries as save_gfa would print them for a graph that holds them in this order per list: unitigs ascending, forward before reverse"""
    return sorted(links, key=lambda l: (abs(l[0]), l[0] < 0))


def rebuild_index(graph):
    graph.unitig_index = {u.number: u for u in graph.unitigs}


def remove_unitigs_by_number(graph, to_remove):
    graph.unitigs = [u for u in graph.unitigs if u.number not in to_remove]
    M.delete_dangling_links(graph)
    rebuild_index(graph)


def duplicate_unitig_by_number(graph, unitig_num, n):
    if unitig_num not in graph.unitig_index:      # (the reference's unwrap panics)
        raise CleanError(f"unitig {unitig_num} no longer exists: it was removed or duplicated earlier in the same call")
    target = graph.unitig_index[unitig_num]
    if len([l for l in target.forward_next + target.reverse_next if l[0] != unitig_num]) != 2:
        raise CleanError(f"unitig {unitig_num} does not contain exactly two non-self links")
    a_num = max([n] + [u.number for u in graph.unitigs]) + 1
    b_num = a_num + 1
    for num in (a_num, b_num):
        copy = M.U.Unitig(num)
        copy.forward_seq, copy.depth, copy.unitig_type, copy.forward_positions, copy.reverse_positions = target.forward_seq, target.depth / 2.0, target.unitig_type, 0, 0
        copy.copy_of = unitig_num
        graph.unitigs.append(copy)
        graph.objects[num] = copy
    remove_unitigs_by_number(graph, {unitig_num})      # (the target keeps its own lists: it is no longer among graph.unitigs)
    for number, strand in target.forward_next:
        if number == unitig_num:
            create_link(graph, a_num, a_num if strand else -a_num)
            create_link(graph, b_num, b_num if strand else -b_num)
    for number, strand in target.reverse_next:
        if number == unitig_num:
            create_link(graph, -a_num, a_num if strand else -a_num)
            create_link(graph, -b_num, b_num if strand else -b_num)
    non_self_links = [(unitig_num, signed(l)) for l in target.forward_next if l[0] != unitig_num] + [(-unitig_num, signed(l)) for l in target.reverse_next if l[0] != unitig_num]
    assert len(non_self_links) == 2
    replace = lambda link, new: tuple(new if x == unitig_num else -new if x == -unitig_num else x for x in link)      # find_replace_i32_tuple
    create_link(graph, *replace(non_self_links[0], a_num))
    create_link(graph, *replace(non_self_links[1], b_num))
    check_links(graph)


def check_links(graph):
    """check_links (:752-793) in the form of its four link_exists questions"""
    for a in graph.unitigs:
        for lst, a_strand in ((a.forward_next, True), (a.reverse_next, False)):
            for b_num, b_strand in lst:
                b = graph.unitig_index[b_num]
                assert (a.number, a_strand) in (b.forward_prev if b_strand else b.reverse_prev)
                assert (a.number, not a_strand) in (b.reverse_next if b_strand else b.forward_next)


def remove_low_depth_unitigs(graph, min_depth):
    """-> the numbers of the low-depth unitigs that stayed"""
    stayed = []
    for idx in reversed(range(len(graph.unitigs))):
        if idx >= len(graph.unitigs):
            continue
        u = graph.unitigs[idx]
        if u.depth > min_depth:
            continue
        ok_to_delete = True
        for next_num, next_strand in list(u.forward_next):
            if next_num == u.number:
                continue
            next_u = graph.unitig_index[next_num]
            if not any(num != u.number for num, _ in (next_u.forward_prev if next_strand else next_u.reverse_prev)):
                ok_to_delete = False
                break
        if ok_to_delete:
            for prev_num, prev_strand in list(u.forward_prev):
                if prev_num == u.number:
                    continue
                prev_u = graph.unitig_index[prev_num]
                if not any(num != u.number for num, _ in (prev_u.forward_next if prev_strand else prev_u.reverse_next)):
                    ok_to_delete = False
                    break
        if not ok_to_delete:
            stayed.append(u.number)
            continue
        graph.unitigs = [x for x in graph.unitigs if x.number != u.number]
        M.delete_dangling_links(graph)
        rebuild_index(graph)
    return stayed


def clean_model(n, links, lens, depths=None, types=None, alive=None, seqs=None, remove=(), duplicate=(), min_depth=None, name="the graph"):
    """clean.rs:31-41 -> dict(n_out, len, alive, depth, type, copy_of, reason, links, seqs, graph)"""
    remove, duplicate = sorted(remove), sorted(duplicate)
    graph = M.MergeGraph(n, [(int(a), int(b)) for a, b in links], alive, seqs, lens, depths, types)
    for tig in list(remove) + list(duplicate):      # check_tig_numbers_are_valid, remove first
        if tig not in graph.unitig_index:
            raise CleanError(f"{name} does not contain tig {tig}")
    reason = [KEPT if u in graph.unitig_index else ABSENT for u in range(1, n + 1)]
    everyone = dict(graph.unitig_index)
    if remove:
        remove_unitigs_by_number(graph, set(remove))
        for tig in remove:
            reason[tig - 1] = REMOVED
    copies = []
    for tig in duplicate:
        duplicate_unitig_by_number(graph, tig, n)
        reason[tig - 1] = DUPLICATED
        copies += graph.unitigs[-2:]
    n_out = n + len(copies)
    assert [u.number for u in copies] == list(range(n + 1, n_out + 1))
    reason += [KEPT] * len(copies)
    for u in copies:
        everyone[u.number] = u
    if min_depth is not None:
        before = {u.number for u in graph.unitigs}
        for tig in remove_low_depth_unitigs(graph, min_depth):
            reason[tig - 1] = KEPT_DEAD_END
        for tig in before - {u.number for u in graph.unitigs}:
            reason[tig - 1] = LOW_DEPTH
    depth_in = [float(depths[u]) if depths is not None else 0.0 for u in range(n)]
    type_in = [int(types[u]) if types is not None else M.OTHER for u in range(n)]
    return dict(n_out=n_out, len=[int(x) for x in lens] + [len(u.forward_seq) for u in copies], alive=[int(u in graph.unitig_index) for u in range(1, n_out + 1)],
                depth=depth_in + [u.depth for u in copies], type=type_in + [u.unitig_type for u in copies], copy_of=[0] * n + [u.copy_of for u in copies], reason=reason,
                links=get_links_for_gfa(graph), graph=graph, seqs=[everyone[u].forward_seq if u in everyone else b"" for u in range(1, n_out + 1)])


def cleaned_text(exp, k, use_other_colour=True):
    """save_gfa of the graph as the edits leave it, before the merge"""
    unitigs = [(u.number, u.number, u.forward_seq, u.depth, u.unitig_type) for u in exp["graph"].unitigs]
    return F.save_gfa(dict(unitigs=unitigs, links=exp["links"]), k, (), use_other_colour)


def merged_model(exp):
    """merge_graph (clean.rs:111-117): merge_linear_paths(graph, &vec![]), renumber_unitigs -> finish_model's dict"""
    graph, _ = F.model_graph(exp["n_out"], exp["links"], exp["len"], exp["alive"], (), exp["depth"], None, None, exp["type"], exp["seqs"])
    return F.finish_model(graph, exp["n_out"], True)[0]


def final_text(exp, k):
    """save_gfa(out, &vec![], true)"""
    return F.save_gfa(merged_model(exp), k, (), True)


def is_multiset(exp):
    return len(set(exp["links"])) != len(exp["links"])


def read_gfa(text):
    """a GFA text whose segments are numbered 1, 2, 3, ...: the arguments of clean_model and k (0 without KM:i)"""
    seqs, depths, types, links, k = [], [], [], [], 0
    for line in (text.decode() if isinstance(text, bytes) else text).splitlines():
        p = line.split("\t")
        if p[0] == "H":
            k = max([int(t[5:]) for t in p if t.startswith("KM:i:")] + [0])
        elif p[0] == "S":
            assert int(p[1]) == len(seqs) + 1
            seqs.append(p[2].encode())
            depths.append(float([t for t in p[3:] if t.startswith("DP:f:")][0][5:]))
            types.append(next((COLOUR_TYPES[c] for c in ("steelblue", "forestgreen", "pink") if f"CL:Z:{c}" in p), M.OTHER))
        elif p[0] == "L":
            links.append((int(p[1]) * (1 if p[2] == "+" else -1), int(p[3]) * (1 if p[4] == "+" else -1)))
    return dict(n=len(seqs), links=l_line_order(links), lens=[len(s) for s in seqs], depths=depths, types=types, seqs=seqs), k


def clean_text_model(text, remove=None, duplicate=None, min_depth=None, name="the graph"):
    """clean.rs:27-43 from text to text"""
    rm, dup = parse_tig_numbers(remove), parse_tig_numbers(duplicate)
    g, k = read_gfa(text)
    return final_text(clean_model(remove=rm, duplicate=dup, min_depth=min_depth, name=name, **g), k)


# ---- the library's result in the model's form ----------------------------------------------------------------------------------------------
def assert_same(cl, exp, what=""):
    import numpy as np
    assert cl.n_out == exp["n_out"], (what, "n_out")
    for key in ("len", "alive", "type", "copy_of", "reason"):
        assert getattr(cl, key).tolist() == exp[key], (what, key, getattr(cl, key).tolist(), exp[key])
    assert cl.depth.tobytes() == np.asarray(exp["depth"], dtype=np.float64).tobytes(), (what, "depth", cl.depth.tolist(), exp["depth"])      # bit for bit
    assert [tuple(l) for l in cl.links.tolist()] == exp["links"], (what, "links", cl.links.tolist(), exp["links"])
    sm = cl.summary
    assert sm["links_out"] == len(exp["links"]) and sm["unitigs_out"] == exp["n_out"], what
    for code, key in ((KEPT, "kept"), (REMOVED, "removed"), (DUPLICATED, "duplicated"), (LOW_DEPTH, "low_depth"), (KEPT_DEAD_END, "kept_dead_end"), (ABSENT, "absent")):
        assert sm[key] == exp["reason"].count(code), (what, key)


def cleaned_bytes(cl):
    """every product as bytes (two runs: identical, not merely equal as values)"""
    return b"|".join([cl.len.tobytes(), cl.alive.tobytes(), cl.depth.tobytes(), cl.type.tobytes(), cl.copy_of.tobytes(), cl.reason.tobytes(), cl.links.tobytes(),
                      b"" if cl.seq_begin is None else cl.seq_begin.tobytes(),
                      repr(sorted((k, v) for k, v in cl.summary.items() if k not in ("launches", "read_backs", "seconds_device"))).encode()])


def has_nan_alive(exp):
    return any(math.isnan(d) and a for d, a in zip(exp["depth"], exp["alive"]))
