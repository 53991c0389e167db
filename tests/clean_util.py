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
that is read off the lists.  The literal walk rebuilds the unitig list, the index and every list per deletion and is quadratic; clean_model_fast
makes the same decisions in the same order on lists edited in place, for the sizes the literal one cannot afford, and is held equal to it on
every case the literal one can."""
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


# ---- the same decisions on lists that are edited in place --------------------------------------------------------------------------------------
class FastUnitig:
    """one unitig of clean_model_fast: what Unitig holds, and whether it is still among `unitigs`"""
    __slots__ = ("number", "forward_seq", "depth", "unitig_type", "copy_of", "here", "forward_next", "forward_prev", "reverse_next", "reverse_prev")

    def __init__(self, number, forward_seq, depth, unitig_type, copy_of=0):
        self.number, self.forward_seq, self.depth, self.unitig_type, self.copy_of, self.here = number, forward_seq, depth, unitig_type, copy_of, True
        self.forward_next, self.forward_prev, self.reverse_next, self.reverse_prev = [], [], [], []

    def lists(self):
        return (self.forward_next, self.forward_prev, self.reverse_next, self.reverse_prev)


class FastGraph:
    """what cleaned_text reads of a graph: `unitigs` in their order"""

    def __init__(self, unitigs):
        self.unitigs = unitigs


def _take_out(by_number, u):
    """retain + delete_dangling_links for one unitig: it leaves `unitigs` with its own lists as they are (nobody walks them again but
    duplicate_unitig_by_number, which wants them so), and every list that names it loses those entries, the others keeping their order"""
    u.here = False
    for num in {e[0] for lst in u.lists() for e in lst if e[0] != u.number}:
        for lst in by_number[num].lists():
            if any(e[0] == u.number for e in lst):
                lst[:] = [e for e in lst if e[0] != u.number]


def _push_link(by_number, start_num, end_num):
    """create_link: both directions at the end of their lists, a link that is its own mirror image once"""
    for a, b in ((start_num, end_num),) if start_num == -end_num else ((start_num, end_num), (-end_num, -start_num)):
        start, end = by_number[abs(a)], by_number[abs(b)]
        (start.forward_next if a > 0 else start.reverse_next).append((abs(b), b > 0))
        (end.forward_prev if b > 0 else end.reverse_prev).append((abs(a), a > 0))


def clean_model_fast(n, links, lens, depths=None, types=None, alive=None, seqs=None, remove=(), duplicate=(), min_depth=None, name="the graph", counts=None):
    """clean_model's decisions in clean_model's order — the removals, the duplications ascending, the reverse walk over `unitigs` with the copies
    first, b before a — on alive flags and per-unitig lists edited in place: a decision costs the unitig's own and its neighbours' lists, not the
    graph.  Its only justification is that it equals clean_model wherever that one is affordable (test_clean_emu.py asserts it on every case at
    or below 4097 unitigs).  -> the same dict, `graph` holding `unitigs` alone; counts (a dict, optional) receives n_edit, the entries after the
    duplications, edited, those entries, and n_candidates, the unitigs the walk does not skip"""
    remove, duplicate = sorted(remove), sorted(duplicate)
    by_number = {}
    for u in range(1, n + 1):
        if alive is None or alive[u - 1]:
            by_number[u] = FastUnitig(u, bytes(seqs[u - 1]) if seqs is not None else b"N" * int(lens[u - 1]), float(depths[u - 1]) if depths is not None else 0.0,
                                      int(types[u - 1]) if types is not None else M.OTHER)
    for a, b in links:      # build_links_from_gfa: line order
        x, y = abs(int(a)), abs(int(b))
        if not (0 < x <= n and 0 < y <= n):
            raise ValueError(f"link refers to nonexistent unitig: {y if 0 < x <= n else x}")
        start, end = by_number.get(x), by_number.get(y)
        if start is not None and end is not None:
            (start.forward_next if a > 0 else start.reverse_next).append((y, b > 0))
            (end.forward_prev if b > 0 else end.reverse_prev).append((x, a > 0))
    for tig in remove + duplicate:
        if tig not in by_number:
            raise CleanError(f"{name} does not contain tig {tig}")
    reason = [KEPT if u in by_number else ABSENT for u in range(1, n + 1)]
    for tig in remove:
        if by_number[tig].here:
            _take_out(by_number, by_number[tig])
        reason[tig - 1] = REMOVED
    copies = []
    for tig in duplicate:
        target = by_number[tig]
        if not target.here:
            raise CleanError(f"unitig {tig} no longer exists: it was removed or duplicated earlier in the same call")
        if len([e for e in target.forward_next + target.reverse_next if e[0] != tig]) != 2:
            raise CleanError(f"unitig {tig} does not contain exactly two non-self links")
        a_num = n + len(copies) + 1      # (max + 1: the copies before this one are all still there)
        b_num = a_num + 1
        for num in (a_num, b_num):
            by_number[num] = FastUnitig(num, target.forward_seq, target.depth / 2.0, target.unitig_type, tig)
            copies.append(by_number[num])
        _take_out(by_number, target)
        for lst, sign in ((target.forward_next, 1), (target.reverse_next, -1)):
            for number, strand in lst:
                if number == tig:
                    _push_link(by_number, sign * a_num, a_num if strand else -a_num)
                    _push_link(by_number, sign * b_num, b_num if strand else -b_num)
        others = [(tig, x if s else -x) for x, s in target.forward_next if x != tig] + [(-tig, x if s else -x) for x, s in target.reverse_next if x != tig]
        for (start, end), new in zip(others, (a_num, b_num)):
            swap = lambda x: new if x == tig else -new if x == -tig else x
            _push_link(by_number, swap(start), swap(end))
        reason[tig - 1] = DUPLICATED
    n_out = n + len(copies)
    reason += [KEPT] * len(copies)
    walk = [by_number[u] for u in sorted(by_number) if by_number[u].here]      # `unitigs`: the originals ascending, then the copies
    if counts is not None:
        counts["edited"] = [(x, b if s else -b) for u in walk for x, lst in ((u.number, u.forward_next), (-u.number, u.reverse_next)) for b, s in lst]
        counts["n_edit"] = len(counts["edited"])
        counts["n_candidates"] = sum(1 for u in walk if not u.depth > min_depth) if min_depth is not None else 0
    if min_depth is not None:
        for u in reversed(walk):
            if u.depth > min_depth:
                continue
            ok_to_delete = True
            for mine, theirs in ((u.forward_next, ("forward_prev", "reverse_prev")), (u.forward_prev, ("forward_next", "reverse_next"))):
                for num, strand in mine:
                    if num == u.number:
                        continue
                    if not any(x != u.number for x, _ in getattr(by_number[num], theirs[0] if strand else theirs[1])):
                        ok_to_delete = False
                        break
                if not ok_to_delete:
                    break
            if ok_to_delete:
                _take_out(by_number, u)
                reason[u.number - 1] = LOW_DEPTH
            else:
                reason[u.number - 1] = KEPT_DEAD_END
    left = [u for u in walk if u.here]
    out_links = []
    for u in left:      # get_links_for_gfa
        out_links += [(u.number, b if s else -b) for b, s in u.forward_next]
        out_links += [(-u.number, b if s else -b) for b, s in u.reverse_next]
    depth_in = [float(depths[u]) if depths is not None else 0.0 for u in range(n)]
    type_in = [int(types[u]) if types is not None else M.OTHER for u in range(n)]
    return dict(n_out=n_out, len=[int(x) for x in lens] + [len(u.forward_seq) for u in copies], alive=[int(u in by_number and by_number[u].here) for u in range(1, n_out + 1)],
                depth=depth_in + [u.depth for u in copies], type=type_in + [u.unitig_type for u in copies], copy_of=[0] * n + [u.copy_of for u in copies], reason=reason,
                links=out_links, graph=FastGraph(left), seqs=[by_number[u].forward_seq if u in by_number else b"" for u in range(1, n_out + 1)])


def assert_models_equal(fast, literal, what=""):
    """every key but `graph`, of which the unitigs that are left and what save_gfa prints of them"""
    for key in ("n_out", "len", "alive", "type", "copy_of", "reason", "links", "seqs"):
        assert fast[key] == literal[key], (what, key)
    import numpy as np
    assert np.asarray(fast["depth"], dtype=np.float64).tobytes() == np.asarray(literal["depth"], dtype=np.float64).tobytes(), (what, "depth")
    of = lambda g: [(u.number, u.forward_seq, repr(u.depth), u.unitig_type) for u in g.unitigs]
    assert of(fast["graph"]) == of(literal["graph"]), (what, "unitigs")


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
