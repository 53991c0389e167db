"""The model the combine tests hold the library to: `autocycler combine` (combine.rs:107-127, 144-224) and `autocycler gfa2fasta`
(gfa2fasta.rs:56-83) restated literally in plain Python on graphs that keep their four lists per unitig.
  from_gfa_text            UnitigGraph::from_gfa_file as combine uses it: S lines in file order, the index by number (the last of a repeated
                           number wins), L lines attached in file order, an L line naming a missing segment dropped, P lines ignored
  load_clusters            the stable sort by Reverse(total_length())
  combine_clusters         the loop with its running offset over lists: the GFA, the FASTA, the metrics
  get_links_for_gfa, topology, link_count, the end tests, cluster_depth, read_depth_value, the yaml, gfa2fasta
It shares no code with kernels_combine.inc or combine_host.cpp and states nothing about ranks, prefix sums or sort keys: the order of
everything is read off the lists."""
import json
import math
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
OTHER, ANCHOR, CONSENTIG, BRIDGE = range(4)
COLOURS = {CONSENTIG: "steelblue", ANCHOR: "forestgreen", BRIDGE: "pink", OTHER: "orangered"}
TYPE_OF_COLOUR = {"steelblue": CONSENTIG, "forestgreen": ANCHOR, "pink": BRIDGE}
U32 = 0xFFFFFFFF


class CombineError(Exception):
    """quit_with_error, or a panic / silent wrap of the reference that the library reports as an error"""


def load_kats():
    return json.loads((GOLDEN / "combine_kats.json").read_text())


class Unitig:
    def __init__(self, number, seq, depth, unitig_type=OTHER):
        self.number, self.seq, self.depth, self.unitig_type = number, seq, depth, unitig_type
        self.read_depth = None
        self.forward_next, self.forward_prev, self.reverse_next, self.reverse_prev = [], [], [], []      # entries: (unitig, strand)

    def length(self):
        return len(self.seq)

    def open_start(self):
        return not self.reverse_next

    def open_end(self):
        return not self.forward_next

    def hairpin_start(self):
        return len(self.reverse_next) == 1 and self.reverse_next[0][1] and self.reverse_next[0][0].number == self.number

    def hairpin_end(self):
        return len(self.forward_next) == 1 and not self.forward_next[0][1] and self.forward_next[0][0].number == self.number

    def is_isolated_and_circular(self):
        if len(self.forward_next) != 1 or len(self.forward_prev) != 1:
            return False
        (n, ns), (p, ps) = self.forward_next[0], self.forward_prev[0]
        return n.number == self.number and ns and p.number == self.number and ps

    def is_isolated_and_linear(self):
        if len(self.forward_next) > 1 or len(self.forward_prev) > 1:
            return False
        if self.is_isolated_and_circular():
            return False
        return (all(u.number == self.number and not s for u, s in self.forward_next) and all(u.number == self.number and not s for u, s in self.forward_prev) and
                all(u.number == self.number and s for u, s in self.reverse_next) and all(u.number == self.number and s for u, s in self.reverse_prev))

    def colour_tag(self):
        return "\tCL:Z:" + COLOURS[self.unitig_type]


class Graph:
    def __init__(self):
        self.unitigs, self.unitig_index = [], {}

    def total_length(self):
        return sum(u.length() for u in self.unitigs)

    def max_unitig_number(self):
        return max((u.number for u in self.unitigs), default=0)

    def link_count(self):
        all_links, one_way = set(), set()
        for a in self.unitigs:
            for lst, a_num in ((a.forward_next, a.number), (a.reverse_next, -a.number)):
                for b, strand in lst:
                    b_num = b.number if strand else -b.number
                    link, rev = (a_num, b_num), (-b_num, -a_num)
                    all_links.add(link); all_links.add(rev)
                    one_way.add(max(link, rev))
        return len(all_links), len(one_way)

    def topology(self):
        if not self.unitigs:
            return "empty"
        if len(self.unitigs) > 1:
            return "fragmented"
        u = self.unitigs[0]
        if self.link_count()[0] == 0:
            return "linear-open-open"
        if u.is_isolated_and_circular():
            return "circular"
        if u.hairpin_start() and u.hairpin_end():
            return "linear-hairpin-hairpin"
        if u.hairpin_start() and u.open_end():
            return "linear-open-hairpin"
        if u.open_start() and u.hairpin_end():
            return "linear-open-hairpin"
        return "other"

    def get_links_for_gfa(self, offset):
        links = []
        for a in self.unitigs:
            for b, strand in a.forward_next:
                links.append((str(a.number + offset), "+", str(b.number + offset), "+" if strand else "-"))
            for b, strand in a.reverse_next:
                links.append((str(a.number + offset), "-", str(b.number + offset), "+" if strand else "-"))
        return links


def from_gfa_text(text):
    """-> Graph; keeps per S line what the array forms need (file order)"""
    if isinstance(text, bytes):
        text = text.decode()
    g = Graph()
    link_lines = []
    for line in text.split("\n"):
        parts = line.split("\t")
        if parts[0] == "S":
            depth = next(float(p[5:]) for p in parts if p.startswith("DP:f:"))
            t = next((TYPE_OF_COLOUR[c] for c in ("steelblue", "forestgreen", "pink") if "CL:Z:" + c in parts), OTHER)
            g.unitigs.append(Unitig(int(parts[1]), parts[2].encode(), depth, t))
        elif parts[0] == "L":
            link_lines.append(parts)
    g.unitig_index = {u.number: u for u in g.unitigs}
    g.dropped_links, g.file_links = 0, []      # file_links: the kept L lines in file order, for the array form only
    for parts in link_lines:
        assert parts[5] == "0M"
        a, b = g.unitig_index.get(int(parts[1])), g.unitig_index.get(int(parts[3]))
        sa, sb = parts[2] == "+", parts[4] == "+"
        if a is None or b is None:
            g.dropped_links += 1
            continue
        (a.forward_next if sa else a.reverse_next).append((b, sb))
        (b.forward_prev if sb else b.reverse_prev).append((a, sa))
        g.file_links.append((a, sa, b, sb))
    return g


def array_form(g):
    """a model graph as ac_combine_graphs takes it: numbers, lengths, depths, types, sequences, and the kept L lines in FILE order as signed
    1-based file-order indices (the index of a repeated number's last S line, as the reference's index has it)"""
    index = {id(u): i + 1 for i, u in enumerate(g.unitigs)}
    links = [(index[id(a)] if sa else -index[id(a)], index[id(b)] if sb else -index[id(b)]) for a, sa, b, sb in g.file_links]
    return dict(number=[u.number for u in g.unitigs], len=[u.length() for u in g.unitigs], depth=[u.depth for u in g.unitigs], type=[u.unitig_type for u in g.unitigs],
                seqs=[u.seq for u in g.unitigs], links=links)


def fixed(v, decimals):
    """Rust's {:.N}"""
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return format(v, f".{decimals}f")


def cluster_depth(graph):
    total, length = 0.0, 0
    for tig in graph.unitigs:
        if tig.read_depth is not None:
            total += tig.read_depth * float(tig.length())
            length += tig.length()
    return total / float(length) if length > 0 else None


def read_depth_value(depth):
    return "unavailable" if depth is None else float(fixed(depth, 1).replace("NaN", "nan"))


def yaml_value(v):
    """serde_yaml 0.9 of a string or an f64 (ryu: the shortest digits that read back, an exponent from 1e16 on)"""
    if isinstance(v, str):
        return v
    if math.isnan(v):
        return ".nan"
    if math.isinf(v):
        return ".inf" if v > 0 else "-.inf"
    return repr(v).replace("e+", "e")


def check_numbers(graphs):
    """what the reference would get silently wrong or panic on, in the library's order: a repeated number (lowest graph, then lowest number)"""
    for g, graph in enumerate(graphs):
        seen, twice = set(), []
        for u in graph.unitigs:
            if u.number in seen:
                twice.append(u.number)
            seen.add(u.number)
        if twice:
            raise CombineError(f"combine: graph {g}: unitig number {min(twice)} occurs more than once")


def load_clusters(graphs):
    """-> [(input index, graph)], the stable sort by Reverse(total_length())"""
    return sorted(enumerate(graphs), key=lambda ig: -ig[1].total_length())


def combine_clusters(clusters, read_depths):
    """combine.rs:144-224 -> (gfa text, fasta text, metrics dict, tigs); clusters: [(input index, graph)] in load_clusters' order"""
    gfa, fasta = ["H\tVN:Z:1.0\n"], []
    metrics = dict(consensus_assembly_bases=0, consensus_assembly_unitigs=0, consensus_assembly_fully_resolved=True, consensus_assembly_clusters=[])
    tigs, offset = [], 0
    for g, graph in clusters:
        component_length = graph.total_length()
        if offset + graph.max_unitig_number() > U32:
            raise CombineError(f"combine: graph {g}: offset {offset} + its highest unitig number {graph.max_unitig_number()} does not fit 32 bits")
        for unitig in graph.unitigs:
            num = unitig.number + offset
            seq = unitig.seq.decode()
            topology = " circular=true topology=circular" if unitig.is_isolated_and_circular() else " circular=false topology=linear" if unitig.is_isolated_and_linear() else ""
            depth = (unitig.read_depth if unitig.read_depth is not None else 0.0) if read_depths else unitig.depth
            depth_header = "" if not read_depths else f" depth={fixed(unitig.read_depth, 1)}" if unitig.read_depth is not None else " depth=unavailable"
            gfa.append(f"S\t{num}\t{seq}\tDP:f:{fixed(depth, 2)}{unitig.colour_tag()}\n")
            fasta.append(f">{num} length={unitig.length()}{depth_header}{topology}\n{seq}\n")
            tigs.append((num, unitig.length(), unitig.read_depth))
        for a, sa, b, sb in graph.get_links_for_gfa(offset):
            gfa.append(f"L\t{a}\t{sa}\t{b}\t{sb}\t0M\n")
        offset += graph.max_unitig_number()
        metrics["consensus_assembly_bases"] += component_length
        metrics["consensus_assembly_unitigs"] += len(graph.unitigs)
        metrics["consensus_assembly_clusters"].append(dict(length=component_length, unitigs=len(graph.unitigs), topology=graph.topology(),
                                                           read_depth=read_depth_value(cluster_depth(graph))))
        if len(graph.unitigs) != 1:
            metrics["consensus_assembly_fully_resolved"] = False
    return "".join(gfa).encode(), "".join(fasta).encode(), metrics, tigs


def metrics_yaml(metrics):
    y = [f"consensus_assembly_bases: {metrics['consensus_assembly_bases']}\n", f"consensus_assembly_unitigs: {metrics['consensus_assembly_unitigs']}\n",
         f"consensus_assembly_fully_resolved: {'true' if metrics['consensus_assembly_fully_resolved'] else 'false'}\n", "consensus_assembly_clusters:\n"]
    for c in metrics["consensus_assembly_clusters"]:
        y += [f"- length: {c['length']}\n", f"  unitigs: {c['unitigs']}\n", f"  topology: {c['topology']}\n", f"  read_depth: {yaml_value(c['read_depth'])}\n"]
    return "".join(y).encode()


def depth_lines(tigs, read_depths):
    if not read_depths:
        return b""
    return ("Sequence depths:\n" + "".join(f"  {n} length={l} depth={fixed(d, 1) if d is not None else 'unavailable'}\n" for n, l, d in tigs)).encode()


def combine_model(graphs, read_depths=None):
    """graphs: model Graphs in command-line order; read_depths: None, or one list per graph (None = no depth) -> dict of everything"""
    if not graphs:
        raise CombineError("combine: at least one graph is required")
    check_numbers(graphs)
    for graph, rd in zip(graphs, read_depths or [None] * len(graphs)):
        for i, u in enumerate(graph.unitigs):
            u.read_depth = rd[i] if rd is not None else None
    clusters = load_clusters(graphs)
    gfa, fasta, metrics, tigs = combine_clusters(clusters, read_depths is not None)
    # what the object's accessors hold, read off the same loop
    cluster_records, unitig_records, links, offset = [], [], [], 0
    for g, graph in clusters:
        cd = cluster_depth(graph)
        cluster_records.append(dict(input_index=g, unitigs=len(graph.unitigs), length=graph.total_length(), links=len(graph.get_links_for_gfa(0)), offset=offset,
                                    max_number=graph.max_unitig_number(), topology=graph.topology(), has_read_depth=cd is not None, read_depth=cd if cd is not None else 0.0))
        for i, u in enumerate(graph.unitigs):
            flags = (1 * u.open_start() + 2 * u.open_end() + 4 * bool(u.hairpin_start()) + 8 * bool(u.hairpin_end()) + 16 * bool(u.is_isolated_and_circular()) +
                     32 * bool(u.is_isolated_and_linear()))
            unitig_records.append(dict(graph=g, index=i, number=u.number + offset, length=u.length(),
                                       depth=((u.read_depth if u.read_depth is not None else 0.0) if read_depths is not None else u.depth),
                                       has_read_depth=u.read_depth is not None, read_depth=u.read_depth if u.read_depth is not None else 0.0, flags=flags, type=u.unitig_type))
        for a, sa, b, sb in graph.get_links_for_gfa(offset):
            links.append((int(a) if sa == "+" else -int(a), int(b) if sb == "+" else -int(b)))
        offset += graph.max_unitig_number()
    return dict(gfa=gfa, fasta=fasta, yaml=metrics_yaml(metrics), metrics=metrics, tigs=tigs, depth_lines=depth_lines(tigs, read_depths is not None),
                clusters=cluster_records, unitigs=unitig_records, links=links)


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def assert_same(combined, exp, names, what=""):
    """a Combined against combine_model's dict, field by field (floats bit for bit); names: TOPOLOGY_NAMES"""
    assert len(combined.clusters) == len(exp["clusters"]), (what, "clusters")
    for c, e in zip(combined.clusters, exp["clusters"]):
        got = dict(input_index=int(c["input_index"]), unitigs=int(c["unitigs"]), length=int(c["length"]), links=int(c["links"]), offset=int(c["offset"]),
                   max_number=int(c["max_number"]), topology=names[int(c["topology"])], has_read_depth=bool(c["has_read_depth"]))
        assert got == {k: v for k, v in e.items() if k != "read_depth"}, (what, got, e)
        assert same_float(float(c["read_depth"]), e["read_depth"]), (what, "cluster depth", float(c["read_depth"]), e["read_depth"])
    assert len(combined.unitigs) == len(exp["unitigs"]), (what, "unitigs")
    for u, e in zip(combined.unitigs, exp["unitigs"]):
        got = dict(graph=int(u["graph"]), index=int(u["index"]), number=int(u["number"]), length=int(u["length"]), has_read_depth=bool(u["has_read_depth"]),
                   flags=int(u["flags"]), type=int(u["type"]))
        assert got == {k: v for k, v in e.items() if k not in ("depth", "read_depth")}, (what, got, e)
        assert same_float(float(u["depth"]), e["depth"]) and same_float(float(u["read_depth"]), e["read_depth"]), (what, "depths", u, e)
    assert [tuple(l) for l in combined.links.tolist()] == exp["links"], (what, "links")
    s, m = combined.summary, exp["metrics"]
    assert (s["bases"], s["unitigs"], s["fully_resolved"], s["graphs"], s["links"]) == (m["consensus_assembly_bases"], m["consensus_assembly_unitigs"],
                                                                                     m["consensus_assembly_fully_resolved"], len(exp["clusters"]), len(exp["links"])), (what, s, m)


def combined_bytes(c):
    return c.clusters.tobytes() + c.unitigs.tobytes() + c.links.tobytes()


def gfa2fasta_model(text):
    """save_graph_to_fasta (gfa2fasta.rs:56-83) -> (fasta bytes, (circular, linear, other))"""
    graph = from_gfa_text(text)
    out, circ, lin, other = [], 0, 0, 0
    for u in graph.unitigs:
        if not u.seq:
            continue
        if u.is_isolated_and_circular():
            circ += 1; topology = " circular=true topology=circular"
        elif u.is_isolated_and_linear():
            lin += 1; topology = " circular=false topology=linear"
        else:
            other += 1; topology = ""
        out.append(f">{u.number} length={u.length()} depth={fixed(u.depth, 1)}{topology}\n{u.seq.decode()}\n")
    return "".join(out).encode(), (circ, lin, other)


def gfa_text(unitigs, links, header="H\tVN:Z:1.0\tKM:i:51"):
    """a cluster GFA: unitigs = [(number, seq bytes, depth text or float, colour or None)], links = [(a, b)] signed NUMBERS, one L line each"""
    lines = [header]
    for number, seq, depth, colour in unitigs:
        d = depth if isinstance(depth, str) else fixed(depth, 2)
        lines.append(f"S\t{number}\t{seq.decode()}\tDP:f:{d}" + (f"\tCL:Z:{colour}" if colour else ""))
    for a, b in links:
        lines.append(f"L\t{abs(a)}\t{'+' if a > 0 else '-'}\t{abs(b)}\t{'+' if b > 0 else '-'}\t0M")
    return ("\n".join(lines) + "\n").encode()
