"""ac_verify_graph (the round-trip verifier behind the ABI) — test bodies shared by the CPU suite (the emulation of the
same kernels) and the device suite: it accepts every oracle-equal graph, it accepts graphs reloaded from their GFA, and it names the
damage in graphs that were corrupted after the build (the result arrays of a handle are plain host memory: the tests write into them)."""
import numpy as np

import oracle_lib as O
import parity_util
import seqgen
from autocycler_amd import _capi, compress_build, graph_from_gfa

F_UNITIG, F_ORDER, F_LINK_RANGE, F_LINK_DUP, F_LINK_MIRROR, F_PATH_RANGE, F_PATH_STEP, F_PATH_LEN, F_SPELL, F_DEPTH, F_STATS = (1 << i for i in range(11))
F_LINK_ORDER, F_MAXIMAL, F_EXPAND = 2048, 4096, 8192                    # round 6: the order-sensitive guarantees
C_LINK_ORDER, C_LINK_ORDER_SEEDS, C_MAXIMAL, C_EXPAND = 1, 2, 4, 8      # report["checks"]: which of them ran


def build(lib_path, k, seqs, fn, hd, repair=True):
    s = O.Seqs.from_raw(k, seqs, filenames=fn, headers=hd, repair=repair)
    loaded = s.all()
    triples = [(q["fwd"], q["length"], q["id"]) for q in loaded]
    g = compress_build(k, max(1, len({q["filename"] for q in loaded})), triples, lib_path=lib_path)
    return g, triples, loaded


def accepts_oracle_equal_graphs(lib_path, ks=(5, 11, 51), seeds=range(12)):
    done = 0
    for k in ks:
        for seed in seeds:
            seqs, fn, hd = seqgen.make_case(seed, k)
            parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path).__getitem__(0).close()      # == the oracle, byte for byte
            g, triples, loaded = build(lib_path, k, seqs, fn, hd)
            rep = g.verify(triples)
            assert rep["failed"] == 0, (k, seed, rep)
            assert rep["checks"] == C_LINK_ORDER | C_LINK_ORDER_SEEDS | C_MAXIMAL | C_EXPAND, rep      # a built graph: all of them, with seed numbers
            assert rep["bases_checked"] == sum(t[1] for t in triples) and rep["unitigs"] == g.unitig_count
            # ... and the writing twin of the spelling check: every sequence decompressed on the device == the host's per-sequence form == the input
            dec = g.decompress_all()
            assert dec == [g.decompress(i) for i in range(len(triples))]
            assert dec == [bytes(t[0])[k // 2:k // 2 + t[1]] for t in triples]
            assert rep["path_entries"] == sum(g.path_counts())
            # the same graph reloaded from its GFA text (ac_graph_from_gfa: what `autocycler cluster` / `decompress` start from)
            gfa = g.gfa([q["filename"] for q in loaded], [q["header"] for q in loaded])
            g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)
            rep2 = g2.verify(triples)
            assert rep2["failed"] == 0, (k, seed, rep2)
            assert rep2["checks"] == C_LINK_ORDER | C_MAXIMAL | C_EXPAND, rep2      # a GFA holds no seed numbers
            g.close(); g2.close()
            done += 1
    return done


def names_the_damage(lib_path, k=21):
    """One flipped base, one dropped link, one swapped path entry and a few more: every corruption is reported with the
    right class, and the graph verifies again once the bytes are restored."""
    from autocycler_amd import synth
    seqs, fn, hd = [], [], []
    for i, contigs in enumerate(synth.make_assemblies(5, genome=30_000, plasmid=2_000, sub=2e-3, indel=2e-4, seed=23)):
        for header, s in contigs:
            seqs.append(s.tobytes().decode()); fn.append(f"assembly_{i:04d}.fasta"); hd.append(header)
    g, triples, _ = build(lib_path, k, seqs, fn, hd)
    b = g.bulk()
    assert g.verify(triples)["failed"] == 0
    U = g.unitig_count
    assert U > 50 and len(b["links"]) > 50 and len(b["path_entries"]) > 200
    for a in (b["seq_bytes"], b["seq_len"], b["depth"], b["links"], b["path_entries"]):
        a.setflags(write=True)

    plain = [bytes(t[0])[k // 2:k // 2 + t[1]] for t in triples]
    rank, block_size = {(int(l["a"]), int(l["b"])): i for i, l in enumerate(b["links"])}, None      # (a built handle: the size of its pooled block is not known)

    def check(expect, must_not=0):
        rep = g.verify(triples)
        detail = {}
        got, want = same_report(rep, M.verify(M.from_handle(g, b, block_size, rank), plain, k, detail), detail)
        assert got == want, (got, want)
        assert rep["failed"] & expect == expect, (bin(rep["failed"]), bin(expect))
        assert rep["failed"] & must_not == 0, (bin(rep["failed"]), bin(must_not))
        return rep

    # one flipped base in the longest unitig: the paths through it no longer spell their sequences
    pos = int(b["seq_begin"][0]) + int(b["seq_len"][0]) // 2
    old = int(b["seq_bytes"][pos])
    b["seq_bytes"][pos] = ord("A") if old != ord("A") else ord("C")
    rep = check(F_SPELL, must_not=F_LINK_MIRROR | F_PATH_STEP | F_DEPTH | F_PATH_LEN)
    assert rep["first_bad_base"] < sum(t[1] for t in triples)
    b["seq_bytes"][pos] = old
    assert g.verify(triples)["failed"] == 0
    # one dropped link (overwritten by its neighbour): a duplicate, a mirror without partner, and path steps that are no links any more
    used = {(int(x), int(y)) for p0, p1 in zip(b["path_off"][:-1], b["path_off"][1:]) for x, y in zip(b["path_entries"][int(p0):int(p1) - 1], b["path_entries"][int(p0) + 1:int(p1)])}
    li = next(i for i in range(len(b["links"]) - 1) if (int(b["links"][i]["a"]), int(b["links"][i]["b"])) in used)
    keep = b["links"][li].copy()
    b["links"][li] = b["links"][li + 1]
    rep = check(F_LINK_DUP | F_LINK_MIRROR | F_PATH_STEP, must_not=F_SPELL | F_DEPTH)
    assert rep["first_bad_link"] <= li + 1
    b["links"][li] = keep
    # a link that points beyond the graph
    keep_b = int(b["links"][3]["b"])
    b["links"][3]["b"] = U + 7
    check(F_LINK_RANGE)
    b["links"][3]["b"] = keep_b
    assert g.verify(triples)["failed"] == 0
    # two neighbouring path entries swapped (different unitigs): steps leave the links, the path spells something else
    po = b["path_off"]
    j = next(j for j in range(int(po[0]), int(po[1]) - 1) if abs(int(b["path_entries"][j])) != abs(int(b["path_entries"][j + 1])))
    x, y = int(b["path_entries"][j]), int(b["path_entries"][j + 1])
    b["path_entries"][j], b["path_entries"][j + 1] = y, x
    rep = check(F_PATH_STEP)
    assert rep["failed"] & (F_SPELL | F_PATH_LEN) and rep["first_bad_path_entry"] <= j + 1
    b["path_entries"][j], b["path_entries"][j + 1] = x, y
    # a path entry that names no unitig; a strand flipped
    b["path_entries"][j] = U + 1
    check(F_PATH_RANGE)
    b["path_entries"][j] = -x
    check(F_PATH_STEP | F_SPELL) if int(b["seq_len"][abs(x) - 1]) > 1 else check(F_PATH_STEP)
    b["path_entries"][j] = x
    # depth off by one; a unitig shortened (path lengths and the statistics no longer add up)
    b["depth"][5] += 1.0
    check(F_DEPTH, must_not=F_SPELL | F_PATH_STEP)
    b["depth"][5] -= 1.0
    b["seq_len"][0] -= 1
    check(F_PATH_LEN | F_STATS)
    b["seq_len"][0] += 1
    # renumber order: two unitigs of different length exchanged in the length table only
    if int(b["seq_len"][0]) != int(b["seq_len"][U - 1]):
        l0, l1 = int(b["seq_len"][0]), int(b["seq_len"][U - 1])
        b["seq_len"][0], b["seq_len"][U - 1] = l1, l0
        check(F_ORDER)
        b["seq_len"][0], b["seq_len"][U - 1] = l0, l1
    rep = g.verify(triples)
    assert rep["failed"] == 0, rep
    # the wrong sequences: same count and lengths, one base changed in the INPUT
    fwd = bytearray(triples[0][0]); mid = len(fwd) // 2
    fwd[mid] = ord("A") if fwd[mid] != ord("A") else ord("C")
    rep = g.verify([(bytes(fwd),) + triples[0][1:]] + triples[1:])
    assert rep["failed"] == F_SPELL and rep["first_bad_base"] == mid - k // 2
    g.close()


# ---- round 6: a unitig cut in two, a shift expand_repeats did not apply, L lines out of order -------------------------------------------
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


class _Gfa:
    """A compress-written GFA as lists the tests can edit (S: [sequence, tags], L: (a, a_strand, b, b_strand) signed pairs, P: [id, entries, tags])."""

    def __init__(self, text):
        self.header, self.segs, self.links, self.paths = "", [], [], []
        for line in text.split("\n"):
            f = line.split("\t")
            if f[0] == "H": self.header = line
            elif f[0] == "S": assert int(f[1]) == len(self.segs) + 1; self.segs.append([f[2], f[3:]])
            elif f[0] == "L": self.links.append(((int(f[1]) if f[2] == "+" else -int(f[1])), (int(f[3]) if f[4] == "+" else -int(f[3]))))
            elif f[0] == "P": self.paths.append([f[1], [(int(e[:-1]) if e[-1] == "+" else -int(e[:-1])) for e in f[2].split(",")], f[3:]])

    def text(self):
        sg = lambda v: f"{abs(v)}\t{'+' if v > 0 else '-'}"
        out = [self.header]
        out += [f"S\t{i + 1}\t{q}\t" + "\t".join(t) for i, (q, t) in enumerate(self.segs)]
        out += [f"L\t{sg(a)}\t{sg(b)}\t0M" for a, b in self.links]
        out += ["P\t" + pid + "\t" + ",".join(f"{abs(e)}{'+' if e > 0 else '-'}" for e in ents) + "\t" + "\t".join(t) for pid, ents, t in self.paths]
        return "\n".join(out) + "\n"

    def succ(self):
        nx = {}
        for a, b in self.links: nx.setdefault(a, []).append(b)
        return nx

    def strand_seq(self, v):
        q = self.segs[abs(v) - 1][0]
        return q if v > 0 else "".join(_COMP[c] for c in reversed(q))

    def depth(self, n):
        return float(next(t for t in self.segs[n - 1][1] if t.startswith("DP:f:"))[5:])

    def permute(self, order):
        """Renumbers consistently: order[i] = the OLD number of the unitig that becomes number i + 1 (S lines with their tags, L lines, paths)."""
        new = {old: i + 1 for i, old in enumerate(order)}
        sg = lambda v: new[v] if v > 0 else -new[-v]
        self.segs = [self.segs[old - 1] for old in order]
        self.links = [(sg(a), sg(b)) for a, b in self.links]
        for pth in self.paths: pth[1] = [sg(v) for v in pth[1]]

    def resort(self):
        """renumber_unitigs (unitig_graph.rs:295-315) on the edited graph: a stable sort by length descending, sequence, depth descending."""
        self.permute(sorted(range(1, len(self.segs) + 1), key=lambda n: (-len(self.segs[n - 1][0]), self.segs[n - 1][0], -self.depth(n))))

    def cut(self, u, h):
        """Unitig u keeps its first h bases, a new last unitig takes the rest; the links out of u's end and the paths follow."""
        q = self.segs[u - 1][0]; V = len(self.segs) + 1
        self.segs[u - 1][0] = q[:h]
        self.segs.append([q[h:], [next(t for t in self.segs[u - 1][1] if t.startswith("DP:f:"))]])
        self.links = [((V if a == u else a), (-V if bb == -u else bb)) for a, bb in self.links] + [(u, V), (-V, -u)]
        for pth in self.paths:
            pth[1] = [x for v in pth[1] for x in ((u, V) if v == u else (-V, -u) if v == -u else (v,))]

    def unshift(self, n, side, src):
        """One base of junction unitig n goes back to each of its exclusive sources: what one shift of expand_repeats had moved."""
        q = self.segs[n - 1][0]
        if side == 0:
            c, self.segs[n - 1][0] = q[0], q[1:]
            for p in src:
                if p > 0: self.segs[p - 1][0] += c
                else: self.segs[-p - 1][0] = _COMP[c] + self.segs[-p - 1][0]
        else:
            c, self.segs[n - 1][0] = q[-1], q[:-1]
            for p in src:
                if p > 0: self.segs[p - 1][0] = c + self.segs[p - 1][0]
                else: self.segs[-p - 1][0] += _COMP[c]

    def candidates(self):
        """(unitig number, side) that pass expand_repeats' static test (graph_simplification.rs:43-86, 190-280), restated on the GFA."""
        nx = self.succ()
        fixed_start, fixed_end = set(), set()
        for _, ents, _ in self.paths:
            (fixed_start if ents[0] > 0 else fixed_end).add(abs(ents[0]))
            (fixed_end if ents[-1] > 0 else fixed_start).add(abs(ents[-1]))
        fs0, fe0 = set(fixed_start), set(fixed_end)
        for u in fs0:
            for t in nx.get(-u, []): (fixed_end if -t > 0 else fixed_start).add(abs(t))
        for u in fe0:
            for t in nx.get(u, []): (fixed_start if t > 0 else fixed_end).add(abs(t))
        out = []
        for u in range(1, len(self.segs) + 1):
            ins = [-t for t in nx.get(-u, [])]
            if len(ins) >= 2 and u not in fixed_start and all(nx.get(p, []) == [u] and abs(p) != u and not ((p > 0 and abs(p) in fixed_end) or (p < 0 and abs(p) in fixed_start)) for p in ins):
                out.append((u, 0, ins))
            outs = list(nx.get(u, []))
            if len(outs) >= 2 and u not in fixed_end and all(nx.get(-q, []) == [-u] and abs(q) != u and not ((q > 0 and abs(q) in fixed_start) or (q < 0 and abs(q) in fixed_end)) for q in outs):
                out.append((u, 1, outs))
        return out


def names_order_sensitive_damage(lib_path, k=21):
    """one split unitig, one un-applied shift and one swapped L line are each reported with their own class."""
    from autocycler_amd import synth
    seqs, fn, hd = [], [], []
    for i, contigs in enumerate(synth.make_assemblies(5, genome=30_000, plasmid=2_000, sub=2e-3, indel=2e-4, seed=23)):
        for header, s in contigs:
            seqs.append(s.tobytes().decode()); fn.append(f"assembly_{i:04d}.fasta"); hd.append(header)
    g, triples, loaded = build(lib_path, k, seqs, fn, hd)
    fns, hds = [q["filename"] for q in loaded], [q["header"] for q in loaded]
    ALL = C_LINK_ORDER | C_LINK_ORDER_SEEDS | C_MAXIMAL | C_EXPAND
    rep = g.verify(triples)
    assert rep["failed"] == 0 and rep["checks"] == ALL, rep
    text = g.gfa(fns, hds)
    U = g.unitig_count

    def verify_text(t):
        g2, _, _ = graph_from_gfa(t, lib_path=lib_path)
        r = g2.verify(triples)
        g2.close()
        detail = {}
        got, want = same_report(r, M.verify(M.from_gfa(_Gfa(t)), [bytes(x[0])[k // 2:k // 2 + x[1]] for x in triples], k, detail), detail)
        assert got == want, (got, want)
        return r

    base = _Gfa(text)
    assert base.text() == text                                     # the editor round-trips the writer's bytes
    assert verify_text(text)["failed"] == 0
    # --- (iii) L lines: two neighbours of different groups, then two of one group, swapped in the handle's own array (seed numbers at hand)
    b = g.bulk()
    L = b["links"]; L.setflags(write=True)
    grp = lambda l: (abs(int(l["a"])), 0 if int(l["a"]) > 0 else 1)
    i_diff = next(i for i in range(len(L) - 1) if grp(L[i]) != grp(L[i + 1]))
    i_same = next(i for i in range(len(L) - 1) if grp(L[i]) == grp(L[i + 1]))
    for i in (i_diff, i_same):
        x, y = L[i].copy(), L[i + 1].copy()
        L[i], L[i + 1] = y, x
        rep = g.verify(triples)
        assert rep["failed"] == F_LINK_ORDER and rep["first_bad_link"] in (i, i + 1), (i, rep)      # the link SET is untouched: nothing else fires
        L[i], L[i + 1] = x, y
    assert g.verify(triples)["failed"] == 0
    # ... and in a GFA (no seed numbers): a forward_next list whose b- comes before its b+ (unitig_graph.rs:248-263)
    e = _Gfa(text)
    j = next(j for j in range(len(e.links) - 1) if e.links[j][0] == e.links[j + 1][0] and e.links[j][0] > 0 and e.links[j][1] > 0 > e.links[j + 1][1])
    e.links[j], e.links[j + 1] = e.links[j + 1], e.links[j]
    rep = verify_text(e.text())
    assert rep["failed"] == F_LINK_ORDER and not rep["checks"] & C_LINK_ORDER_SEEDS, rep
    # --- (i) one unitig cut in two: u keeps its first half, a new unitig U + 1 takes the rest, the links out of u's end and the paths follow
    e = _Gfa(text)
    depth_of = lambda tags: next(t for t in tags if t.startswith("DP:f:"))
    u = next(n for n in range(1, U + 1) if len(e.segs[n - 1][0]) >= 4 and all(abs(a) != n or abs(bb) != n for a, bb in e.links))
    q = e.segs[u - 1][0]; h = len(q) // 2; V = U + 1
    e.segs[u - 1][0] = q[:h]
    e.segs.append([q[h:], [depth_of(e.segs[u - 1][1])]])
    e.links = [((V if a == u else a), (-V if bb == -u else bb)) for a, bb in e.links] + [(u, V), (-V, -u)]
    for pth in e.paths:
        pth[1] = [x for v in pth[1] for x in ((u, V) if v == u else (-V, -u) if v == -u else (v,))]
    rep = verify_text(e.text())
    assert rep["failed"] & F_MAXIMAL and rep["checks"] & C_MAXIMAL, rep
    assert rep["failed"] & ~(F_MAXIMAL | F_ORDER | F_STATS) == 0, bin(rep["failed"])      # lossless and consistent all the same: what round 5 could not tell apart
    assert rep["failed"] & (F_SPELL | F_PATH_STEP | F_LINK_MIRROR | F_DEPTH | F_EXPAND) == 0
    # --- (ii) one shift un-applied: the first base of a junction unitig goes back to the end of each of its exclusive inputs (or the last one to the outputs)
    done = 0
    for want_side in (0, 1):
        e = _Gfa(text)
        cands = [(n, side, src) for n, side, src in e.candidates() if side == want_side and len(e.segs[n - 1][0]) >= 3 and len({abs(v) for v in src}) == len(src)]
        if not cands: continue
        n, side, src = cands[0]
        q = e.segs[n - 1][0]
        if side == 0:
            c, e.segs[n - 1][0] = q[0], q[1:]
            for p in src:
                if p > 0: e.segs[p - 1][0] += c
                else: e.segs[-p - 1][0] = _COMP[c] + e.segs[-p - 1][0]
        else:
            c, e.segs[n - 1][0] = q[-1], q[:-1]
            for p in src:
                if p > 0: e.segs[p - 1][0] = c + e.segs[p - 1][0]
                else: e.segs[-p - 1][0] += _COMP[c]
        rep = verify_text(e.text())
        assert rep["failed"] & F_EXPAND and rep["first_bad_junction"] == 2 * (n - 1) + side, (n, side, rep)
        assert rep["failed"] & ~(F_EXPAND | F_ORDER) == 0, bin(rep["failed"])      # every path still spells its sequence
        done += 1
    assert done == 2, "the test graph has no junction of one of the two kinds"
    g.close()


# ---- mutation sweeps: the whole report of every mutant against tests/verify_model.py -----------------------------------------------------
import random

import verify_model as M

_OTHER = {65: 67, 67: 71, 71: 84, 84: 65}      # A -> C -> G -> T -> A


def same_report(lib_rep, mod_rep, detail):
    """model == library over every decidable field.  The one relaxation: the L-line order names either member of the first out-of-order
    adjacent pair (never beyond the smallest link another class reports)."""
    lib = {f: lib_rep[f] for f in M.FIELDS}
    if mod_rep["failed"] & M.F_LINK_ORDER and lib["failed"] == mod_rep["failed"]:
        if lib["first_bad_link"] in {min(c, detail["link_min_other"]) for c in detail["order_pair"]}: lib["first_bad_link"] = mod_rep["first_bad_link"]
    return lib, mod_rep


class Sweep:
    """One graph handle — built, or reloaded from its GFA — whose result arrays the mutants are written into."""

    def __init__(self, lib_path, k, seqs, fn, hd, reload=False):
        self.k, self.lib_path = k, lib_path
        self.built, self.triples, loaded = build(lib_path, k, seqs, fn, hd)
        self.text = self.built.gfa([q["filename"] for q in loaded], [q["header"] for q in loaded])
        self.g = graph_from_gfa(self.text, lib_path=lib_path)[0] if reload else self.built
        self.plain = [bytes(t[0])[k // 2:k // 2 + t[1]] for t in self.triples]
        self.b = self.g.bulk()
        for a in self.b.values(): a.setflags(write=True)
        self.clean = {n: a.copy() for n, a in self.b.items()}
        self.block_size = len(self.b["seq_bytes"]) if reload else None
        # a reloaded handle holds its sequences in a block of exactly their size; a built one in a pooled block with slack behind them
        # (graph_impl / gfa_reader): only the first bounds a range that runs over the end by a few bytes, see lengths_family
        self.reload = reload
        self.rank = None if reload else {(int(l["a"]), int(l["b"])): i for i, l in enumerate(self.clean["links"])}
        self.U, self.n_links, self.n_ent, self.S = self.g.unitig_count, len(self.b["links"]), len(self.b["path_entries"]), len(self.triples)
        self.reports = []
        rep = self.g.verify(self.triples)
        assert rep["failed"] == 0 and self.model()["failed"] == 0, rep
        assert rep["checks"] == (13 if reload else 15)

    def model(self, plain=None, detail=None):
        return M.verify(M.from_handle(self.g, self.b, self.block_size, self.rank), plain or self.plain, self.k, detail)

    def mutant(self, label, triples=None, also=None):
        """The arrays hold a mutant now: model == library, then the bytes go back and the handle verifies clean again."""
        triples = triples or self.triples
        detail = {}
        mod = self.model([bytes(t[0])[self.k // 2:self.k // 2 + t[1]] for t in triples], detail)
        lib, want = same_report(self.g.verify(triples), mod, detail)
        assert lib == want, (label, {f: (lib[f], want[f]) for f in M.FIELDS if lib[f] != want[f]}, detail)
        if also: also(mod)
        self.reports.append((label, mod))
        for n, a in self.b.items(): a[...] = self.clean[n]
        assert self.g.verify(self.triples)["failed"] == 0, label
        return mod

    def close(self):
        if self.g is not self.built: self.g.close()
        self.built.close()


def _pick(r, n, count, edges=()):
    """count seeded positions below n, and the named edges among them"""
    out = [e for e in edges if 0 <= e < n]
    out += [r.randrange(n) for _ in range(count)] if n > 0 else []
    return list(dict.fromkeys(out))


def bases_family(h, r, count):
    """A flipped base of a unitig: first_bad_base is exact wherever the first wrong base of the job falls."""
    b = h.b
    pe, ln, bg = [int(x) for x in b["path_entries"]], [int(x) for x in b["seq_len"]], [int(x) for x in b["seq_begin"]]
    csum = [0]
    for p in pe: csum.append(csum[-1] + ln[abs(p) - 1])

    def flip(label, pos, expect_g=None):
        b["seq_bytes"][pos] = _OTHER.get(int(b["seq_bytes"][pos]), 65)
        mod = h.mutant(label)
        assert mod["failed"] & M.F_SPELL and (expect_g is None or mod["first_bad_base"] == expect_g), (label, mod, expect_g)

    for u in _pick(r, h.U, count, (0, h.U - 1)):
        flip("base:first", bg[u]); flip("base:last", bg[u] + ln[u] - 1)
    signs = {}
    for p in pe: signs.setdefault(abs(p) - 1, set()).add(p > 0)
    for u in [u for u in range(h.U) if signs.get(u) == {False}][:count]: flip("base:reverse-only", bg[u] + r.randrange(ln[u]))
    for u in [u for u in range(h.U) if ln[u] == 1][:count]: flip("base:1-base-unitig", bg[u])
    # the first wrong base of the job lies in the first path entry that names the unitig: choose it on a span edge / a sequence edge
    first_at = {}
    for j, p in enumerate(pe): first_at.setdefault(abs(p) - 1, j)
    sbase = [0]
    for t in h.triples: sbase.append(sbase[-1] + t[1])
    done = {0: 0, 31: 0}
    for u, j in sorted(first_at.items(), key=lambda x: x[1]):
        for m in (0, 31):
            within = (m - csum[j]) % 32
            if within < ln[u] and done[m] < count:
                flip(f"base:span-edge-{m}", bg[u] + (within if pe[j] > 0 else ln[u] - 1 - within), csum[j] + within); done[m] += 1
    po = [int(x) for x in b["path_off"]]
    for s in range(1, h.S):
        j0, j1 = po[s], po[s + 1] - 1
        if j1 < j0: continue
        if first_at[abs(pe[j0]) - 1] == j0:
            u = abs(pe[j0]) - 1; flip("base:sequence-start", bg[u] + (0 if pe[j0] > 0 else ln[u] - 1), sbase[s])
        if first_at[abs(pe[j1]) - 1] == j1:
            u = abs(pe[j1]) - 1; flip("base:sequence-end", bg[u] + (ln[u] - 1 if pe[j1] > 0 else 0), sbase[s + 1] - 1)


def _refuses(h, mod):
    """ac_decompress_device on paths that no longer add up: an error that names the model's first bad sequence, never bytes."""
    try:
        h.g.decompress_all()
    except _capi.AutocyclerError as e:
        assert "do not add up" in str(e) and f"(sequence {mod['first_bad_sequence'] + 1})" in str(e), (str(e), mod)
    else:
        raise AssertionError("decompress_all accepted paths that do not add up")


def lengths_family(h, r, count):
    """Lengths of 0 and +-1; on a reloaded handle (its block is exactly the sequences: the library bounds the copy by it) a begin pushed over
    the end.  A length + 1 stays inside the block."""
    b = h.b
    end = int((h.clean["seq_begin"] + h.clean["seq_len"]).max())
    for u in _pick(r, h.U, count, (0, h.U - 1)):
        b["seq_len"][u] = 0
        h.mutant("len:0", also=lambda mod: _refuses(h, mod))
        if int(b["seq_len"][u]) > 1:
            b["seq_len"][u] -= 1
            h.mutant("len:-1", also=lambda mod: _refuses(h, mod))
        if int(b["seq_begin"][u]) + int(b["seq_len"][u]) < end:
            b["seq_len"][u] += 1; h.mutant("len:+1", also=lambda mod: _refuses(h, mod))
    assert h.g.decompress_all() == h.plain
    if h.reload:
        last = int((h.clean["seq_begin"] + h.clean["seq_len"]).argmax())
        for u, push in [(last, 1), (last, 5)] + [(u, 2) for u in _pick(r, h.U, count)]:
            b["seq_begin"][u] += push
            mod = h.mutant("begin:pushed")
            assert u != last or mod["failed"] & M.F_UNITIG
        if last > 0:      # ... and longer than its predecessor as well: out of order by its length alone, whatever its range
            b["seq_begin"][last] += 1; b["seq_len"][last] = int(b["seq_len"][last - 1]) + 1
            mod = h.mutant("begin:pushed-and-longer")
            assert mod["failed"] & M.F_UNITIG and mod["failed"] & M.F_ORDER and mod["first_bad_unitig"] == last - 1, mod


def depth_family(h, r, count):
    b = h.b
    for u in _pick(r, h.U, count, (0, h.U - 1)):
        b["depth"][u] += 1.0; h.mutant("depth:+1")
        b["depth"][u] -= 1.0; h.mutant("depth:-1")
        b["depth"][u] = float("nan"); h.mutant("depth:nan")
    seq = lambda u: bytes(h.clean["seq_bytes"][int(b["seq_begin"][u]):int(b["seq_begin"][u]) + int(b["seq_len"][u])])
    for u in [u for u in range(h.U - 1) if seq(u) == seq(u + 1) and h.clean["depth"][u] != h.clean["depth"][u + 1]][:count]:
        b["depth"][u], b["depth"][u + 1] = h.clean["depth"][u + 1], h.clean["depth"][u]
        assert h.mutant("depth:exchanged")["failed"] == M.F_ORDER | M.F_DEPTH


def _links_damaged(h, r, count):
    L, n, U = h.b["links"], h.n_links, h.U
    for i in _pick(r, n - 1, count, (0, n - 2)):
        L[i] = L[i + 1]; h.mutant("link:overwritten-by-next")
        L[i + 1] = L[i]; h.mutant("link:overwritten-by-previous")
    combos = [(f, v) for f in "ab" for v in (0, U + 1, -(U + 1))]
    for t, i in enumerate(_pick(r, n, 2 * count, (0, n - 1))):
        for f, v in (combos[(2 * t) % 6], combos[(2 * t + 3) % 6]):      # (both ends, every value, in turn)
            L[i][f] = v; h.mutant(f"link:endpoint-{'0' if v == 0 else 'U+1'}")
    for i in _pick(r, n - 2, count, (0, n - 3)):
        L[i + 1] = L[i]; L[i + 2] = L[i]; h.mutant("link:triple")


def links_family(h, r, count, part=0):
    """The link SET damaged.  A link the clean graph does not hold has no place in a built graph's seed order, so those mutants run on the
    reloaded handle, where the order rule needs no seed numbers."""
    L, n, U = h.b["links"], h.n_links, h.U
    if n < 3: return
    if part == 0: return _links_damaged(h, r, count)
    for t, i in enumerate(_pick(r, n, 2 * count, (0, n - 1)) if h.reload else []):
        f = "ab"[t % 2]; L[i][f] = -int(L[i][f]); h.mutant("link:sign-flipped")
    mirrors = [i for i in range(n) if int(L[i]["a"]) == -int(L[i]["b"])]
    for i in mirrors[:count]:
        L[i] = L[i - 1] if i else L[i + 1]
        assert h.mutant("link:self-mirror-removed")["self_mirror_links"] == len(mirrors) - 1
    if h.reload:
        for i in _pick(r, n, count):
            if i in mirrors: continue
            L[i]["b"] = -int(L[i]["a"])
            assert h.mutant("link:self-mirror-added")["self_mirror_links"] == len(mirrors) + 1
        # a mirrored pair that no path uses becomes two self-mirror links: a link set that holds, one more link than the statistics say
        pe, po = h.clean["path_entries"], h.clean["path_off"]
        used = {(int(x), int(y)) for p0, p1 in zip(po[:-1], po[1:]) for x, y in zip(pe[int(p0):int(p1) - 1], pe[int(p0) + 1:int(p1)])}
        at = {(int(l["a"]), int(l["b"])): i for i, l in enumerate(h.clean["links"])}
        free = [(i, at[(-b_, -a_)]) for (a_, b_), i in at.items() if (a_, b_) not in used and (-b_, -a_) not in used and a_ != -b_
                and (a_, -a_) not in at and (-b_, b_) not in at and abs(a_) != abs(b_) and i < at[(-b_, -a_)]]
        for i, m in free[:2 * count]:
            L[i]["b"] = -int(L[i]["a"]); L[m]["b"] = -int(L[m]["a"])
            h.mutant("link:pair-to-self-mirrors")


def link_kinds_family(h, r, count):
    """Self-mirror links removed and added, signs flipped, a mirrored pair turned into two self-mirror links."""
    links_family(h, r, count, part=1)


def link_order_family(h, r, count):
    """The links permuted, the set kept: only the L-line order can fire."""
    L, n = h.b["links"], h.n_links
    grp = lambda i: (abs(int(h.clean["links"][i]["a"])), int(h.clean["links"][i]["a"]) < 0)
    same = [i for i in range(n - 1) if grp(i) == grp(i + 1)]
    diff = [i for i in range(n - 1) if grp(i) != grp(i + 1)]
    for i in _pick(r, n - 1, count, (n - 2,)) + r.sample(same, min(count, len(same))) + r.sample(diff, min(count, len(diff))):
        x, y = L[i].copy(), L[i + 1].copy()
        L[i], L[i + 1] = y, x
        mod = h.mutant("links:swapped-across" if grp(i) != grp(i + 1) else "links:swapped-within")
        assert mod["failed"] & ~M.F_LINK_ORDER == 0 and (mod["failed"] or h.reload), mod
    split = [i for i in range(n - 2) if grp(i) == grp(i + 1) != grp(i + 2)]
    for i in r.sample(split, min(count, len(split))):
        x = L[i].copy(); L[i] = L[i + 1]; L[i + 1] = L[i + 2]; L[i + 2] = x
        assert h.mutant("links:group-split")["failed"] == M.F_LINK_ORDER


def paths_family(h, r, count):
    P, U = h.b["path_entries"], h.U
    po = [int(x) for x in h.b["path_off"]]
    edges = [po[s] for s in range(h.S) if po[s] < po[s + 1]][:2] + [po[s + 1] - 1 for s in range(h.S) if po[s] < po[s + 1]][:2]
    for j in _pick(r, h.n_ent, count, edges):
        kinds = ((0, "0"), (U + 1, "U+1"), (-(U + 1), "U+1"), (-int(P[j]), "sign-flipped"))
        for v, name in (kinds[j % 4], kinds[(j + 1 + j // 4 % 3) % 4]):      # (two of the four per entry, in turn)
            P[j] = v; h.mutant(f"path:{name}")
        if j + 1 < h.n_ent and j % 2 == 0:
            P[j], P[j + 1] = int(P[j + 1]), int(P[j]); h.mutant("path:neighbours-swapped")


def path_off_family(h, r, count):
    """Offsets moved by one (two sequences no longer add up: the lower one is named), offsets that do not ascend from 0 (the early return).
    Every offset stays inside the entries."""
    O_ = h.b["path_off"]
    po = [int(x) for x in O_]
    for s in _pick(r, h.S - 1, count, (0, h.S - 2)):
        s += 1                                     # an interior offset
        if po[s] + 1 <= po[s + 1]:
            O_[s] = po[s] + 1
            assert h.mutant("path_off:+1", also=lambda mod: _refuses(h, mod))["first_bad_sequence"] == s - 1
        if po[s] - 1 >= po[s - 1]:
            O_[s] = po[s] - 1
            assert h.mutant("path_off:-1", also=lambda mod: _refuses(h, mod))["first_bad_sequence"] == s - 1
        if s >= 2 and po[s - 1] >= 1:
            O_[s] = po[s - 1] - 1
            mod = h.mutant("path_off:descending", also=lambda mod: _refuses(h, mod))
            assert mod["failed"] == M.F_PATH_LEN and mod["checks"] == 0 and mod["first_bad_sequence"] == s - 1, mod
    if po[1] >= 1:
        O_[0] = 1
        assert h.mutant("path_off:first-not-0", also=lambda mod: _refuses(h, mod))["first_bad_sequence"] == 0
    assert h.g.decompress_all() == h.plain


def inputs_family(h, r, count):
    """The graph untouched, the job's sequences changed: one base, or two sequences of one length exchanged."""
    k = h.k
    for s in _pick(r, h.S, count, (0, 1, h.S - 1)):
        n = h.triples[s][1]
        for pos, name in ((0, "start"), (n - 1, "end"), (r.randrange(n), "inside")):
            fwd = bytearray(h.triples[s][0]); fwd[k // 2 + pos] = _OTHER.get(fwd[k // 2 + pos], 65)
            mod = h.mutant(f"input:{name}", triples=h.triples[:s] + [(bytes(fwd),) + tuple(h.triples[s][1:])] + h.triples[s + 1:])
            assert mod["failed"] == M.F_SPELL and mod["first_bad_base"] == sum(t[1] for t in h.triples[:s]) + pos
    pairs = [(s, t) for s in range(h.S) for t in range(s + 1, h.S) if h.triples[s][1] == h.triples[t][1] and h.plain[s] != h.plain[t]]
    for s, t in pairs[:count]:
        tr = list(h.triples); tr[s], tr[t] = (h.triples[t][0],) + tuple(h.triples[s][1:]), (h.triples[s][0],) + tuple(h.triples[t][1:])
        assert h.mutant("input:exchanged", triples=tr)["failed"] == M.F_SPELL


# the named edges of the sweep: each must occur (sweep_coverage)
NAMED = ("base:first", "base:last", "base:reverse-only", "base:1-base-unitig", "base:span-edge-0", "base:span-edge-31", "base:sequence-start",
         "base:sequence-end", "len:0", "len:+1", "len:-1", "begin:pushed", "begin:pushed-and-longer", "depth:+1", "depth:-1", "depth:nan",
         "depth:exchanged", "link:overwritten-by-next", "link:overwritten-by-previous", "link:endpoint-0", "link:endpoint-U+1", "link:sign-flipped",
         "link:triple", "link:self-mirror-removed", "link:self-mirror-added", "link:pair-to-self-mirrors", "links:swapped-within",
         "links:swapped-across", "links:group-split", "path:0", "path:U+1", "path:sign-flipped", "path:neighbours-swapped", "path_off:+1",
         "path_off:-1", "path_off:descending", "path_off:first-not-0", "input:start", "input:end", "input:inside", "input:exchanged",
         "gfa:exchanged", "gfa:cut-path-start", "gfa:cut-path-end", "gfa:cut-reverse-only", "gfa:cut-hairpin", "gfa:cut-self-loop",
         "gfa:cut-every-position", "gfa:unshift", "gfa:l-order", "junction:dup", "junction:dup-clamped", "junction:short-source",
         "junction:source-of-2", "junction:beside-fixed-start", "junction:beside-fixed-end")


INPLACE = dict(bases=bases_family, lengths=lengths_family, depth=depth_family, links=links_family, link_kinds=link_kinds_family, link_order=link_order_family,
               paths=paths_family, path_off=path_off_family, inputs=inputs_family)


def gfa_family(h, r, count):
    """Edits a consistent writer could have made, reloaded with ac_graph_from_gfa; the model reads the EDITED GFA, not the handle."""
    reports = []

    def check(label, e):
        detail = {}
        mod = M.verify(M.from_gfa(e), h.plain, h.k, detail)
        g2 = graph_from_gfa(e.text(), lib_path=h.lib_path)[0]
        lib, want = same_report(g2.verify(h.triples), mod, detail)
        g2.close()
        assert lib == want, (label, {f: (lib[f], want[f]) for f in M.FIELDS if lib[f] != want[f]}, detail)
        reports.append((label, mod))
        return mod

    base = _Gfa(h.text)
    U = len(base.segs)
    assert check("gfa:unchanged", base)["failed"] == 0
    # two neighbours of one length exchanged, everything renumbered with them: the tie-breaks of the renumber order
    ties = [n for n in range(1, U) if len(base.segs[n - 1][0]) == len(base.segs[n][0])]
    for n in r.sample(ties, min(count, len(ties))):
        e = _Gfa(h.text); e.permute([m if m not in (n, n + 1) else 2 * n + 1 - m for m in range(1, U + 1)])
        assert check("gfa:exchanged", e)["failed"] & ~(M.F_ORDER | M.F_LINK_ORDER) == 0
    # a unitig cut in two, with and without the renumbering a writer would have applied afterwards
    pe = [v for _, ents, _ in base.paths for v in ents]
    starts = {abs(ents[0]) for _, ents, _ in base.paths}; ends = {abs(ents[-1]) for _, ents, _ in base.paths}
    rev_only = {abs(v) for v in pe} - {v for v in pe if v > 0}
    loops = {abs(a) for a, bb in base.links if a == bb}; hairpins = {abs(a) for a, bb in base.links if a == -bb}
    cuttable = [n for n in range(1, U + 1) if len(base.segs[n - 1][0]) >= 2]
    chosen = []
    for name, pool in (("path-start", starts), ("path-end", ends), ("reverse-only", rev_only), ("self-loop", loops), ("hairpin", hairpins), ("any", set(cuttable))):
        chosen += [(name, n) for n in [n for n in cuttable if n in pool][:count]]
    short = min(cuttable, key=lambda n: (len(base.segs[n - 1][0]) < 3, len(base.segs[n - 1][0])), default=None)
    for name, n in chosen + ([("every-position", short)] if short else []):
        q = base.segs[n - 1][0]
        for hh in (range(1, len(q)) if name == "every-position" else (r.randrange(1, len(q)),)):
            for resort in (False, True):
                e = _Gfa(h.text); e.cut(n, hh)
                if resort: e.resort()
                check(f"gfa:cut-{name}", e)
    # a shift of expand_repeats un-applied, on every candidate junction of both sides
    cands = base.candidates()
    if len(cands) > 12 * count: cands = r.sample(cands, 12 * count)      # (a small graph: every junction it offers)
    for n, side, src in cands:
        if len(base.segs[n - 1][0]) < 2: continue
        for resort in (False, True):
            e = _Gfa(h.text); e.unshift(n, side, src)
            if resort: e.resort()
            check("gfa:unshift-dup" if len({abs(v) for v in src}) != len(src) else "gfa:unshift", e)
    # the seed-free L-order rule: forward_next with a b- before a b+; reverse_next with a b+ behind the second run of a'-
    runs, i = [], 0
    while i < len(base.links):
        j = i
        while j < len(base.links) and base.links[j][0] == base.links[i][0]: j += 1
        runs.append((i, j)); i = j
    done = 0
    for i, j in runs:
        if j - i < 2 or done >= 3 * count: continue
        signs = [bb > 0 for _, bb in base.links[i:j]]
        orders = []
        if base.links[i][0] > 0 and True in signs and False in signs: orders.append(sorted(range(i, j), key=lambda x: base.links[x][1] > 0))      # b- first
        if base.links[i][0] < 0 and signs.count(True) >= 2 and False in signs:
            plus, minus = [x for x in range(i, j) if base.links[x][1] > 0], [x for x in range(i, j) if base.links[x][1] < 0]
            orders.append(plus[:1] + minus + plus[1:])
        orders.append(list(range(i + 1, j)) + [i])                       # rotated: for the model to decide
        for o in orders:
            e = _Gfa(h.text); e.links[i:j] = [base.links[x] for x in o]
            check("gfa:l-order", e); done += 1
    return reports


# The graphs.  small: the seqgen.make_case graphs (hairpins, self loops, palindromes, 1-base unitigs); synthetic: the 5 x 30 kbp graph of
# names_the_damage; large: more than one 2048-item tile of the scan and the sort the verifier calls, in U, links and path entries.
def _synthetic(n, genome, plasmid, sub, indel, seed):
    from autocycler_amd import synth
    seqs, fn, hd = [], [], []
    for i, contigs in enumerate(synth.make_assemblies(n, genome=genome, plasmid=plasmid, sub=sub, indel=indel, seed=seed)):
        for header, s in contigs:
            seqs.append(s.tobytes().decode()); fn.append(f"assembly_{i:04d}.fasta"); hd.append(header)
    return seqs, fn, hd


SMALL = [(5, 0), (5, 3), (11, 1), (11, 5), (21, 2), (21, 4)]      # (k, seqgen seed)
FAMILIES = list(INPLACE) + ["gfa", "junctions", "large"]
_done = {}


def sweep(lib_path, family):
    """Runs one family over its graphs (once per library: the coverage test reads the same reports) -> [(label, model report)]."""
    if (lib_path, family) in _done: return _done[(lib_path, family)]
    out = []
    both = (False, True)
    if family in ("bases", "paths"): both = (False,)                      # (the same arrays in either kind of handle)
    jobs = [(k, seqgen.make_case(seed, k), 2, 100 * k + seed, (True,) if family in ("links", "link_kinds") and i % 2 else both) for i, (k, seed) in enumerate(SMALL)]
    if family in ("bases", "lengths"):      # long unitigs and sequences (span edges, a block of some size): where its geometry matters
        jobs.append((21, _synthetic(5, 30_000, 2_000, 2e-3, 2e-4, 23), 0 if family == "lengths" else 1, 7, (True,) if family == "lengths" else (False,)))
    if family == "junctions":
        _done[(lib_path, family)] = junctions_family(lib_path)
        return _done[(lib_path, family)]
    if family == "large":      # the named edges of four families only: a few dozen mutants
        h = Sweep(lib_path, 21, *_synthetic(4, 40_000, 2_000, 1e-2, 1e-3, 31))
        assert h.U > 2048 and h.n_links > 2048 and h.n_ent > 2048, (h.U, h.n_links, h.n_ent)
        for f in ("links", "link_order"): INPLACE[f](h, random.Random(9), 0)
        P = h.b["path_entries"]
        for j, v in ((0, 0), (h.n_ent - 1, h.U + 1), (2049, -int(P[2049])), (int(h.b["path_off"][1]), -(h.U + 1))):
            P[j] = v; h.mutant("path:edge")
        h.close()
        _done[(lib_path, family)] = h.reports
        return h.reports
    for k, (seqs, fn, hd), count, seed, kinds in jobs:
        for reload in ((False,) if family in ("gfa", "inputs") else kinds):
            h = Sweep(lib_path, k, seqs, fn, hd, reload=reload)
            r = random.Random(seed)
            if family == "gfa": out += gfa_family(h, r, count)
            else:
                INPLACE[family](h, r, count); out += h.reports
            h.close()
    _done[(lib_path, family)] = out
    return out


def sweep_coverage(lib_path):
    """The sweep reaches what it claims, judged on the MODEL's reports.  With the seeds above (emulation build): 1130 mutants, 39 of them
    harmless.  Mutants per failed bit: 1: 60, 2: 197, 4: 88, 8: 102, 16: 212, 32: 53, 64: 240, 128: 234, 256: 181, 512: 171, 1024: 122,
    2048: 132, 4096: 168, 8192: 55.  The only bit set: 1 in 15 mutants, 2 in 7, 512 in 96, 1024 in 6, 2048 in 78, 4096 in 91, 8192 in 30.
    checks 0, 1, 3, 5, 7, 13 and 15 all occur, and every label of NAMED at least once (the rarest: junction:short-source, junction:source-of-2
    and junction:beside-fixed-start once each, junction:dup twice, base:sequence-end 3 times, gfa:cut-self-loop 4 times)."""
    reps = [rep for f in FAMILIES for _, rep in sweep(lib_path, f)]
    bits = {1 << i: sum(1 for m in reps if m["failed"] >> i & 1) for i in range(14)}
    alone = {f: sum(1 for m in reps if m["failed"] == f) for f in (1, 2, 512, 1024, 2048, 4096, 8192)}
    checks = {m["checks"] for m in reps}
    harmless = sum(1 for m in reps if m["failed"] == 0)
    summary = dict(mutants=len(reps), bits=bits, alone=alone, checks=sorted(checks), harmless=harmless)
    assert all(v >= 5 for v in bits.values()), summary
    assert all(v >= 1 for v in alone.values()), summary
    assert checks == {0, 1, 5, 13, 3, 7, 15}, summary      # none ran (early return); no seeds: order, + maximality, + fixed point; the same with seeds
    assert 4 * harmless <= len(reps), summary
    labels = {}
    for f in FAMILIES:
        for label, _ in sweep(lib_path, f): labels[label] = labels.get(label, 0) + 1
    for label in NAMED: assert labels.get(label, 0) >= 1, (label, labels)
    summary["labels"] = labels
    return summary


def device_text_equals_host(lib_path=None):
    """ac_verify_graph_device on damaged graphs: against a text resident on the device it returns the report ac_verify_graph returns."""
    import ctypes as C
    import torch
    k = 21
    seqs, fn, hd = seqgen.make_case(2, k)
    h = Sweep(lib_path, k, seqs, fn, hd)
    lib = _capi.load_library(lib_path)
    n = h.S
    views = (_capi.SeqView * n)()
    keep = [bytes(t[0]) for t in h.triples]
    for i, t in enumerate(h.triples): views[i].fwd, views[i].length, views[i].id = keep[i], t[1], t[2]
    lib.ac_text_size.restype = C.c_uint64
    n_text = lib.ac_text_size(C.c_uint32(k), views, C.c_uint32(n))
    text = np.empty(n_text, dtype=np.uint8)
    off = (C.c_uint64 * n)(); d1 = (C.c_uint16 * n)(); d2 = (C.c_uint16 * n)()
    assert lib.ac_layout_text(C.c_uint32(k), views, C.c_uint32(n), text.ctypes.data_as(C.c_void_p), off, d1, d2) == 0
    d_text = torch.from_numpy(text).to("cuda:0")
    lens = [t[1] for t in h.triples]
    b, U = h.b, h.U
    mutants = [lambda: b["seq_bytes"].__setitem__(int(b["seq_begin"][0]), _OTHER.get(int(b["seq_bytes"][int(b["seq_begin"][0])]), 65)),
               lambda: b["seq_len"].__setitem__(0, 0), lambda: b["seq_len"].__setitem__(U - 1, int(b["seq_len"][U - 1]) + 1),
               lambda: b["depth"].__setitem__(1, float("nan")), lambda: b["links"].__setitem__(0, b["links"][1]),
               lambda: b["links"]["b"].__setitem__(2, U + 1), lambda: b["links"]["a"].__setitem__(h.n_links - 1, 0),
               lambda: b["links"].__setitem__(slice(0, 2), b["links"][1::-1].copy()), lambda: b["path_entries"].__setitem__(0, 0),
               lambda: b["path_entries"].__setitem__(h.n_ent - 1, -int(b["path_entries"][h.n_ent - 1])),
               lambda: b["path_entries"].__setitem__(1, U + 1), lambda: b["path_off"].__setitem__(1, int(b["path_off"][1]) - 1),
               lambda: b["path_off"].__setitem__(0, 1)]
    if int(b["seq_begin"][U - 1]) + int(b["seq_len"][U - 1]) == len(b["seq_bytes"]): del mutants[2]      # (a length + 1 stays inside the block)
    assert len(mutants) >= 12
    failed = set()
    for m in mutants:
        m()
        host = h.g.verify(h.triples)
        dev = h.g.verify_device(d_text.data_ptr(), n_text, list(off), lens)
        assert {f: dev[f] for f in M.FIELDS} == {f: host[f] for f in M.FIELDS} and host["failed"], (host, dev)
        failed.add(host["failed"])
        for name, a in b.items(): a[...] = h.clean[name]
    assert h.g.verify_device(d_text.data_ptr(), n_text, list(off), lens)["failed"] == 0 and len(failed) >= 8
    h.close()


def junctions_family(lib_path, k=5):
    """Hand-made GFAs for the junction geometry no built graph offers on demand.  One sequence walks B+ J- X- J+ C+ D+ (another E+ D+): both strands of X
    lead to J+ and nowhere else (the `dup` divisor of avoid_zero_len_unitigs, graph_simplification.rs:152), B- and C+ are J's exclusive
    outputs.  The variants set the sources' lengths and facing bases, and add a second sequence that fixes a start or an end next to the
    junction.  A second graph holds a unitig with a self loop, cut at every position."""
    reports = []

    def graph(segs, links, paths):
        e = _Gfa("")
        e.header = f"H\tVN:Z:1.0\tKM:i:{k}"
        names = list(segs)
        num = lambda v: (names.index(v[:-1]) + 1) * (1 if v[-1] == "+" else -1)
        flip = lambda v: v[:-1] + ("-" if v[-1] == "+" else "+")
        ents = [[num(v) for v in pth.split()] for pth in paths]
        e.segs = [[segs[n], [f"DP:f:{sum(abs(x) == i + 1 for p_ in ents for x in p_):.2f}"]] for i, n in enumerate(names)]
        for a, b_ in links: e.links += [(num(a), num(b_))] + ([(num(flip(b_)), num(flip(a)))] if (flip(b_), flip(a)) != (a, b_) else [])
        plain = [b"".join(e.strand_seq(v).encode() for v in p_) for p_ in ents]
        e.paths = [[str(i + 1), p_, [f"LN:i:{len(plain[i])}", f"FN:Z:hand_{i}.fasta", f"HD:Z:contig_{i}"]] for i, p_ in enumerate(ents)]
        return e, plain, names

    def check(label, e, plain):
        e.resort()
        detail = {}
        mod = M.verify(M.from_gfa(e), plain, k, detail)
        g2 = graph_from_gfa(e.text(), lib_path=lib_path)[0]
        triples = [(b"." * (k // 2) + q + b"." * (k // 2), len(q), i + 1) for i, q in enumerate(plain)]
        lib, want = same_report(g2.verify(triples), mod, detail)
        g2.close()
        assert lib == want, (label, {f: (lib[f], want[f]) for f in M.FIELDS if lib[f] != want[f]}, detail)
        reports.append((label, mod))
        return mod

    links = [("J+", "C+"), ("B+", "J-"), ("J-", "X-"), ("X-", "J+"), ("C+", "D+"), ("E+", "D+")]      # (E: a second way into D, so that C | D is no cut unitig)
    walk = "B+ J- X- J+ C+ D+"
    # (label, X, B, C, further sequences, the junction side that still shifts: None = the graph is at its fixed point)
    for label, X, B, C, more, side in (
            ("junction:dup", "TCA", "GGTC", "CCG", [], 0),                        # X+ and X- both end in A; 3 > 1 x 2 leaves one base to shift
            ("junction:dup-clamped", "TA", "GGTC", "CCG", [], None),              # ... 2 <= 1 x 2: the clamp leaves nothing
            ("junction:dup-clamped", "A", "GGTC", "CCG", [], None),
            ("junction:dup", "TCCA", "GGTC", "CCG", [], 0),
            ("junction:source-of-2", "TCG", "GGCT", "AG", [], 1),                 # rc(B) and C both begin with A; the shorter has 2 bases: one may go
            ("junction:short-source", "TCG", "GGCT", "A", [], None),              # ... 1 base: none may
            ("junction:beside-fixed-start", "TCG", "GGCT", "AG", ["C+ D+"], None),      # a sequence begins with the output C+: J's end is fixed
            ("junction:beside-fixed-end", "TCA", "GGTC", "CCG", ["X- J+ C+ D+"], None),      # a sequence begins with the input strand X-
            ("junction:beside-fixed-end", "TCA", "GGTC", "CCG", ["B+ J- X-"], None)):        # ... or ends with it
        e, plain, names = graph(dict(B=B, J="ACGTTGCA", X=X, C=C, D="GATTACA", E="CTTGT"), links, [walk, "E+ D+"] + more)
        mod = check(label, e, plain)
        if side is None: assert mod["failed"] == 0, (label, mod)
        else:
            J = next(i for i, (q, _) in enumerate(e.segs) if q == "ACGTTGCA")
            assert mod["failed"] == M.F_EXPAND and mod["first_bad_junction"] == 2 * J + side, (label, mod)
    # a unitig with a self loop, walked twice in a row, cut at every position
    segs = dict(A="GGATCCA", R="ACCGT", Z="TTGACGG")
    for hh in range(1, len(segs["R"])):
        e, plain, names = graph(segs, [("A+", "R+"), ("R+", "R+"), ("R+", "Z+")], ["A+ R+ R+ Z+", "A+ R+ Z+"])
        assert (2, 2) in e.links
        e.cut(2, hh)
        check("gfa:cut-self-loop", e, plain)
    return reports
