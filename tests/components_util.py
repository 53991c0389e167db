"""The model the connected-components tests hold the library to: UnitigGraph::connected_components, component_is_circular_loop, link_count
and topology (unitig_graph.rs:478-545, 905-967) and the per-unitig end tests of unitig.rs:197-215, 276-293, restated line by line in plain
Python over (n_unitigs, links, alive) — plus the generators of the random sweep and the boundary shapes, whose expected values are built by
construction.  It shares no code with kernels_components.inc."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
FORWARD, REVERSE = True, False
OPEN_START, OPEN_END, HAIRPIN_START, HAIRPIN_END, ISOLATED_CIRCULAR, ISOLATED_LINEAR = 1, 2, 4, 8, 16, 32
NOT_ALIVE = 0xFFFFFFFF
TOPOLOGIES = ("empty", "fragmented", "linear-open-open", "circular", "linear-hairpin-hairpin", "linear-open-hairpin", "other")
RECORD_FIELDS = ("first", "unitigs", "length", "links_all", "links_one_way", "open_ends", "marked", "circular_loop")


def load_kats():
    return json.loads((GOLDEN / "components_kats.json").read_text())


def gfa_links(name):
    """(n_unitigs, [(a, b)] in L-line order, [unitig lengths]) of a golden GFA"""
    lens, links = {}, []
    for line in (GOLDEN / name).read_text().splitlines():
        p = line.split("\t")
        if p[0] == "S":
            lens[int(p[1])] = len(p[2])
        elif p[0] == "L":
            links.append((int(p[1]) * (1 if p[2] == "+" else -1), int(p[3]) * (1 if p[4] == "+" else -1)))
    assert sorted(lens) == list(range(1, len(lens) + 1))
    return len(lens), links, [lens[u] for u in range(1, len(lens) + 1)]


# ---- the reference, literally ---------------------------------------------------------------------------------------------------------------
class Unitig:
    def __init__(self, number):
        self.number = number
        self.forward_next, self.forward_prev, self.reverse_next, self.reverse_prev = [], [], [], []      # entries: (number, strand)

    # unitig.rs:197-215
    def open_start(self):
        return len(self.reverse_next) == 0

    def open_end(self):
        return len(self.forward_next) == 0

    def hairpin_start(self):
        return len(self.reverse_next) == 1 and self.reverse_next[0][1] == FORWARD and self.reverse_next[0][0] == self.number

    def hairpin_end(self):
        return len(self.forward_next) == 1 and self.forward_next[0][1] == REVERSE and self.forward_next[0][0] == self.number

    # unitig.rs:276-293
    def is_isolated_and_circular(self):
        if len(self.forward_next) != 1 or len(self.forward_prev) != 1:
            return False
        nxt, prev = self.forward_next[0], self.forward_prev[0]
        return nxt[0] == self.number and nxt[1] and prev[0] == self.number and prev[1]

    def is_isolated_and_linear(self):
        if len(self.forward_next) > 1 or len(self.forward_prev) > 1:
            return False
        if self.is_isolated_and_circular():
            return False
        valid_fn = all(u[0] == self.number and not u[1] for u in self.forward_next)
        valid_fp = all(u[0] == self.number and not u[1] for u in self.forward_prev)
        valid_rn = all(u[0] == self.number and u[1] for u in self.reverse_next)
        valid_rp = all(u[0] == self.number and u[1] for u in self.reverse_prev)
        return valid_fn and valid_fp and valid_rn and valid_rp

    def flags(self):
        return (OPEN_START * self.open_start() + OPEN_END * self.open_end() + HAIRPIN_START * self.hairpin_start() + HAIRPIN_END * self.hairpin_end() +
                ISOLATED_CIRCULAR * bool(self.is_isolated_and_circular()) + ISOLATED_LINEAR * bool(self.is_isolated_and_linear()))


class UnitigGraph:
    """unitigs 1 .. n_unitigs with the links in line order (build_links_from_gfa, unitig_graph.rs:91-115); alive: the numbers that were not
    removed (remove_unitigs_by_number) — links that touch a removed unitig are gone (delete_dangling_links)"""

    def __init__(self, n_unitigs, links, alive=None):
        for a, b in links:
            for x in (a, b):
                if x == 0 or abs(x) > n_unitigs:
                    raise ValueError(f"link refers to nonexistent unitig: {abs(x)}")
        keep = [u for u in range(1, n_unitigs + 1) if alive is None or alive[u - 1]]
        self.unitigs = [Unitig(u) for u in keep]
        self.unitig_index = {u.number: u for u in self.unitigs}
        for a, b in links:
            seg_1, seg_2, strand_1, strand_2 = abs(a), abs(b), a > 0, b > 0
            if seg_1 not in self.unitig_index or seg_2 not in self.unitig_index:
                continue
            unitig_1, unitig_2 = self.unitig_index[seg_1], self.unitig_index[seg_2]
            (unitig_1.forward_next if strand_1 else unitig_1.reverse_next).append((seg_2, strand_2))
            (unitig_2.forward_prev if strand_2 else unitig_2.reverse_prev).append((seg_1, strand_1))

    # unitig_graph.rs:478-507, over all unitigs or over the given ones
    def link_count(self, numbers=None):
        all_links, one_way_links = set(), set()
        for a in (self.unitigs if numbers is None else [self.unitig_index[u] for u in numbers]):
            a_num = a.number
            for b in a.forward_next:
                b_num = b[0] if b[1] else -b[0]
                link, rev_link = (a_num, b_num), (-b_num, -a_num)
                all_links.add(link); all_links.add(rev_link)
                one_way_links.add(link if link > rev_link else rev_link)
            for b in a.reverse_next:
                b_num = b[0] if b[1] else -b[0]
                link, rev_link = (-a_num, b_num), (-b_num, a_num)
                all_links.add(link); all_links.add(rev_link)
                one_way_links.add(link if link > rev_link else rev_link)
        return len(all_links), len(one_way_links)

    # unitig_graph.rs:527-545
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

    # unitig_graph.rs:905-947
    def connected_components(self):
        visited, components = set(), []
        for unitig in self.unitigs:
            if unitig.number not in visited:
                component = []
                self.dfs(unitig.number, visited, component)
                component.sort()
                components.append(component)
        components.sort()
        return components

    def dfs(self, unitig_num, visited, component):
        stack = [unitig_num]
        while stack:
            current = stack.pop()
            if current not in visited:
                visited.add(current)
                component.append(current)
                for neighbor in self.connected_unitigs(current):
                    if neighbor not in visited:
                        stack.append(neighbor)

    def connected_unitigs(self, unitig_num):
        connections = set()
        unitig = self.unitig_index.get(unitig_num)
        if unitig is not None:
            for lst in (unitig.forward_next, unitig.forward_prev, unitig.reverse_next, unitig.reverse_prev):
                for c in lst:
                    connections.add(c[0])
        return connections

    # unitig_graph.rs:949-967
    def component_is_circular_loop(self, component):
        if not component:
            return False
        first = component[0]
        num, strand, visited = first, FORWARD, set()
        while num != first or not visited:
            if num in visited:
                return False
            visited.add(num)
            unitig = self.unitig_index[num]
            if len(unitig.forward_next) != 1 or len(unitig.forward_prev) != 1 or len(unitig.reverse_next) != 1 or len(unitig.reverse_prev) != 1:
                return False
            nxt = unitig.forward_next[0] if strand else unitig.reverse_next[0]
            num, strand = nxt
        return len(visited) == len(component)

    # resolve.rs:273-282
    def unitigs_not_connected_to_anchor(self, anchors):
        gone = set()
        for component in self.connected_components():
            if not any(u in anchors for u in component):
                gone.update(component)
        return gone


# ---- one form for what the model says, what a shape is built to give and what the library returned ------------------------------------------
def result_from_components(n_unitigs, components, records, flags, topology):
    """components: ascending member lists in order; records: dicts of RECORD_FIELDS; flags: per unitig"""
    component_of = np.full(n_unitigs, NOT_ALIVE, dtype=np.uint32)
    for c, members in enumerate(components):
        component_of[np.asarray(members, dtype=np.int64) - 1] = c
    rec = {f: np.array([r[f] for r in records], dtype=np.uint64) for f in RECORD_FIELDS}
    return result_from_arrays(component_of, rec, np.asarray(flags, dtype=np.uint8), topology)


def result_from_arrays(component_of, rec, flags, topology):
    """component_of: per unitig its component index (in order of lowest member) or NOT_ALIVE; rec: {field: array per component}"""
    alive = component_of != NOT_ALIVE
    nc = int(component_of[alive].max()) + 1 if alive.any() else 0
    counts = np.bincount(component_of[alive].astype(np.int64), minlength=nc)
    order = np.argsort(np.where(alive, component_of, nc).astype(np.int64), kind="stable")
    members = (order[:int(alive.sum())] + 1).astype(np.uint32)
    member_off = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    rec = {f: np.asarray(rec[f], dtype=np.uint64) for f in RECORD_FIELDS}
    assert all(len(rec[f]) == nc for f in RECORD_FIELDS) and np.array_equal(rec["unitigs"], counts.astype(np.uint64))
    assert nc == 0 or np.array_equal(rec["first"], members[member_off[:-1].astype(np.int64)].astype(np.uint64))
    return dict(component_of=component_of.astype(np.uint32), member_off=member_off, members=members, records=rec, flags=flags.astype(np.uint8), topology=topology,
                unitigs=int(alive.sum()), components=nc, links_all=int(rec["links_all"].sum()), links_one_way=int(rec["links_one_way"].sum()),
                total_length=int(rec["length"].sum()))


def model_expected(n_unitigs, links, unitig_len=None, alive=None, marked=None):
    g = UnitigGraph(n_unitigs, [(int(a), int(b)) for a, b in links], alive)
    components = g.connected_components()
    records = []
    for comp in components:
        la, lo = g.link_count(comp)
        records.append(dict(first=comp[0], unitigs=len(comp), length=sum(int(unitig_len[u - 1]) for u in comp) if unitig_len is not None else 0,
                            links_all=la, links_one_way=lo, open_ends=sum(g.unitig_index[u].open_start() + g.unitig_index[u].open_end() for u in comp),
                            marked=sum(1 for u in comp if marked is not None and marked[u - 1]), circular_loop=int(g.component_is_circular_loop(comp))))
    flags = [g.unitig_index[u].flags() if u in g.unitig_index else 0 for u in range(1, n_unitigs + 1)]
    exp = result_from_components(n_unitigs, components, records, flags, g.topology())
    assert (exp["links_all"], exp["links_one_way"]) == g.link_count()      # (components partition the links)
    return exp


def library_result(c):
    """an autocycler_amd.Components in the same form"""
    rec = {f: c.records[f].astype(np.uint64) for f in RECORD_FIELDS}
    sm = c.summary
    return dict(component_of=c.component_of, member_off=c.member_off, members=c.members, records=rec, flags=c.flags, topology=c.topology, unitigs=sm["unitigs"],
                components=sm["components"], links_all=sm["links_all"], links_one_way=sm["links_one_way"], total_length=sm["total_length"])


def assert_same(got, exp, what=""):
    for k in ("topology", "unitigs", "components", "links_all", "links_one_way", "total_length"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ("component_of", "member_off", "members", "flags"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k)
    for f in RECORD_FIELDS:
        assert np.array_equal(got["records"][f], exp["records"][f]), (what, f)


def result_bytes(c):
    """every accessor's output as bytes (scheduling independence: identical, not merely equal as values)"""
    return b"|".join([c.records.tobytes(), c.component_of.tobytes(), c.member_off.tobytes(), c.members.tobytes(), c.flags.tobytes(), c.topology.encode(),
                      repr(sorted((k, v) for k, v in c.summary.items() if k not in ("launches", "read_backs", "seconds_device"))).encode()])


# ---- the random sweep ------------------------------------------------------------------------------------------------------------------------
def rc(link):
    return (-link[1], -link[0])


def ring_links(rng, numbers):
    """a ring through `numbers` in the given order, a random strand each, both directions"""
    s = [u if rng.random() < 0.5 else -u for u in numbers]
    out = []
    for i in range(len(s)):
        l = (s[i], s[(i + 1) % len(s)])
        out += [l] if rc(l) == l else [l, rc(l)]
    return out


def random_case(rng):
    """(n, links, unitig_len, alive, marked).  Two graphs in three are 1-60 unitigs with 0-3n random signed links; every third one (and
    every graph of one unitig: a tenth of all) is planted first — its unitigs cut into groups that each become a ring, a unitig with a circularising link, with one or two hairpins, or
    stay unlinked — with up to n / 4 random links on top half of the time: circular loops of several members, and single unitigs of every
    topology, do not come out of random links often enough.  Then: two thirds are closed under reverse complement, the rest left as drawn;
    a tenth of the lines duplicated; the line order shuffled; half get a random alive mask, half a random marked."""
    n = 1 if rng.random() < 0.1 else rng.randint(1, 60)
    signed = lambda: rng.choice((1, -1)) * rng.randint(1, n)
    links = []
    if n == 1 or rng.random() < 1 / 3:
        order = list(range(1, n + 1))
        rng.shuffle(order)
        while order:
            kind = rng.random()
            if kind < 0.4:
                size = min(len(order), rng.randint(1, 6))
                links += ring_links(rng, order[:size])
                order = order[size:]
            else:
                u = order.pop()
                links += [[], [(u, u), (-u, -u)], [(u, -u)], [(-u, u)], [(u, -u), (-u, u)], [(u, u), (-u, -u), (u, -u)]][rng.randrange(6)]
        if rng.random() < 0.5:
            links += [(signed(), signed()) for _ in range(rng.randint(0, max(1, n // 4)))]
    else:
        links = [(signed(), signed()) for _ in range(rng.randint(0, 3 * n))]
    if rng.random() < 2 / 3:
        have = set(links)
        links += [rc(l) for l in links if rc(l) not in have and not have.add(rc(l))]
    links += [l for l in links if rng.random() < 0.1]
    rng.shuffle(links)
    unitig_len = [rng.randint(1, 5000) for _ in range(n)]
    alive = [int(rng.random() < 0.8) for _ in range(n)] if rng.random() < 0.5 else None
    marked = [int(rng.random() < 0.2) for _ in range(n)] if rng.random() < 0.5 else None
    return n, links, unitig_len, alive, marked


# ---- the boundary shapes: (n, links as an (m, 2) int32 array, expected by construction) ---------------------------------------------------------
def _both(links):
    """the links and their reverse complements, line by line"""
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2)
    out = np.empty((2 * len(links), 2), dtype=np.int64)
    out[0::2] = links
    out[1::2, 0] = -links[:, 1]; out[1::2, 1] = -links[:, 0]
    return out.astype(np.int32)


def _one_component(n, length, links_all, links_one_way, open_ends, loop, flags, topology="fragmented"):
    rec = dict(first=[1], unitigs=[n], length=[length], links_all=[links_all], links_one_way=[links_one_way], open_ends=[open_ends], marked=[0], circular_loop=[loop])
    return result_from_arrays(np.zeros(n, dtype=np.uint32), rec, flags, topology)


def lengths(n):
    return ((np.arange(n, dtype=np.uint64) * 2654435761) % 4999 + 1).astype(np.uint32)


def shape_chain(n, order):
    """a chain order[0]+ -> order[1]+ -> ...: deep parent trees, diameter n"""
    order = np.asarray(order, dtype=np.int64)
    flags = np.zeros(n, dtype=np.uint8)
    flags[order[0] - 1] |= OPEN_START; flags[order[-1] - 1] |= OPEN_END
    return n, _both(np.stack([order[:-1], order[1:]], axis=1)), _one_component(n, int(lengths(n).sum(dtype=np.uint64)), 2 * (n - 1), n - 1, 2, 0, flags)


def shape_chain_permuted(n, seed=5):
    return shape_chain(n, np.random.default_rng(seed).permutation(n) + 1)


def shape_chain_descending(n):
    return shape_chain(n, np.arange(n, 0, -1))


def shape_star(n):
    """1+ -> k+ for every other k: all hooks on one root, n contributors to one component's counters"""
    leaves = np.arange(2, n + 1, dtype=np.int64)
    flags = np.full(n, OPEN_END, dtype=np.uint8)
    flags[0] = OPEN_START
    return n, _both(np.stack([np.ones(n - 1, dtype=np.int64), leaves], axis=1)), _one_component(n, int(lengths(n).sum(dtype=np.uint64)), 2 * (n - 1), n - 1, n, 0, flags)


def shape_singletons(n):
    ln = lengths(n).astype(np.uint64)
    one, zero = np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rec = dict(first=np.arange(1, n + 1), unitigs=one, length=ln, links_all=zero, links_one_way=zero, open_ends=2 * one, marked=zero, circular_loop=zero)
    return n, np.zeros((0, 2), dtype=np.int32), result_from_arrays(np.arange(n, dtype=np.uint32), rec, np.full(n, OPEN_START | OPEN_END | ISOLATED_LINEAR, dtype=np.uint8),
                                                                   "fragmented" if n > 1 else "linear-open-open")


def shape_pairs(n):
    """unitig 1 alone, then (2, 3), (4, 5), ...: (n - 1) / 2 components of two"""
    assert n % 2 == 1 and n >= 3
    a = np.arange(2, n, 2, dtype=np.int64)
    p = len(a)
    ln = lengths(n).astype(np.uint64)
    component_of = np.concatenate(([0], np.repeat(np.arange(1, p + 1), 2))).astype(np.uint32)
    cat = lambda first, rest: np.concatenate(([first], np.full(p, rest))).astype(np.uint64)
    rec = dict(first=np.concatenate(([1], a)), unitigs=cat(1, 2), length=np.concatenate(([ln[0]], ln[1::2] + ln[2::2])), links_all=cat(0, 2), links_one_way=cat(0, 1),
               open_ends=cat(2, 2), marked=cat(0, 0), circular_loop=cat(0, 0))
    flags = np.empty(n, dtype=np.uint8)
    flags[0] = OPEN_START | OPEN_END | ISOLATED_LINEAR; flags[1::2] = OPEN_START; flags[2::2] = OPEN_END
    return n, _both(np.stack([a, a + 1], axis=1)), result_from_arrays(component_of, rec, flags, "fragmented")


def _ring_signed(n, seed):
    s = np.arange(1, n + 1, dtype=np.int64)
    s[np.random.default_rng(seed).random(n) < 0.5] *= -1
    return s


def shape_ring(n, seed=9):
    """one ring through 1 .. n with mixed strands: a circular loop, the walker takes n steps"""
    assert n >= 3
    s = _ring_signed(n, seed)
    return n, _both(np.stack([s, np.roll(s, -1)], axis=1)), _one_component(n, int(lengths(n).sum(dtype=np.uint64)), 2 * n, n, 0, 1, np.zeros(n, dtype=np.uint8))


def shape_ring_one_way_once(n, seed=9):
    """the same ring with the reverse complement of ONE link removed: no loop (two list lengths are 0), same link sets"""
    n, links, _ = shape_ring(n, seed)
    j = (n // 3) * 2 + 1      # the line that holds the reverse complement of link n // 3
    a = int(links[j, 0])
    links = np.delete(links, j, axis=0)
    flags = np.zeros(n, dtype=np.uint8)
    flags[abs(a) - 1] = OPEN_END if a > 0 else OPEN_START      # a's next list is empty now
    return n, links, _one_component(n, int(lengths(n).sum(dtype=np.uint64)), 2 * n, n, 1, 0, flags)


def shape_self_rc_ring():
    """1+ -> 2+ -> 2- -> 1- -> 1+: every list has one entry, the strand orbit is a ring that is its own reverse complement and meets both
    unitigs twice: not a loop"""
    ln = lengths(2)
    flags = np.array([HAIRPIN_START, HAIRPIN_END], dtype=np.uint8)
    return 2, np.array([(1, 2), (2, -2), (-2, -1), (-1, 1)], dtype=np.int32), _one_component(2, int(ln.sum()), 4, 3, 0, 0, flags)


def shape_double_hairpin():
    """one unitig with a hairpin link at both ends: the walk calls it a loop; topology linear-hairpin-hairpin"""
    flags = np.array([HAIRPIN_START | HAIRPIN_END | ISOLATED_LINEAR], dtype=np.uint8)
    return 1, np.array([(1, -1), (-1, 1)], dtype=np.int32), _one_component(1, int(lengths(1)[0]), 2, 2, 0, 1, flags, "linear-hairpin-hairpin")


def ceil_log2(n):
    return max(1, (n - 1).bit_length())
