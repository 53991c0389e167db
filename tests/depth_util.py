"""A specification-level checker of the read-based unitig depths: depth.rs of `autocycler combine --reads` restated in plain Python
(dicts and lists; nothing of the library's structure), a numpy tally for larger read sets, and generators for the tests.

A graph is (seqs, links): seqs[u - 1] = forward sequence of unitig u as bytes; links = (a, b) pairs of signed unitig numbers in L-line
order with both directions present (build_links_from_gfa, unitig_graph.rs:91-113: a link only extends the next-list of its first end)."""
import math
import random

import numpy as np

MIN_READ_HIT_RATE = 0.005
MAX_WALK_STEPS = 10000
BITS = {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}
COMP = {65: 84, 84: 65, 71: 67, 67: 71, 46: 46}      # misc.rs:358-367: everything else becomes N


def reverse_complement(seq):
    return bytes(COMP.get(b, 78) for b in reversed(seq))


def kmer_value(s):
    """canonical value of a k-mer given as str / bytes (the tests' own encoder, depth.rs:476-482)"""
    s = s.encode() if isinstance(s, str) else s

    def enc(x):
        v = 0
        for b in x:
            v = (v << 2) | BITS[b]
        return v
    return min(enc(s), enc(reverse_complement(s.upper())))


def each_kmer(seq, k):
    """(start, canonical k-mer) of every k-mer of seq (depth.rs:161-184)"""
    out = []
    if len(seq) < k:
        return out
    mask, shift = (1 << (2 * k)) - 1, 2 * (k - 1)
    fwd = rev = valid = 0
    for i, b in enumerate(seq):
        bits = BITS.get(b)
        if bits is None:
            fwd = rev = valid = 0
            continue
        fwd = ((fwd << 2) | bits) & mask
        rev = (rev >> 2) | ((3 - bits) << shift)
        valid += 1
        if valid >= k:
            out.append((i + 1 - k, min(fwd, rev)))
    return out


def encode_kmer(seq):
    k = len(seq)
    fwd = rev = 0
    for b in seq:
        bits = BITS.get(b)
        if bits is None:
            return None
        fwd = ((fwd << 2) | bits) & ((1 << (2 * k)) - 1)
        rev = (rev >> 2) | ((3 - bits) << (2 * (k - 1)))
    return fwd, rev


class GraphModel:
    def __init__(self, seqs, links):
        self.seqs = [bytes(s) for s in seqs]
        self.rev = [reverse_complement(s) for s in self.seqs]
        self.next = {}
        for u in range(1, len(self.seqs) + 1):
            self.next[u] = []
            self.next[-u] = []
        for a, b in links:
            self.next[a].append(b)

    def strand_seq(self, s):
        return self.seqs[s - 1] if s > 0 else self.rev[-s - 1]

    def extensions(self, nxt, length, steps):
        """depth.rs:252-279; steps is a one-element list (the shared budget)"""
        seqs = []
        for strand in nxt:
            if steps[0] == 0:
                break
            steps[0] -= 1
            seq = self.strand_seq(strand)[:length]
            if len(seq) == length:
                seqs.append(seq)
                continue
            further = self.extensions(self.next[strand], length - len(seq), steps)
            if not further:
                seqs.append(seq)
            else:
                seqs.extend(seq + f for f in further)
        return seqs

    def junction_kmers(self, u, k):
        out = []
        for strand in (u, -u):
            seq = self.strand_seq(strand)
            steps = [MAX_WALK_STEPS]
            walks = self.extensions(self.next[strand], k - 1, steps)
            for start in range(max(0, len(seq) - (k - 1)), len(seq)):
                needed = k - (len(seq) - start)
                for walk in walks:
                    if needed > len(walk):
                        continue
                    e = encode_kmer(seq[start:] + walk[:needed])
                    if e is not None and e[0] < e[1]:
                        out.append(e[0])
        return out

    def context_kmers(self, u, k):
        """-> [(offset, [variants])], offsets ascending (depth.rs:187-232)"""
        fseq = self.seqs[u - 1]
        n = len(fseq)
        steps = [MAX_WALK_STEPS]
        left = self.extensions(self.next[-u], k - 1, steps)
        right = self.extensions(self.next[u], k - 1, steps)
        left = [reverse_complement(s) for s in left] or [b""]
        right = right or [b""]
        found = {}

        def add(context, first_offset):
            for i, kmer in each_kmer(context, k):
                offset = first_offset + i
                if offset < 0 or offset > n - k:
                    v, have = found.setdefault(offset, ([], set()))      # (the set only answers `contains`)
                    if kmer not in have:
                        have.add(kmer); v.append(kmer)
        if n >= k:
            for s in left:
                add(s + fseq[:k - 1], -len(s))
            for s in right:
                add(fseq[n - k + 1:] + s, n - k + 1)
        else:
            for l in left:
                for r in right:
                    add(l + fseq + r, -len(l))
        return [(o, found[o][0]) for o in sorted(found)]


def build_kmer_table(graphs, k):
    """{canonical k-mer: occurrences} over all graphs (depth.rs:79-98)"""
    table = {}
    models = [GraphModel(*g) for g in graphs]
    for m in models:
        for s in m.seqs:
            for _, kmer in each_kmer(s, k):
                table[kmer] = table.get(kmer, 0) + 1
    for m in models:
        for u in range(1, len(m.seqs) + 1):
            for kmer in m.junction_kmers(u, k):
                table[kmer] = table.get(kmer, 0) + 1
    return table, models


def count_one_read(seq, k, table, counts):
    """depth.rs:394-419 -> (reads, rejected, read_bases, span_bases, span_kmers, hits); adds the read's hits to counts"""
    hits = []
    first = last = kmer_count = 0
    for i, kmer in each_kmer(seq, k):
        kmer_count += 1
        if kmer in table:
            if not hits:
                first = i
            last = i
            hits.append(kmer)
    if kmer_count == 0:
        return (0, 0, 0, 0, 0, 0)
    if float(len(hits)) < MIN_READ_HIT_RATE * float(kmer_count):
        return (0, 1, 0, 0, 0, 0)
    for kmer in hits:
        counts[kmer] += 1
    span = last - first + 1
    return (1, 0, len(seq), span + k - 1, span, len(hits))


TOTAL_NAMES = ("reads", "rejected_reads", "read_bases", "span_bases", "span_kmers", "hits")


def clipped_mean(counts):
    """depth.rs:345-360 with its two sums as sequential loops; -> (mean or None, whether a count was clipped)"""
    if not counts:
        return None, False
    count = float(len(counts))
    total = 0.0
    for c in counts:
        total += float(c)
    mean = total / count
    limit = max(mean + 6.0 * math.sqrt(mean), 2.0 * mean)
    clipped, any_clipped = 0.0, False
    for c in counts:
        v = float(c)
        if v > limit:
            any_clipped = True
        clipped += min(v, limit)
    return clipped / count, any_clipped


class Checker:
    """set_read_depths (depth.rs:45-76) in steps, as the library's handle does them."""

    def __init__(self, k, graphs):
        self.k = k
        self.table, self.models = build_kmer_table(graphs, k)
        self.repeats = {kmer for kmer, c in self.table.items() if c > 1}
        self.counts = {kmer: 0 for kmer in self.table}
        self.totals = [0] * 6
        self.notes = dict(clipped=0, no_depth=0, context_skipped=0)

    def add_reads(self, reads):
        for r in reads:
            t = count_one_read(bytes(r), self.k, self.table, self.counts)
            self.totals = [a + b for a, b in zip(self.totals, t)]

    def add_reads_numpy(self, reads):
        t = tally_numpy(reads, self.k, self.table, self.counts)
        self.totals = [a + b for a, b in zip(self.totals, t)]

    def totals_dict(self):
        d = dict(zip(TOTAL_NAMES, self.totals))
        d["distinct_kmers"] = len(self.table)
        d["repeat_kmers"] = len(self.repeats)
        return d

    def depths(self, graph_index, scale=None):
        """scale: the reference's unit tests pass one to set_tig_depths; None = set_read_depths' own (and its check_read_totals)"""
        if scale is None:
            if self.totals[0] == 0:
                raise ValueError("no reads were found which match the consensus assembly")
            hits, span_bases = self.totals[5], self.totals[3]
            scale = float(span_bases) / float(hits) if hits > 0 else 0.0
        m = self.models[graph_index]
        out = []
        for u in range(1, len(m.seqs) + 1):
            counts = [self.counts[kmer] for _, kmer in each_kmer(m.seqs[u - 1], self.k) if kmer not in self.repeats]
            for _, variants in m.context_kmers(u, self.k):
                if any(v in self.repeats for v in variants):
                    self.notes["context_skipped"] += 1
                    continue
                counts.append(sum(self.counts[v] for v in variants if v in self.counts) & 0xFFFFFFFF)
            mean, clipped = clipped_mean(counts)
            self.notes["clipped"] += 1 if clipped else 0
            self.notes["no_depth"] += 1 if mean is None else 0
            out.append(None if mean is None else mean * scale)
        return out


# ---- numpy tally ---------------------------------------------------------------------------------------------------------------------
_CODE = np.full(256, 4, dtype=np.uint8)
for _b, _v in BITS.items():
    _CODE[_b] = _v


def tally_numpy(reads, k, table, counts):
    """count_one_read over many reads at once; same results as the plain loop (tested equal on random cases)."""
    keys = np.array(sorted(table), dtype=np.uint64)
    add = np.zeros(len(keys), dtype=np.int64)
    totals = [0] * 6
    chunk, size = [], 0
    for r in reads:
        chunk.append(r); size += len(r) + 1
        if size >= (4 << 20):
            _tally_chunk(chunk, k, keys, add, totals); chunk, size = [], 0
    if chunk:
        _tally_chunk(chunk, k, keys, add, totals)
    for kmer, a in zip(keys.tolist(), add.tolist()):
        if a:
            counts[kmer] += a
    return tuple(totals)


def _tally_chunk(reads, k, keys, add, totals):
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lens + 1)))[:-1]
    text = np.frombuffer(b"\n".join(bytes(r) for r in reads) + b"\n", dtype=np.uint8)
    code = _CODE[text]
    n = len(code)
    if n < k:
        return
    bad = (code > 3).astype(np.int64)
    cb = np.concatenate(([0], np.cumsum(bad)))
    valid = (cb[k:] - cb[:n - k + 1]) == 0                    # k-mer starting at p has no masked byte
    c64 = (code & 3).astype(np.uint64)
    fwd = np.zeros(n - k + 1, dtype=np.uint64)
    rev = np.zeros(n - k + 1, dtype=np.uint64)
    for j in range(k):
        w = c64[j:n - k + 1 + j]
        fwd = (fwd << np.uint64(2)) | w
        rev |= (np.uint64(3) - w) << np.uint64(2 * j)
    canon = np.minimum(fwd, rev)
    pos = np.nonzero(valid)[0]
    read_of = np.searchsorted(starts, pos, side="right") - 1
    km = canon[pos]
    idx = np.searchsorted(keys, km)
    idx[idx >= len(keys)] = 0
    hit = (keys[idx] == km) if len(keys) else np.zeros(len(km), dtype=bool)
    nr = len(reads)
    kmers_per = np.bincount(read_of, minlength=nr)
    hits_per = np.bincount(read_of[hit], minlength=nr)
    within = pos - starts[read_of]
    first = np.full(nr, np.iinfo(np.int64).max, dtype=np.int64)
    last = np.full(nr, -1, dtype=np.int64)
    np.minimum.at(first, read_of[hit], within[hit])
    np.maximum.at(last, read_of[hit], within[hit])
    counted = kmers_per > 0
    rejected = counted & (hits_per.astype(np.float64) < MIN_READ_HIT_RATE * kmers_per.astype(np.float64))
    accepted = counted & ~rejected
    span = np.where(accepted, last - first + 1, 0)
    totals[0] += int(accepted.sum()); totals[1] += int(rejected.sum()); totals[2] += int(lens[accepted].sum())
    totals[3] += int((span[accepted] + k - 1).sum()); totals[4] += int(span[accepted].sum()); totals[5] += int(hits_per[accepted].sum())
    use = hit & accepted[read_of]
    np.add.at(add, idx[use], 1)


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def random_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def both_directions(links):
    """every link followed by its mirror (b' -> a'), duplicates dropped, order kept"""
    out, seen = [], set()
    for a, b in links:
        for l in ((a, b), (-b, -a)):
            if l not in seen:
                seen.add(l); out.append(l)
    return out


def random_graph(rng, genome_len, n_cuts, n_bubbles, circular=True, short=(1, 8)):
    """A random genome cut into unitigs, some stretches doubled into two-way bubbles (the second arm a mutated copy, often shorter than any
    k-mer); -> (seqs, links, genome).  Repeats in the genome make repeat k-mers; short arms make context-only unitigs."""
    genome = random_seq(rng, genome_len)
    cuts = sorted(rng.sample(range(10, genome_len - 10), n_cuts))
    pieces = [genome[a:b] for a, b in zip([0] + cuts, cuts + [genome_len])]
    seqs, links = [], []
    main = []
    for p in pieces:
        seqs.append(p); main.append(len(seqs))
    for i in range(len(main) - 1):
        links.append((main[i], main[i + 1]))
    if circular:
        links.append((main[-1], main[0]))
    # bubbles: an alternative to piece i between its neighbours
    for i in rng.sample(range(1, len(main) - 1), min(n_bubbles, len(main) - 2)):
        alt = bytearray(random_seq(rng, rng.randint(*short)))
        seqs.append(bytes(alt))
        u = len(seqs)
        links.append((main[i - 1], u)); links.append((u, main[i + 1]))
    return seqs, both_directions(links), genome


def sample_reads(rng, genome, n_reads, length, sub=0.05, circular=True):
    out = []
    g2 = genome + genome if circular else genome
    for _ in range(n_reads):
        ln = max(1, int(rng.gauss(length, length * 0.2)))
        ln = min(ln, len(genome))
        s = rng.randrange(len(genome) if circular else len(genome) - ln + 1)
        r = bytearray(g2[s:s + ln])
        for i in range(len(r)):
            if rng.random() < sub:
                r[i] = rng.choice(b"ACGT")
        r = bytes(r)
        out.append(reverse_complement(r) if rng.random() < 0.5 else r)
    return out


def sample_reads_numpy(seed, genome, n_reads, length, sub, foreign_every=5):
    """the same kind of read set, vectorised (mid-size jobs): every foreign_every-th read is random sequence"""
    rs = np.random.RandomState(seed)
    g = np.frombuffer(genome + genome, dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in COMP.items():
        comp[a] = b
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n_reads):
        ln = int(min(len(genome), max(1, rs.normal(length, length * 0.2))))
        if foreign_every and i % foreign_every == foreign_every - 1:
            out.append(acgt[rs.randint(0, 4, ln)].tobytes())
            continue
        s = rs.randint(0, len(genome))
        r = g[s:s + ln].copy()
        m = rs.random_sample(ln) < sub
        r[m] = acgt[rs.randint(0, 4, int(m.sum()))]
        if rs.random_sample() < 0.5:
            r = comp[r[::-1]]
        out.append(r.tobytes())
    return out


def foreign_reads(rng, n_reads, length):
    return [random_seq(rng, max(1, int(rng.gauss(length, length * 0.2)))) for _ in range(n_reads)]


def load_gfa(path):
    """S and L lines of a GFA fixture -> (seqs, links) with unitig numbers 1..n in file order (the fixtures number them so)"""
    seqs, links = {}, []
    for line in open(path):
        p = line.rstrip("\n").split("\t")
        if p[0] == "S":
            seqs[int(p[1])] = p[2].encode()
        elif p[0] == "L":
            links.append((int(p[1]) * (1 if p[2] == "+" else -1), int(p[3]) * (1 if p[4] == "+" else -1)))
    assert sorted(seqs) == list(range(1, len(seqs) + 1))
    return [seqs[i] for i in range(1, len(seqs) + 1)], links
