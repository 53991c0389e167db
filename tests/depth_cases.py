"""The cases of the read-depth tests, shared by test_depth_emu.py (CPU emulation) and test_depth_gpu.py (device): every comparison of the
library (ReadDepth, ac_depth_*) with the checker of depth_util.py is equality — totals, per-k-mer present / occurrences / read count for
all assembly k-mers and a sample of absent ones, has_depth, and the depths as exact f64.

Kernel geometry the shapes aim at: a lane rolls over 32 positions (one packed word), a wavefront over 2048, a workgroup over 8192."""
import gzip
import json
import random
from pathlib import Path

import pytest

import depth_util as D
from autocycler_amd import AutocyclerError, ReadDepth

GOLDEN = Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLDEN / "depth_kats.json").read_text())
TOTALS = D.TOTAL_NAMES + ("distinct_kmers", "repeat_kmers")
LANE, WAVE, GROUP = 32, 2048, 8192


def gfa(n):
    return D.load_gfa(GOLDEN / f"test_gfa_{n}.gfa")


def compare(rd, chk, seed=1, finish=True):
    """library handle against checker; -> the checker's notes"""
    t = rd.totals()
    want = chk.totals_dict()
    assert {n: t[n] for n in TOTALS} == want
    assert t["table_slots"] >= 2 * sum(chk.table.values()) and t["table_slots"] & (t["table_slots"] - 1) == 0
    rng = random.Random(seed)
    keys = sorted(chk.table)
    absent = [0, (1 << (2 * chk.k)) - 1, 1 << 62, (1 << 64) - 1] + [rng.randrange(1 << (2 * chk.k)) for _ in range(200)] + [x ^ 1 for x in keys[:100]]
    absent = [x for x in absent if x not in chk.table]
    present, occ, cnt = rd.kmer_counts(keys + absent)
    assert present == [1] * len(keys) + [0] * len(absent)
    assert occ == [chk.table[x] for x in keys] + [0] * len(absent)
    assert cnt == [chk.counts[x] for x in keys] + [0] * len(absent)
    if finish:
        for gi in range(len(chk.models)):
            assert rd.depths(gi) == chk.depths(gi), gi
    return chk.notes


def run(lib_path, k, graphs, reads, seed=1, numpy_tally=False):
    chk = D.Checker(k, graphs)
    (chk.add_reads_numpy if numpy_tally else chk.add_reads)(reads)
    with ReadDepth(k, graphs, lib_path=lib_path) as rd:
        rd.add_reads(reads)
        notes = compare(rd, chk, seed)
        return chk, notes, rd.totals()


def planted(rng, genome, k, n_kmers):
    """a read of exactly n_kmers k-mers of which exactly one (its first) is in the genome: a genome k-mer, then foreign sequence"""
    s = rng.randrange(len(genome) - k)
    return genome[s:s + k] + D.random_seq(rng, n_kmers - 1)


# 1. the reference's known answers: the checker reproduces them at their own k (3, 5, 25); the library, whose k starts at 11, equals the
#    checker on the same graphs and reads at k = 11
def check_kats_checker():
    n = 0
    for c in KATS["add_seq_kmers"] + KATS["find_repeats"]:
        table = {}
        for _, km in D.each_kmer(c["seq"].encode(), c["k"]):
            table[km] = table.get(km, 0) + 1
        assert len(table) == c["distinct"]
        if "total" in c:
            assert sum(table.values()) == c["total"]
        for s, v in c.get("counts", {}).items():
            assert table[D.kmer_value(s)] == v
        for s in c.get("repeats", []):
            assert table[D.kmer_value(s)] > 1
        if "repeats" in c:
            assert sum(1 for v in table.values() if v > 1) == len(c["repeats"])
        for s in c.get("not_repeat", []):
            assert table[D.kmer_value(s)] == 1
        n += 1
    for c in KATS["both_strands"]:
        s = c["seq"].encode()
        assert sorted(km for _, km in D.each_kmer(s, c["k"])) == sorted(km for _, km in D.each_kmer(D.reverse_complement(s), c["k"]))
        n += 1
    for c in KATS["junction_kmers"]:
        got = D.GraphModel(*gfa(c["gfa"])).junction_kmers(c["unitig"], c["k"])
        assert len(got) == c["count"] and all(D.kmer_value(s) in got for s in c["contains"])
        n += 1
    for c in KATS["build_kmer_table"]:
        table, _ = D.build_kmer_table([gfa(g) for g in c["gfas"]], c["k"])
        for s, v in c["counts"].items():
            assert table[D.kmer_value(s)] == v
        for name, val in (("total", sum(table.values())), ("distinct", len(table)), ("count_one", sum(1 for v in table.values() if v == 1)),
                          ("repeats", sum(1 for v in table.values() if v > 1))):
            if name in c:
                assert val == c[name], name
        n += 1
    for c in KATS["count_one_read"] + KATS["count_read_kmers"]:
        chk = D.Checker(c["k"], [gfa(c["gfa"])])
        chk.add_reads([r.encode() for r in c.get("reads", [c.get("read")])])
        t = chk.totals_dict()
        assert {name: t[name] for name in c["totals"]} == c["totals"]
        for s, v in c.get("counts", {}).items():
            assert chk.counts[D.kmer_value(s)] == v
        if c.get("all_zero"):
            assert not any(chk.counts.values())
        n += 1
    for c in KATS["clipped_mean"]:
        got, _ = D.clipped_mean(c["counts"])
        if c["expected"] is None or c["tol"] == 0:
            assert got == c["expected"]
        else:
            assert abs(got - c["expected"]) <= c["tol"]
        if "below" in c:
            assert got < c["below"]
        n += 1
    for c in KATS["set_tig_depths"]:
        chk = D.Checker(c["k"], [gfa(c["gfa"])])
        chk.add_reads([r.encode() for r in c["reads"]])
        got = chk.depths(0, scale=c["scale"])
        for u, v in c["depths"].items():
            assert got[int(u) - 1] == v
        n += 1
    for c in KATS["context_kmers"]:
        got = D.GraphModel(*gfa(c["gfa"])).context_kmers(c["unitig"], c["k"])
        assert [o for o, _ in got] == c["offsets"]
        for i, want in c.get("variants", {}).items():
            assert got[int(i)][1] == [D.kmer_value(s) for s in want]
        if c.get("single_variants"):
            assert all(len(v) == 1 for _, v in got)
        if "any_first" in c:
            assert any(v[0] == D.kmer_value(c["any_first"]) for _, v in got)
        n += 1
    return n


def check_kat_graphs(lib_path):
    seq = b"AGCATCGACATCGACTACG"
    for graphs, reads in (([gfa(8)], [seq, seq, b"T" * 19]), ([gfa(8), gfa(9)], [seq] * 3), ([gfa(10)], [b"TTTTTTTTTT" + seq]),
                          ([gfa(15)], [b"ATTGTAGGTACCGATCGATCGT"] * 2 + [b"CTTGTAGGTACCGATCGATCGT"] * 3), ([gfa(16)], [b"AAAACCCCGGGGTTTTACGTTTGCATGCCTTAAGGCC"])):
        run(lib_path, 11, graphs, reads)


# the handle form (ac_depth_begin_handles): the graph's own arrays through ac_unitigs_bulk + ac_links, checked with the links the handle reports
def check_handles(lib_path):
    import ctypes as C
    from autocycler_amd import _capi, graph_from_gfa
    for n in (15, 16):
        g, _, _ = graph_from_gfa((GOLDEN / f"test_gfa_{n}.gfa").read_text(), lib_path=lib_path)
        links, cnt = C.POINTER(_capi.Link)(), C.c_uint64()
        assert g._lib.ac_links(g._h, C.byref(links), C.byref(cnt)) == 0
        graph = (gfa(n)[0], [(links[i].a, links[i].b) for i in range(cnt.value)])
        reads = [b"ATTGTAGGTACCGATCGATCGT", b"AAAACCCCGGGGTTTTACGTTTGCATGCCTTAAGGCC", b"AAAACCCCGGGGTTTTACGTGCATGCCTTAAGGCC"]
        chk = D.Checker(11, [graph]); chk.add_reads(reads)
        with ReadDepth(11, [g], lib_path=lib_path) as rd:
            rd.add_reads(reads)
            compare(rd, chk)
        g.close()


# 2-7, 10: a random graph with bubbles and short arms; reads at every length edge, N at every position class, lower case
def edge_lengths(k):
    return sorted({1, k - 1, k, k + 1, LANE - 1, LANE, LANE + 1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP + 1})


def check_random_graph(lib_path, k, seed):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 9000)
    genome = genome[:4000] + genome[1000:1400] + genome[4000:]      # a 400 bp repeat: repeat k-mers, clipped counts where the reads pile up
    seqs, links, _ = cut_genome(rng, genome, 40, 12)
    reads = []
    for ln in edge_lengths(k):
        for _ in range(1 if ln > WAVE + 1 else 2):
            s = rng.randrange(len(genome) - ln)
            r = genome[s:s + ln]
            reads.append(r if rng.random() < 0.5 else D.reverse_complement(r))
    reads += D.sample_reads(rng, genome, 25, 300, sub=0.05)
    reads += D.foreign_reads(rng, 40, 600)      # (at k = 11 a random 600-mer meets the table two or three times: some of these are accepted)
    reads += [r.lower() for r in D.sample_reads(rng, genome, 4, 150, sub=0.0)]
    # N at every position class of a lane's stretch, around a word boundary
    base = genome[2000:2000 + 200]
    for p in (0, 1, k - 1, LANE - 1, LANE, LANE + 1, 2 * LANE - 1, 199):
        r = bytearray(base); r[p] = ord("N"); reads.append(bytes(r))
    reads += [b"N" * 5, b"N" * 40, b"N" * (WAVE + 3), b"", b"A"]      # neither counted nor rejected
    reads += [genome[3000:3050] * 6] * 20                              # the same k-mers many times in one read, many reads deep: clipped counts
    rng.shuffle(reads)
    chk, notes, _ = run(lib_path, k, [(seqs, links)], reads, seed)
    t = chk.totals_dict()
    n_counted = t["reads"] + t["rejected_reads"]
    assert t["reads"] * 10 >= n_counted and t["rejected_reads"] * 10 >= n_counted
    assert t["repeat_kmers"] > 0 and notes["clipped"] > 0 and notes["no_depth"] > 0 and notes["context_skipped"] > 0, (t, notes)


def cut_genome(rng, genome, n_cuts, n_bubbles):
    """D.random_graph on a given genome: pieces in a ring, bubbles whose second arm is 1-8 bp, and one isolated 5 bp unitig (no depth)"""
    cuts = sorted(rng.sample(range(10, len(genome) - 10), n_cuts))
    seqs = [genome[a:b] for a, b in zip([0] + cuts, cuts + [len(genome)])]
    n_main = len(seqs)
    links = [(i + 1, (i + 1) % n_main + 1) for i in range(n_main)]
    for i in rng.sample(range(1, n_main - 1), n_bubbles):
        seqs.append(D.random_seq(rng, rng.randint(1, 8)))
        links += [(i, len(seqs)), (len(seqs), i + 2)]
    seqs.append(b"ACGTA")
    return seqs, D.both_directions(links), genome


# 3 (long read) and 4 (hundreds of short reads in one wavefront)
def check_long_and_short_reads(lib_path, k=21, seed=5):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 3000)
    graphs = [([genome], [])]
    # one 20 000 bp read: foreign but for a genome stretch near each end, so that first and last hit lie in different workgroups
    long_read = D.random_seq(rng, 300) + genome[100:200] + D.random_seq(rng, 19000) + genome[500:600] + D.random_seq(rng, 500)
    shorts = [genome[s:s + 40] for s in (rng.randrange(2900) for _ in range(400))]
    chk, _, t = run(lib_path, k, graphs, shorts[:150] + [long_read] + shorts[150:], seed)
    assert chk.totals[0] == 401 and len(long_read) == 20000


# 8. the acceptance threshold, planted exactly
def check_threshold(lib_path, k=21, seed=9):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 2000)
    graphs = [([genome], [])]
    table = D.Checker(k, graphs).table
    for n_kmers, hit, want in ((200, True, (1, 0)), (201, True, (0, 1)), (200, False, (0, 1))):
        while True:      # (a foreign tail that happens to hit the genome would spoil the plant: draw again)
            r = planted(rng, genome, k, n_kmers) if hit else D.random_seq(rng, n_kmers + k - 1)
            kms = [km for _, km in D.each_kmer(r, k)]
            if len(kms) == n_kmers and sum(km in table for km in kms) == (1 if hit else 0):
                break
        chk = D.Checker(k, graphs); chk.add_reads([r])
        assert (chk.totals[0], chk.totals[1]) == want, (n_kmers, hit)
        with ReadDepth(k, graphs, lib_path=lib_path) as rd:
            rd.add_reads([r])
            compare(rd, chk, seed, finish=want[0] == 1)


# 9. key 0 (poly-A / poly-T) and a slot hit thousands of times; 10. the same k-mer twice in a read
def check_poly_a(lib_path, k=31, seed=11):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 500) + b"A" * 60 + D.random_seq(rng, 500)
    reads = [b"A" * 300, b"T" * 300, b"a" * 2100, genome[450:620], D.reverse_complement(genome[450:620]), genome[100:200] + genome[100:200]] * 3
    chk, _, _ = run(lib_path, k, [([genome], [])], reads, seed)
    assert chk.table[0] >= 30 and chk.counts[0] > 2000


# 11. two graphs holding the same sequence; 12. unitigs shorter than k, a dead end, a hairpin link, a circular self link
def check_two_graphs_and_shapes(lib_path, k=11, seed=13):
    rng = random.Random(seed)
    a = D.random_seq(rng, 120)
    g1 = ([a], [(1, 1), (-1, -1)])                                  # circular
    g2 = ([a], [])                                                  # the same sequence, linear
    b, c = D.random_seq(rng, 90), D.random_seq(rng, 70)
    g3 = ([b, b"ACG", b"T", b"G", c, b"TTGCA"],                      # b -> ACG -> (T | G) -> c; b hairpins back on itself; TTGCA a dead end off c
          D.both_directions([(1, 2), (2, 3), (2, 4), (3, 5), (4, 5), (-1, 1), (5, 6)]))
    reads = [a + a[:40], a[60:] + a[:60], b + b"ACG" + b"T" + c, b + b"ACGG" + c[:30], D.reverse_complement(b[:50]) + b[:50], c + b"TTGCA"] * 2
    chk, notes, _ = run(lib_path, k, [g1, g2, g3], reads, seed)
    assert chk.totals_dict()["repeat_kmers"] >= 110 and notes["no_depth"] >= 1


# 13. a chain of all-to-all linked levels of two 1-bp unitigs: 2^14 walks against a budget of 10000 steps, links in a shuffled order
def check_step_budget(lib_path, k=31, seed=17, levels=14):
    rng = random.Random(seed)
    seqs = [D.random_seq(rng, 8)]
    links, prev = [], [1]
    for _ in range(levels):
        pair = rng.choice([(b"A", b"C"), (b"G", b"T"), (b"A", b"G"), (b"C", b"T")])
        cur = []
        for s in pair:
            seqs.append(s); cur.append(len(seqs))
        links += [(p, c) for p in prev for c in cur]
        prev = cur
    seqs.append(D.random_seq(rng, 24))
    links += [(p, len(seqs)) for p in prev]
    links = D.both_directions(links)
    rng.shuffle(links)
    m = D.GraphModel(seqs, links)
    steps = [D.MAX_WALK_STEPS]
    assert len(m.extensions(m.next[1], k - 1, steps)) < 2 ** levels and steps[0] == 0      # the budget ran out
    path = [1] + [rng.choice((2 * i + 2, 2 * i + 3)) for i in range(levels)] + [len(seqs)]
    read = b"".join(seqs[u - 1] for u in path)
    run(lib_path, k, [(seqs, links)], [read, D.reverse_complement(read), read], seed)


# 14. batches
def check_batches(lib_path, monkeypatch, k=21, seed=19):
    rng = random.Random(seed)
    seqs, links, genome = cut_genome(rng, D.random_seq(rng, 5000), 10, 3)
    reads = D.sample_reads(rng, genome, 30, 400, sub=0.03) + D.foreign_reads(rng, 8, 300) + [genome[:4500]]      # one read longer than the cap
    rng.shuffle(reads)
    graphs = [(seqs, links)]
    chk = D.Checker(k, graphs); chk.add_reads(reads)
    with ReadDepth(k, graphs, lib_path=lib_path) as rd:
        rd.add_reads(reads)
        compare(rd, chk, seed)
        assert rd.totals()["batches"] == 1
    monkeypatch.setenv("AC_DEPTH_BATCH_BYTES", "3000")
    with ReadDepth(k, graphs, lib_path=lib_path) as rd:
        rd.add_reads(reads)
        compare(rd, D_copy(chk), seed)
        assert rd.totals()["batches"] >= 3
    monkeypatch.delenv("AC_DEPTH_BATCH_BYTES")
    with ReadDepth(k, graphs, lib_path=lib_path) as rd:
        rd.add_reads(reads[:17]); rd.add_reads(reads[17:])
        compare(rd, D_copy(chk), seed)
        assert rd.totals()["batches"] == 2


def D_copy(chk):
    chk.notes = dict(clipped=0, no_depth=0, context_skipped=0)
    return chk


# 15. FASTQ, plain and gzip; a truncated file
def check_fastq(lib_path, tmp_path, k=21, seed=23):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 3000)
    graphs = [([genome], [])]
    reads = D.sample_reads(rng, genome, 20, 300, sub=0.02, circular=False) + D.foreign_reads(rng, 5, 200) + [b"ACGTN" * 10]
    text = b"".join(b"@r%d some text\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    plain, gz, cut, cut_gz = tmp_path / "r.fastq", tmp_path / "r.fastq.gz", tmp_path / "cut.fastq", tmp_path / "cut.fastq.gz"
    plain.write_bytes(text)
    gz.write_bytes(gzip.compress(text))
    cut.write_bytes(text[:len(text) - len(reads[-1]) - 4])      # ends inside the last record
    cut_gz.write_bytes(gzip.compress(text)[:-40])
    chk = D.Checker(k, graphs); chk.add_reads(reads)
    for p in (plain, gz):
        with ReadDepth(k, graphs, lib_path=lib_path) as rd:
            rd.add_fastq(p)
            compare(rd, D_copy(chk), seed)
    for p in (cut, cut_gz):
        with ReadDepth(k, graphs, lib_path=lib_path) as rd:
            with pytest.raises(AutocyclerError, match="truncated FASTQ"):
                rd.add_fastq(p)


# 16. every error of the ABI, matched on its text
def check_errors(lib_path):
    import ctypes as C
    g = ([b"ACGTACGTACGTTTGACCA"], [])
    for k in (10, 12, 9, 33, 5):
        with pytest.raises(AutocyclerError, match="odd number between 11 and 31"):
            ReadDepth(k, [g], lib_path=lib_path)
    for links in ([(1, 0)], [(0, 1)], [(1, 2)], [(-3, 1)]):
        with pytest.raises(AutocyclerError, match="has an end that is 0 or beyond the graph"):
            ReadDepth(11, [(g[0], links)], lib_path=lib_path)
    with ReadDepth(11, [g], lib_path=lib_path) as rd:
        with pytest.raises(AutocyclerError, match="read_off must ascend"):
            rd.add_reads_raw(b"ACGTACGTACGT", [0, 8, 4, 12])
        with pytest.raises(AutocyclerError, match="no reads were found .* which match the consensus assembly"):
            rd.depths(0)
        rd.add_reads([b"GGGGGGGGGGGGGGGGGGGGGG", b"NNNN"])      # a rejected read and an uncounted one: still nothing accepted
        with pytest.raises(AutocyclerError, match="no reads were found .* which match the consensus assembly"):
            rd.depths(0)
        assert rd._lib.ac_depth_finish(rd._h, C.c_uint32(1), None, None) == 1 and b"graph index out of range" in rd._lib.ac_last_error()
        rd.add_reads([g[0][0]])
        assert rd.depths(0) == D_run_single(g, [b"GGGGGGGGGGGGGGGGGGGGGG", b"NNNN", g[0][0]])


def D_run_single(g, reads):
    chk = D.Checker(11, [g]); chk.add_reads(reads)
    return chk.depths(0)


# the numpy tally equals the plain one
def check_numpy_tally(seed):
    rng = random.Random(seed)
    k = rng.choice((11, 21, 31))
    seqs, links, genome = cut_genome(rng, D.random_seq(rng, 3000), 8, 3)
    reads = D.sample_reads(rng, genome, 20, 200, sub=0.05) + D.foreign_reads(rng, 6, 150) + [b"N" * 30, b"ACGT", b"", genome[:100].lower(), b"ACNGT" * 30]
    a, b = D.Checker(k, [(seqs, links)]), D.Checker(k, [(seqs, links)])
    a.add_reads(reads); b.add_reads_numpy(reads)
    assert a.totals == b.totals and a.counts == b.counts and a.totals[0] > 0 and a.totals[1] > 0


# 17. (device only) a mid-size job against the numpy tally
def check_midsize(lib_path, k=21, seed=29):
    rng = random.Random(seed)
    genome = D.random_seq(rng, 150_000)
    genome = genome + genome[20_000:50_000] + D.random_seq(rng, 20_000)      # 200 kbp with a 30 kbp repeat
    seqs, links, _ = cut_genome(rng, genome, 300, 60)
    reads = D.sample_reads_numpy(seed, genome, 1600, 5000, 0.05, foreign_every=5)
    reads += [genome[60_000:60_200] * 4] * 300                               # a pile-up: clipped counts
    chk, notes, t = run(lib_path, k, [(seqs, links)], reads, seed, numpy_tally=True)
    d = chk.totals_dict()
    n = d["reads"] + d["rejected_reads"]
    assert sum(len(r) for r in reads) > 7_500_000
    assert d["reads"] * 10 >= n and d["rejected_reads"] * 10 >= n and d["repeat_kmers"] > 0
    assert notes["clipped"] > 0 and notes["no_depth"] > 0 and notes["context_skipped"] > 0, notes
