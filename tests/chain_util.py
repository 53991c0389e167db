"""compress -> cluster -> trim -> resolve as one chain on planted genomes.

Three parts:
  planted_case   assemblies built from known replicons with differences in known places (plain random.Random(seed)).  What the chain has to
                 return is then known without reading the reference: one unitig per replicon, circular or linear as planted, equal base for
                 base to the planted sequence up to rotation and strand.
  run_chain      the caller's share of the four commands, restated from the reference with its line numbers; everything else is the library.
                 It returns one record of plain values per case (labels, unitig counts, trims, exclusions, the texts, the final S and L lines).
  check_*        what must hold at every stage, stated without a model of the library; every message begins with the stage that broke.

The same functions run on the CPU emulation (test_chain_emu.py) and on the device (test_chain_gpu.py)."""
import math
import random
from collections import Counter

import numpy as np

import parity_util
from autocycler_amd import AutocyclerError, cluster_min_assemblies, graph_from_gfa, graph_subsets, subsets_from_paths

COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
CUTOFF = 0.2            # cluster's --cutoff default
MIN_IDENTITY = 0.75     # trim's --min_identity default
MAX_UNITIGS = 5000      # trim's --max_unitigs default
MAD = 5.0               # trim's --mad default
FAIL_TOO_FEW_ASSEMBLIES = 2


def rc(s):
    return s.translate(COMPLEMENT)[::-1]


def same_circular(a, b):
    """equal canonical rotation over both strands: b is a rotation of a or of its reverse complement"""
    return len(a) == len(b) and (a in b + b or rc(a) in b + b)


def same_linear(a, b):
    return a == b or rc(a) == b


def same_replicon(a, b, circular):
    return same_circular(a, b) if circular else same_linear(a, b)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------------
def _random_bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _kmers(seq, k, circular):
    s = seq + seq[:k - 1] if circular else seq
    for i in range(len(s) - k + 1):
        x = s[i:i + k]
        y = rc(x)
        yield x if x <= y else y


def _check_unique_kmers(k, replicons):
    """no k-mer of the truth occurs twice outside the planted repeat: the only k-mers counted twice are those that lie inside a repeat copy"""
    count, allowed = Counter(), set()
    for r in replicons:
        count.update(_kmers(r["root"], k, r["circular"]))
        if r["repeat"]:
            a, _, n = r["repeat"]
            allowed.update(_kmers(r["root"][a:a + n], k, False))
    twice = {x for x, c in count.items() if c > 1}
    assert all(c <= 2 for c in count.values()) and twice == allowed, "generator: a k-mer of the truth occurs twice outside the planted repeat"


def _free_intervals(length, forbidden):
    """[0, length) without the forbidden intervals (inclusive, already clipped to the sequence)"""
    free, at = [], 0
    for lo, hi in sorted(forbidden):
        if lo > at:
            free.append((at, lo - 1))
        at = max(at, hi + 1)
    if at < length:
        free.append((at, length - 1))
    return free


def _site_candidates(rng, free, length, circular, gap, wanted):
    """positions in the free intervals, consecutive ones at least `gap` apart (around the origin too on a circle): a walk with steps of gap + a
    random extra, the extra as large as still yields `wanted` positions"""
    if wanted == 0:
        return []
    room = sum(hi - lo + 1 for lo, hi in free)
    extra = max(0, 2 * (room // wanted - gap))
    state = rng.getstate()
    while True:
        rng.setstate(state)
        out = []
        for lo, hi in free:
            p = lo + rng.randint(0, extra // 2)
            while p <= hi:
                out.append(p)
                p += gap + rng.randint(0, extra)
        if circular and len(out) > 1 and out[0] + length - out[-1] < gap:
            out.pop()
        if len(out) >= wanted:
            return out
        assert extra > 0, f"generator: no room for {wanted} sites {gap} apart in {room} free bases of {length}"
        extra = extra * 3 // 4


def planted_case(k, replicons, n_assemblies, n_diffs, seed, overrun=(), hairpin=None, missing=None, contaminant=None, junk_tail=None, majority=None,
                 site_gap=None, end_gap=None, name=""):
    """Assemblies of known replicons.

    replicons     [dict(length=, circular=, repeat=0)]: repeat = length of a stretch planted twice (a quarter and three quarters along)
    n_diffs       differences (substitution, one-base insertion, one-base deletion; as many insertions as deletions in every contig) per
                  assembly, spread over the replicons it carries by the room they have: one number, or one per assembly
    overrun       the assemblies whose circular contigs get a start-end overrun, s + s[:m], m = max(2 k, len / 10)
    hairpin       {assembly: "end" or "both"}: the linear contigs of these get s + rc(s[-m:]), or rc(s[:m]) + s + rc(s[-m:])
    missing       {replicon index: [assemblies that lack it]}
    contaminant   (assembly, length): one more contig of random bases in that assembly only
    junk_tail     (assembly, replicon index): that contig gets 15 % random bases behind its end
    majority      (replicon index, [assemblies]): one more site where all of these carry the same substitution; the truth becomes the variant
    site_gap      least distance between two sites of a replicon over all assemblies (default 2 k; always above k, so that no k-mer covers two
                  sites and neighbouring bubbles share at least one k-mer of the truth)
    end_gap       least distance of a site from every contig end, overrun boundary and repeat copy of every assembly (default 2 k)

    Returns a dict: k, seqs, filenames, headers (compress's order: file names ascending, contigs in file order), truth [dict(seq, root,
    circular)], contigs [dict(replicon, free, overrun)] per sequence (replicon None = the contaminant; overrun "", "start_end", "hairpin_end",
    "hairpin_both"), plus what was asked for."""
    rng = random.Random(seed)
    site_gap = 2 * k if site_gap is None else site_gap
    end_gap = 2 * k if end_gap is None else end_gap
    assert site_gap > k and end_gap > k, "generator: a k-mer would cover two sites, or a site and a contig end"
    hairpin, missing = dict(hairpin or {}), dict(missing or {})
    per_assembly = list(n_diffs) if isinstance(n_diffs, (list, tuple)) else [n_diffs] * n_assemblies
    assert len(per_assembly) == n_assemblies
    # the truth
    for _ in range(20):
        truth = []
        for spec in replicons:
            root, rep = bytearray(_random_bases(rng, spec["length"])), None
            if spec.get("repeat"):
                n, a, b = spec["repeat"], spec["length"] // 4, 3 * spec["length"] // 4
                assert n > k and a + n < b and b + n < spec["length"]
                root[b:b + n] = root[a:a + n]
                rep = (a, b, n)
            truth.append(dict(root=bytes(root), circular=bool(spec["circular"]), repeat=rep))
        extra = [dict(root=_random_bases(rng, contaminant[1]), circular=False, repeat=None)] if contaminant else []
        try:
            _check_unique_kmers(k, truth + extra)
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("generator: a k-mer of the truth occurs twice outside the planted repeat")
    # per replicon: who carries it, where every contig begins, where its overrun ends, and what that leaves free for sites
    plans = []
    most = max(per_assembly)      # (an insertion or deletion before a boundary moves it by one base)
    for ri, t in enumerate(truth):
        L = len(t["root"])
        carriers = [a for a in range(n_assemblies) if a not in missing.get(ri, ())]
        is_majority = majority is not None and majority[0] == ri
        forbidden, rotation = [], {}
        if t["repeat"]:
            a, b, n = t["repeat"]
            forbidden += [(a - end_gap, a + n - 1 + end_gap), (b - end_gap, b + n - 1 + end_gap)]
        for a in carriers:
            if t["circular"]:
                rotation[a] = rng.randrange(L)
                points = [rotation[a]] + ([rotation[a] + max(2 * k, L // 10)] if a in overrun else [])
            else:
                m = max(2 * k, L // 10)
                points = [0, L - 1] + ([L - m] if a in hairpin else []) + ([m] if hairpin.get(a) == "both" else [])
            for p in points:
                lo, hi = p - most - end_gap, p + most + end_gap
                if hi - lo + 1 >= L:
                    forbidden.append((0, L - 1))
                elif t["circular"]:      # (an interval that crosses the origin is cut in two)
                    lo, hi = lo % L, hi % L
                    forbidden += [(lo, hi)] if lo <= hi else [(lo, L - 1), (0, hi)]
                else:
                    forbidden.append((max(lo, 0), min(hi, L - 1)))
        # (a replicon that fewer than 5 assemblies carry takes no sites: with 3 or 4 one diverted contig can leave two paths at a bridge, a tie)
        free = _free_intervals(L, forbidden) if len(carriers) >= 5 or is_majority else []
        plans.append(dict(carriers=carriers, rotation=rotation, forbidden=forbidden, free=free, variant=None, is_majority=is_majority,
                          capacity=sum((hi - lo + 1) // site_gap for lo, hi in free) - int(is_majority), sites={a: 0 for a in carriers}))
    # an assembly's differences go to the replicons it carries, by the room they have left
    for a in range(n_assemblies):
        for _ in range(per_assembly[a]):
            room = [max(p["capacity"] - sum(p["sites"].values()), 0) if a in p["carriers"] else 0 for p in plans]
            assert sum(room) > 0, f"generator: no room left for the differences of assembly {a}"
            plans[rng.choices(range(len(plans)), weights=room)[0]]["sites"][a] += 1
    for t, plan in zip(truth, plans):
        L = len(t["root"])
        wanted = sum(plan["sites"].values()) + int(plan["is_majority"])
        sites = rng.sample(_site_candidates(rng, plan["free"], L, t["circular"], site_gap, wanted), wanted)
        ordered = sorted(sites)
        for x, y in zip(ordered, ordered[1:] + ([ordered[0] + L] if t["circular"] and len(ordered) > 1 else [])):
            assert y - x >= site_gap, "generator: two sites are too close"
        for s in sites:
            assert not any(lo <= s <= hi for lo, hi in plan["forbidden"]), "generator: a site is too close to a contig end, an overrun boundary or the repeat"
        if plan["is_majority"]:
            s = sites.pop()
            plan["variant"] = (s, rng.choice([c for c in b"ACGT" if c != t["root"][s]]))
            assert 2 * len(majority[1]) > len(plan["carriers"]) and set(majority[1]) <= set(plan["carriers"])
        # in every contig insertions and deletions balance: exclude_outliers_in_length (trim.rs:236-240) allows median +- 5 MAD, and with most
        # contigs at the planted length the MAD is 0: the reference then excludes a contig that is one base longer
        drawn = {}
        for a, n in plan["sites"].items():
            pairs = rng.randint(min(1, n // 2), n // 2)
            kinds = ["ins", "del"] * pairs + ["sub"] * (n - 2 * pairs)
            rng.shuffle(kinds)
            drawn[a] = [(sites.pop(), kind) for kind in kinds]
        plan["sites"] = drawn
        t["seq"] = t["root"]
        if plan["variant"]:
            v = bytearray(t["root"]); v[plan["variant"][0]] = plan["variant"][1]
            t["seq"] = bytes(v)
    # the contigs
    seqs, filenames, headers, contigs = [], [], [], []
    for a in range(n_assemblies):
        for ri, (t, plan) in enumerate(zip(truth, plans)):
            if a not in plan["carriers"]:
                continue
            L = len(t["root"])
            s = bytearray(t["root"])
            edits = list(plan["sites"][a])
            carries_variant = plan["variant"] is not None and a in majority[1]
            if carries_variant:
                s[plan["variant"][0]] = plan["variant"][1]
            for pos, kind in sorted(edits, reverse=True):      # (from the back, so that the positions before an edit stay put)
                if kind == "sub":
                    s[pos] = rng.choice([c for c in b"ACGT" if c != s[pos]])
                elif kind == "ins":
                    s[pos:pos] = bytes([rng.choice(b"ACGT")])
                else:
                    del s[pos]
            s = bytes(s)
            what = ""
            if t["circular"]:
                cut = plan["rotation"][a] + sum((kind == "ins") - (kind == "del") for pos, kind in edits if pos < plan["rotation"][a])
                s = s[cut:] + s[:cut]
                if a in overrun:
                    s, what = s + s[:max(2 * k, len(s) // 10)], "start_end"
            elif a in hairpin:
                m = max(2 * k, len(s) // 10)
                s, what = (rc(s[:m]) if hairpin[a] == "both" else b"") + s + rc(s[-m:]), "hairpin_" + hairpin[a]
            if rng.random() < 0.5:
                s = rc(s)
            if junk_tail == (a, ri):
                assert not what
                s += _random_bases(rng, len(s) * 15 // 100)
            seqs.append(s.decode()); filenames.append(f"assembly_{a:02d}.fasta"); headers.append(f"contig_{ri + 1} replicon {ri}")
            contigs.append(dict(replicon=ri, free=not edits and (plan["variant"] is None or carries_variant), overrun=what, junk=junk_tail == (a, ri)))
        if contaminant and contaminant[0] == a:
            seqs.append(extra[0]["root"].decode()); filenames.append(f"assembly_{a:02d}.fasta"); headers.append("contig_9 contaminant")
            contigs.append(dict(replicon=None, free=False, overrun="", junk=False))
    return dict(name=name, k=k, seed=seed, seqs=seqs, filenames=filenames, headers=headers, contigs=contigs,
                truth=[dict(seq=t["seq"], root=t["root"], circular=t["circular"]) for t in truth], majority=majority, junk_tail=junk_tail,
                contaminant=contaminant)


# ---- the glue -----------------------------------------------------------------------------------------------------------------------------------
def median_isize(values):
    """misc.rs:433-440"""
    if not values:
        return 0
    v = sorted(values)
    n = len(v)
    return (v[n // 2 - 1] + v[n // 2]) // 2 if n % 2 == 0 else v[n // 2]      # (lengths and deviations are never negative: // is Rust's /)


def mad_isize(values):
    """misc.rs:452-457"""
    if not values:
        return 0
    m = median_isize(values)
    return median_isize([abs(v - m) for v in values])


def allowed_length_range(lengths, mad=MAD):
    """exclude_outliers_in_length, trim.rs:236-240: f64::round is half away from zero and `as usize` saturates at 0"""
    median, dev = median_isize(lengths), mad_isize(lengths)
    rnd = lambda x: max(0, int(math.floor(x + 0.5)))
    return rnd(float(median) - float(dev) * mad), rnd(float(median) + float(dev) * mad)


def choose_trim_type(results):
    """trim.rs:189-226: the kind with more successes, start-end on a tie; None when neither kind trimmed anything"""
    c_se, c_hp = sum(r["start_end"]["status"] == 1 for r in results), sum(r["hairpin"]["status"] == 1 for r in results)
    if c_se == 0 and c_hp == 0:
        return None
    return "start_end" if c_se >= c_hp else "hairpin"


def graph_arrays(graph):
    """a handle's unitigs, links and paths as the plain-array entries take them (copies: they outlive the handle)"""
    b = graph.bulk()
    links = np.stack([b["links"]["a"], b["links"]["b"]], axis=1).astype(np.int32) if len(b["links"]) else np.zeros((0, 2), dtype=np.int32)
    off = b["path_off"].tolist()
    entries = b["path_entries"].tolist()
    return dict(n=graph.unitig_count, links=links, lens=np.array(b["seq_len"], dtype=np.uint32), depth=np.array(b["depth"]),
                sequences=(np.append(np.array(b["seq_bytes"], dtype=np.uint8), np.uint8(0)), np.array(b["seq_begin"], dtype=np.uint64)),
                paths=[entries[off[i]:off[i + 1]] for i in range(len(off) - 1)])


def finish_cluster(stage, sub, c, k, meta, lengths, sequences=None, tag=None, device=0):
    """merge_linear_paths and save_gfa on cluster c of `sub`, then the file read again: (Graph, text, kept sequence indices)"""
    try:
        plan = sub.merge_plan(c, sequences=sequences, device=device)
        mp = sub.merged_paths(c, plan, device=device, keep=True)
        fin = sub.finish(c, plan, mp, renumber=True, sequences=sequences, device=device)
        kept = fin.path_seq.tolist()
        args = ([meta["ids"][s] for s in kept], [lengths[s] for s in kept], [meta["filenames"][s] for s in kept], [meta["headers"][s] for s in kept])
        graph = fin.to_graph(k, *args)
        text = fin.gfa(k, *args, cluster_tags=[tag] * len(kept) if tag is not None else None)
    except AutocyclerError as e:
        raise AssertionError(f"{stage}: the library refuses the graph: {e}") from e
    fin.close(); mp.close(); plan.close()
    return graph, text, kept


def gfa_segments_and_links(text):
    """the S lines as (number, sequence, depth) and the L lines as signed pairs"""
    segs, links = [], []
    for line in text.decode().splitlines():
        f = line.split("\t")
        if f[0] == "S":
            depth = [float(x[5:]) for x in f[3:] if x.startswith("DP:f:")]
            segs.append((int(f[1]), f[2], depth[0] if depth else None))
        elif f[0] == "L":
            links.append((int(f[1]) if f[2] == "+" else -int(f[1]), int(f[3]) if f[4] == "+" else -int(f[3])))
    return segs, links


def check_handle(stage, graph, want, exact=True, lengths=None):
    """what holds of every handle in play: each sequence decompresses to its input bytes (after trim: to a substring of its input of exactly
    the trimmed length), every unitig's depth is the number of path entries that name it on either strand, every consecutive pair of path
    entries is a link, and the link set is closed under reverse complement"""
    a = graph_arrays(graph)
    assert len(a["paths"]) == len(want), f"{stage}: {len(a['paths'])} paths for {len(want)} sequences"
    for i, w in enumerate(want):
        got = graph.decompress(i)
        if exact:
            assert got == w, f"{stage}: sequence {i} does not decompress to its input"
        else:
            assert len(got) == lengths[i] and got in w, f"{stage}: sequence {i} does not decompress to {lengths[i]} bytes of its input"
    named = np.bincount(np.abs(np.array([e for p in a["paths"] for e in p], dtype=np.int64)), minlength=a["n"] + 1)[1:] if a["n"] else np.zeros(0)
    assert a["depth"].tolist() == [float(x) for x in named.tolist()], f"{stage}: a unitig's depth is not the number of path entries that name it"
    links = {(int(x), int(y)) for x, y in a["links"].tolist()}
    assert len(links) == len(a["links"]), f"{stage}: a link is listed twice"
    for p in a["paths"]:
        for pair in zip(p, p[1:]):
            assert pair in links, f"{stage}: consecutive path entries {pair} are not a link"
    for x, y in links:
        assert (-y, -x) in links, f"{stage}: link {x} -> {y} has no reverse complement"
    return a


def run_from(case, graph, meta, inputs, lib_path, device, checks=True):
    """cluster, trim and resolve from one handle of the compressed graph: a record of plain values"""
    k, n_seqs = case["k"], len(case["seqs"])
    originals = [s.encode() for s in case["seqs"]]
    rec = dict(clusters={})
    if checks:
        check_handle("compress", graph, originals)
    # cluster (cluster.rs:44-56): the tree, generate_clusters with the default cutoff and the automatic --min_assemblies
    tree, distances = graph.cluster_tree(device=device, want_distances=True)
    qc = tree.generate(distances, inputs["seq_len"], inputs["assembly"], inputs["cluster_weight"], inputs["trusted"], CUTOFF,
                       cluster_min_assemblies(inputs["assembly"], lib_path), device=device)
    tree.close()
    rec["clustered"] = list(qc.cluster_of_seq)
    rec["fail"] = [r["fail"] for r in qc.records]
    # save_qc_pass_clusters (cluster.rs:735-760): only a cluster that passed goes on; its number stays, so the numbers of failed ones are left empty
    labels = [c if qc.records[c - 1]["fail"] == 0 else 0 for c in qc.cluster_of_seq]
    rec["labels"] = labels
    sub = graph_subsets(graph, labels, max(max(labels), 1), device=device)
    rec["empty_clusters"] = [c for c in range(1, sub.n_clusters + 1) if c not in labels]
    lengths = [len(s) for s in originals]
    for c in range(1, sub.n_clusters + 1):
        if c not in labels:
            continue
        # save_cluster_gfa (cluster.rs:794-806).  The file's unitig numbers are those after the merge; the handle's are renumbered, a bijection
        # that nothing downstream reads: trim compares path entries for equality only and renumbers at its end
        gc, untrimmed, kept = finish_cluster(f"cluster {c} untrimmed", sub, c, k, meta, lengths, tag=c, device=device)
        want = [originals[s] for s in kept]
        if checks:
            check_handle(f"cluster {c} untrimmed", gc, want)
        a = graph_arrays(gc)
        # trim (trim.rs:43-50) with the reference's defaults
        results, summary = gc.trim_paths(MIN_IDENTITY, MAX_UNITIGS, device=device)
        assert all(r["start_end"]["status"] != 2 and r["hairpin"]["status"] != 2 for r in results), f"cluster {c} trim: a slice the reference would reject"
        kind = choose_trim_type(results)
        assert summary["chosen"] == {None: 0, "start_end": 1, "hairpin": 2}[kind], f"cluster {c} trim: the library's count of the two kinds differs"
        sliced, trimmed_len = [], []
        for p, r, s in zip(a["paths"], results, kept):
            if kind is not None and r[kind]["status"] == 1:      # (create_sequence_and_positions with the trimmed path and trimmed_length)
                sliced.append(p[r[kind]["begin"]:r[kind]["end"]]); trimmed_len.append(r[kind]["trimmed_length"])
            else:
                sliced.append(p); trimmed_len.append(lengths[s])
        lo, hi = allowed_length_range(trimmed_len)
        keep = [1 if lo <= n <= hi else 0 for n in trimmed_len]      # (an excluded sequence: label 0)
        # clean_up_graph (trim.rs:260-269): recalculate_depths, remove_zero_depth_unitigs, merge_linear_paths, renumber_unitigs
        sub_t = subsets_from_paths(a["n"], a["links"], a["lens"], sliced, keep, 1, device=device, lib_path=lib_path)
        local_meta = dict(ids=[meta["ids"][s] for s in kept], filenames=[meta["filenames"][s] for s in kept], headers=[meta["headers"][s] for s in kept])
        gt, trimmed, kept_t = finish_cluster(f"cluster {c} trimmed", sub_t, 1, k, local_meta, trimmed_len, sequences=a["sequences"], device=device)
        sub_t.close()
        if checks:
            check_handle(f"cluster {c} trimmed", gt, [want[i] for i in kept_t], exact=False, lengths=[trimmed_len[i] for i in kept_t])
        # resolve (resolve.rs:41-67)
        bridged, merged, final, culled = gt.resolve_graphs(device=device)
        segs, links = gfa_segments_and_links(final)
        rec["clusters"][c] = dict(
            seqs=kept, unitigs_before=gc.unitig_count, longest_path=max(len(p) for p in a["paths"]), chosen=kind or "",
            trimmed_start_end=[s for s, r in zip(kept, results) if r["start_end"]["status"] == 1],
            trimmed_hairpin=[s for s, r in zip(kept, results) if r["hairpin"]["status"] == 1],
            hairpin_both=[s for s, r in zip(kept, results) if r["hairpin_start_trimmed"] and r["hairpin_end_trimmed"]],
            trimmed_lengths=trimmed_len, length_range=(lo, hi), excluded=[s for s, x in zip(kept, keep) if not x],
            resolved_seqs=[kept[i] for i in kept_t], unitigs_after=gt.unitig_count, trimmed_sequences=[gt.decompress(i) for i in range(len(kept_t))],
            untrimmed_gfa=untrimmed, trimmed_gfa=trimmed, bridged_gfa=bridged, merged_gfa=merged, final_gfa=final, culled=culled,
            final_segments=[(n, s) for n, s, _ in segs], final_links=links)
        gc.close(); gt.close()
    sub.close()
    return rec


TEXTS = ("untrimmed_gfa", "trimmed_gfa", "bridged_gfa", "merged_gfa", "final_gfa")


def run_chain(case, lib_path=None, device=0, checks=True):
    """The whole chain on one planted case, from the built handle and from the GFA text read again; both must print the same text at every
    stage.  Returns the record of the built handle's run, with the compress facts added."""
    k = case["k"]
    g, gfa, loaded = parity_util.check_case(k, case["seqs"], case["filenames"], case["headers"], lib_path=lib_path, device=device)      # compress, held to the oracle
    assert [q["filename"] for q in loaded] == case["filenames"] and [q["header"] for q in loaded] == case["headers"], "compress: the generator's order is not compress's"
    assert [q["length"] for q in loaded] == [len(s) for s in case["seqs"]]
    meta = dict(ids=[q["id"] for q in loaded], filenames=case["filenames"], headers=case["headers"])
    g2, fns, hds = graph_from_gfa(gfa, lib_path=lib_path)
    assert fns == case["filenames"] and hds == case["headers"], "compress: the text does not read back with its file names and headers"
    inputs = g2.cluster_inputs()      # (per sequence, from the file names and headers: the same for both handles)
    rec = run_from(case, g, meta, inputs, lib_path, device, checks)
    again = run_from(case, g2, meta, inputs, lib_path, device, checks)
    for key in ("clustered", "fail", "labels", "empty_clusters"):
        assert rec[key] == again[key], f"two entry forms: {key} differs between the built handle and the text read again"
    assert sorted(rec["clusters"]) == sorted(again["clusters"]), "two entry forms: the clusters differ"
    for c in rec["clusters"]:
        for key in rec["clusters"][c]:
            assert rec["clusters"][c][key] == again["clusters"][c][key], f"two entry forms: cluster {c} {key} differs between the built handle and the text read again"
    rec.update(name=case["name"], k=k, compress_unitigs=g.unitig_count, compress_gfa=gfa, lib_path=str(lib_path) if lib_path else None)
    g.close(); g2.close()
    return rec


# ---- the checks on the record ---------------------------------------------------------------------------------------------------------------
def replicon_clusters(case, rec):
    """cluster: the labels partition the sequences exactly by planted replicon -> {replicon index: cluster number}"""
    by_replicon = {}
    for s, (c, label) in enumerate(zip(case["contigs"], rec["labels"])):
        if c["replicon"] is None:
            continue
        if c["junk"] and label == 0:
            continue
        by_replicon.setdefault(c["replicon"], set()).add(label)
    assert all(len(v) == 1 and 0 not in v for v in by_replicon.values()), f"cluster: a replicon's contigs are spread over the labels {by_replicon}"
    assert len({next(iter(v)) for v in by_replicon.values()}) == len(by_replicon), f"cluster: two replicons share a label {by_replicon}"
    assert sorted(by_replicon) == list(range(len(case["truth"]))), "cluster: a replicon has no cluster"
    return {r: next(iter(v)) for r, v in by_replicon.items()}


def check_cluster(case, rec, junk_fails_alone=None):
    """junk_fails_alone: for a case with a junk tail, whether that contig fails QC in a cluster of its own (True) or stays with its replicon"""
    of = replicon_clusters(case, rec)
    for s, c in enumerate(case["contigs"]):
        if c["replicon"] is None:      # the contaminant: a cluster of its own that fails for too few assemblies, and only for that
            own = rec["clustered"][s]
            assert rec["clustered"].count(own) == 1 and rec["fail"][own - 1] == FAIL_TOO_FEW_ASSEMBLIES and rec["labels"][s] == 0, \
                f"cluster: the contaminant is in cluster {own} with fail bits {rec['fail'][own - 1]}"
            assert own in rec["empty_clusters"], "cluster: the contaminant's cluster number was not left empty"
        elif c["junk"]:
            assert junk_fails_alone is not None, "cluster: say per case what becomes of the junk-tailed contig"
            own = rec["clustered"][s]
            if junk_fails_alone:
                assert rec["labels"][s] == 0 and rec["clustered"].count(own) == 1 and rec["fail"][own - 1] & FAIL_TOO_FEW_ASSEMBLIES, \
                    f"cluster: the junk-tailed contig was expected to fail alone, it is in cluster {own} with label {rec['labels'][s]}"
            else:
                assert rec["labels"][s] == of[c["replicon"]], f"cluster: the junk-tailed contig was expected in its replicon's cluster, its label is {rec['labels'][s]}"
        else:
            assert rec["labels"][s] == of[c["replicon"]], f"cluster: sequence {s} has label {rec['labels'][s]}"
    passing = sorted(set(rec["labels"]) - {0})
    assert passing == sorted(of.values()) == sorted(rec["clusters"]), f"cluster: the passing clusters {passing} are not the replicons' {of}"
    return of


def check_trim(case, rec, of):
    for r, c in of.items():
        cl, t = rec["clusters"][c], case["truth"][r]
        planted_se = [s for s in cl["seqs"] if case["contigs"][s]["overrun"] == "start_end"]
        planted_hp = [s for s in cl["seqs"] if case["contigs"][s]["overrun"].startswith("hairpin")]
        planted_both = [s for s in cl["seqs"] if case["contigs"][s]["overrun"] == "hairpin_both"]
        if t["circular"]:
            assert cl["chosen"] == ("start_end" if planted_se else ""), f"cluster {c} trim: kind {cl['chosen']!r} chosen for a circular replicon"
            assert cl["trimmed_start_end"] == planted_se, f"cluster {c} trim: start-end trimmed {cl['trimmed_start_end']}, planted {planted_se}"
        else:
            assert cl["chosen"] == ("hairpin" if planted_hp else ""), f"cluster {c} trim: kind {cl['chosen']!r} chosen for a linear replicon"
            assert cl["trimmed_hairpin"] == planted_hp, f"cluster {c} trim: hairpin trimmed {cl['trimmed_hairpin']}, planted {planted_hp}"
            assert cl["hairpin_both"] == planted_both, f"cluster {c} trim: trimmed at both ends {cl['hairpin_both']}, planted {planted_both}"
        junk = [s for s in cl["seqs"] if case["contigs"][s]["junk"]]
        assert cl["excluded"] == junk, f"cluster {c} trim: excluded by length {cl['excluded']}, the junk-tailed contigs are {junk}"
        assert cl["resolved_seqs"] == [s for s in cl["seqs"] if s not in junk]
        for s, got in zip(cl["resolved_seqs"], cl["trimmed_sequences"]):
            if case["contigs"][s]["free"]:
                assert same_replicon(got, t["seq"], t["circular"]), f"cluster {c} trim: sequence {s} has no differences and is not its replicon after trim"


def check_resolve(case, rec, of):
    for r, c in of.items():
        cl, t = rec["clusters"][c], case["truth"][r]
        assert cl["culled"] == 0, f"cluster {c} resolve: {cl['culled']} bridges culled"
        assert len(cl["final_segments"]) == 1, f"cluster {c} resolve: {len(cl['final_segments'])} unitigs in the final graph"
        (u, seq), = cl["final_segments"]
        seq = seq.encode()
        assert len(seq) == len(t["seq"]), f"cluster {c} resolve: the unitig has {len(seq)} bases, planted {len(t['seq'])}"
        assert same_replicon(seq, t["seq"], t["circular"]), f"cluster {c} resolve: the unitig is not the planted sequence"
        if t["seq"] != t["root"]:
            assert not same_replicon(seq, t["root"], t["circular"]), f"cluster {c} resolve: the unitig is the root, not the majority's variant"
        hairpins = any(case["contigs"][s]["overrun"].startswith("hairpin") for s in cl["seqs"])
        want = [(u, u), (-u, -u)] if t["circular"] else ([(u, -u), (-u, u)] if hairpins else [])
        assert sorted(cl["final_links"]) == sorted(want), f"cluster {c} resolve: links {cl['final_links']}, expected {want}"
        # resolve.rs:57-67: with nothing culled the final graph is the merged one, saved with the other colour
        b_segs, _ = gfa_segments_and_links(cl["bridged_gfa"])
        m_segs, m_links = gfa_segments_and_links(cl["merged_gfa"])
        assert [(n, s) for n, s, _ in m_segs] == cl["final_segments"] and m_links == cl["final_links"], f"cluster {c} resolve: the final graph is not the merged one"
        assert len(m_segs) <= len(b_segs), f"cluster {c} resolve: more unitigs after the merge than before"
        weigh = lambda segs: sum(len(s) * d for _, s, d in segs)      # (a merged unitig's depth is the length-weighted mean of its parts)
        assert math.isclose(weigh(b_segs), weigh(m_segs), rel_tol=1e-9), f"cluster {c} resolve: bases times depth {weigh(b_segs)} before the merge, {weigh(m_segs)} after"
        # (3_bridged.gfa keeps the trimmed graph's numbers with holes in them, which the library's loader does not take: the reference reads that
        # file nowhere either; its lines are read by gfa_segments_and_links above)
        for key in ("merged_gfa", "final_gfa"):
            g, _, _ = graph_from_gfa(cl[key], lib_path=rec["lib_path"])
            segs, links = gfa_segments_and_links(cl[key])
            assert g.unitig_count == len(segs) and g.stats_post["total_length"] == sum(len(s) for _, s, _ in segs), f"cluster {c} resolve: {key} does not read back"
            g.close()
    total = sum(len(s) for c in of.values() for _, s in rec["clusters"][c]["final_segments"])
    assert total == sum(len(t["seq"]) for t in case["truth"]), f"resolve: {total} bases in the final graphs"


def check_record(case, rec, junk_fails_alone=None):
    of = check_cluster(case, rec, junk_fails_alone)
    check_trim(case, rec, of)
    check_resolve(case, rec, of)
    return of


def facts(case, rec):
    """the per-case facts the documentation quotes"""
    return dict(name=rec["name"], k=rec["k"], sequences=len(case["seqs"]), compress_unitigs=rec["compress_unitigs"], labels=rec["labels"], fail=rec["fail"],
                clusters={c: dict(unitigs_before=cl["unitigs_before"], unitigs_after=cl["unitigs_after"], longest_path=cl["longest_path"], chosen=cl["chosen"],
                                  start_end=len(cl["trimmed_start_end"]), hairpin=len(cl["trimmed_hairpin"]), excluded=len(cl["excluded"]),
                                  final=[(n, len(s)) for n, s in cl["final_segments"]], links=cl["final_links"]) for c, cl in rec["clusters"].items()})


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
CIRC = lambda length, repeat=0: dict(length=length, circular=True, repeat=repeat)
LIN = lambda length: dict(length=length, circular=False, repeat=0)


def make_case(name, seed=1):
    """The table of cases.  Sites are 2 k apart and 2 k from every end wherever the row's differences fit its replicons that way; the rows
    where they cannot (60 sites 102 apart do not fit 8 000 bases) state their own gaps, always above k."""
    small = dict(overrun=(0, 2, 4), missing={1: [3]})
    if name == "small":
        return planted_case(21, [CIRC(3000), CIRC(500)], 5, 3, seed, name=name, **small)
    if name == "clean":
        return planted_case(21, [CIRC(3000), CIRC(500)], 5, 0, seed, missing={1: [3]}, name=name)
    if name == "wide51":
        return planted_case(51, [CIRC(8000), CIRC(900)], 6, 10, seed, overrun=(1, 3), name=name, site_gap=60)
    if name == "wide101":
        return planted_case(101, [CIRC(8000), CIRC(900)], 5, 10, seed, overrun=(1, 3), name=name, site_gap=102, end_gap=102)
    if name == "repeat_contaminant":
        return planted_case(21, [CIRC(6000, 200), CIRC(500)], 7, 12, seed, overrun=(0, 2, 4, 6), contaminant=(3, 800), name=name)
    if name == "medium":
        return planted_case(51, [CIRC(20000, 300), CIRC(900)], 8, 30, seed, overrun=(0, 2, 4, 6), name=name, site_gap=56)
    if name == "hairpin21":
        return planted_case(21, [CIRC(3000), LIN(800)], 6, [2, 2, 0, 2, 0, 2], seed, overrun=(0, 2, 4), hairpin={0: "end", 1: "both", 3: "end", 4: "end"}, name=name)
    if name == "hairpin51":
        return planted_case(51, [CIRC(6000), LIN(1500)], 6, [2, 2, 0, 2, 0, 2], seed, overrun=(0, 2, 4), hairpin={0: "end", 1: "both", 3: "end", 4: "end"}, name=name)
    if name == "outlier":
        return planted_case(21, [CIRC(3000), CIRC(500)], 5, 3, seed, junk_tail=(1, 0), name=name, **small)
    if name == "majority":
        return planted_case(21, [CIRC(3000), CIRC(500)], 5, 3, seed, majority=(0, [0, 1, 2]), name=name, **small)
    if name == "large":
        return planted_case(21, [CIRC(120000), CIRC(900)], 8, 180, seed, overrun=(0, 2, 4, 6), name=name)
    raise KeyError(name)
