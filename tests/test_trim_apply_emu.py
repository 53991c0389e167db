"""ac_trim_apply / ac_graph_trim_apply / ac_graph_trim, the Trimmed object, ac_trim_gfa, ac_trim_dir and the `trim` and `resolve` commands of
the CLI on the CPU emulation of the shipped kernels (kernels_trim_apply.inc, then the stages of kernels_subset.inc) against the literal Python
model of trim_apply_util.py: choose_trim_type, the slices with create_sequence_and_positions' assertion, exclude_outliers_in_length,
clean_up_graph, save_gfa and the yaml.  Every comparison is equality.  The chain check does not rest on that model: it holds Graph.trim to
the glue of chain_util.run_from.  The same checks run on the device in test_trim_apply_gpu.py."""
import random
import re
import subprocess
import tempfile
from pathlib import Path

import pytest

import chain_util as CU
import emu_lib
import finish_util as F
import merge_util as M
import parity_util
import subset_util as S
import trim_apply_util as TA
import trim_util as T
from autocycler_amd import AutocyclerError, graph_from_gfa, resolve_dir, trim_apply, trim_dir, trim_gfa
from autocycler_amd import _capi
from test_chain_emu import CASES as CHAIN_CASES      # (the cases the emulation's chain test uses; test_chain_gpu.py adds only the large one)

NEW_SYMBOLS = ("ac_trim_apply", "ac_graph_trim_apply", "ac_graph_trim", "ac_trimmed_records", "ac_trimmed_summary_get_sized", "ac_trimmed_free", "ac_trimmed_subsets",
               "ac_trimmed_finish", "ac_trimmed_yaml_string", "ac_trim_gfa", "ac_trim_dir", "ac_resolve_dir")
K = 7      # the k-mer size the texts are printed with (the H line only)
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def scan_tile():
    """the device scan's tile, read from device_prims.hpp"""
    text = (ROOT / "autocycler_amd" / "csrc" / "device_prims.hpp").read_text()
    m = re.search(r"SCAN_ITEMS = (\d+), SCAN_TILE = (\d+) \* SCAN_ITEMS", text)
    return int(m.group(1)) * int(m.group(2))


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_trim_apply(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


# ---- cases on plain arrays ---------------------------------------------------------------------------------------------------------------------
def full_results(paths, lens):
    """nothing trimmed, as the library reports it: the slice is the whole path"""
    out = []
    for p in paths:
        full = dict(status=0, begin=0, end=len(p), trimmed_length=sum(lens[abs(e) - 1] for e in p if 0 < abs(e) <= len(lens)))
        out.append(dict(start_end=dict(full), hairpin=dict(full), hairpin_start_trimmed=0, hairpin_end_trimmed=0))
    return out


def make_case(paths, lens, slices=(), mad=5.0, chosen="auto", alive=None, seq_lengths=None, with_seqs=True, links=None):
    """slices: (sequence, kind, begin, end[, status[, length]]); the length defaults to what the slice adds up to"""
    n = len(lens)
    results = full_results(paths, lens)
    for sl in slices:
        s, kind, b, e = sl[:4]
        status = sl[4] if len(sl) > 4 else 1
        length = sl[5] if len(sl) > 5 else sum(lens[abs(x) - 1] for x in paths[s][b:e])
        TA.with_slice(results, s, kind, b, e, length, status)
    return dict(n=n, links=M.closed_set(TA.path_links(paths)) if links is None else links, lens=list(lens), paths=[list(p) for p in paths],
                seq_lengths=list(seq_lengths) if seq_lengths is not None else [sum(lens[abs(e) - 1] for e in p) for p in paths], results=results, mad=mad,
                chosen=chosen, alive=alive, seqs=[M._seq_of(u, l) for u, l in enumerate(lens, 1)] if with_seqs else None)


def run_library(case, lib_path, device=0):
    return trim_apply(case["n"], case["links"], case["lens"], case["paths"], case["seq_lengths"], case["results"], chosen=case["chosen"], mad=case["mad"],
                      alive=case["alive"], device=device, lib_path=lib_path)


def run_model(case, finish=True):
    return TA.trim_apply_model(case["n"], case["links"], case["lens"], case["paths"], case["seq_lengths"], case["results"], case["chosen"], case["mad"], case["alive"],
                               case["seqs"]) if finish else None


def metas_of(n_seqs):
    return [s + 1 for s in range(n_seqs)], [f"hand_{s % 3}.fasta" for s in range(n_seqs)], [f"contig_{s}" for s in range(n_seqs)]


def library_text(t, fin, k, ids, filenames, headers, tags=None):
    kept = t.kept
    assert fin.path_seq.tolist() == kept
    return fin.gfa(k, [ids[s] for s in kept], [int(t.records["length"][s]) for s in kept], [filenames[s] for s in kept], [headers[s] for s in kept],
                   [tags[s] for s in kept] if tags else None)


def check_case(case, lib_path, device=0, what=""):
    """one case: summary, records, the trimmed graph before the merge, the finished graph, the text and the yaml against the model -> (model, summary)"""
    exp = run_model(case)
    t = run_library(case, lib_path, device)
    sm = t.summary
    assert (sm["chosen"], sm["c_se"], sm["c_hp"], sm["rejected"]) == (exp["kind"], exp["c_se"], exp["c_hp"], exp["rejected"]), (what, sm)
    assert (sm["median"], sm["mad"], sm["min_length"], sm["max_length"]) == (exp["median"], exp["mad"], exp["min"], exp["max"]), (what, sm)
    assert [tuple(r) for r in t.records.tolist()] == exp["records"], (what, t.records.tolist(), exp["records"])
    assert (sm["sequences"], sm["trimmed"], sm["excluded"]) == (len(exp["records"]), sum(r[3] for r in exp["records"]), sum(r[4] for r in exp["records"])), what
    assert t.kept == exp["kept"], what
    S.assert_cluster_same(S.library_cluster(t.subsets, 1), exp["cluster"], what)
    assert (sm["unitigs_in"], sm["unitigs_alive"], sm["entries_kept"], sm["links"]) == (case["n"], len(exp["cluster"]["unitigs"]), exp["cluster"]["entries"],
                                                                                      len(exp["cluster"]["links"])), (what, sm)
    fin = t.finish(sequences=TA.seq_arrays(case["seqs"]), device=device)
    F.assert_model_same(F.library_model(fin, True), exp["model"], what)
    ids, fns, hds = metas_of(len(case["paths"]))
    assert library_text(t, fin, K, ids, fns, hds) == TA.model_gfa(exp, K, ids, fns, hds), f"{what}: text"
    assert t.yaml() == TA.model_yaml(exp), f"{what}: yaml"
    fin.close(); t.close()
    return exp, sm


# ---- the known answers, through the summary --------------------------------------------------------------------------------------------------------
def check_kats(lib_path, device=0):
    kats = TA.load_kats()
    for row in kats["median"]:
        assert TA.median_int(row["values"]) == row["median"]
    for row in kats["mad"]:
        assert TA.mad_int(row["values"]) == row["mad"]
    for row in kats["median"] + kats["mad"]:      # one unitig per sequence, as long as the value says: the library's median and MAD of the new lengths
        v = row["values"]
        if not v:
            continue
        t = trim_apply(len(v), [], v, [[u] for u in range(1, len(v) + 1)], v, None, chosen="none", mad=0.0, device=device, lib_path=lib_path)
        assert t.summary["median"] == TA.median_int(v) and t.summary["mad"] == TA.mad_int(v), (v, t.summary)
        assert "median" not in row or t.summary["median"] == row["median"]
        assert "mad" not in row or t.summary["mad"] == row["mad"]
        t.close()
    for row in kats["ranges"]:
        v = row["lengths"]
        assert TA.length_range(v, row["threshold"]) == (row["median"], row["mad"], row["min"], row["max"]), row["name"]
        t = trim_apply(len(v), [], v, [[u] for u in range(1, len(v) + 1)], v, None, chosen="none", mad=row["threshold"], device=device, lib_path=lib_path)
        sm = t.summary
        assert (sm["median"], sm["mad"], sm["min_length"], sm["max_length"]) == (row["median"], row["mad"], row["min"], row["max"]), (row["name"], sm)
        assert t.kept == row["kept"], (row["name"], t.kept)
        assert t.subsets.unitigs(1).tolist() == [s + 1 for s in row["kept"]], row["name"]
        t.close()
    return True


def test_reference_known_answers(emu):
    assert check_kats(emu)


# ---- named cases ----------------------------------------------------------------------------------------------------------------------------------
LENS6 = [5, 3, 4, 6, 2, 7]
HAIRPIN = [1, 2, 3, -3, -2, -1]


def named_cases():
    """(name, case, what the model must say for the case to be the one its name promises)"""
    ring = [1, 2, 3, 4, 1]
    return [
        ("nothing trimmed, mad 0", make_case([[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3]], LENS6[:4], mad=0.0),
         lambda e: e["kind"] is None and not any(r[3] or r[4] for r in e["records"])),
        ("start-end chosen", make_case([ring, [1, 2, 3, 4], ring], LENS6[:4], [(0, "start_end", 0, 4), (2, "start_end", 1, 5)]),
         lambda e: e["kind"] == "start_end" and [r[3] for r in e["records"]] == [1, 0, 1] and not any(r[4] for r in e["records"])),
        ("hairpin chosen", make_case([HAIRPIN, [1, 2, 3], HAIRPIN], LENS6[:3], [(0, "hairpin", 0, 3), (2, "hairpin", 3, 6), (0, "start_end", 0, 5)]),
         lambda e: e["kind"] == "hairpin" and (e["c_se"], e["c_hp"]) == (1, 2) and e["records"][0][:3] == (0, 3, 12)),
        ("a tie goes to start-end", make_case([ring, HAIRPIN[:4] + [4], [1, 2, 3, 4]], LENS6[:4], [(0, "start_end", 0, 4), (1, "hairpin", 0, 3)], mad=0.0),
         lambda e: e["kind"] == "start_end" and (e["c_se"], e["c_hp"]) == (1, 1) and [r[3] for r in e["records"]] == [1, 0, 0]),
        ("a status-2 result counts as not trimmed", make_case([ring, ring, [1, 2, 3, 4]], LENS6[:4], [(0, "start_end", 0, 4, 2), (1, "hairpin", 0, 4, 2)], mad=0.0),
         lambda e: e["kind"] is None and e["rejected"] == 2 and not any(r[3] for r in e["records"])),
        ("trimmed, then excluded", make_case([ring, [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]], LENS6[:4], [(0, "start_end", 0, 2)]),
         lambda e: e["records"][0][3:] == (1, 1) and sum(r[4] for r in e["records"]) == 1),
        ("excluded, and its unitigs die with their links", make_case([[1, 2, 3], [1, 2, 3], [1, 2, 3, 4, 5, 6], [1, 2, 3]], LENS6),
         lambda e: [r[4] for r in e["records"]] == [0, 0, 1, 0] and e["cluster"]["unitigs"] == [1, 2, 3] and len(e["cluster"]["links"]) == 4),
        ("a hairpin slice on both strands of a unitig", make_case([HAIRPIN, [1, 2, 3, -3], [1, 2, 3, -3]], LENS6[:3], [(0, "hairpin", 0, 4)]),
         lambda e: e["kind"] == "hairpin" and e["cluster"]["fwd"][2] == 6 and not any(r[4] for r in e["records"])),
        ("everyone excluded", make_case([[1], [2]], [10, 20], mad=0.1),
         lambda e: e["kept"] == [] and e["cluster"]["unitigs"] == [] and e["model"]["unitigs"] == []),
        ("one sequence alone", make_case([[1, 2, 3]], LENS6[:3]),
         lambda e: e["kept"] == [0] and (e["median"], e["mad"], e["min"], e["max"]) == (12, 0, 12, 12)),
    ]


def check_named_cases(lib_path, device=0):
    for name, case, holds in named_cases():
        exp, sm = check_case(case, lib_path, device, name)
        assert holds(exp), (name, exp["records"], exp["kind"])
        if name == "everyone excluded":      # the H line alone; the slice stage alone has run, with its one read-back
            t = run_library(case, lib_path, device)
            fin = t.finish(sequences=TA.seq_arrays(case["seqs"]), device=device)
            assert fin.gfa(K) == f"H\tVN:Z:1.0\tKM:i:{K}\n".encode() and t.yaml().startswith(b"trimmed_cluster_size: 0\ntrimmed_cluster_lengths: []\n")
            kept = run_library(dict(case, mad=0.0), lib_path, device)      # the same slices with everyone kept: the subset stages run as well
            assert t.summary["read_backs"] == 1 < kept.summary["read_backs"] and t.summary["launches"] < kept.summary["launches"], (t.summary, kept.summary)
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


# ---- the chain: Graph.trim against the glue of chain_util.run_from -------------------------------------------------------------------------------------
_CHAIN = {}


def chain_record(name, seed, lib_path, device=0):
    """chain_util.run_chain's first form alone: compress, then cluster, trim and resolve from the built handle"""
    key = (name, seed, str(lib_path))
    if key not in _CHAIN:
        case = CU.make_case(name, seed)
        g, gfa, loaded = parity_util.check_case(case["k"], case["seqs"], case["filenames"], case["headers"], lib_path=lib_path, device=device)
        meta = dict(ids=[q["id"] for q in loaded], filenames=case["filenames"], headers=case["headers"])
        g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)
        rec = CU.run_from(case, g, meta, g2.cluster_inputs(), lib_path, device, checks=False)
        rec["k"] = case["k"]
        g.close(); g2.close()
        _CHAIN[key] = rec
    return _CHAIN[key]


def check_chain_case(name, seed, lib_path, device=0):
    """per cluster: the untrimmed text read again is the handle the glue trimmed; Graph.trim on it must print the glue's 2_trimmed text"""
    rec = chain_record(name, seed, lib_path, device)
    assert rec["clusters"]
    for c, cl in rec["clusters"].items():
        g, fns, hds = graph_from_gfa(cl["untrimmed_gfa"], lib_path=lib_path)
        ids = [int(line.split("\t")[1]) for line in cl["untrimmed_gfa"].decode().splitlines() if line.startswith("P\t")]
        t = g.trim(CU.MIN_IDENTITY, CU.MAX_UNITIGS, CU.MAD, device=device)
        fin = t.finish(device=device)
        assert library_text(t, fin, rec["k"], ids, fns, hds) == cl["trimmed_gfa"], f"{name} {seed} cluster {c}: 2_trimmed differs from the glue's"
        assert [cl["seqs"][s] for s, x in enumerate(t.records["excluded"].tolist()) if x] == cl["excluded"], f"{name} {seed} cluster {c}: excluded"
        assert t.records["length"].tolist() == cl["trimmed_lengths"], f"{name} {seed} cluster {c}: trimmed lengths"
        assert (t.summary["chosen"] or "") == cl["chosen"] and (t.summary["min_length"], t.summary["max_length"]) == tuple(cl["length_range"])
        # the text form on the file `cluster` writes (its CL:i tags come back on the P lines)
        text, yaml, sm = trim_gfa(cl["untrimmed_gfa"], CU.MIN_IDENTITY, CU.MAX_UNITIGS, CU.MAD, device=device, lib_path=lib_path)
        assert re.sub(rb"\tCL:i:\d+", b"", text) == cl["trimmed_gfa"] and text.count(f"\tCL:i:{c}\n".encode()) == len(t.kept)
        assert yaml == t.yaml() and sm["chosen"] == t.summary["chosen"] and sm["align_launches"] == t.summary["align_launches"]
        fin.close(); t.close(); g.close()
    return True


@pytest.mark.parametrize("name,seed", CHAIN_CASES)
def test_chain_agrees_with_the_glue(emu, name, seed):
    assert check_chain_case(name, seed, emu)


# ---- segment numbers do not matter ---------------------------------------------------------------------------------------------------------------------
def renumbered_text(text, seed=3):
    """the same graph with its segment numbers permuted and spread out (holes, no order); S, L and P lines rewritten to match"""
    lines = text.decode().splitlines()
    old = [int(line.split("\t")[1]) for line in lines if line.startswith("S\t")]
    rng = random.Random(seed)
    new = rng.sample(range(1, 50 * len(old) + 10), len(old))
    table = dict(zip(old, new))
    out = []
    for line in lines:
        f = line.split("\t")
        if f[0] == "S":
            f[1] = str(table[int(f[1])])
        elif f[0] == "L":
            f[1], f[3] = str(table[int(f[1])]), str(table[int(f[3])])
        elif f[0] == "P":
            f[2] = ",".join(f"{table[int(e[:-1])]}{e[-1]}" for e in f[2].split(","))
        out.append("\t".join(f))
    assert sorted(new) != new and max(new) > len(new)
    return ("\n".join(out) + "\n").encode()


def check_numbers_do_not_matter(lib_path, device=0):
    rec = chain_record("small", 1, lib_path, device)
    for c, cl in rec["clusters"].items():
        dense = cl["untrimmed_gfa"]
        spread = renumbered_text(dense)
        a = trim_gfa(dense, device=device, lib_path=lib_path)
        b = trim_gfa(spread, device=device, lib_path=lib_path)
        assert a[0] == b[0] and a[1] == b[1], f"cluster {c}: the output depends on the input's segment numbers"
        assert a[0].count(f"\tCL:i:{c}\n".encode()) == len(cl["seqs"]) - len(cl["excluded"]) > 0
        with pytest.raises(AutocyclerError, match="segments numbered 1, 2, 3, ... in order"):
            graph_from_gfa(spread, lib_path=lib_path)
    return True


def test_segment_numbers_do_not_matter(emu):
    assert check_numbers_do_not_matter(emu)


# ---- the boundary table --------------------------------------------------------------------------------------------------------------------------------
def line_case(n_entries, n_seqs=2, extra=2):
    """n_seqs sequences over a line of n_entries + extra unitigs; sequence 0 is trimmed to the n_entries entries from 1 on"""
    n = n_entries + extra
    lens = [(u % 5) + 1 for u in range(1, n + 1)]
    path = list(range(1, n + 1))
    return make_case([path] * n_seqs, lens, [(0, "start_end", 1, 1 + n_entries)], mad=0.0)


def exclusion_case(n_seqs, pattern):
    """kept sequences walk 1,2 (100 bases); the excluded ones walk 2 alone (40) or 1,2,3 (190) in turns: the rule must exclude exactly `pattern`"""
    lens = [60, 40, 90]
    shapes, turn, paths = ([2], [1, 2, 3]), 0, []
    for s in range(n_seqs):
        if pattern[s]:
            paths.append(shapes[turn % 2]); turn += 1
        else:
            paths.append([1, 2])
    return make_case(paths, lens, mad=0.5, links=M.closed_set([(1, 2), (2, 3)]))


def check_boundary_table(lib_path, device=0):
    tile = scan_tile()
    assert tile == 4096
    for n_entries in (1, 63, 64, 65, tile - 1, tile, tile + 1):
        exp, sm = check_case(line_case(n_entries), lib_path, device, f"slice of {n_entries}")
        assert exp["records"][0][:2] == (1, 1 + n_entries)
    for n_seqs in (1, 2, 64, 65):
        check_case(line_case(5, n_seqs), lib_path, device, f"{n_seqs} sequences")
    for n_seqs in (3, 64, 65):
        patterns = dict(first=[s == 0 for s in range(n_seqs)], last=[s == n_seqs - 1 for s in range(n_seqs)], alternating=[s % 2 == 1 for s in range(n_seqs)])
        if n_seqs % 2:
            patterns["all but one"] = [s != n_seqs // 2 for s in range(n_seqs)]
        for name, pattern in patterns.items():
            exp, sm = check_case(exclusion_case(n_seqs, pattern), lib_path, device, f"{n_seqs} sequences, excluded {name}")
            assert [bool(r[4]) for r in exp["records"]] == pattern, (n_seqs, name, exp["median"], exp["mad"], exp["min"], exp["max"])
    # sums beyond 32 bits: few long unitigs given by length only.  One sequence of 3 * 2^30 + 5 bases (a signed 32-bit sum would show) next to
    # two of 2^30 + 5: prefixes beyond 2^32.  Without bytes there is no text: the trimmed graph before the merge is compared
    big = make_case([[1, 2, 1, 1], [2, 1], [1, 2]], [2 ** 30, 5, 7], mad=0.0, with_seqs=False)
    assert big["seq_lengths"][0] == 3 * 2 ** 30 + 5 > 2 ** 31
    t = run_library(big, lib_path, device)
    m = S.model_cluster(big["n"], big["links"], big["lens"], None, big["paths"], [1, 1, 1], 1)
    S.assert_cluster_same(S.library_cluster(t.subsets, 1), m, "long unitigs")
    assert t.records["length"].tolist() == big["seq_lengths"] and t.summary["median"] == 2 ** 30 + 5
    t.close()
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


# ---- the random sweep ----------------------------------------------------------------------------------------------------------------------------------
def sweep_case(seed):
    """a few sequences that are variants of one random path (trim_util.random_case, or a planted overlap), their slices by trim_util's model"""
    rng = random.Random(seed)
    if seed % 3 == 2:
        base, w = T.planted_overlap_path(rng, rng.randint(12, 40), rng.randint(2, 6), n_unitigs=rng.randint(6, 30), hairpin=rng.random() < 0.5)
        min_identity, max_unitigs = 0.75, 1000
    else:
        base, w, min_identity, max_unitigs = T.random_case(rng, 4, 40)
    paths = []
    for _ in range(rng.randint(2, 7)):
        p = list(base)
        x = rng.random()
        if x < 0.25 and len(p) > 4:
            p = p[:rng.randint(2, len(p) - 1)]      # a shorter one: a candidate for exclusion
        elif x < 0.4:
            p = p + [rng.choice((-1, 1)) * rng.randint(1, len(w)) for _ in range(rng.randint(1, 6))]
        paths.append(p)
    results, _ = T.trim_paths_expected(paths, w, min_identity, max_unitigs)
    case = make_case(paths, w, mad=rng.choice((0.0, 0.5, 2.0, 5.0)))
    case["results"] = results
    return case


def check_sweep(lib_path, seeds, device=0):
    met = dict(start_end=0, hairpin=0, nothing=0, excluded=0, unitig_died=0)
    for seed in seeds:
        case = sweep_case(seed)
        exp, sm = check_case(case, lib_path, device, f"seed {seed}")
        met["start_end" if exp["kind"] == "start_end" else "hairpin" if exp["kind"] == "hairpin" else "nothing"] += 1
        met["excluded"] += any(r[4] for r in exp["records"])
        met["unitig_died"] += len(exp["cluster"]["unitigs"]) < len({abs(e) for p in case["paths"] for e in p})
    return met


def test_sweep_seeds(emu):
    met = check_sweep(emu, range(24))
    assert met["start_end"] and met["hairpin"] and met["nothing"] and met["excluded"] and met["unitig_died"], met


# ---- errors, each by its text ----------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, device=0):
    lens = LENS6[:4]
    paths = [[1, 2, 3, 4, 1], [1, 2, 3, 4]]

    def fails(match, **kw):
        case = make_case(kw.pop("paths", paths), kw.pop("lens", lens), **kw)
        with pytest.raises(AutocyclerError, match=match):
            run_library(case, lib_path, device)

    fails(r"Position calculation mismatch.*sequence 0 add up to 18 bases, its new length is 17", slices=[(0, "start_end", 0, 4, 1, 17)])
    fails(r"Position calculation mismatch.*sequence 1 add up to 18 bases, its new length is 19", seq_lengths=[23, 19])
    fails(r"Position calculation mismatch.*sequence 0 add up to 4294967303 bases, its new length is 7", paths=[[1, 1, 1, 1, 2]], lens=[2 ** 30, 7], seq_lengths=[7],
          with_seqs=False)      # (a 32-bit sum would let this one through)
    fails(r"the slice of sequence 0 begins at 3, after its end 2", slices=[(0, "start_end", 3, 2, 1, 0)])
    fails(r"the slice of sequence 1 ends at 5, beyond its path of 4 entries", slices=[(1, "start_end", 0, 5, 1, 18)])
    fails(r"sequence 0 is kept with an empty slice", slices=[(0, "start_end", 2, 2)], mad=0.0)
    fails(r"entry 1 of the path of sequence 1 \(0\) names no unitig: unitig numbers run from 1 to 4", paths=[[1, 2], [1, 0, 2]], seq_lengths=[8, 8], links=[])
    fails(r"entry 2 of the path of sequence 0 \(-5\) names no unitig", paths=[[1, 2, -5], [1, 2]], lens=lens, seq_lengths=[8, 8], links=[])
    fails(r"entry 1 of the path of sequence 1 \(-3\) enters a unitig that is not alive in the input", paths=[[1, 2], [1, -3]], alive=[1, 1, 0, 1], links=[])
    fails(r"--mad cannot be less than 0", mad=-0.5)
    # an excluded sequence may have an empty slice
    ok = make_case([[1, 2, 3, 4, 1]] + [[1, 2, 3, 4]] * 3, lens, [(0, "start_end", 2, 2)])
    exp, _ = check_case(ok, lib_path, device, "an empty slice, excluded")
    assert exp["records"][0][2:] == (0, 1, 1)
    # the settings of the whole command, and null pointers
    g, _, _ = graph_from_gfa(S.hand_gfa_text(4, M.closed_set(TA.path_links(paths)), [M._seq_of(u, l) for u, l in enumerate(lens, 1)], paths), lib_path=lib_path)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(AutocyclerError, match=r"--min_identity must be between 0.0 and 1 \(inclusive\)"):
            g.trim(min_identity=bad, device=device)
    with pytest.raises(AutocyclerError, match="--mad cannot be less than 0"):
        g.trim(mad=-1.0, device=device)
    with pytest.raises(AutocyclerError, match="one per sequence expected"):
        g.trim_apply(full_results(paths, lens)[:1], device=device)
    lib = _capi.load_library(lib_path)
    h = _capi.C.c_void_p()
    assert lib.ac_graph_trim(None, 0.75, 5000, 5.0, device, _capi.C.byref(h)) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_graph_trim(g._h, 0.75, 5000, 5.0, device, None) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_graph_trim_apply(g._h, None, 0, 5.0, device, _capi.C.byref(h)) == 1 and b"null pointer: results" in lib.ac_last_error()
    assert lib.ac_trim_apply(4, None, 0, None, None, None, None, None, None, 1, None, 1, 5.0, device, _capi.C.byref(h)) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_trimmed_finish(None, None, None, device, _capi.C.byref(h)) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_trimmed_yaml_string(None, _capi.C.byref(h), None) == 1 and lib.ac_trimmed_subsets(None) is None
    assert lib.ac_trim_gfa(None, 5, 0.75, 5000, 5.0, device, _capi.C.byref(h), None, _capi.C.byref(h), None) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_trim_dir(None, 0.75, 5000, 5.0, device) == 1 and lib.ac_resolve_dir(None, device) == 1
    g.close()
    return True


def test_errors(emu):
    assert check_errors(emu)


# ---- handle, plain arrays, text, directory and CLI give the same bytes --------------------------------------------------------------------------------------
def check_forms(lib_path, device=0, cli=None):
    rec = chain_record("small", 1, lib_path, device)
    c, cl = sorted(rec["clusters"].items())[0]
    text = cl["untrimmed_gfa"]
    want_gfa, want_yaml, _ = trim_gfa(text, device=device, lib_path=lib_path)
    # the handle
    g, fns, hds = graph_from_gfa(text, lib_path=lib_path)
    ids = [int(line.split("\t")[1]) for line in text.decode().splitlines() if line.startswith("P\t")]
    t = g.trim(device=device)
    fin = t.finish(device=device)
    assert library_text(t, fin, rec["k"], ids, fns, hds, [c] * len(ids)) == want_gfa and t.yaml() == want_yaml
    # the handle with the table made first
    results, _ = g.trim_paths(device=device)
    t2 = g.trim_apply(results, device=device)
    assert t2.records.tobytes() == t.records.tobytes() and S.subsets_bytes(t2.subsets) == S.subsets_bytes(t.subsets)
    # plain arrays
    a = CU.graph_arrays(g)
    lengths = [int(re.search(rb"\tLN:i:(\d+)", line).group(1)) for line in text.splitlines() if line.startswith(b"P\t")]
    t3 = trim_apply(a["n"], a["links"], a["lens"], a["paths"], lengths, results, device=device, lib_path=lib_path)
    fin3 = t3.finish(sequences=a["sequences"], device=device)
    assert library_text(t3, fin3, rec["k"], ids, fns, hds, [c] * len(ids)) == want_gfa and t3.yaml() == want_yaml
    # the trimmed handle is what resolve starts from
    kept = t.kept
    gt = fin.to_graph(rec["k"], [ids[s] for s in kept], [int(t.records["length"][s]) for s in kept], [fns[s] for s in kept], [hds[s] for s in kept])
    bridged, merged, final, _ = gt.resolve_graphs(device=device)
    assert (bridged, merged, final) == (cl["bridged_gfa"], cl["merged_gfa"], cl["final_gfa"])
    # the directory, through the library and through the CLI
    runs = [lambda d: (trim_dir(d, device=device, lib_path=lib_path), resolve_dir(d, device=device, lib_path=lib_path))]
    if cli is not None:
        def by_cli(d):
            for cmd in (["trim", "-c", str(d), "--min_identity", "0.75", "--max_unitigs", "5000", "--mad", "5.0"], ["resolve", "--cluster_dir", str(d)]):
                p = subprocess.run([str(cli)] + cmd + ["--device", str(device)], capture_output=True, text=True)
                assert p.returncode == 0, p.stderr
        runs.append(by_cli)
    for run in runs:
        with tempfile.TemporaryDirectory() as tmp:
            d = Path(tmp)
            (d / "1_untrimmed.gfa").write_bytes(text)
            run(d)
            assert (d / "2_trimmed.gfa").read_bytes() == want_gfa and (d / "2_trimmed.yaml").read_bytes() == want_yaml
            assert [(d / f).read_bytes() for f in ("3_bridged.gfa", "4_merged.gfa", "5_final.gfa")] == [cl["bridged_gfa"], cl["merged_gfa"], cl["final_gfa"]]
            assert sorted(p.name for p in d.iterdir()) == ["1_untrimmed.gfa", "2_trimmed.gfa", "2_trimmed.yaml", "3_bridged.gfa", "4_merged.gfa", "5_final.gfa"]
    if cli is not None:
        p = subprocess.run([str(cli), "--help"], capture_output=True, text=True)
        assert " trim --cluster_dir" in p.stderr and " resolve --cluster_dir" in p.stderr
        with tempfile.TemporaryDirectory() as tmp:
            p = subprocess.run([str(cli), "trim", "-c", tmp], capture_output=True, text=True)
            assert p.returncode == 1 and "1_untrimmed.gfa" in p.stderr
    for x in (fin, fin3, t, t2, t3, gt, g):
        x.close()
    return True


def test_forms_give_the_same_bytes(emu):
    assert check_forms(emu)


# ---- two runs, and the launch counts ------------------------------------------------------------------------------------------------------------------------
def trimmed_bytes(t, fin):
    return b"|".join([t.records.tobytes(), S.subsets_bytes(t.subsets), F.finished_bytes(fin), t.yaml(),
                      repr(sorted((k, v) for k, v in t.summary.items() if "seconds" not in k)).encode()])


def check_two_runs_identical(lib_path, device=0):
    for case in (sweep_case(2), exclusion_case(65, [s % 2 == 1 for s in range(65)]), line_case(scan_tile() + 1)):
        got = []
        for _ in range(2):
            t = run_library(case, lib_path, device)
            fin = t.finish(sequences=TA.seq_arrays(case["seqs"]), device=device)
            got.append(trimmed_bytes(t, fin))
            fin.close(); t.close()
        assert got[0] == got[1]
    return True


def test_two_runs_give_identical_products(emu):
    assert check_two_runs_identical(emu)


def check_launch_counts(lib_path, device=0):
    """the same key width (3 unitigs), 2, 3 and 65 sequences, short and long slices: one count without an exclusion, one with; they differ by the
    compaction pass (flag, scan, scatter) and no read-back"""
    counts = {}
    for n_seqs in (2, 3, 65):      # (of two sequences the rule excludes both or neither: its range is symmetric about their mean)
        for excluded in (False, True):
            if n_seqs == 2 and excluded:
                continue
            pattern = [excluded and s == 0 for s in range(n_seqs)]
            case = exclusion_case(n_seqs, pattern)
            if n_seqs == 65:      # (longer slices too: the kept ones walk their two unitigs 40 times over)
                case = make_case([p * (40 if p == [1, 2] else 1) for p in case["paths"]], case["lens"], mad=0.5, links=M.closed_set([(1, 2), (2, 3), (2, 1)]))
            t = run_library(case, lib_path, device)
            assert t.summary["excluded"] == int(excluded), (n_seqs, excluded, t.summary)
            counts[(n_seqs, excluded)] = (t.summary["launches"], t.summary["read_backs"])
            assert t.subsets.summary["launches"] == t.summary["launches"]
            t.close()
    assert counts[(2, False)] == counts[(3, False)] == counts[(65, False)] and counts[(3, True)] == counts[(65, True)], counts
    assert counts[(3, True)][0] - counts[(2, False)][0] == 3 and counts[(3, True)][1] == counts[(2, False)][1], counts
    return True


def test_launches_follow_the_key_width_and_the_exclusion_alone(emu):
    assert check_launch_counts(emu)
