"""ac_combine_graphs / ac_combine_handles, the Combined object, ac_combine_gfas, ac_combine, ac_gfa2fasta_string and ac_gfa2fasta on the CPU
emulation of the shipped kernels (kernels_combine.inc) against the literal Python model of combine_util.py: load_clusters' stable sort, the
running offset of combine_clusters over lists, get_links_for_gfa, topology, cluster_depth and the three texts.  Every comparison is equality
(depths bit for bit, link order included).  The chain tests finish compress -> cluster -> trim -> resolve in a consensus FASTA that is held to
the planted genomes, and with reads to the depth model of depth_util.py.  The same checks run on the device in test_combine_gpu.py."""
import ctypes
import random
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import chain_util
import combine_util as CU
import depth_util
import emu_lib
from autocycler_amd import (TOPOLOGY_NAMES, AutocyclerError, Combined, ReadDepth, combine_dir, combine_gfas, combine_graphs, combine_handles, gfa2fasta, gfa2fasta_file,
                            gfa_segment_types, graph_from_gfa)
from autocycler_amd import _capi

NEW_SYMBOLS = ("ac_combine_graphs", "ac_combine_handles", "ac_combined_clusters", "ac_combined_unitigs", "ac_combined_links", "ac_combined_summary_get_sized",
               "ac_combined_free", "ac_combined_gfa_string", "ac_combined_fasta_string", "ac_combined_yaml_string", "ac_combined_depth_lines", "ac_combine_gfas", "ac_combine",
               "ac_gfa2fasta_string", "ac_gfa2fasta")
ROOT = Path(__file__).resolve().parent.parent
SCAN_TILE, RADIX_TILE = 4096, 2048      # device_prims.hpp: SCAN_TILE, RS_TILE
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_combine(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


# ---- one input through the model, the object and the text entry -------------------------------------------------------------------------------
def seq_of(tag, n):
    rng = random.Random(tag * 7919 + n)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def check_texts(texts, lib_path, device=0, read_depths=None, what=""):
    """cluster GFA texts -> (the model's dict, the object's summary); the object on arrays and the text entry must both give the model's bytes"""
    models = [CU.from_gfa_text(t) for t in texts]
    exp = CU.combine_model(models, read_depths)
    c = combine_graphs([CU.array_form(m) for m in models], read_depths=read_depths, device=device, lib_path=lib_path)
    assert isinstance(c, Combined)
    CU.assert_same(c, exp, TOPOLOGY_NAMES, what)
    assert c.gfa() == exp["gfa"], (what, "gfa")
    assert c.fasta() == exp["fasta"], (what, "fasta")
    assert c.yaml() == exp["yaml"], (what, "yaml")
    assert c.depth_lines() == exp["depth_lines"], (what, "depth lines")
    assert c.summary["with_reads"] == (read_depths is not None) and c.summary["read_backs"] == (2 if exp["unitigs"] else 0), (what, c.summary)
    gfa, fasta, yaml, sm = combine_gfas(texts, read_depths=read_depths, device=device, lib_path=lib_path)
    assert (gfa, fasta, yaml) == (exp["gfa"], exp["fasta"], exp["yaml"]), (what, "text entry")
    assert (sm["launches"], sm["read_backs"], sm["bases"]) == (c.summary["launches"], c.summary["read_backs"], c.summary["bases"])
    summary = c.summary
    c.close()
    return exp, summary


def one_tig(number, length, links=(), depth=3.0, colour="steelblue", tag=1):
    return CU.gfa_text([(number, seq_of(tag, length), depth, colour)], links)


# ---- the reference's known answers ----------------------------------------------------------------------------------------------------------------
def check_kats(lib_path, device=0):
    kats = CU.load_kats()["topology"]
    assert len(kats) == 13
    for kat in kats:
        text = (CU.GOLDEN / kat["gfa"]).read_bytes()
        assert CU.from_gfa_text(text).topology() == kat["expected"], kat
        exp, _ = check_texts([text], lib_path, device, what=kat["gfa"])
        assert exp["clusters"][0]["topology"] == kat["expected"]
    # all thirteen at once: every graph keeps its own answer on the concatenation
    texts = [(CU.GOLDEN / kat["gfa"]).read_bytes() for kat in kats]
    exp, _ = check_texts(texts, lib_path, device, what="all kats")
    assert sorted(c["topology"] for c in exp["clusters"]) == sorted(k["expected"] for k in kats)
    return True


def test_reference_known_answers(emu):
    assert check_kats(emu)


# ---- named cases ------------------------------------------------------------------------------------------------------------------------------------
def unresolved_graph():
    """five unitigs, numbers out of order and with holes, links on both strands, one L line whose segment is missing"""
    unitigs = [(7, seq_of(7, 9), 4.0, "forestgreen"), (2, seq_of(2, 4), "2.675", None), (11, seq_of(11, 6), "0.125", "pink"), (5, seq_of(5, 3), 1.5, "steelblue"),
               (3, seq_of(3, 5), "0.05", "orangered")]
    links = [(2, 7), (-7, -2), (7, 11), (-11, -7), (7, -5), (5, -7), (-2, 3), (-3, 2), (11, 99), (3, 3), (-3, -3), (-5, 5), (7, 2)]
    return CU.gfa_text(unitigs, links)


def named_cases():
    return {
        "one circular unitig": [one_tig(1, 30, [(1, 1), (-1, -1)])],
        "two graphs out of size order": [one_tig(1, 10, [(1, 1), (-1, -1)], tag=2), one_tig(1, 40, [(1, 1), (-1, -1)], tag=3)],
        "equal totals keep the input order": [one_tig(1, 12, tag=4), one_tig(1, 12, [(1, 1), (-1, -1)], tag=5), one_tig(1, 12, [(1, -1)], tag=6), one_tig(1, 13, tag=7)],
        "holes: the offset is the maximum, not the count": [CU.gfa_text([(4, seq_of(1, 20), 2.0, None), (9, seq_of(2, 20), 2.0, None)], [(4, 9), (-9, -4)]),
                                                            one_tig(3, 15, [(3, 3), (-3, -3)]), one_tig(1, 5)],
        "numbers out of order in the file": [CU.gfa_text([(3, seq_of(3, 8), 1.0, None), (1, seq_of(1, 9), 1.0, None), (2, seq_of(2, 7), 1.0, None)],
                                                         [(1, 2), (-2, -1), (2, 3), (-3, -2), (3, 1), (-1, -3)])],
        "unresolved: several unitigs, both strands": [one_tig(1, 50, [(1, 1), (-1, -1)]), unresolved_graph()],
        "an empty graph among others": [one_tig(1, 9), b"H\tVN:Z:1.0\tKM:i:51\n", one_tig(2, 30, [(2, 2), (-2, -2)]), b""],
        "hairpin at one end": [one_tig(1, 20, [(1, -1)]), one_tig(1, 19, [(-1, 1)])],
        "hairpin at both ends": [one_tig(1, 20, [(1, -1), (-1, 1)])],
        "circular plus hairpin: other": [one_tig(1, 20, [(1, 1), (-1, -1), (-1, 1)])],
        "a dropped L line naming a missing segment": [one_tig(1, 20, [(1, 1), (-1, -1), (1, 2), (-2, -1), (5, 1)])],
        "each type's colour": [CU.gfa_text([(1, seq_of(1, 5), 1.0, "steelblue"), (2, seq_of(2, 5), 1.0, "forestgreen"), (3, seq_of(3, 5), 1.0, "pink"),
                                            (4, seq_of(4, 5), 1.0, "orangered"), (5, seq_of(5, 5), 1.0, None), (6, seq_of(6, 5), 1.0, "purple")], [])],
        "depths on a printing tie": [CU.gfa_text([(1, seq_of(1, 5), "0.125", None), (2, seq_of(2, 5), "2.675", None), (3, seq_of(3, 5), "0.05", None),
                                                  (4, seq_of(4, 5), "0.375", None), (5, seq_of(5, 5), "1e3", None), (6, seq_of(6, 5), "0.005", None)], [])],
        "a unitig without bases": [CU.gfa_text([(1, b"", 1.0, None), (2, seq_of(2, 6), 2.0, None)], [(1, 2), (-2, -1)]), CU.gfa_text([(1, b"", 1.0, None)], [])],
        "number 0": [one_tig(5, 20), one_tig(0, 10, [(0, 0)])],
    }


def read_depth_cases():
    two = [CU.gfa_text([(1, seq_of(1, 10), 2.0, None), (2, seq_of(2, 30), 2.0, None), (3, seq_of(3, 7), 2.0, None)], [(1, 2), (-2, -1)]), one_tig(1, 100, [(1, 1), (-1, -1)])]
    return {
        "read depths all present": (two, [[10.25, 20.5, 0.05], [33.349999]]),
        "some None": (two, [[None, 20.5, 0.125], [0.0]]),
        "all None in one graph": (two, [[None, None, None], [12.34]]),
        "all None everywhere": (two, [[None, None, None], [None]]),
        "ties": (two, [[0.25, 0.35, 2.675], [0.05]]),
        "not a number": (two, [[NAN, 1.0, None], [INF]]),
    }


def check_named_cases(lib_path, device=0):
    seen = {}
    for name, texts in named_cases().items():
        exp, _ = check_texts(texts, lib_path, device, what=name)
        seen[name] = exp
    assert [c["input_index"] for c in seen["two graphs out of size order"]["clusters"]] == [1, 0]
    assert [c["input_index"] for c in seen["equal totals keep the input order"]["clusters"]] == [3, 0, 1, 2]
    holes = seen["holes: the offset is the maximum, not the count"]
    assert [c["offset"] for c in holes["clusters"]] == [0, 9, 12] and [u["number"] for u in holes["unitigs"]] == [4, 9, 12, 13]
    assert not seen["unresolved: several unitigs, both strands"]["metrics"]["consensus_assembly_fully_resolved"]
    assert seen["one circular unitig"]["metrics"]["consensus_assembly_fully_resolved"]
    assert [c["topology"] for c in seen["an empty graph among others"]["clusters"]] == ["circular", "linear-open-open", "empty", "empty"]
    assert [c["topology"] for c in seen["hairpin at one end"]["clusters"]] == ["linear-open-hairpin"] * 2
    assert seen["hairpin at both ends"]["clusters"][0]["topology"] == "linear-hairpin-hairpin" and b"circular=false topology=linear" in seen["hairpin at both ends"]["fasta"]
    assert seen["circular plus hairpin: other"]["clusters"][0]["topology"] == "other" and b"topology=" not in seen["circular plus hairpin: other"]["fasta"]
    dropped = seen["a dropped L line naming a missing segment"]
    assert dropped["clusters"][0]["topology"] == "circular" and dropped["links"] == [(1, 1), (-1, -1)]
    assert [l.split(b"CL:Z:")[1] for l in seen["each type's colour"]["gfa"].split(b"\n") if l.startswith(b"S")] == [b"steelblue", b"forestgreen", b"pink"] + [b"orangered"] * 3
    assert [l.split(b"DP:f:")[1].split(b"\t")[0] for l in seen["depths on a printing tie"]["gfa"].split(b"\n") if l.startswith(b"S")] == \
        [b"0.12", b"2.67", b"0.05", b"0.38", b"1000.00", b"0.01"]
    for name, (texts, rd) in read_depth_cases().items():
        exp, _ = check_texts(texts, lib_path, device, read_depths=rd, what=name)
        seen[name] = exp
    assert b"depth=unavailable" in seen["some None"]["fasta"] and b"DP:f:0.00" in seen["some None"]["gfa"] and b"read_depth: 0.0\n" in seen["some None"]["yaml"]
    assert [c["read_depth"] for c in seen["all None in one graph"]["metrics"]["consensus_assembly_clusters"]] == [12.3, "unavailable"]
    assert seen["all None everywhere"]["yaml"].count(b"read_depth: unavailable\n") == 2
    assert b"depth=0.2\n" in seen["ties"]["fasta"] and b"depth=0.3\n" in seen["ties"]["fasta"] and b"DP:f:2.67\t" in seen["ties"]["gfa"]
    assert b"depth=NaN" in seen["not a number"]["fasta"] and b"depth=inf" in seen["not a number"]["fasta"] and b"read_depth: .inf\n" in seen["not a number"]["yaml"]
    assert b"read_depth: .nan\n" in seen["not a number"]["yaml"]
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


# ---- boundary table -----------------------------------------------------------------------------------------------------------------------------------
def chain_graph(n, first=1, step=1, closed=False, tag=0):
    """n unitigs of 1 .. 3 bases in a chain (a ring when closed), numbered first, first + step, ...: 2 (n - 1) links (2 n closed)"""
    numbers = [first + i * step for i in range(n)]
    links = []
    for a, b in zip(numbers, numbers[1:] + (numbers[:1] if closed else [])):
        links += [(a, b), (-b, -a)]
    return CU.gfa_text([(u, seq_of(tag + u, 1 + u % 3), float(u % 5), None) for u in numbers], links)


def link_count_graph(n_links):
    """one graph with exactly n_links L lines over 40 unitigs (links may repeat: the reference pushes every line)"""
    rng = random.Random(n_links)
    numbers = list(range(1, 41))
    links = [(rng.choice(numbers) * rng.choice((1, -1)), rng.choice(numbers) * rng.choice((1, -1))) for _ in range(n_links)]
    return CU.gfa_text([(u, seq_of(u, 2), 1.0, None) for u in numbers], links)


def check_boundary_table(lib_path, device=0):
    for G in (1, 2, 63, 64, 65):
        texts = [one_tig(1 + g % 3, 5 + (g * 7) % 11, [(1 + g % 3, 1 + g % 3), (-(1 + g % 3), -(1 + g % 3))] if g % 2 else [], tag=g) for g in range(G)]
        exp, _ = check_texts(texts, lib_path, device, what=f"G = {G}")
        assert len(exp["clusters"]) == G
    for n in (1, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        check_texts([one_tig(1, 2), chain_graph(n, first=3, step=2, closed=n % 2 == 0), one_tig(9, 3, [(9, -9)])], lib_path, device, what=f"{n} unitigs")
    for nl in (RADIX_TILE - 3, RADIX_TILE - 2, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1):      # (the sort runs over two more keys than there are links)
        check_texts([link_count_graph(nl), one_tig(1, 7)], lib_path, device, what=f"{nl} links")
    # a total beyond 2^32 from the lengths alone: the object needs no bases
    big = [dict(number=[1, 2, 3], len=[0xFFFFFFF0, 0xFFFFFFF0, 17], links=[(1, 2), (-2, -1)]), dict(number=[1], len=[0xFFFFFFFF], links=[(1, 1), (-1, -1)]),
           dict(number=[6, 2], len=[0xFFFFFFFF, 0xFFFFFFFF], links=[])]
    c = combine_graphs(big, device=device, lib_path=lib_path)
    assert [int(x) for x in c.clusters["length"]] == [2 * 0xFFFFFFFF, 2 * 0xFFFFFFF0 + 17, 0xFFFFFFFF] and [int(x) for x in c.clusters["input_index"]] == [2, 0, 1]
    assert [int(x) for x in c.clusters["offset"]] == [0, 6, 9] and [int(x) for x in c.unitigs["number"]] == [6, 2, 7, 8, 9, 10]
    assert c.summary["bases"] == 2 * 0xFFFFFFF0 + 17 + 3 * 0xFFFFFFFF and c.links.tolist() == [[7, 8], [-8, -7], [10, 10], [-10, -10]]
    assert [TOPOLOGY_NAMES[int(t)] for t in c.clusters["topology"]] == ["fragmented", "fragmented", "circular"]
    with pytest.raises(AutocyclerError, match="missing sequences"):
        c.gfa()
    assert c.yaml().startswith(b"consensus_assembly_bases: 21474836462\n")
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


# ---- a seeded sweep ---------------------------------------------------------------------------------------------------------------------------------------
def random_texts(rng, max_graphs=6, max_unitigs=9):
    texts, depths = [], []
    for g in range(rng.randint(1, max_graphs)):
        n = rng.choice((0, 1, 1, 1, 2, 3, rng.randint(0, max_unitigs)))
        numbers = rng.sample(range(0 if rng.random() < 0.1 else 1, 4 * max_unitigs), n)      # a random injection: no case is an error case
        unitigs = [(u, seq_of(g * 100 + u, rng.choice((0, 1, 2, 5, 12, 30))), rng.choice(("0.125", "3.00", "17.455", "0.05", "250.5")),
                    rng.choice((None, "steelblue", "forestgreen", "pink", "orangered"))) for u in numbers]
        links = []
        if n:
            style = rng.random()
            for _ in range(rng.randint(0, 3 * n) if style < 0.7 else rng.choice((0, 1, 2))):
                a, b = rng.choice(numbers), rng.choice(numbers) if rng.random() < 0.9 else 77777
                if n == 1 and rng.random() < 0.5:
                    links += rng.choice(([(a, a), (-a, -a)], [(a, -a)], [(-a, a)], [(a, -a), (-a, a)]))
                else:
                    links.append((a * rng.choice((1, -1)) if a else 0, b * rng.choice((1, -1)) if b else 0))
        texts.append(CU.gfa_text(unitigs, [l for l in links if l[0] != 0 or l[1] != 0 or rng.random() < 0.5]))
        depths.append([rng.choice((None, 0.0, 0.05, 12.25, 7.349, 1e-9, 123456.789)) for _ in numbers])
    return texts, depths


def check_sweep(lib_path, seeds, device=0):
    met = dict(empty=0, unresolved=0, reads=0, ties_in_length=0, dropped=0, hairpin=0, circular=0)
    for seed in seeds:
        rng = random.Random(seed)
        texts, depths = random_texts(rng)
        rd = depths if seed % 2 else None
        exp, _ = check_texts(texts, lib_path, device, read_depths=rd, what=f"seed {seed}")
        lengths = [c["length"] for c in exp["clusters"]]
        met["empty"] += any(c["topology"] == "empty" for c in exp["clusters"]); met["unresolved"] += not exp["metrics"]["consensus_assembly_fully_resolved"]
        met["reads"] += rd is not None; met["ties_in_length"] += len(set(lengths)) < len(lengths)
        met["dropped"] += any(CU.from_gfa_text(t).dropped_links for t in texts)
        met["hairpin"] += any("hairpin" in c["topology"] for c in exp["clusters"]); met["circular"] += any(c["topology"] == "circular" for c in exp["clusters"])
    return met


def test_sweep(emu):
    met = check_sweep(emu, range(120))
    assert all(met.values()), met


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, device=0):
    def fails(message, graphs, **kw):
        with pytest.raises(AutocyclerError) as e:
            combine_graphs(graphs, device=device, lib_path=lib_path, **kw)
        assert str(e.value) == message, (str(e.value), message)

    ok = dict(number=[1, 2], len=[5, 6], links=[(1, 2), (-2, -1)])
    fails("combine: at least one graph is required", [])
    fails("combine: graph 1: unitig number 3 occurs more than once", [ok, dict(number=[7, 3, 7, 3, 7], len=[1] * 5, links=[])])      # (the lowest such number)
    fails("combine: graph 0: unitig number 3 occurs more than once", [dict(number=[9, 3, 9, 3], len=[1] * 4, links=[]), dict(number=[1, 1], len=[1, 1], links=[])])
    fails("combine: graph 2: unitig number 0 occurs more than once", [ok, ok, dict(number=[0, 0], len=[1, 1], links=[])])
    for graphs, message in (([dict(number=[7, 7], len=[1, 1], links=[])], "combine: graph 0: unitig number 7 occurs more than once"),):
        texts = [CU.gfa_text([(n, b"A" * l, 1.0, None) for n, l in zip(g["number"], g["len"])], []) for g in graphs]
        with pytest.raises(CU.CombineError) as m:
            CU.combine_model([CU.from_gfa_text(t) for t in texts])
        assert str(m.value) == message
        with pytest.raises(AutocyclerError) as e:
            combine_gfas(texts, device=device, lib_path=lib_path)
        assert str(e.value) == message
    # the sum of the maxima leaves u32: the first graph in output order that does not fit is named, with the model's words
    over = [dict(number=[0xFFFFFFF0], len=[9], links=[]), dict(number=[0x10], len=[5], links=[]), dict(number=[1], len=[7], links=[])]
    fails("combine: graph 1: offset 4294967281 + its highest unitig number 16 does not fit 32 bits", over)
    texts = [CU.gfa_text([(g["number"][0], b"A" * g["len"][0], 1.0, None)], []) for g in over]
    with pytest.raises(CU.CombineError, match="combine: graph 1: offset 4294967281 \\+ its highest unitig number 16 does not fit 32 bits"):
        CU.combine_model([CU.from_gfa_text(t) for t in texts])
    fits = [dict(number=[0xFFFFFFF0], len=[9], links=[]), dict(number=[0xF], len=[5], links=[(1, 1)])]
    c = combine_graphs(fits, device=device, lib_path=lib_path)
    assert [int(x) for x in c.unitigs["number"]] == [0xFFFFFFF0, 0xFFFFFFFF] and c.links.tolist() == [[-1, -1]]      # (a printed number above 2^31 leaves a signed entry)
    # a link entry that is 0 or beyond its own graph: the lowest such link, its index within its graph
    fails("combine: graph 1: link 1 (2 -> 3) names no unitig of its graph: its entries are 1-based file-order indices, 2 unitigs here",
          [ok, dict(number=[5, 9], len=[1, 1], links=[(1, 2), (2, 3), (0, 1)])])
    fails("combine: graph 0: link 0 (0 -> 1) names no unitig of its graph: its entries are 1-based file-order indices, 2 unitigs here",
          [dict(number=[5, 9], len=[1, 1], links=[(0, 1)]), ok])
    fails("combine: graph 1: link 0 (1 -> 1) names no unitig of its graph: its entries are 1-based file-order indices, 0 unitigs here",
          [ok, dict(number=[], len=[], links=[(1, 1)])])
    fails("combine: graph 0: link 0 (1 -> 1) names no unitig of its graph: its entries are 1-based file-order indices, 0 unitigs here", [dict(number=[], len=[], links=[(1, 1)])])
    # 2^46 bases
    fails("combine: graph 1: the total of bases reaches 2^46 with this graph", [dict(number=list(range(1, 9001)), len=[0xFFFFFFFF] * 9000, links=[]),
                                                                                  dict(number=list(range(1, 9001)), len=[0xFFFFFFFF] * 9000, links=[])])
    with pytest.raises(AutocyclerError, match="one entry per unitig expected"):
        combine_graphs([ok], read_depths=[[1.0]], device=device, lib_path=lib_path)
    # null pointers and offsets, straight at the ABI
    lib = _capi.load_library(lib_path)
    h = ctypes.c_void_p()
    off = (ctypes.c_uint64 * 2)(0, 1)
    zero = (ctypes.c_uint64 * 2)(0, 0)
    one = (ctypes.c_uint32 * 1)(1)
    rd = (ctypes.c_double * 1)(1.0)

    def abi(message, *args):
        assert lib.ac_combine_graphs(*args) == 1 and lib.ac_last_error().decode() == message, lib.ac_last_error()
    abi("null pointer: unitig_off and link_off are required", 1, None, zero, one, one, None, None, None, None, None, None, None, device, ctypes.byref(h))
    abi("null pointer: number and len are required", 1, off, zero, None, one, None, None, None, None, None, None, None, device, ctypes.byref(h))
    abi("null pointer: links", 1, off, off, one, one, None, None, None, None, None, None, None, device, ctypes.byref(h))
    abi("null pointer: read_depth and has_read_depth come together or not at all", 1, off, zero, one, one, None, None, None, rd, None, None, None, device, ctypes.byref(h))
    abi("null pointer: seq_bytes and seq_begin come together or not at all", 1, off, zero, one, one, None, None, None, None, None, one, None, device, ctypes.byref(h))
    abi("combine: unitig_off and link_off must start at 0", 1, (ctypes.c_uint64 * 2)(1, 1), zero, one, one, None, None, None, None, None, None, None, device, ctypes.byref(h))
    abi("combine: graph 1: unitig_off does not ascend", 2, (ctypes.c_uint64 * 3)(0, 1, 0), (ctypes.c_uint64 * 3)(0, 0, 0), one, one, None, None, None, None, None, None, None, device,
        ctypes.byref(h))
    assert lib.ac_combine_graphs(1, off, zero, one, one, None, None, None, None, None, None, None, device, None) == 1 and lib.ac_last_error() == b"null pointer: out"
    # the loader's and the command's own
    for text, message in ((b"S\t1\tACGT\n", "Could not find a depth tag"), (b"S\tx\tACGT\tDP:f:1\n", "Unable to parse unitig number."), (b"S\t1\n", "Segment line does not have enough parts."),
                          (b"S\t1\tAC\tDP:f:1\nL\t1\t+\t1\t+\t5M\n", "non-zero overlap found on the GFA link line")):
        with pytest.raises(AutocyclerError, match=message):
            combine_gfas([text], device=device, lib_path=lib_path)
        with pytest.raises(AutocyclerError, match=message):
            gfa2fasta(text, device=device, lib_path=lib_path)
    with pytest.raises(AutocyclerError, match="at least one graph is required"):
        combine_gfas([], device=device, lib_path=lib_path)
    with tempfile.TemporaryDirectory() as tmp:
        gfa = Path(tmp) / "a.gfa"
        gfa.write_bytes(one_tig(1, 20))
        reads = Path(tmp) / "r.fastq"
        reads.write_bytes(b"@r\nACGT\n+\nIIII\n")
        with pytest.raises(AutocyclerError, match="file does not exist: .*missing.gfa"):
            combine_dir(Path(tmp) / "out", [gfa, Path(tmp) / "missing.gfa"], device=device, lib_path=lib_path)
        with pytest.raises(AutocyclerError, match="file does not exist: .*missing.fastq"):
            combine_dir(Path(tmp) / "out", [gfa], reads=[Path(tmp) / "missing.fastq"], device=device, lib_path=lib_path)
        for k, message in ((9, "--depth_kmer cannot be less than 11"), (33, "--depth_kmer cannot be greater than 31"), (20, "--depth_kmer must be odd")):
            with pytest.raises(AutocyclerError, match=message):
                combine_dir(Path(tmp) / "out", [gfa], reads=[reads], depth_kmer=k, device=device, lib_path=lib_path)
        with pytest.raises(AutocyclerError, match="at least one graph is required"):
            combine_dir(Path(tmp) / "out", [], device=device, lib_path=lib_path)
        assert not (Path(tmp) / "out").exists()
        with pytest.raises(AutocyclerError, match="file does not exist"):
            gfa2fasta_file(Path(tmp) / "missing.gfa", Path(tmp) / "x.fasta", device=device, lib_path=lib_path)
    return True


def test_errors(emu):
    assert check_errors(emu)


# ---- the five entry forms ---------------------------------------------------------------------------------------------------------------------------------
def renumbered_clusters():
    """three clusters as resolve leaves them (numbers 1, 2, 3, ... in order, L lines in save_gfa's order): what every entry form can read"""
    ring = CU.gfa_text([(1, seq_of(31, 40), 5.5, "steelblue")], [(1, 1), (-1, -1)])
    two = CU.gfa_text([(1, seq_of(32, 25), "2.675", "steelblue"), (2, seq_of(33, 70), 9.0, "forestgreen"), (3, seq_of(34, 6), 0.5, None)],
                      [(1, 2), (1, -3), (2, 2), (-2, -2), (-2, -1), (3, -1)])
    hairpin = CU.gfa_text([(1, seq_of(35, 33), 4.0, "steelblue")], [(1, -1), (-1, 1)])
    return [ring, two, hairpin]


def check_entry_forms(lib_path, device=0, cli=None):
    texts = renumbered_clusters()
    for rd in (None, [[7.25], [1.05, None, 3.0], [None]]):
        exp, _ = check_texts(texts, lib_path, device, read_depths=rd, what="entry forms")      # arrays and texts
        want = (exp["gfa"], exp["fasta"], exp["yaml"])
        graphs = [graph_from_gfa(t, lib_path)[0] for t in texts]
        c = combine_handles(graphs, types=[gfa_segment_types(t, lib_path) for t in texts], read_depths=rd, device=device, lib_path=lib_path)
        CU.assert_same(c, exp, TOPOLOGY_NAMES, "handles")
        assert (c.gfa(), c.fasta(), c.yaml()) == want
        c.close()
        for g in graphs:
            g.close()
    # the directory and the CLI take files; their read depths come from reads, so these two forms run without
    exp, _ = check_texts(texts, lib_path, device, what="entry forms")
    want = (exp["gfa"], exp["fasta"], exp["yaml"])
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        paths = []
        for i, t in enumerate(texts):
            paths.append(tmp / f"cluster_{i}.gfa")
            paths[-1].write_bytes(t)
        out = tmp / "not" / "yet" / "there"
        report = combine_dir(out, paths, device=device, lib_path=lib_path)
        assert report == "One or more clusters failed to fully resolve\n"
        names = ("consensus_assembly.gfa", "consensus_assembly.fasta", "consensus_assembly.yaml")
        assert tuple((out / n).read_bytes() for n in names) == want and sorted(p.name for p in out.iterdir()) == sorted(names)
        assert combine_dir(out, [paths[0], paths[2]], device=device, lib_path=lib_path) == "Consensus assembly is fully resolved\n"      # (written over)
        assert b"fully_resolved: true" in (out / names[2]).read_bytes()
        if cli is not None:
            done = subprocess.run([str(cli), "combine", "-a", str(tmp / "cli"), "-i"] + [str(p) for p in paths], capture_output=True, timeout=120)
            assert done.returncode == 0, done.stderr
            assert tuple((tmp / "cli" / n).read_bytes() for n in names) == want
            assert b"One or more clusters failed to fully resolve" in done.stderr
            done = subprocess.run([str(cli), "gfa2fasta", "-i", str(paths[1]), "-o", str(tmp / "cli.fasta")], capture_output=True, timeout=120)
            assert done.returncode == 0, done.stderr
            assert (tmp / "cli.fasta").read_bytes() == CU.gfa2fasta_model(texts[1])[0]
            assert b"0 circular sequences\n0 linear sequences\n3 other sequences\n" in done.stderr
    return True


def test_arrays_handles_texts_and_directory_give_the_same_bytes(emu):
    assert check_entry_forms(emu)


# ---- two runs, and what the launches follow ---------------------------------------------------------------------------------------------------------------
def check_two_runs_identical(lib_path, device=0):
    rng = random.Random(5)
    for texts in [random_texts(rng)[0] for _ in range(5)] + [[chain_graph(700, closed=True), link_count_graph(3000)]]:
        forms = [CU.array_form(CU.from_gfa_text(t)) for t in texts]
        a, b = combine_graphs(forms, device=device, lib_path=lib_path), combine_graphs(forms, device=device, lib_path=lib_path)
        assert CU.combined_bytes(a) == CU.combined_bytes(b) and (a.gfa(), a.fasta(), a.yaml()) == (b.gfa(), b.fasta(), b.yaml())
        assert (a.summary["launches"], a.summary["read_backs"]) == (b.summary["launches"], b.summary["read_backs"])
    return True


def test_two_runs_give_identical_results(emu):
    assert check_two_runs_identical(emu)


def check_launch_counts(lib_path, device=0):
    def run(texts, rd=None):
        return check_texts(texts, lib_path, device, read_depths=rd, what="launches")[1]
    # G = 1 and G = 65, one unitig each way too: 65 unitigs and 1 unitig (both inside one digit of the link sort's key: the passes follow its width)
    one, many = run([one_tig(1, 9)]), run([one_tig(1, 3 + g) for g in range(65)])
    assert one["launches"] == many["launches"] and one["read_backs"] == many["read_backs"] == 2, (one, many)
    single, chain = run([one_tig(1, 9, [(1, 1), (-1, -1)])]), run([chain_graph(65, closed=True)])
    assert single["launches"] == chain["launches"] == one["launches"], (single, chain, one)
    # links or none, read depths or none: the same
    assert run([chain_graph(65)], rd=[[1.0] * 65])["launches"] == one["launches"]
    # a wider link key costs one more pass of the link sort per 8 bits, nothing else
    wide = run([chain_graph(200)])
    assert wide["launches"] == one["launches"] + 1, (wide, one)
    return True


def test_launches_do_not_follow_the_sizes(emu):
    assert check_launch_counts(emu)


# ---- gfa2fasta ---------------------------------------------------------------------------------------------------------------------------------------------
def check_gfa2fasta(lib_path, device=0):
    cases = [t for texts in named_cases().values() for t in texts] + renumbered_clusters() + [(CU.GOLDEN / k["gfa"]).read_bytes() for k in CU.load_kats()["topology"]]
    totals = [0, 0, 0]
    for text in cases:
        want, counts = CU.gfa2fasta_model(text)
        assert gfa2fasta(text, device=device, lib_path=lib_path) == (want, counts), text
        totals = [a + b for a, b in zip(totals, counts)]
    assert all(totals), totals
    skipped = CU.gfa_text([(1, b"", 1.0, None), (2, seq_of(2, 6), "0.25", None), (3, b"", 2.0, None)], [(2, 2), (-2, -2)])
    assert gfa2fasta(skipped, device=device, lib_path=lib_path) == (b">2 length=6 depth=0.2 circular=true topology=circular\n" + seq_of(2, 6) + b"\n", (1, 0, 0))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in.gfa", Path(tmp) / "out.fasta"
        src.write_bytes(unresolved_graph())
        assert gfa2fasta_file(src, dst, device=device, lib_path=lib_path) == CU.gfa2fasta_model(unresolved_graph())[1]
        assert dst.read_bytes() == CU.gfa2fasta_model(unresolved_graph())[0]
    return True


def test_gfa2fasta(emu):
    assert check_gfa2fasta(emu)


# ---- the chain, finished ------------------------------------------------------------------------------------------------------------------------------------
CHAIN_CASES = [("small", 1), ("hairpin21", 1), ("clean", 1)]      # two circular replicons of different size; a linear replicon; no differences at all
COVERAGE = (12, 5, 30)      # planted per replicon, by size rank; the last replicon of a case gets no reads
DEPTH_K = 19


def tile_reads(seq, circular, coverage, length=150):
    """error-free reads that tile the replicon `coverage` times, each pass shifted: every base is covered `coverage` times (a circular one exactly)"""
    reads, n = [], len(seq)
    for c in range(coverage):
        shift = (c * 37) % length
        src = seq[shift:] + seq[:shift] if circular else seq
        reads += [src[i:i + length] for i in range(0, n, length)]
    return reads


def fasta_records(text):
    lines = text.decode().split("\n")
    return [(lines[i][1:], lines[i + 1].encode()) for i in range(0, len(lines) - 1, 2)]


_CHAIN = {}


def chain_record(name, seed, lib_path, device):
    key = (name, seed, str(lib_path), device)
    if key not in _CHAIN:
        case = chain_util.make_case(name, seed)
        _CHAIN[key] = (case, chain_util.run_chain(case, lib_path=lib_path, device=device, checks=False))
    return _CHAIN[key]


def check_chain(name, seed, lib_path, device=0):
    case, rec = chain_record(name, seed, lib_path, device)
    of = chain_util.replicon_clusters(case, rec)
    by_size = sorted(range(len(case["truth"])), key=lambda r: -len(case["truth"][r]["seq"]))
    texts = [rec["clusters"][of[r]]["final_gfa"] for r in reversed(by_size)]      # in reverse size order: the sort has something to do
    gfa, fasta, yaml, sm = combine_gfas(texts, device=device, lib_path=lib_path)
    exp = CU.combine_model([CU.from_gfa_text(t) for t in texts])
    assert (gfa, fasta, yaml) == (exp["gfa"], exp["fasta"], exp["yaml"])
    records = fasta_records(fasta)
    assert len(records) == len(case["truth"]) and sm["fully_resolved"] and b"consensus_assembly_fully_resolved: true\n" in yaml
    for i, (r, (header, seq)) in enumerate(zip(by_size, records), 1):
        t = case["truth"][r]
        assert header == f"{i} length={len(t['seq'])} " + ("circular=true topology=circular" if t["circular"] else "circular=false topology=linear"), header
        assert chain_util.same_replicon(seq, t["seq"], t["circular"]), f"{name}: record {i} is not the planted replicon"
    # with reads: the whole command against the depth model
    reads_of = {r: tile_reads(case["truth"][r]["seq"], case["truth"][r]["circular"], COVERAGE[rank]) for rank, r in enumerate(by_size[:-1])}
    graphs = [CU.from_gfa_text(t) for t in texts]
    checker = depth_util.Checker(DEPTH_K, [([u.seq for u in g.unitigs], [(l[0], l[1]) for l in CU.array_form(g)["links"]]) for g in graphs])
    checker.add_reads([read for r in sorted(reads_of) for read in reads_of[r]])
    model_depths = [checker.depths(i) for i in range(len(graphs))]
    exp = CU.combine_model(graphs, model_depths)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        paths = []
        for i, t in enumerate(texts):
            paths.append(tmp / f"{i}.gfa"); paths[-1].write_bytes(t)
        fq = tmp / "reads.fastq"
        fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, read, b"I" * len(read)) for i, read in enumerate(read for r in sorted(reads_of) for read in reads_of[r])))
        report = combine_dir(tmp / "out", paths, reads=[fq], depth_kmer=DEPTH_K, device=device, lib_path=lib_path)
        got = tuple((tmp / "out" / f"consensus_assembly.{e}").read_bytes() for e in ("gfa", "fasta", "yaml"))
        assert got == (exp["gfa"], exp["fasta"], exp["yaml"]), f"{name}: with reads the command's files are not the model's"
        assert report == exp["depth_lines"].decode() + "Consensus assembly is fully resolved\n"
    # ReadDepth results go straight into the object form
    with ReadDepth(DEPTH_K, [([u.seq for u in g.unitigs], CU.array_form(g)["links"]) for g in graphs], device=device, lib_path=lib_path) as rd:
        rd.add_reads([read for r in sorted(reads_of) for read in reads_of[r]])
        c = combine_graphs([CU.array_form(g) for g in graphs], read_depths=rd, device=device, lib_path=lib_path)
        assert (c.gfa(), c.fasta(), c.yaml()) == (exp["gfa"], exp["fasta"], exp["yaml"])
        c.close()
    found = {}
    for rank, r in enumerate(by_size):
        depth = exp["tigs"][rank][2]
        text = "unavailable" if depth is None else CU.fixed(depth, 1)
        assert f"{rank + 1} length={len(case['truth'][r]['seq'])} depth={text}" in fasta_records(exp["fasta"])[rank][0]
        found[rank] = (COVERAGE[rank] if r in reads_of else 0, depth)
    assert found[len(by_size) - 1][1] in (None, 0.0), found      # the replicon without reads: whatever the model says, and it says one of these
    return found


@pytest.mark.parametrize("name,seed", CHAIN_CASES)
def test_chain_ends_in_the_planted_consensus(emu, name, seed):
    found = check_chain(name, seed, emu)
    print("planted coverage and the model's depth per replicon:", found)
