"""ac_clean_graph / ac_graph_clean, the Cleaned object, the composed entries, ac_parse_tig_numbers, ac_gfa_segment_types, ac_clean_gfa and
ac_clean on the CPU emulation of the shipped kernels (kernels_clean.inc) against the literal Python model of clean_util.py: removal, the
sequential duplication with its list pushes, the reverse walk of remove_low_depth_unitigs, then merge_util, finish_util.finish_model and
finish_util.save_gfa for the texts.  Every comparison is equality (depths bit for bit, link order included).  The same checks run on the
device in test_clean_gpu.py.  The boundary table's rows beyond one wavefront (tile sizes, wide keys, rounds side by side) are judged by
clean_util.clean_model_fast, which the tests here hold equal to the literal model wherever that one is affordable."""
import ctypes
import math
import random
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import clean_util as CU
import emu_lib
import finish_util as F
import merge_util as M
from autocycler_amd import AutocyclerError, Cleaned, clean_gfa, clean_graph, gfa_segment_types, graph_from_gfa, parse_tig_numbers
from autocycler_amd import _capi

NEW_SYMBOLS = ("ac_clean_graph", "ac_graph_clean", "ac_cleaned_unitigs", "ac_cleaned_links", "ac_cleaned_summary_get_sized", "ac_cleaned_free", "ac_cleaned_merge_plan",
               "ac_cleaned_finish", "ac_cleaned_gfa_string", "ac_parse_tig_numbers", "ac_gfa_segment_types", "ac_clean_gfa", "ac_clean")
K = 7      # the k-mer size the texts are printed with (the H line only)
NAN = float("nan")
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_clean(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


# ---- cases on plain arrays ---------------------------------------------------------------------------------------------------------------------
def make_case(n, links, depths=None, lens=None, types=None, alive=None, remove=(), duplicate=(), min_depth=None):
    """links: one direction is enough; they are closed under reverse complement and put into L-line order"""
    lens = list(lens) if lens is not None else [(u % 5) + 1 for u in range(1, n + 1)]
    return dict(n=n, links=CU.l_line_order(M.closed_set(links)), lens=lens, depths=list(depths) if depths is not None else [4.0] * n, types=types, alive=alive,
                seqs=[M._seq_of(u, l) for u, l in enumerate(lens, 1)], remove=list(remove), duplicate=list(duplicate), min_depth=min_depth)


def run_library(case, lib_path, device=0, sequences=True):
    return clean_graph(case["n"], case["links"], case["lens"], depth=case["depths"], unitig_type=case["types"], alive=case["alive"],
                       sequences=case["seqs"] if sequences else None, remove=case["remove"], duplicate=case["duplicate"], min_depth=case["min_depth"], device=device,
                       lib_path=lib_path)


def run_model(case):
    return CU.clean_model(case["n"], case["links"], case["lens"], case["depths"], case["types"], case["alive"], case["seqs"], case["remove"], case["duplicate"], case["min_depth"])


def run_model_fast(case, counts=None):
    """clean_util.clean_model_fast: the judge where the literal model is not affordable, held equal to it where it is (test_fast_model_*)"""
    return CU.clean_model_fast(case["n"], case["links"], case["lens"], case["depths"], case["types"], case["alive"], case["seqs"], case["remove"], case["duplicate"],
                               case["min_depth"], counts=counts)


def check_case(case, lib_path, device=0, what="", texts=True, exp=None):
    """one graph: the arrays, reasons and link order, the edited graph's text, and the merged graph with its text against the model -> (model, summary).
    texts=False: the arrays, reasons, depths bit for bit, link order and summary only (no Python merge, finish or save_gfa); exp: the model's
    result where the caller has it already"""
    exp = run_model(case) if exp is None else exp
    cl = run_library(case, lib_path, device)
    assert isinstance(cl, Cleaned) and cl.n_unitigs == case["n"]
    CU.assert_same(cl, exp, what)
    seq_begin = [0] + np.cumsum(case["lens"]).tolist()[:-1] if case["n"] else []
    assert ([] if cl.seq_begin is None else cl.seq_begin.tolist()) == [seq_begin[(c or u + 1) - 1] for u, c in enumerate(exp["copy_of"])], (what, "seq_begin")
    assert cl.summary["rounds_per_batch"] >= 2 and cl.summary["links_in"] == len(case["links"])
    if not texts:
        sm = cl.summary
        cl.close()
        return exp, sm
    if not CU.has_nan_alive(exp):      # (a NaN depth prints differently in Rust, C and Python: the arrays above have compared it)
        for colour in (False, True):
            assert cl.gfa(K, use_other_colour=colour) == CU.cleaned_text(exp, K, colour), (what, "text of the edited graph")
    if CU.is_multiset(exp):
        with pytest.raises(AutocyclerError, match="is a duplicate: the merge plan needs the links among alive unitigs as a set"):
            cl.merge_plan()
    elif CU.has_nan_alive(exp):      # (renumber_unitigs' comparator is no total order over a NaN depth: the finished graph refuses it, as it always has)
        plan = cl.merge_plan()
        with pytest.raises(AutocyclerError, match="is NaN: renumber_unitigs' comparator is no total order there"):
            cl.finish(plan, renumber=True)
        plan.close()
    else:
        plan = cl.merge_plan()
        fin = cl.finish(plan, renumber=True)
        want = CU.merged_model(exp)
        F.assert_model_same(F.library_model(fin, False), want, what)
        assert fin.gfa(K, use_other_colour=True) == F.save_gfa(want, K, (), True), (what, "final text")
        fin.close(); plan.close()
    sm = cl.summary
    cl.close()
    return exp, sm


# ---- the reference's own known answers ------------------------------------------------------------------------------------------------------------
def link_count(links):
    every = {tuple(l) for l in links}
    return [len(every), len({max(l, (-l[1], -l[0])) for l in every})]


def fixture_case(name, **kw):
    g = M.gfa_graph(name)
    return dict(n=g["n"], links=CU.l_line_order(g["links"]), lens=g["lens"], depths=g["depths"], types=None, alive=g["alive"], seqs=g["seqs"],
                remove=kw.get("remove", []), duplicate=kw.get("duplicate", []), min_depth=kw.get("min_depth"))


def state_of(alive, lens, links):
    return dict(unitigs=int(sum(alive)), bases=int(sum(l for l, a in zip(lens, alive) if a)), links=link_count(links))


def check_kats(lib_path, device=0):
    kats = CU.load_kats()
    # remove_low_depth_unitigs, merge_linear_paths, remove_low_depth_unitigs
    kat = kats["low_depth"]
    case = fixture_case(kat["fixture"])
    assert state_of([1] * case["n"] if case["alive"] is None else case["alive"], case["lens"], case["links"]) == kat["before"]
    case["min_depth"] = kat["min_depth"]
    exp, _ = check_case(case, lib_path, device, "kat low depth")
    cl = run_library(case, lib_path, device)
    assert state_of(cl.alive.tolist(), cl.len.tolist(), cl.links.tolist()) == kat["after_low_depth"]
    plan = cl.merge_plan()
    fin = cl.finish(plan, renumber=True)
    lens, links = [int(u["length"]) for u in fin.unitigs], [tuple(l) for l in fin.links.tolist()]
    assert state_of([1] * len(lens), lens, links) == kat["after_merge"]
    again = dict(n=len(lens), links=links, lens=lens, depths=[float(u["depth"]) for u in fin.unitigs], types=[int(u["type"]) for u in fin.unitigs], alive=None,
                 seqs=fin.unitig_sequences(), remove=[], duplicate=[], min_depth=kat["min_depth"])
    check_case(again, lib_path, device, "kat low depth again")
    cl2 = run_library(again, lib_path, device)
    assert state_of(cl2.alive.tolist(), cl2.len.tolist(), cl2.links.tolist()) == kat["after_low_depth_again"]
    # duplicate_unitig_by_number
    for kat in kats["duplicate"]:
        case = fixture_case(kat["fixture"], duplicate=[kat["number"]])
        assert state_of([1] * case["n"] if case["alive"] is None else case["alive"], case["lens"], case["links"]) == kat["before"]
        exp = run_model(case)
        cl = run_library(case, lib_path, device)
        CU.assert_same(cl, exp, kat["fixture"])
        assert state_of(cl.alive.tolist(), cl.len.tolist(), cl.links.tolist()) == kat["after"], kat["fixture"]
    # remove_unitigs_by_number
    kat = kats["remove"]
    case = fixture_case(kat["fixture"])
    assert M.U.UnitigGraph(case["n"], case["links"], case["alive"]).connected_components() == kat["before"]
    gone = []
    for step in kat["steps"]:
        gone += step["remove"]
        case["remove"] = list(gone)
        exp, _ = check_case(case, lib_path, device, "kat remove")
        cl = run_library(case, lib_path, device)
        assert M.U.UnitigGraph(cl.n_out, [tuple(l) for l in cl.links.tolist()], cl.alive.tolist()).connected_components() == step["components"]
    # parse_tig_numbers
    for text, want in kats["parse_tig_numbers"]["ok"]:
        assert parse_tig_numbers(text, lib_path) == want == CU.parse_tig_numbers(text)
    for text in kats["parse_tig_numbers"]["errors"]:
        with pytest.raises(AutocyclerError, match="failed to parse '.*' as a node number"):
            parse_tig_numbers(text, lib_path)
        with pytest.raises(CU.CleanError):
            CU.parse_tig_numbers(text)
    return True


def test_reference_known_answers(emu):
    assert check_kats(emu)


# ---- named cases -------------------------------------------------------------------------------------------------------------------------------
def named_cases():
    ring6 = [(1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 1)]
    return {
        "removal splits a component": make_case(7, [(1, 2), (2, 3), (3, 4), (4, 5), (3, 6), (6, 7)], remove=[3]),
        "removal listed twice": make_case(4, [(1, 2), (2, 3), (3, 4)], remove=[2, 2]),
        "duplication, plain": make_case(5, [(1, 3), (3, 4), (2, 5)], duplicate=[3], depths=[4.0, 2.0, 7.0, 1.0, 1.0]),
        "duplication, both links on one strand": make_case(4, [(1, 2), (1, 3), (4, 2)], duplicate=[1], depths=[9.0, 1.0, 1.0, 1.0]),
        "duplication with a hairpin": make_case(4, [(1, 2), (2, -2), (3, 2)], duplicate=[2], depths=[1.0, 5.0, 1.0, 1.0]),
        "duplication with a start hairpin": make_case(3, [(-2, 2), (2, 1), (2, 3)], duplicate=[2]),
        "duplication with a loop: doubled links": make_case(3, [(1, 2), (2, 2), (2, 3)], duplicate=[2], depths=[1.0, 6.0, 1.0]),
        "two duplicated tigs linked to each other": make_case(6, [(1, 2), (2, 3), (3, 4), (5, 6)], duplicate=[2, 3]),
        "two duplicated tigs linked twice": make_case(4, [(2, 3), (2, -3), (1, 4)], duplicate=[2, 3]),
        "neighbour's list order decides the L lines": make_case(5, [(1, 3), (1, 4), (1, 5), (2, 3)], duplicate=[3], depths=[1.0, 1.0, 3.0, 1.0, 1.0]),
        "duplicate then low depth: the copies are low": make_case(4, [(1, 2), (2, 3)], duplicate=[2], depths=[5.0, 3.0, 5.0, 5.0], min_depth=1.5),
        "copies low between forks": make_case(6, [(3, 4), (1, 5), (5, 4), (2, 6), (6, 4)], duplicate=[5], depths=[5.0, 5.0, 5.0, 5.0, 2.0, 5.0], min_depth=1.0),
        "low depth, depth == min_depth": make_case(4, [(1, 2), (1, 3), (2, 4), (3, 4)], depths=[5.0, 1.0, 5.0, 5.0], min_depth=1.0),
        "low depth, just above": make_case(4, [(1, 2), (1, 3), (2, 4), (3, 4)], depths=[5.0, math.nextafter(1.0, 2.0), 5.0, 5.0], min_depth=1.0),
        "low depth, NaN depth": make_case(4, [(1, 2), (1, 3), (2, 4), (3, 4)], depths=[5.0, NAN, 5.0, 5.0], min_depth=1.0),
        "low depth, NaN depth kept at a dead end": make_case(3, [(1, 2), (2, 3)], depths=[5.0, NAN, 5.0], min_depth=1.0),
        "low depth, NaN min_depth": make_case(5, [(1, 2), (1, 3), (2, 4), (3, 4), (4, 5)], depths=[5.0, 1.0, 9.0, 5.0, 2.0], min_depth=NAN),
        "low depth, neighbour's only other entry is its self link": make_case(3, [(1, 2), (2, 2), (2, 3)], depths=[0.5, 5.0, 5.0], min_depth=1.0),
        "low depth, neighbour's only other entry is a hairpin": make_case(2, [(1, 2), (2, -2)], depths=[0.5, 5.0], min_depth=1.0),
        "low depth, two bubble arms: the later number goes, the earlier stays": make_case(4, [(1, 2), (1, 3), (2, 4), (3, 4)], depths=[5.0, 1.0, 1.0, 5.0], min_depth=1.0),
        "low depth, ring of low unitigs": make_case(6, ring6, depths=[0.5] * 6, min_depth=1.0),
        "low depth with an alive mask and types": make_case(6, ring6 + [(2, 5)], depths=[5.0, 5.0, 0.5, 5.0, 5.0, 0.2], types=[1, 0, 3, 2, 0, 0], alive=[1, 1, 1, 0, 1, 1],
                                                                min_depth=1.0),
        "all three options": make_case(8, ring6 + [(7, 1), (2, 8), (8, 4)], depths=[5.0, 5.0, 0.5, 5.0, 5.0, 5.0, 0.1, 0.3], remove=[6], duplicate=[8], min_depth=1.0),
    }


def check_named_cases(lib_path, device=0):
    met = dict(multiset=0, low_removed=0, dead_end=0, copies_low=0)
    for name, case in named_cases().items():
        exp, sm = check_case(case, lib_path, device, name)
        met["multiset"] |= CU.is_multiset(exp)
        met["low_removed"] |= sm["low_depth"] > 0
        met["dead_end"] |= sm["kept_dead_end"] > 0
        met["copies_low"] |= any(r in (CU.LOW_DEPTH, CU.KEPT_DEAD_END) for r in exp["reason"][case["n"]:])
        if name == "duplication with a loop: doubled links":
            n = case["n"]
            assert exp["links"].count((n + 1, n + 1)) == 2 and exp["links"].count((-(n + 2), -(n + 2))) == 2, "each copy carries the loop twice"
        if name == "duplication with a hairpin":
            n = case["n"]
            assert exp["links"].count((n + 1, -(n + 1))) == 1 and exp["links"].count((n + 2, -(n + 2))) == 1, "a hairpin is created once"
    assert all(met.values()), met
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


# ---- the boundary table ----------------------------------------------------------------------------------------------------------------------------
def chain_case(n, descending=False, low=None):
    """1 - 2 - ... - n in a row, every unitig low (or the first `low` of them): as many rounds.  descending: the chain runs n, n - 1, ..., 1"""
    order = list(range(n, 0, -1)) if descending else list(range(1, n + 1))
    return make_case(n, list(zip(order, order[1:])), depths=[0.5 if low is None or u < low else 5.0 for u in range(n)], min_depth=1.0)


def hub_case(degree):
    """a hub of the given degree whose spokes are low and lead on to a common sink: all spokes but one go"""
    n = degree + 2
    spokes = list(range(2, degree + 2))
    return make_case(n, [(1, s) for s in spokes] + [(s, n) for s in spokes], depths=[5.0] + [0.5] * degree + [5.0], min_depth=1.0)


def candidates_case(count):
    """`count` separate bubbles with one low arm each: one round decides them all"""
    links, depths = [], []
    for b in range(count):
        o = 4 * b
        links += [(o + 1, o + 2), (o + 1, o + 3), (o + 2, o + 4), (o + 3, o + 4)]
        depths += [5.0, 0.5, 5.0, 5.0]
    return make_case(4 * count, links, depths=depths, min_depth=1.0)


# ---- rows beyond one wavefront: the tiles of device_prims.hpp (RS_TILE = 2048, SCAN_TILE = 4096), the key widths, rounds side by side ----------------
TILE_SIZES = (2047, 2048, 2049, 4095, 4096, 4097)
LITERAL_MAX = 4097      # up to here the literal model judges or is compared with the fast one; above it clean_model_fast alone
TEXTS_MAX = 4097        # up to here the Python merge, finish and save_gfa are run as well


def bit_width(x):
    return int(x).bit_length()


def tile_case(seed, n, nl=None, ne=None, candidates=None, n_remove=50, n_dup=40, link_factor=1.3, low=1 / 3, special=0.02):
    """a random closed graph of n unitigs: about link_factor links per unitig, `special` of them loops and hairpins, n_remove removals, n_dup
    duplications of pairwise non-adjacent duplicable unitigs without a loop (a quarter of them of a depth whose half is low), about `low` of the
    unitigs low.  nl, ne, candidates: the exact number of link entries, of entries after the duplications, of low unitigs the walk meets — links
    between unitigs that are neither removed nor duplicated are added until nl or ne holds (a hairpin for an odd rest).  The caller states the
    counts it wants as case["expect"]; check_row asserts them."""
    rng = random.Random(seed)
    signed = lambda: rng.randint(1, n) * rng.choice((1, -1))
    links = {}

    def add(a, b):
        links[(a, b)] = links[(-b, -a)] = True

    factor = link_factor if nl is None and ne is None else link_factor - 0.05      # (below the target: the rest is added)
    for _ in range(int(factor * n)):
        a = signed()
        add(a, (a if rng.random() < 0.5 else -a) if rng.random() < special else signed())
    remove = sorted(rng.sample(range(1, n + 1), n_remove))
    gone = set(remove)
    others, loop = [[] for _ in range(n + 1)], [False] * (n + 1)
    for a, b in links:
        if abs(a) in gone or abs(b) in gone:
            continue
        if abs(a) == abs(b):
            loop[abs(a)] |= a == b
        else:
            others[abs(a)].append(abs(b))
    able = [u for u in range(1, n + 1) if u not in gone and len(others[u]) == 2 and not loop[u]]
    rng.shuffle(able)
    duplicate, near = [], set()
    for u in able:
        if len(duplicate) < n_dup and u not in near:
            duplicate.append(u)
            near |= {u} | set(others[u])
    assert len(duplicate) == n_dup, "too few duplicable unitigs: another seed"
    low_dups = set(duplicate[:n_dup // 4])
    free = [u for u in range(1, n + 1) if u not in gone and u not in duplicate]
    n_low = (round(low * n) if candidates is None else candidates) - 2 * len(low_dups)
    low_set = set(rng.sample(free, n_low))
    depths = [1.5 if u in low_dups else 9.0 if u in duplicate else 0.5 if u in low_set else rng.choice((0.0, 0.5, 1.0)) if u in gone else rng.choice((1.5, 7.0, 20.0))
              for u in range(1, n + 1)]
    case = lambda: make_case(n, list(links), depths=depths, lens=[1 + (u * 7) % 6 for u in range(n)], types=[(u * 5 + u // 3) % 4 for u in range(n)], remove=remove,
                             duplicate=sorted(duplicate), min_depth=1.0)
    if nl is not None or ne is not None:
        counts = {}
        if ne is not None:
            run_model_fast(dict(case(), min_depth=None), counts)
        rest = nl - len(links) if nl is not None else ne - counts["n_edit"]
        assert rest >= 0, "the base graph is above the target: a lower link_factor"
        while rest:
            a, b = signed(), signed()
            if abs(a) in gone or abs(b) in gone or abs(a) in duplicate or abs(b) in duplicate or (a, b) in links:
                continue
            if rest == 1:
                b = -a
            elif abs(a) == abs(b):
                continue
            if (a, b) in links:
                continue
            add(a, b)
            rest -= 1 if a == -b else 2
    return case()


def multi_arm_case(bubbles, arms, seed=31, spare=0):
    """`bubbles` bubbles of `arms` low arms and one high arm between the same two ends, the numbers dealt in a shuffled order, random strands: the
    arms of one bubble lie within distance two of each other, so one goes per round; the high arm keeps every end off a dead end, so all go.
    spare: as many high unitigs without a link among them (they widen the keys and nothing else)"""
    rng = random.Random(seed)
    n = bubbles * (arms + 3) + spare
    numbers = list(range(1, n + 1))
    rng.shuffle(numbers)
    strand = [rng.choice((1, -1)) for _ in range(n + 1)]
    depths, links = [5.0] * n, []
    for b in range(bubbles):
        mine = numbers[b * (arms + 3):(b + 1) * (arms + 3)]
        start, end = mine[0] * strand[mine[0]], mine[1] * strand[mine[1]]
        for arm in mine[2:]:
            links += [(start, arm * strand[arm]), (arm * strand[arm], end)]
        for arm in mine[3:]:
            depths[arm - 1] = 0.5
    case = make_case(n, links, depths=depths, min_depth=1.0)
    case["expect"] = dict(rounds=arms, low_depth=bubbles * arms, kept_dead_end=0, candidates=bubbles * arms)
    return case


def with_expect(case, **expect):
    case["expect"] = expect
    return case


def tile_rows(batch):
    """the rows of part 2 of the boundary table; each states in `expect` the counts that make it the row it is"""
    rows = {}
    for t in TILE_SIZES:
        # n and n_out = n + 2 * 40 at the tile; with n_out the duplications alone carry the unitig count to and over it
        rows[f"tile: n = {t}"] = with_expect(tile_case(t, t), n=t, n_out=t + 80)
        rows[f"tile: n_out = {t}"] = with_expect(tile_case(100 + t, t - 80), n=t - 80, n_out=t)
        # the link entries (the first sort and the two flag scans), the edited entries (the second sort, the out-link scan, the offset search)
        rows[f"tile: nl = {t}"] = with_expect(tile_case(200 + t, int(t / 2.6) + 1, nl=t), nl=t)
        rows[f"tile: ne = {t}"] = with_expect(tile_case(300 + t, int((t + 260) / 2.6) + 1, ne=t), ne=t)
        # the candidates (their scan, the work lists): three times as many unitigs
        rows[f"tile: candidates = {t}"] = with_expect(tile_case(400 + t, 3 * t, candidates=t), candidates=t, n=3 * t)
    rows["tile: one duplication carries n_out from 2047 over 2048"] = with_expect(tile_case(7, 2047, n_dup=1), n=2047, n_out=2049)
    for n in (32767, 32768):      # the link key is 2 * bit_width(2 n) bits wide: 32, then 34 — the first width whose upper half is not zero
        rows[f"wide keys: n = {n}"] = with_expect(tile_case(500 + (n & 1), n, n_remove=0, n_dup=10, low=0.01), n=n, link_key_bits=2 * bit_width(2 * n))
    assert rows["wide keys: n = 32767"]["expect"]["link_key_bits"] == 32 and rows["wide keys: n = 32768"]["expect"]["link_key_bits"] == 34
    for arms in (12, 2 * batch + 1):
        rows[f"multi-arm bubbles: 300 of {arms} low arms"] = multi_arm_case(300, arms)
    rows["dense: 4096 unitigs, 2.5 links each, half low"] = with_expect(tile_case(11, 4096, n_remove=0, n_dup=0, link_factor=2.5, low=0.5), n=4096, dense=True)
    return rows


def round_schedule(case, exp, counts):
    """-> per candidate the round that decides it, by the rule of DESIGN 9l read off the model's edited entries: a candidate is decided in the
    round after the last larger candidate whose closed neighbourhood meets its own (they share a slot), in the first round without one"""
    first = {}
    for a, b in counts["edited"]:
        first.setdefault(abs(a), {abs(a)}).add(abs(b))
    slot, rounds = {}, {}
    for u in range(exp["n_out"], 0, -1):
        if exp["reason"][u - 1] in (CU.LOW_DEPTH, CU.KEPT_DEAD_END):
            hood = first.get(u, {u})
            rounds[u] = 1 + max(slot.get(s, 0) for s in hood)
            for s in hood:
                slot[s] = rounds[u]
    return rounds


def row_facts(case, exp, counts, batch):
    rounds = round_schedule(case, exp, counts)
    return dict(n=case["n"], n_out=exp["n_out"], nl=len(case["links"]), ne=counts["n_edit"], candidates=counts["n_candidates"], link_key_bits=2 * bit_width(2 * case["n"]),
                low_depth=exp["reason"].count(CU.LOW_DEPTH), kept_dead_end=exp["reason"].count(CU.KEPT_DEAD_END), rounds=max(rounds.values(), default=0),
                left_after_a_batch=sum(1 for r in rounds.values() if r > batch))


def check_row(name, case, facts, rounds, batch):
    """what makes the row the row it is, as assertions; rounds: the library's"""
    expect = case.get("expect", {})
    for key, want in expect.items():
        if key != "dense":
            assert facts[key] == want, (name, key, facts[key], want)
    assert rounds == facts["rounds"], (name, "rounds", rounds, facts["rounds"])
    if "expect" in case:
        assert facts["low_depth"] >= 1, (name, "no deletion: the row passes vacuously")
    if name.startswith(("tile:", "wide keys", "dense")):
        assert facts["kept_dead_end"] >= 1, (name, "no dead end")
    if expect.get("dense"):
        assert rounds > 2 * batch and facts["low_depth"] > 256 and facts["kept_dead_end"] > 256 and facts["left_after_a_batch"] > 256, (name, facts)


_ROWS = {}      # per batch size: the cases, and per row the model's result — built once, shared by the emulation, the device and the guard drivers, read only


def boundary_expected(batch, name):
    """-> (model, facts) of one row: the literal model for the rows at the scale of one wavefront, clean_model_fast for the tile rows (held equal
    to the literal one up to LITERAL_MAX unitigs by test_fast_model_equals_the_literal_model_on_the_boundary_table)"""
    cases, cache = boundary_cases(batch), _ROWS[batch][1]
    if name not in cache:
        case, counts = cases[name], {}
        fast = run_model_fast(case, counts)
        cache[name] = (fast if "expect" in case else run_model(case), row_facts(case, fast, counts, batch))
    return cache[name]


def boundary_cases(batch):
    if batch not in _ROWS:
        _ROWS[batch] = (dict(small_rows(batch), **tile_rows(batch)), {})
    return _ROWS[batch][0]


def small_rows(batch):
    cases = {}
    for c in (63, 64, 65):
        cases[f"{c} candidates"] = candidates_case(c)
    for d in (63, 64, 65, 257):
        cases[f"hub of degree {d}"] = hub_case(d)
    for length in (batch - 1, batch, batch + 1, 2 * batch + 1):
        cases[f"chain of {length} ascending"] = chain_case(length)
        cases[f"chain of {length} descending"] = chain_case(length, descending=True)
    cases["empty graph"] = make_case(0, [])
    cases["nothing to do"] = make_case(5, [(1, 2), (2, 3), (3, 4), (4, 5)])
    cases["nothing low"] = make_case(5, [(1, 2), (2, 3), (3, 4), (4, 5)], min_depth=1.0)
    cases["no links"] = make_case(3, [], depths=[0.5, 5.0, 0.5], min_depth=1.0)
    cases["everything removed"] = make_case(4, [(1, 2), (2, 3), (3, 4)], remove=[1, 2, 3, 4])
    cases["everything low and free"] = make_case(3, [], depths=[0.5] * 3, min_depth=1.0)
    return cases


def rounds_per_batch(lib_path, device=0):
    cl = run_library(make_case(1, []), lib_path, device)
    return cl.summary["rounds_per_batch"]


def check_boundary_table(lib_path, device=0, only=None):
    """only: the rows whose names begin so (a tuple), or "one wavefront" for the rows that state no counts; every row without it"""
    batch = rounds_per_batch(lib_path, device)
    chosen = {name: case for name, case in boundary_cases(batch).items() if only is None or ("expect" not in case if only == "one wavefront" else name.startswith(only))}
    assert chosen, only
    for name, case in chosen.items():
        model, facts = boundary_expected(batch, name)
        exp, sm = check_case(case, lib_path, device, name, texts=case["n"] <= TEXTS_MAX, exp=model)
        check_row(name, case, facts, sm["rounds"], batch)
        if name.startswith("multi-arm"):
            assert sm["rounds"] == case["expect"]["rounds"] and sm["low_depth"] == case["n"] // (sm["rounds"] + 3) * sm["rounds"] and sm["kept_dead_end"] == 0, name
        if name.startswith("chain of"):
            assert sm["rounds"] == case["n"], (name, sm["rounds"])
        if name.endswith("candidates"):
            assert sm["rounds"] == 1 and sm["low_depth"] == case["n"] // 4, name
        if name.startswith("hub"):
            assert sm["low_depth"] == case["n"] - 3 and sm["kept_dead_end"] == 1, name
        if name in ("empty graph", "nothing to do", "nothing low", "everything removed"):
            assert sm["rounds"] == 0, name
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


def check_large(case, lib_path, device=0, what=""):
    """a case beyond the literal model: two runs held to clean_model_fast without the texts, and to each other as bytes -> (model, summary)"""
    exp = run_model_fast(case)
    a, b = run_library(case, lib_path, device), run_library(case, lib_path, device)
    CU.assert_same(a, exp, what)
    assert CU.cleaned_bytes(a) == CU.cleaned_bytes(b), (what, "two runs")
    assert (a.summary["launches"], a.summary["read_backs"], a.summary["rounds"]) == (b.summary["launches"], b.summary["read_backs"], b.summary["rounds"]), what
    sm = a.summary
    a.close(); b.close()
    return exp, sm


def test_bubbles_beyond_a_tile(emu):
    """2049 bubbles side by side: one round, 2049 decisions in 33 wavefronts"""
    _, sm = check_large(candidates_case(2049), emu, what="2049 bubbles")
    assert sm["rounds"] == 1 and sm["low_depth"] == 2049 and sm["kept_dead_end"] == 0


def test_hub_of_degree_4097(emu):
    """4097 rounds, 513 batches, a range off[2u] .. off[2u + 2] of 4097 entries: the emulation only (16 s here; the guard drivers and the device's
    launch count are spared)"""
    hub = hub_case(4097)
    _, sm = check_case(hub, emu, what="hub of degree 4097", texts=False, exp=run_model_fast(hub))
    assert sm["rounds"] == 4097 and sm["low_depth"] == 4096 and sm["kept_dead_end"] == 1


# ---- the fast model is the literal one ---------------------------------------------------------------------------------------------------------------
def assert_fast_is_literal(case, what, literal=None):
    try:
        literal = run_model(case) if literal is None else literal
    except CU.CleanError as e:
        with pytest.raises(CU.CleanError) as fast:
            run_model_fast(case)
        assert str(fast.value) == str(e), what
        return None
    CU.assert_models_equal(run_model_fast(case), literal, what)
    return literal


def test_fast_model_equals_the_literal_model_on_the_existing_cases():
    """the known answers' graphs with their options, the named cases, the error list's cases, every case of the four sweeps and of the order and two-run checks"""
    kats = CU.load_kats()
    assert_fast_is_literal(fixture_case(kats["low_depth"]["fixture"], min_depth=kats["low_depth"]["min_depth"]), "kat low depth")
    for kat in kats["duplicate"]:
        assert_fast_is_literal(fixture_case(kat["fixture"], duplicate=[kat["number"]]), kat["fixture"])
    gone = []
    for step in kats["remove"]["steps"]:
        gone += step["remove"]
        assert_fast_is_literal(fixture_case(kats["remove"]["fixture"], remove=list(gone)), "kat remove")
    for name, case in named_cases().items():
        assert_fast_is_literal(case, name)
    base = dict(n=5, links=CU.l_line_order(M.closed_set([(1, 2), (2, 3), (3, 4), (3, 5)])), lens=[3] * 5, depths=[4.0] * 5, types=None, alive=[1, 1, 1, 1, 0], seqs=None,
                remove=[], duplicate=[], min_depth=None)
    for kw in (dict(remove=[9]), dict(remove=[0]), dict(remove=[5]), dict(duplicate=[6]), dict(remove=[1], duplicate=[2, 7]), dict(duplicate=[1]), dict(duplicate=[3], alive=None),
               dict(remove=[2], duplicate=[2]), dict(duplicate=[2, 2]), dict(remove=[4], duplicate=[3])):
        assert assert_fast_is_literal(dict(base, **kw), f"error {kw}") is None
    for seeds, kw in SWEEPS:
        for seed in seeds:
            rng = random.Random(9000 + seed)
            for i in range(25):
                assert_fast_is_literal(random_case(rng, **kw), f"seed {seed} case {i}")
    for seed, count in ((4711, 12), (77, 6)):
        rng = random.Random(seed)
        for i in range(count):
            assert_fast_is_literal(random_case(rng), f"rng {seed} case {i}")
    for case in (bubbles_with_extras(2, 1, 0), bubbles_with_extras(6, 3, 2), multi_arm_case(50, 12, spare=1400), chain_case(24), chain_case(8, low=2)):
        assert_fast_is_literal(case, "launch counts")


def literal_rows(batch):
    return [name for name, case in boundary_cases(batch).items() if case["n"] <= LITERAL_MAX]


ROW_GROUPS = ("chain", "hub", "tile: n =", "tile: n_out", "tile: nl", "tile: ne", "tile: one", "dense", "other")


@pytest.mark.parametrize("group", ROW_GROUPS)
def test_fast_model_equals_the_literal_model_on_the_boundary_table(emu, group):
    """every row at or below LITERAL_MAX unitigs (the rows above it are the candidate tiles, the wide keys and the multi-arm bubbles, whose
    shape at 50 bubbles is among the existing cases' test); in groups, since the literal model takes seconds per tile row"""
    batch = rounds_per_batch(emu)
    names = [n for n in literal_rows(batch) if n.startswith(group) or (group == "other" and not n.startswith(ROW_GROUPS[:-1]))]
    assert names, group
    for name in names:
        case = boundary_cases(batch)[name]
        model, _ = boundary_expected(batch, name)
        assert_fast_is_literal(case, name, literal=None if "expect" in case else model)


def test_every_row_is_in_a_group_or_above_the_literal_model(emu):
    batch = rounds_per_batch(emu)
    above = [n for n, c in boundary_cases(batch).items() if c["n"] > LITERAL_MAX]
    assert all(n.startswith(("tile: candidates", "wide keys", "multi-arm")) for n in above), above
    assert len(literal_rows(batch)) + len(above) == len(boundary_cases(batch)) and len(above) == 6 + 2 + 2


# ---- the random sweep --------------------------------------------------------------------------------------------------------------------------------
def random_case(rng, max_unitigs=40, link_factor=2.0):
    n = rng.randint(1, max_unitigs)
    links = []
    for _ in range(rng.randint(0, int(link_factor * n))):
        a, b = rng.randint(1, n) * rng.choice((1, -1)), rng.randint(1, n) * rng.choice((1, -1))
        if rng.random() < 0.08:
            b = a if rng.random() < 0.5 else -a      # loops and hairpins
        links.append((a, b))
    threshold = rng.choice((1.0, 2.5))
    depths = [rng.choice((0.0, 0.5, threshold, threshold, threshold + 0.5, 7.0, 20.0)) for _ in range(n)]
    alive = [int(rng.random() < 0.85) for _ in range(n)] if rng.random() < 0.4 else None
    case = make_case(n, links, depths=depths, lens=[rng.randint(1, 9) for _ in range(n)], types=[rng.choice((0, 0, 1, 2, 3)) for _ in range(n)] if rng.random() < 0.5 else None,
                     alive=alive, min_depth=threshold if rng.random() < 0.75 else None)
    live = [u for u in range(1, n + 1) if alive is None or alive[u - 1]]
    if live and rng.random() < 0.6:
        case["remove"] = sorted(rng.sample(live, rng.randint(1, min(3, len(live)))))
    # duplicate what can be duplicated, judged on the graph after the removal (a number that cannot is an error: the error list has those)
    graph = M.MergeGraph(n, case["links"], [int(u in live and u not in case["remove"]) for u in range(1, n + 1)], case["seqs"], case["lens"], case["depths"], None)
    able = [u.number for u in graph.unitigs if len([l for l in u.forward_next + u.reverse_next if l[0] != u.number]) == 2]
    if able and rng.random() < 0.7:
        picked = []
        for u in sorted(rng.sample(able, rng.randint(1, min(3, len(able))))):
            trial = dict(case, duplicate=picked + [u], min_depth=None)
            try:
                run_model(trial)
                picked.append(u)
            except CU.CleanError:      # (an earlier duplication changed this one's links)
                pass
        case["duplicate"] = picked
    return case


def check_sweep(lib_path, seeds, per_seed=25, device=0, **kw):
    met = dict(multiset=0, removed=0, duplicated=0, low=0, dead_end=0, rounds_above_one=0)
    for seed in seeds:
        rng = random.Random(9000 + seed)
        for i in range(per_seed):
            case = random_case(rng, **kw)
            exp, sm = check_case(case, lib_path, device, f"seed {seed} case {i}")
            met["multiset"] |= CU.is_multiset(exp); met["removed"] |= sm["removed"] > 0; met["duplicated"] |= sm["duplicated"] > 0
            met["low"] |= sm["low_depth"] > 0; met["dead_end"] |= sm["kept_dead_end"] > 0; met["rounds_above_one"] |= sm["rounds"] > 1
    return met


SWEEPS = [((0, 1, 2, 3, 4, 5), {}), ((6, 7, 8, 9, 10, 11), dict(max_unitigs=16, link_factor=1.2)),
          ((12, 13, 14, 15, 16, 17), dict(max_unitigs=40, link_factor=0.9)), ((18, 19, 20, 21, 22, 23), dict(max_unitigs=8, link_factor=2.0))]


@pytest.mark.parametrize("seeds,kw", SWEEPS)
def test_sweep(emu, seeds, kw):
    met = check_sweep(emu, seeds, **kw)
    assert met["removed"] and met["duplicated"] and met["low"] and met["dead_end"] and met["rounds_above_one"], met


def test_sweep_is_order_free(emu, monkeypatch):
    """the emulation visits the logical threads descending and shuffled: the products are the same bytes"""
    rng = random.Random(4711)
    cases = [random_case(rng) for _ in range(12)] + beyond_a_wavefront(rounds_per_batch(emu))
    want = []
    for case in cases:
        cl = run_library(case, emu)
        want.append(CU.cleaned_bytes(cl))
    for order in ("1", "2"):
        monkeypatch.setenv("AC_EMU_ORDER", order)
        for case, w in zip(cases, want):
            assert CU.cleaned_bytes(run_library(case, emu)) == w


# ---- the handle, the text entry and the command ------------------------------------------------------------------------------------------------------
def chain_final_text():
    """a 5_final-like text: coloured segments, a bubble with a low arm, a shared tig, a tail of low unitigs"""
    case = make_case(9, [(1, 2), (1, 3), (2, 4), (3, 4), (4, 6), (6, 7), (8, 5), (5, 9), (9, 8)], depths=[6.0, 0.4, 5.0, 6.0, 12.0, 6.0, 0.2, 6.0, 6.0],
                     types=[2, 0, 0, 1, 3, 2, 0, 0, 0], lens=[9, 3, 4, 8, 7, 6, 2, 5, 5])
    unitigs = [(u + 1, u + 1, case["seqs"][u], case["depths"][u], case["types"][u]) for u in range(case["n"])]
    return F.save_gfa(dict(unitigs=unitigs, links=case["links"]), 51, (), True)


def check_handle_form(lib_path, device=0, cli=None):
    text = chain_final_text()
    lib = _capi.load_library(lib_path)
    for options in (dict(min_depth=1.0), dict(remove="2, 7"), dict(duplicate="5"), dict(remove="7", duplicate="5", min_depth=0.5), dict()):
        want = CU.clean_text_model(text, options.get("remove"), options.get("duplicate"), options.get("min_depth"))
        assert b"KM:i:51" in want and b"CL:Z:" in want
        assert clean_gfa(text, device=device, lib_path=lib_path, **options) == want, options
        g, _, _ = graph_from_gfa(text, lib_path)
        cl = g.clean(unitig_type=gfa_segment_types(text, lib_path), device=device, **options)
        plan = cl.merge_plan(device=device)
        fin = cl.finish(plan, renumber=True, device=device)
        assert fin.gfa(51, use_other_colour=True) == want, options
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = Path(tmp) / "in.gfa", Path(tmp) / "out.gfa"
            src.write_bytes(text)
            enc = lambda v: None if v is None else v.encode()
            rc = lib.ac_clean(str(src).encode(), str(dst).encode(), enc(options.get("remove")), enc(options.get("duplicate")), int("min_depth" in options),
                              float(options.get("min_depth", 0.0)), device)
            assert rc == 0, lib.ac_last_error()
            assert dst.read_bytes() == want, options
            assert lib.ac_clean(str(src).encode(), str(dst).encode(), b"77", None, 0, 0.0, device) == 1
            assert lib.ac_last_error().decode() == f"{src} does not contain tig 77"
            if cli is not None:
                args = [str(cli), "clean", "-i", str(src), "-o", str(Path(tmp) / "cli.gfa")]
                for flag, key in (("-r", "remove"), ("-d", "duplicate"), ("-m", "min_depth")):
                    if key in options:
                        args += [flag, str(options[key])]
                done = subprocess.run(args, capture_output=True, timeout=120)
                assert done.returncode == 0, done.stderr
                assert (Path(tmp) / "cli.gfa").read_bytes() == want, options
    # a text without KM:i prints KM:i:0, as combine writes it
    bare = text.replace(b"\tKM:i:51", b"")
    assert clean_gfa(bare, min_depth=1.0, device=device, lib_path=lib_path) == CU.clean_text_model(bare, None, None, 1.0)
    assert clean_gfa(bare, min_depth=1.0, device=device, lib_path=lib_path).startswith(b"H\tVN:Z:1.0\tKM:i:0\n")
    assert gfa_segment_types(text, lib_path).tolist() == [2, 0, 0, 1, 3, 2, 0, 0, 0]
    return True


def test_handle_text_and_command_give_the_same_bytes(emu):
    assert check_handle_form(emu)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, device=0):
    base = dict(n=5, links=CU.l_line_order(M.closed_set([(1, 2), (2, 3), (3, 4), (3, 5)])), lens=[3] * 5, depths=[4.0] * 5, types=None, alive=[1, 1, 1, 1, 0], seqs=None,
                remove=[], duplicate=[], min_depth=None)

    def fails(message, **kw):
        case = dict(base, **kw)
        with pytest.raises(AutocyclerError) as e:
            run_library(case, lib_path, device, sequences=False)
        assert str(e.value) == message, (str(e.value), message)
        if "links" not in kw:      # the model says the same
            with pytest.raises(CU.CleanError) as m:
                run_model(case)
            assert str(m.value) == message

    fails("the graph does not contain tig 9", remove=[9])
    fails("the graph does not contain tig 0", remove=[0])
    fails("the graph does not contain tig 5", remove=[5])              # not alive at entry
    fails("the graph does not contain tig 6", duplicate=[6])           # a copy's number cannot be asked for
    fails("the graph does not contain tig 7", remove=[1], duplicate=[2, 7])
    fails("unitig 1 does not contain exactly two non-self links", duplicate=[1])
    fails("unitig 3 does not contain exactly two non-self links", duplicate=[3], alive=None)
    fails("unitig 2 no longer exists: it was removed or duplicated earlier in the same call", remove=[2], duplicate=[2])
    fails("unitig 2 no longer exists: it was removed or duplicated earlier in the same call", duplicate=[2, 2])
    fails("unitig 3 does not contain exactly two non-self links", remove=[4], duplicate=[3])      # judged after the removal: one link is left
    for text in ("", "ABC", "1,X,3", "1,,2", "-1", "4294967296", "1;2"):
        with pytest.raises(AutocyclerError) as e:
            parse_tig_numbers(text, lib_path)
        with pytest.raises(CU.CleanError) as m:
            CU.parse_tig_numbers(text)
        assert str(e.value) == str(m.value) and "as a node number" in str(e.value)
        with pytest.raises(AutocyclerError, match="as a node number"):
            clean_gfa(chain_final_text(), remove=text, device=device, lib_path=lib_path)
    assert parse_tig_numbers("+3, 1", lib_path) == [1, 3] == CU.parse_tig_numbers("+3, 1")
    # the links: a set closed under reverse complement, in L-line order, naming unitigs — the first offender is quoted
    closed = base["links"]
    fails("link 1 (1 -> 2) is a duplicate: the merge plan needs the links among alive unitigs as a set", links=[closed[0]] + closed)
    fails("link 0 (1 -> 2) has no reverse complement (-2 -> -1): the merge plan needs a link set that is closed under reverse complement",
          links=[l for l in closed if l != (-2, -1)])
    swapped = [closed[1], closed[0]] + closed[2:]
    with pytest.raises(AutocyclerError, match=r"clean: link entry 1 \(.*\) stands behind an entry that leaves .*: the links must be in L-line order"):
        run_library(dict(base, links=swapped), lib_path, device, sequences=False)
    with pytest.raises(AutocyclerError, match=r"link 0 \(1 -> 9\) names no unitig"):
        run_library(dict(base, links=[(1, 9), (-9, -1)]), lib_path, device, sequences=False)
    with pytest.raises(AutocyclerError, match="both or neither"):
        lib = _capi.load_library(lib_path)
        ln = (ctypes.c_uint32 * 1)(3)
        h = ctypes.c_void_p()
        _capi._check(lib, lib.ac_clean_graph(1, None, 0, ln, None, None, None, ln, None, None, 0, None, 0, 0, 0.0, device, ctypes.byref(h)))
    return True


def test_errors(emu):
    assert check_errors(emu)


# ---- two runs, and what the launches follow -----------------------------------------------------------------------------------------------------------
def beyond_a_wavefront(batch):
    """two rows in which the work list is compacted by many wavefronts, whose atomics the device orders anew in every run: a random graph of
    2049 unitigs and the multi-arm bubbles across a batch edge"""
    rows = boundary_cases(batch)
    return [rows["tile: n = 2049"], rows[f"multi-arm bubbles: 300 of {2 * batch + 1} low arms"]]


def check_two_runs_identical(lib_path, device=0, more=()):
    rng = random.Random(77)
    for case in [random_case(rng) for _ in range(6)] + [hub_case(65), chain_case(11)] + beyond_a_wavefront(rounds_per_batch(lib_path, device)) + list(more):
        a, b = run_library(case, lib_path, device), run_library(case, lib_path, device)
        assert CU.cleaned_bytes(a) == CU.cleaned_bytes(b)
        assert (a.summary["launches"], a.summary["read_backs"]) == (b.summary["launches"], b.summary["read_backs"])
    return True


def test_two_runs_give_identical_products(emu):
    assert check_two_runs_identical(emu)


def bubbles_with_extras(bubbles, tails, dups):
    """`bubbles` bubbles with a low arm each (one round), plus `tails` removable tails and `dups` duplicable tigs: sizes and option counts differ,
    the rounds do not"""
    case = candidates_case(bubbles)
    n, links, depths = case["n"], [], list(case["depths"])
    remove, duplicate = [], []
    for _ in range(tails):
        links.append((n, n + 1)); depths.append(5.0); remove.append(n + 1); n += 1
    for _ in range(dups):
        links += [(n + 1, n + 2), (n + 2, n + 3)]; depths += [5.0, 8.0, 5.0]; duplicate.append(n + 2); n += 3
    base = [l for l in case["links"] if l[0] > 0 and abs(l[1]) > abs(l[0])]
    return make_case(n, base + links, depths=depths, remove=remove, duplicate=duplicate, min_depth=1.0)


def check_launch_counts(lib_path, device=0):
    batch = rounds_per_batch(lib_path, device)
    # different sizes (inside one radix digit: the sorts' passes follow the key width), different numbers of removals and duplications, one round each
    small, large = bubbles_with_extras(2, 1, 0), bubbles_with_extras(6, 3, 2)
    (_, a), (_, b) = check_case(small, lib_path, device, "small"), check_case(large, lib_path, device, "large")
    assert a["rounds"] == b["rounds"] == 1 and a["unitigs_in"] < b["unitigs_in"] and a["removed"] < b["removed"] and a["duplicated"] < b["duplicated"]
    assert a["launches"] == b["launches"], (a, b)
    # chains of R, 2R and 3R rounds: the same step each time; the read-backs follow the batches, not the rounds
    runs = [check_case(chain_case(m * batch), lib_path, device, f"chain {m}")[1] for m in (1, 2, 3)]
    assert [r["rounds"] for r in runs] == [batch, 2 * batch, 3 * batch]
    assert runs[1]["launches"] - runs[0]["launches"] == runs[2]["launches"] - runs[1]["launches"] > 0, runs
    assert runs[1]["read_backs"] - runs[0]["read_backs"] == runs[2]["read_backs"] - runs[1]["read_backs"] == 1, runs
    # bubbles of 12 arms, 50 and 300 of them: 12 rounds each, one workgroup and several — the same launches and read-backs
    few_bubbles, many_bubbles = multi_arm_case(50, 12, spare=1400), multi_arm_case(300, 12)
    a, b = check_case(few_bubbles, lib_path, device, "50 bubbles of 12 arms")[1], check_case(many_bubbles, lib_path, device, "300 bubbles", exp=run_model_fast(many_bubbles))[1]
    assert a["rounds"] == b["rounds"] == 12 and a["low_depth"] == 600 and b["low_depth"] == 3600
    for bits in (lambda n: 2 * bit_width(2 * n), lambda n: bit_width(2 * n - 1)):      # (the sorts' passes follow the key widths: the spare unitigs keep both inside one digit)
        assert (bits(few_bubbles["n"]) + 7) // 8 == (bits(many_bubbles["n"]) + 7) // 8
    assert (a["launches"], a["read_backs"]) == (b["launches"], b["read_backs"]), (a, b)
    # within one batch the read-backs do not move at all
    few, more = check_case(chain_case(batch, low=2), lib_path, device, "2 rounds")[1], check_case(chain_case(batch), lib_path, device, "a batch of rounds")[1]
    assert few["rounds"] < more["rounds"] and few["read_backs"] == more["read_backs"] and few["launches"] == more["launches"], (few, more)
    return True


def test_launches_follow_the_rounds_alone(emu):
    assert check_launch_counts(emu)
