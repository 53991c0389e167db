"""ac_apply_bridges / ac_graph_resolve_apply, the Applied object, the composed entries and ac_resolve_graphs on the CPU emulation of the shipped
kernels (kernels_apply.inc) against the literal Python model of apply_util.py: the sequential loop over the bridges with its list edits,
one depth visit at a time, the components by the model's own search, the removals, then merge_util, finish_util.finish_model and
finish_util.save_gfa for the texts.  Every comparison is equality (depths bit for bit).  The same checks run on the device in
test_apply_gpu.py."""
import math
import random

import numpy as np
import pytest

import apply_util as A
import emu_lib
import finish_util as F
import merge_util as M
import parity_util
from autocycler_amd import Applied, AutocyclerError, apply_bridges, components_from_links, graph_from_gfa, resolve_bridge_paths
from autocycler_amd import _capi
from test_resolve_emu import variant_assemblies

NEW_SYMBOLS = ("ac_apply_bridges", "ac_graph_resolve_apply", "ac_applied_unitigs", "ac_applied_bridge_of", "ac_applied_links", "ac_applied_bridge_sequences",
               "ac_applied_summary_get_sized", "ac_applied_free", "ac_applied_merge_plan", "ac_applied_finish", "ac_applied_gfa_string", "ac_resolve_graphs")
K = 7      # the k-mer size the texts are printed with (the H line only)


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


def check_exports(lib_path):
    lib = _capi.load_library(lib_path)
    assert lib.ac_abi_version() == 13
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS and getattr(lib, name)
    return True


def test_abi_is_13_and_exports_apply(emu):
    """without the feature this fails outright: the library has none of these symbols"""
    assert check_exports(emu)


# ---- cases on plain arrays ---------------------------------------------------------------------------------------------------------------------
def bridge(start, end, best, distinct=None, conflicting=0, culled=0):
    """a bridge as resolve_bridge_paths returns it; distinct defaults to the best path once"""
    return dict(start=start, end=end, status=0, best_path=list(best), distinct_paths=[(list(p), c) for p, c in (distinct if distinct is not None else [(best, 1)])],
                conflicting=conflicting, culled=culled)


def seq_of(u, length):
    return bytes(b"ACGT"[(u * 7 + i * (u % 3 + 1) + i // 4) & 3] for i in range(length))


def make_case(n, links, anchors, bridges, lens=None, depths=None, alive=None, applied=None, bridge_depth=3.0, closed=True):
    lens = list(lens) if lens is not None else [(u % 5) + 1 for u in range(1, n + 1)]
    return dict(n=n, links=M.closed_set(links) if closed else list(links), lens=lens, anchors=list(anchors), bridges=bridges,
                applied=list(applied) if applied is not None else [not b["conflicting"] for b in bridges], bridge_depth=bridge_depth, alive=alive,
                depths=list(depths) if depths is not None else [4.0] * n, seqs=[seq_of(u, l) for u, l in enumerate(lens, 1)])


def run_library(case, lib_path, device=0, sequences=True):
    return apply_bridges(case["n"], case["links"], case["lens"], case["anchors"], case["bridges"], case["applied"], case["bridge_depth"], alive=case["alive"],
                         depth=case["depths"], sequences=case["seqs"] if sequences else None, device=device, lib_path=lib_path)


def check_case(case, lib_path, device=0, what="", texts=True):
    """one graph: the arrays, 3_bridged's text and the merged graph's text against the model -> (coverage, the Applied's summary)"""
    exp, met = A.apply_model(case["n"], case["links"], case["lens"], case["anchors"], case["bridges"], case["applied"], case["bridge_depth"], case["alive"],
                             case["depths"], case["seqs"])
    ap = run_library(case, lib_path, device)
    assert isinstance(ap, Applied) and ap.n_unitigs == case["n"]
    A.assert_same(ap, exp, what)
    sm = ap.summary
    assert sm["links_in"] == len(case["links"]) and sm["bridges_applied"] == sum(bool(x) for x in case["applied"])
    assert sm["removed_no_anchor"] + sm["removed_zero_depth"] == sum(1 for u in range(exp["n_total"]) if not exp["alive"][u] and (u >= case["n"] or case["alive"] is None or case["alive"][u])), what
    if texts:
        for colour in (False, True):
            assert ap.gfa(K, use_other_colour=colour) == A.bridged_text(exp, K, colour), (what, "bridged text")
        if not any(math.isnan(d) and a for d, a in zip(exp["depth"], exp["alive"])):
            exp_merged, members, _ = A.merged_model(exp)
            met["merged_chain"] = int(bool(members))
            plan = ap.merge_plan(device=device)
            assert plan.chain_members() == members, (what, "chains")
            fin = ap.finish(plan, renumber=True, device=device)
            F.assert_model_same(F.library_model(fin, False), exp_merged, f"{what} merged")
            assert fin.gfa(K) == F.save_gfa(exp_merged, K), (what, "merged text")
            fin.close(); plan.close()
    ap.close()
    return met, sm


def ring_links(order):
    return [(a, b) for a, b in zip(order, order[1:] + order[:1])]


def named_cases():
    """the hand-built cases of the issue, as small as they come: {name: case}"""
    c = {}
    # two anchors on a circle, two ways from 1 to 2 (3 twice, 4 once), straight back from 2 to 1
    two = [(1, 3), (3, 2), (1, 4), (4, 2), (2, 1)]
    c["bridge unitig and direct link"] = make_case(4, two, [1, 2], [bridge(1, 2, [3], [([3], 2), ([4], 1)]), bridge(2, 1, [], [([], 3)])])
    # an empty best path while other paths are not empty: no depth is reduced
    c["empty best path, other paths not empty"] = make_case(5, two + [(2, 5), (5, 1)], [1, 2], [bridge(1, 2, [3], [([3], 2), ([4], 1)]), bridge(2, 1, [], [([], 2), ([5], 1)])],
                                                            depths=[3.0, 3.0, 2.0, 1.0, 1.0])
    c["start == end, non-empty best path"] = make_case(2, [(1, 2), (2, 1)], [1], [bridge(1, 1, [2])], depths=[2.0, 2.0])
    c["start == end, empty best path"] = make_case(2, [(1, 1), (1, 2), (2, 1)], [1], [bridge(1, 1, [], [([], 2), ([2], 1)])], depths=[3.0, 1.0])
    # start == -end: determine_ambiguity counts its start twice, so it conflicts with itself and cull_ambiguity removes it
    hairpin = [(1, 2), (2, -1)]
    c["start == -end is skipped"] = make_case(2, hairpin, [1], [bridge(1, -1, [2], conflicting=1, culled=1)])
    c["start == -end applied, best path"] = make_case(2, hairpin, [1], [bridge(1, -1, [2], conflicting=1, culled=1)], applied=[True])
    c["start == -end applied, direct"] = make_case(2, hairpin + [(1, -1)], [1], [bridge(1, -1, [], [([], 1), ([2], 1)], conflicting=1, culled=1)], applied=[True])
    # visits above, equal to and below a depth: 3 x3, 4 x2, 5 x3, 6 x3, 7 x2, 8 x2
    paths = [([3, 4, 5, 6, 7, 8], 2), ([3, 5, 6], 1)]
    chain = [(1, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 2), (3, 5), (6, 2), (2, 1)]
    c["visits and depths"] = make_case(8, chain, [1, 2], [bridge(1, 2, [3, 4, 5, 6, 7, 8], paths), bridge(2, 1, [])],
                                       depths=[3.0, 3.0, 2.5, 2.5, 3.0, float("nan"), 5.0, 2.0 ** 53 + 2.0])
    c["visits and depths, odd cases"] = make_case(8, chain, [1, 2], [bridge(1, 2, [3, 4, 5, 6, 7, 8], paths), bridge(2, 1, [])],
                                                  depths=[3.0, 3.0, -2.0, -0.0, float("inf"), 2.0 ** 53, 2.0 ** 54, 2.0 ** 53 + 4.0])
    # unitig 2 (depth 0) alone ties 3 to the anchor: 3 survives, 2 does not; 4 - 5 hold no anchor
    c["zero depth tie and anchorless component"] = make_case(5, [(1, 2), (2, 3), (4, 5)], [1], [], depths=[2.0, 0.0, 4.0, 4.0, 4.0])
    # the same with a bridge: anchor 1's other side still holds 2 - 3 (the bridge 1 -> 6 strips 1's forward side only)
    c["zero depth tie beside a bridge"] = make_case(7, [(2, 1), (3, 2), (1, 7), (7, 6), (6, 3)], [1, 6], [bridge(1, 6, [7])], depths=[2.0, 0.0, 4.0, 4.0, 4.0, 3.0, 1.0])
    # members on the reverse strand, one without bases
    c["reverse members and an empty member"] = make_case(5, [(1, -3), (-3, 4), (4, -5), (-5, 2), (2, 1)], [1, 2], [bridge(1, 2, [-3, 4, -5]), bridge(2, 1, [])], lens=[3, 2, 5, 0, 17])
    c["no bridge applied"] = make_case(4, two, [1, 2], [bridge(1, 2, [3]), bridge(2, 1, [])], applied=[False, False])
    c["no anchors at all"] = make_case(3, [(1, 2), (2, 3)], [], [])
    c["dead unitigs at entry"] = make_case(6, two + [(4, 5), (5, 6)], [1, 2], [bridge(1, 2, [3]), bridge(2, 1, [])], alive=[1, 1, 1, 1, 0, 1])
    return c


def check_named_cases(lib_path, device=0):
    met = dict.fromkeys(A.COVERAGE, 0)
    for name, case in named_cases().items():
        got, _ = check_case(case, lib_path, device, name)
        for k in got:
            met[k] |= got[k]
    for flag in ("bridge_unitig", "direct_link", "skipped_bridge", "reverse_member", "depth_clamped", "depth_reduced_above_zero", "anchorless_removed", "zero_depth_removed",
                 "zero_depth_was_tie", "dangling_link_removed", "nothing_applied"):
        assert met[flag], flag
    # n_unitigs == 0: an empty result, the texts are the header line alone
    ap = apply_bridges(0, [], [], [], [], [], 1.0, device=device, lib_path=lib_path)
    assert ap.n_total == 0 and len(ap.links) == 0 and ap.gfa(K) == f"H\tVN:Z:1.0\tKM:i:{K}\n".encode()
    none = make_case(3, [(1, 2), (2, 3)], [], [])
    ap = run_library(none, lib_path, device)
    assert ap.alive.tolist() == [0, 0, 0] and ap.summary["removed_no_anchor"] == 3 and ap.gfa(K) == f"H\tVN:Z:1.0\tKM:i:{K}\n".encode()
    plan = ap.merge_plan(device=device)
    assert ap.finish(plan, device=device).gfa(K) == f"H\tVN:Z:1.0\tKM:i:{K}\n".encode()
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


def test_culling_makes_kept_differ_from_unique(emu):
    assert check_culling_case(emu)


def check_culling_case(lib_path, device=0):
    """three sequences go 1 -> 2 -> 3, one goes 1 -> 3 -> 2: every bridge conflicts, the single-copy ones are culled, and the final
    pass applies what the first one could not"""
    paths = [[1, 4, 2, 5, 3, 6]] * 3 + [[1, 7, 3, 8, 2, 9]]
    case = dict(n=9, links=A.links_of_paths(paths), lens=[5, 4, 3, 2, 1, 2, 3, 4, 5], depths=[4.0, 4.0, 4.0, 3.0, 3.0, 3.0, 1.0, 1.0, 1.0], paths=paths, cw=[1, 1, 1, 1])
    case["seqs"] = [seq_of(u, l) for u, l in enumerate(case["lens"], 1)]
    met = check_resolve_arrays(case, lib_path, device, "culling")
    assert met["culled"] and met["passes_differ"] and met["nothing_applied"]
    return True


# ---- the two-pass flow on arrays: resolve_bridge_paths, then apply ---------------------------------------------------------------------------------
def check_resolve_arrays(case, lib_path, device=0, what=""):
    """both passes of resolve.rs:44-67 through resolve_bridge_paths and apply_bridges: the arrays, the three texts and the cull count"""
    exp, met = A.resolve_model(case["n"], case["links"], case["lens"], case["depths"], case["seqs"], case["paths"], case["cw"], K)
    anchors, bridges, _ = resolve_bridge_paths(case["paths"], case["lens"], case["cw"], device=device, lib_path=lib_path)
    assert list(anchors) == exp["anchors"], what
    assert sum(b["culled"] for b in bridges) == exp["cull_count"], what
    texts = {}
    for which in ("unique", "kept"):
        ap = apply_bridges(case["n"], case["links"], case["lens"], anchors, bridges, which, float(len(case["paths"])), depth=case["depths"], sequences=case["seqs"],
                           device=device, lib_path=lib_path)
        A.assert_same(ap, exp[which], f"{what} {which}")
        if which == "unique":
            texts["bridged"] = ap.gfa(K)
        plan = ap.merge_plan(device=device)
        fin = ap.finish(plan, renumber=True, device=device)
        if which == "unique":
            texts["merged"] = fin.gfa(K, use_other_colour=False)
        if which == "kept" or exp["cull_count"] == 0:
            texts["final"] = fin.gfa(K, use_other_colour=True)
        fin.close(); plan.close(); ap.close()
    for name in ("bridged", "merged", "final"):
        assert texts[name] == exp[name], (what, name)
    return met


SWEEP_SEEDS = tuple(range(60))
SWEEP_MUST_MEET = A.COVERAGE


def check_sweep(lib_path, seeds, device=0, must_meet=()):
    met = dict.fromkeys(A.COVERAGE, 0)
    for seed in seeds:
        got = check_resolve_arrays(A.random_case(random.Random(9000 + seed)), lib_path, device, f"seed {seed}")
        for k in got:
            met[k] |= got[k]
    for flag in must_meet:
        assert met[flag], f"the sweep never met {flag}"
    return met


def test_random_sweep_meets_every_coverage_flag(emu):
    check_sweep(emu, SWEEP_SEEDS, must_meet=SWEEP_MUST_MEET)


# ---- the boundary table ------------------------------------------------------------------------------------------------------------------------
BRIDGE_BYTES = (1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 8193)
TILE_SIZES = (65, 257, 2049, 4097)


def members_for(length):
    """a best path of `length` bases from unitigs of 17 (number 1), 16 (2) and 1 (3) bases, strands alternating"""
    out, left, sign = [], length, 1
    while left:
        u = 1 if left >= 17 and (left - 17) != 15 else 2 if left >= 16 else 3
        out.append(sign * u); sign = -sign
        left -= (17, 16, 1)[u - 1]
    return out


def bridge_length_case():
    """a ring of anchors 4 .. 13, the bridge from the i-th to the next with a best path of BRIDGE_BYTES[i] bases"""
    na = len(BRIDGE_BYTES)
    anchors = list(range(4, 4 + na))
    bridges = [bridge(a, b, members_for(L)) for (a, b), L in zip(ring_links(anchors), BRIDGE_BYTES)]
    bridges.sort(key=lambda b: (abs(b["start"]), -b["start"], abs(b["end"]), -b["end"]))
    return make_case(3 + na, ring_links(anchors) + [(4, 1), (1, 2), (2, 3), (3, 5)], anchors, bridges, lens=[17, 16, 1] + [2] * na, depths=[1e6] * (3 + na))


def ring_case(n, every=8, applied=None):
    """a ring of n unitigs, every `every`-th one an anchor, a bridge from each anchor to the next over the unitigs between them (one copy
    takes a short cut past the first of them), a chord per anchor"""
    order = list(range(1, n + 1))
    anchors = order[::every]
    links = ring_links(order)
    bridges = []
    for a, b in zip(anchors, anchors[1:] + anchors[:1]):
        between = list(range(a + 1, b)) if b > a else list(range(a + 1, n + 1))
        bridges.append(bridge(a, b, between, [(between, 2), (between[1:], 1)]))
        if len(between) > 1:
            links.append((a, between[1]))
    bridges.sort(key=lambda b: (abs(b["start"]), -b["start"], abs(b["end"]), -b["end"]))
    lens = [(u % 3) + 1 for u in order]
    return make_case(n, links, anchors, bridges, lens=lens, depths=[3.0 if u % 5 else 2.0 for u in order], applied=applied)


def hub_case(n_bridges=300):
    """a ring of anchors whose bridges all run through one unitig (n + 1, depth 250.5: clamped) and then another (n + 2, depth 1000)"""
    anchors = list(range(1, n_bridges + 1))
    hub, hub2 = n_bridges + 1, n_bridges + 2
    bridges = [bridge(a, b, [hub, hub2]) for a, b in ring_links(anchors)]
    bridges.sort(key=lambda b: (abs(b["start"]), -b["start"], abs(b["end"]), -b["end"]))
    links = [l for a in anchors for l in ((a, hub), (hub2, a))] + [(hub, hub2)]
    return make_case(n_bridges + 2, links, anchors, bridges, depths=[2.0] * n_bridges + [250.5, 1000.0])


def check_boundary_table(lib_path, device=0, sizes=TILE_SIZES):
    assert [sum((17, 16, 1)[abs(e) - 1] for e in members_for(L)) for L in BRIDGE_BYTES] == list(BRIDGE_BYTES)
    case = bridge_length_case()
    exp, _ = A.apply_model(case["n"], case["links"], case["lens"], case["anchors"], case["bridges"], case["applied"], case["bridge_depth"], None, case["depths"], case["seqs"])
    assert sorted(len(s) for s in exp["bridge_seqs"]) == sorted(BRIDGE_BYTES)
    check_case(case, lib_path, device, "bridge lengths")
    for n in sizes:
        _, sm = check_case(ring_case(n), lib_path, device, f"ring of {n}", texts=n <= 257)
        assert sm["links_out"] > 0
    met, sm = check_case(hub_case(), lib_path, device, "hub")
    assert met["depth_clamped"] and met["depth_reduced_above_zero"] and sm["bridges_applied"] == 300
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


# ---- a graph handle: built, written, reloaded --------------------------------------------------------------------------------------------------
def handle_case(g):
    """a Graph's arrays as apply_util takes them"""
    n = g.unitig_count
    units = [g.unitig(i) for i in range(n)]
    links = [(a if af else -a, b if bf else -b) for a, af, b, bf in g.links()]
    return dict(n=n, links=links, lens=[len(s) for s, _ in units], depths=[d for _, d in units], seqs=[s for s, _ in units],
                paths=[list(g.path(s)) for s in range(g.n_seqs)], cw=[1] * g.n_seqs)


def check_graph(lib_path, seed, k, device=0):
    seqs, fn, hd = variant_assemblies(seed, k)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)      # what `autocycler resolve` itself starts from: 2_trimmed.gfa
    case = handle_case(g2)
    exp, met = A.resolve_model(case["n"], case["links"], case["lens"], case["depths"], case["seqs"], case["paths"], case["cw"], k)
    assert met["bridge_unitig"] and exp["anchors"]
    for graph in (g, g2):
        bridged, merged, final, culled = graph.resolve_graphs(device=device)
        assert culled == exp["cull_count"]
        assert bridged == exp["bridged"] and merged == exp["merged"] and final == exp["final"]
    for which in ("unique", "kept"):
        ap = g2.resolve_apply(which, device=device)
        A.assert_same(ap, exp[which], f"handle {which}")
        ap.close()
    return True


@pytest.mark.parametrize("seed,k", [(3, 11), (8, 21)])
def test_graph_built_and_reloaded(emu, seed, k):
    assert check_graph(emu, seed, k)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, device=0):
    """every error of the header returns 1 with a message that names the offender; a valid call right after it succeeds"""
    base = named_cases()["bridge unitig and direct link"]

    def fails(match, **changes):
        case = dict(base, **changes)
        with pytest.raises(AutocyclerError, match=match):
            run_library(case, lib_path, device)
        got, _ = check_case(base, lib_path, device, "after an error", texts=False)
        assert got["bridge_unitig"]
    b0, b1 = base["bridges"]
    fails(r"bridge 0 \(1 -> 2\) has status 2", bridges=[dict(b0, status=2, best_path=None), b1])
    fails(r"conflict: bridge 0 \(1 -> 2\) and bridge 1 \(1 -> 2\)", bridges=[b0, dict(b0)], applied=[True, True])
    fails(r"conflict: bridge 0 \(1 -> 2\) and bridge 1 \(-2 -> 1\)", bridges=[b0, dict(b1, start=-2)], applied=[True, True])
    fails(r"the start of bridge 0 \(0 -> 2\) is 0", bridges=[dict(b0, start=0), b1])
    fails(r"the end of bridge 0 \(1 -> 9\) is beyond n_unitigs", bridges=[dict(b0, end=9), b1])
    fails(r"the end of bridge 0 \(1 -> 2\) names a unitig that is not alive", alive=[1, 0, 1, 1])
    fails(r"the end of bridge 0 \(1 -> 3\) is not among the anchors", bridges=[dict(b0, end=3), b1])
    fails(r"entry 0 of the best-path pool \(0\), on a path of bridge 0 \(1 -> 2\), is 0", bridges=[dict(b0, best_path=[0]), b1])
    fails(r"entry 0 of the best-path pool \(-7\), on a path of bridge 0 \(1 -> 2\), is beyond n_unitigs", bridges=[dict(b0, best_path=[-7]), b1])
    fails(r"entry 1 of the distinct-path pool \(4\), on a path of bridge 0 \(1 -> 2\), names a unitig that is not alive", alive=[1, 1, 1, 0],
          links=M.closed_set([(1, 3), (3, 2), (2, 1)]))
    fails(r"entry 1 of the distinct-path pool \(12\)", bridges=[dict(b0, distinct_paths=[([3], 2), ([12], 1)]), b1])
    fails(r"link 1 \(1 -> 3\) is a duplicate", links=[base["links"][0]] + base["links"])
    fails(r"link 0 \(1 -> 3\) has no reverse complement", links=[l for l in base["links"] if l != (-3, -1)])
    fails(r"nonexistent unitig", links=base["links"] + [(1, 8), (-8, -1)])
    fails(r"anchors must ascend", anchors=[2, 1])
    lib = _capi.load_library(lib_path)
    C = _capi.C
    one = np.zeros(4, dtype=np.uint64)
    h = C.c_void_p()
    args = [4, None, 0, one.ctypes.data, None, None, None, 0, one.ctypes.data, None, None, 0, None, 0, None, None, None, 0, None, 1.0, device]
    assert lib.ac_apply_bridges(*args, C.byref(h)) == 1 and b"seq_bytes and seq_begin: both or neither" in lib.ac_last_error()
    args[8] = None
    assert lib.ac_apply_bridges(*args, None) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_graph_resolve_apply(None, None, 0, device, C.byref(h)) == 1 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_applied_merge_plan(None, 1, device, C.byref(h)) == 1 and lib.ac_applied_gfa_string(None, K, 0, None, None) == 1
    assert lib.ac_resolve_graphs(None, device, None, None, None, None) == 1 and b"null pointer" in lib.ac_last_error()
    # n_unitigs + bridge unitigs above what a signed number can name: refused before anything is read
    args[0] = 0x7FFFFFFF
    assert lib.ac_apply_bridges(*args, C.byref(h)) == 1 and b"signed unitig number" in lib.ac_last_error()
    check_case(base, lib_path, device, "after the raw calls", texts=False)
    return True


def test_errors(emu):
    assert check_errors(emu)


# ---- determinism, launches -------------------------------------------------------------------------------------------------------------------
def check_two_runs_identical(lib_path, device=0):
    for case in (ring_case(257), bridge_length_case(), hub_case(64)):
        a, b = run_library(case, lib_path, device), run_library(case, lib_path, device)
        assert A.applied_bytes(a) == A.applied_bytes(b)
        assert a.gfa(K) == b.gfa(K)
    return True


def test_two_runs_give_identical_products(emu):
    assert check_two_runs_identical(emu)


def check_launches_do_not_follow_bridges(lib_path, device=0):
    """1 and 500 applied bridges on graphs of the same n_unitigs and n_links: the step's own launches are equal"""
    n = 4000
    many = ring_case(n)
    assert len(many["bridges"]) == 500
    few = ring_case(n, applied=[i == 0 for i in range(500)])
    assert few["n"] == many["n"] and len(few["links"]) == len(many["links"])
    a, b = run_library(few, lib_path, device), run_library(many, lib_path, device)
    assert (a.summary["bridges_applied"], b.summary["bridges_applied"]) == (1, 500)
    assert a.summary["launches"] == b.summary["launches"] > 0
    return True


def test_launches_do_not_follow_the_bridges(emu):
    assert check_launches_do_not_follow_bridges(emu)


def test_launches_and_read_backs_are_the_runtimes_counters(emu):
    """Under the emulation a launch is a kernel and nothing else (fills are memsets), so the counts can be stated from the stage list of
    kernels_apply.inc: phase A marks, check, visits, depths, members, scan, bridge offsets, flags, sort (histogram + one pass for 8 key
    bits), link check, scan, compact, create, copy = 15; phase B alive, keys, sort (2), gather = 5.  Read-backs: header and arrays of either
    phase, and the two of the components step.  The components' own launches are what the same graph costs through ac_components_from_links
    (nothing is removed in this case, so the edited graph is the result)."""
    case = named_cases()["bridge unitig and direct link"]
    ap = run_library(case, emu)
    comp = components_from_links(ap.n_total, ap.links.tolist(), ap.len.tolist(), lib_path=emu)      # (its launches follow n_total and "any link" alone)
    assert ap.summary["launches"] == 20 and ap.summary["read_backs"] == 6
    assert ap.summary["launches_components"] == comp.summary["launches"]
    without = run_library(case, emu, sequences=False)
    assert without.summary["launches"] == 19 and without.summary["seconds_copy"] == 0
    assert ap.summary["seconds_device"] >= ap.summary["seconds_copy"] > 0
