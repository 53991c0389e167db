"""ac_graph_components / ac_components_from_links on the CPU emulation of the shipped kernels (kernels_components.inc; its wave kernels under
the lockstep emulation of wave_rt.hpp) against the reference's own known answers (golden/components_kats.json) and the plain-Python model
(components_util.py).  Every comparison is equality.  The same checks run on the device in test_components_gpu.py."""
import random

import pytest

import components_util as U
import emu_lib
import parity_util
import seqgen
from autocycler_amd import AutocyclerError, Components, components_from_links, graph_components, graph_from_gfa
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = U.load_kats()


def without_links(links, deleted):
    """delete_link (unitig_graph.rs:821-824): the link and its reverse complement, every copy"""
    gone = {tuple(d) for d in deleted} | {U.rc(tuple(d)) for d in deleted}
    return [l for l in links if l not in gone]


# ---- the model reproduces the reference's known answers ------------------------------------------------------------------------------------
def test_model_reproduces_kats():
    graph = lambda name: U.UnitigGraph(*U.gfa_links(name)[:2])
    assert [c["gfa"] for c in KATS["connected_components"]] == [f"test_gfa_{i}.gfa" for i in range(1, 8)]
    for c in KATS["connected_components"]:
        assert graph(c["gfa"]).connected_components() == c["expected"], c["gfa"]
    assert len(KATS["component_is_circular_loop"]) == 13
    for c in KATS["component_is_circular_loop"]:
        assert graph(c["gfa"]).component_is_circular_loop(c["component"]) == c["expected"], c
    for c in KATS["graph_stats"]:
        n, links, lens = U.gfa_links(c["gfa"])
        assert (n, sum(lens), list(U.UnitigGraph(n, links).link_count())) == (c["unitigs"], c["total_length"], c["link_count"]), c["gfa"]
    assert [c["gfa"] for c in KATS["topology"]] == [f"test_gfa_{i}.gfa" for i in range(1, 14)]
    for c in KATS["topology"]:
        assert graph(c["gfa"]).topology() == c["expected"], c["gfa"]
    for key in ("is_isolated_and_circular", "is_isolated_and_linear"):
        for c in KATS[key]:
            assert [u.number for u in graph(c["gfa"]).unitigs if getattr(u, key)()] == c["unitigs_true"], (key, c["gfa"])
    assert len(KATS["edits"]) == 6
    for c in KATS["edits"]:
        n, links, _ = U.gfa_links(c["gfa"])
        alive = [int(u not in c["remove_unitigs"]) for u in range(1, n + 1)]
        assert U.UnitigGraph(n, without_links(links, c["delete_links"]), alive).connected_components() == c["expected"], c


def test_model_walk_equals_the_strand_orbit():
    """Where every link's reverse complement is present, component_is_circular_loop is "all four lists hold one entry, and the strand orbit
    of (first, +) meets every member once — or the component is a single unitig".  A cross-check of the model's literal walk."""
    rng, seen = random.Random(3), [0, 0]
    for _ in range(600):
        n, links, _, alive, _ = U.random_case(rng)
        links = links + sorted({U.rc(l) for l in links} - set(links))
        g = U.UnitigGraph(n, links, alive)
        for comp in g.connected_components():
            ones = all(len(l) == 1 for u in comp for l in (g.unitig_index[u].forward_next, g.unitig_index[u].forward_prev, g.unitig_index[u].reverse_next,
                                                             g.unitig_index[u].reverse_prev))
            orbit = []
            if ones:
                at = (comp[0], True)
                while at not in orbit:
                    orbit.append(at)
                    u = g.unitig_index[at[0]]
                    at = (u.forward_next if at[1] else u.reverse_next)[0]
            short = ones and (len(comp) == 1 or sorted(x for x, _ in orbit) == comp)
            assert g.component_is_circular_loop(comp) == short, (n, links, alive, comp)
            seen[short] += 1
    assert min(seen) > 20


def test_host_functions_stand_alone(tmp_path):
    """components_host.cpp without the library (tests/c_client/components_host_check.cpp), under the address and undefined-behaviour
    sanitizers: the topology chain over every combination of flag bits, the totals, the refusal of arrays that do not fit together"""
    import subprocess
    root = emu_lib.ROOT
    exe = tmp_path / "components_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(root / "autocycler_amd" / "csrc"),
                           str(root / "tests" / "c_client" / "components_host_check.cpp"), str(root / "autocycler_amd" / "csrc" / "components_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "components_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


# ---- through the library ----------------------------------------------------------------------------------------------------------------------
def run_raw(lib_path, n, links, unitig_len=None, alive=None, marked=None, device=0):
    c = components_from_links(n, links, unitig_len, alive, marked, device=device, lib_path=lib_path)
    assert isinstance(c, Components)
    return c


def check_against_model(c, n, links, unitig_len=None, alive=None, marked=None, what=""):
    U.assert_same(U.library_result(c), U.model_expected(n, links, unitig_len, alive, marked), what)


def check_kats(lib_path, device=0):
    loops = {}
    for c in KATS["component_is_circular_loop"]:
        if c["component"] == sorted(c["component"]) and c["component"]:
            loops[(c["gfa"], c["component"][0])] = c["expected"]
    expected = {key: {c["gfa"]: c for c in KATS[key]} for key in ("connected_components", "graph_stats", "topology", "is_isolated_and_circular", "is_isolated_and_linear")}
    for i in range(1, 14):
        name = f"test_gfa_{i}.gfa"
        n, links, lens = U.gfa_links(name)
        g, _, _ = graph_from_gfa((U.GOLDEN / name).read_text(), lib_path=lib_path)
        by_handle = graph_components(g, device=device)
        by_arrays = run_raw(lib_path, n, links, lens, device=device)
        assert U.result_bytes(by_handle) == U.result_bytes(by_arrays), name
        for c in (by_handle, by_arrays):
            check_against_model(c, n, links, lens, what=name)
            assert c.topology == expected["topology"][name]["expected"], name
            if name in expected["connected_components"]:
                assert c.components() == expected["connected_components"][name]["expected"], name
                st = expected["graph_stats"][name]
                sm = c.summary
                assert (sm["unitigs"], sm["total_length"], [sm["links_all"], sm["links_one_way"]]) == (st["unitigs"], st["total_length"], st["link_count"]), name
            for r in c.record_dicts():
                if (name, r["first"]) in loops:
                    assert bool(r["circular_loop"]) == loops[(name, r["first"])], (name, r)
            for key, bit in (("is_isolated_and_circular", U.ISOLATED_CIRCULAR), ("is_isolated_and_linear", U.ISOLATED_LINEAR)):
                if name in expected[key]:
                    assert [u + 1 for u in range(n) if c.flags[u] & bit] == expected[key][name]["unitigs_true"], (key, name)
    assert sum(loops.values()) == 3 and len(loops) == 9      # gfa_4: both components; gfa_5: [4] alone
    for c in KATS["edits"]:
        n, links, lens = U.gfa_links(c["gfa"])
        alive = [int(u not in c["remove_unitigs"]) for u in range(1, n + 1)] if c["remove_unitigs"] else None
        kept = without_links(links, c["delete_links"])
        got = run_raw(lib_path, n, kept, lens, alive, device=device)
        assert got.components() == c["expected"], c
        check_against_model(got, n, kept, lens, alive, what=str(c))
        for u in c["remove_unitigs"]:
            assert got.component_of[u - 1] == Components.NOT_ALIVE and got.flags[u - 1] == 0
    return True


def test_kats(emu):
    assert check_kats(emu)


# ---- random sweep -----------------------------------------------------------------------------------------------------------------------------
def check_sweep(lib_path, seed, cases, device=0):
    """returns what the sweep met: {topology: graphs}, components that are circular loops of more than one member, unclosed link sets"""
    rng = random.Random(seed)
    topologies, big_loops, unclosed = {}, 0, 0
    for i in range(cases):
        n, links, unitig_len, alive, marked = U.random_case(rng)
        got = run_raw(lib_path, n, links, unitig_len, alive, marked, device=device)
        check_against_model(got, n, links, unitig_len, alive, marked, what=f"seed {seed} case {i}")
        topologies[got.topology] = topologies.get(got.topology, 0) + 1
        big_loops += sum(1 for r in got.record_dicts() if r["circular_loop"] and r["unitigs"] > 1)
        unclosed += any(U.rc(l) not in set(links) for l in links)
    return topologies, big_loops, unclosed


def assert_sweep_coverage(results):
    topologies = set().union(*(r[0] for r in results))
    assert topologies >= set(U.TOPOLOGIES) - {"empty"}, topologies      # ("empty" too, where the alive mask leaves nothing)
    assert sum(r[1] for r in results) >= 1 and sum(r[2] for r in results) >= 1


_sweeps = {}


@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(emu, seed):
    _sweeps[seed] = check_sweep(emu, 7000 + seed, 150)
    assert_sweep_coverage([_sweeps[seed]])      # (each seed on its own already meets every topology and a loop of several members)


# ---- boundary table ---------------------------------------------------------------------------------------------------------------------------
TILE_SIZES = (2047, 2048, 2049, 4095, 4096, 4097)      # one radix-sort tile (RS_TILE) and one scan tile (SCAN_TILE) of device_prims.hpp, each +- 1


def boundary_shapes(n_big):
    """(name, shape) — n_big is odd"""
    yield "chain, permuted", U.shape_chain_permuted(n_big)
    yield "chain, descending", U.shape_chain_descending(n_big)
    yield "star", U.shape_star(n_big)
    yield "singletons", U.shape_singletons(n_big)
    yield "pairs", U.shape_pairs(n_big)
    yield "ring", U.shape_ring(n_big)
    yield "ring, one link one-way", U.shape_ring_one_way_once(n_big)
    yield "ring of two that is its own reverse complement", U.shape_self_rc_ring()
    yield "double hairpin", U.shape_double_hairpin()
    for n in TILE_SIZES:
        yield f"chain, permuted, n = {n}", U.shape_chain_permuted(n, seed=n)
        yield f"ring, n = {n}", U.shape_ring(n, seed=n)
        yield f"singletons, n = {n}", U.shape_singletons(n)
        yield f"pairs, n = {n | 1}", U.shape_pairs(n | 1)


def check_boundary_table(lib_path, n_big, with_model, device=0):
    for name, (n, links, exp) in boundary_shapes(n_big):
        ln = U.lengths(n)
        if with_model:
            U.assert_same(U.model_expected(n, links.tolist(), ln), exp, "model: " + name)
        got = run_raw(lib_path, n, links, ln, device=device)
        U.assert_same(U.library_result(got), exp, name)
        if name == "chain, permuted":
            assert 0 < got.summary["launches"] <= 25 * U.ceil_log2(n), got.summary
            assert got.summary["read_backs"] <= 4
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu, 20001, True)


# ---- scheduling independence ----------------------------------------------------------------------------------------------------------------
def scheduling_case(seed=77, n=3000):
    """rings, chains, a hub and loose links in one graph, with an alive mask and marks"""
    rng = random.Random(seed)
    order = list(range(1, n + 1))
    rng.shuffle(order)
    links, at = [], 0
    while at < n:
        size = min(n - at, rng.randint(1, 40))
        links += U.ring_links(rng, order[at:at + size]) if rng.random() < 0.5 else [l for a, b in zip(order[at:at + size], order[at + 1:at + size]) for l in ((a, -b), (b, -a))]
        at += size
    links += [(order[0], rng.choice((1, -1)) * rng.randint(1, n)) for _ in range(200)]
    links += [(rng.choice((1, -1)) * rng.randint(1, n), rng.choice((1, -1)) * rng.randint(1, n)) for _ in range(100)]
    return n, links, [rng.randint(1, 5000) for _ in range(n)], [int(rng.random() < 0.9) for _ in range(n)], [int(rng.random() < 0.1) for _ in range(n)]


def check_scheduling(lib_path, device=0):
    n, links, ln, alive, marked = scheduling_case()
    first = run_raw(lib_path, n, links, ln, alive, marked, device=device)
    check_against_model(first, n, links, ln, alive, marked)
    assert first.summary["components"] > 20 and any(r["circular_loop"] and r["unitigs"] > 1 for r in first.record_dicts())
    want = U.result_bytes(first)
    shuffled = list(links)
    random.Random(1).shuffle(shuffled)
    for variant in (links, links[::-1], shuffled):
        assert U.result_bytes(run_raw(lib_path, n, variant, ln, alive, marked, device=device)) == want
    return True


@pytest.mark.parametrize("order", [0, 1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))      # the emulation's launch order: ascending, descending, pseudo-random
    assert check_scheduling(emu)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def handle_without_host_arrays(lib_path, torch_device):
    """what a rank of a sharded build that is not the writing rank holds: every phase of the protocol in a world of one, root elsewhere"""
    import oracle_lib as O
    import sharded_util
    from autocycler_amd import sharded
    lib = _capi.load_library(lib_path)
    seqs, fn, hd = seqgen.make_case(1, 11)
    loaded = O.Seqs.from_raw(11, seqs, filenames=fn, headers=hd).all()
    shard = sharded_util.local_shard(lib, 11, loaded, 0, len(loaded), 1, torch_device)
    return sharded.sharded_build(lib, shard, sharded.Comm(torch_device), root=1, direct_when_alone=False)[0]


def check_errors(lib_path, torch_device, device=0):
    import ctypes as C
    lib = _capi.load_library(lib_path)
    ok_links = [(1, 2), (-2, -1)]
    for bad, n in (((1, 0), 3), ((0, -2), 3), ((1, 4), 3), ((-4, 2), 3), ((1, -2147483648), 3)):
        with pytest.raises(AutocyclerError, match="names no unitig"):
            run_raw(lib_path, n, ok_links + [bad] + ok_links, device=device)
        assert run_raw(lib_path, n, ok_links, device=device).components() == [[1, 2], [3]]      # a call after a failed one works
    with pytest.raises(AutocyclerError, match=r"link 2 \(1 -> 4\)"):
        run_raw(lib_path, 3, ok_links + [(1, 4), (0, 0)], device=device)
    with pytest.raises(AutocyclerError, match="names no unitig"):
        run_raw(lib_path, 0, [(1, 1)], device=device)
    links = (_capi.Link * 2)(_capi.Link(1, 2), _capi.Link(-2, -1))
    h = C.c_void_p()
    assert lib.ac_components_from_links(3, links, 2, None, None, None, device, None) != 0 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_components_from_links(3, None, 2, None, None, None, device, C.byref(h)) != 0 and b"without links" in lib.ac_last_error() and not h.value
    g, _, _ = graph_from_gfa((U.GOLDEN / "test_gfa_4.gfa").read_text(), lib_path=lib_path)
    assert lib.ac_graph_components(g._h, None, device, None) != 0 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_graph_components(None, None, device, C.byref(h)) != 0 and b"null pointer" in lib.ac_last_error()
    assert graph_components(g, device=device).components() == [[1, 2, 3], [4, 5]]
    with pytest.raises(AutocyclerError, match="one entry per unitig"):
        graph_components(g, marked=[1, 0], device=device)
    bare = handle_without_host_arrays(lib_path, torch_device)
    with pytest.raises(AutocyclerError, match="kept no host arrays"):
        graph_components(bare, device=device)
    empty = run_raw(lib_path, 0, [], device=device)
    assert empty.components() == [] and empty.topology == "empty" and empty.summary["components"] == 0 and empty.summary["unitigs"] == 0
    assert len(empty.member_off) == 1 and len(empty.flags) == 0
    nothing_alive = run_raw(lib_path, 3, ok_links, [5, 6, 7], [0, 0, 0], device=device)
    assert nothing_alive.components() == [] and nothing_alive.topology == "empty" and list(nothing_alive.component_of) == [Components.NOT_ALIVE] * 3
    assert lib.ac_topology_name(7) is None and lib.ac_topology_name(3) == b"circular"
    return True


def test_errors(emu):
    import torch
    assert check_errors(emu, torch.device("cpu"))


# ---- on a graph handle ------------------------------------------------------------------------------------------------------------------------
def check_graph(lib_path, seed, k, device=0):
    seqs, fn, hd = seqgen.make_case(seed, k)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    n = g.unitig_count
    links = [(a if fa else -a, b if fb else -b) for a, fa, b, fb in g.links()]
    lens = [len(g.unitig(i)[0]) for i in range(n)]
    got = graph_components(g, device=device)
    check_against_model(got, n, links, lens, what=f"built graph, seed {seed}, k {k}")
    assert got.summary["links_one_way"] == g.stats_post["links"] and got.summary["total_length"] == g.stats_post["total_length"]
    g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)
    assert U.result_bytes(graph_components(g2, device=device)) == U.result_bytes(got)
    # resolve.rs:273-282: the unitigs of components without an anchor
    anchors = g.resolve_bridges(device=device)[0]
    marked = [int(u in set(anchors)) for u in range(1, n + 1)]
    with_marks = graph_components(g, marked=marked, device=device)
    check_against_model(with_marks, n, links, lens, marked=marked)
    comps = with_marks.components()
    gone = {u for c, r in zip(comps, with_marks.record_dicts()) if r["marked"] == 0 for u in c}
    assert gone == U.UnitigGraph(n, links).unitigs_not_connected_to_anchor(set(anchors))
    return len(comps), len(anchors), len(gone)


@pytest.mark.parametrize("seed,k", [(3, 11), (8, 51)])
def test_graph_built_and_reloaded(emu, seed, k):
    comps, _, _ = check_graph(emu, seed, k)
    assert comps >= 1
