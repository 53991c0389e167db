"""ac_graph_merge_plan / ac_merge_plan_from_links on the CPU emulation of the shipped kernels (kernels_merge.inc; its wave kernel under the
lockstep emulation of wave_rt.hpp) against the reference's own known answers (golden/merge_kats.json) and the literal Python model of
merge_linear_paths (merge_util.py).  Every comparison is equality, depths bit for bit.  The same checks run on the device in
test_merge_gpu.py."""
import random

import numpy as np
import pytest

import components_util as U
import emu_lib
import merge_util as M
import parity_util
import seqgen
from autocycler_amd import AutocyclerError, MergePlan, graph_from_gfa, graph_merge_plan, merge_plan_from_links
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = M.load_kats()


def test_abi_is_13_and_exports_merge(emu):
    """without the feature this fails outright: the library is ABI 12 and has none of these symbols"""
    lib = _capi.load_library(emu)
    assert lib.ac_abi_version() == 13
    for name in ("ac_graph_merge_plan", "ac_merge_plan_from_links", "ac_merge_chains", "ac_merge_members", "ac_merge_chain_of_unitig", "ac_merge_fixed_flags",
                 "ac_merge_sequences", "ac_merge_links", "ac_merge_summary_get_sized", "ac_merge_free"):
        assert name in _capi.EXPORTS and getattr(lib, name)


# ---- the model reproduces the reference's known answers ------------------------------------------------------------------------------------
def model_of_gfa(name):
    g = M.gfa_graph(name)
    return g, M.model_expected(g["n"], g["links"], g["lens"], g["alive"], g["path_ends"], g["depths"], g["fwd"], g["rev"], None, g["seqs"])


def assert_kat(case, got, what):
    """one test_merge_linear_paths case against a result in merge_util's form"""
    g = M.gfa_graph(case["gfa"])
    assert sum(1 for u in range(g["n"]) if g["alive"] is None or g["alive"][u]) == case["unitigs_before"], what
    assert got["unitigs_after"] == case["unitigs_after"], (what, got["unitigs_after"])
    by_number = dict(zip(got["numbers"], got["seqs"]))
    for number, seq in case["sequences"].items():
        assert by_number[int(number)] == seq.encode(), (what, number)
    if case["links"] is not None:
        assert got["links"].tolist() == sorted(list(l) for l in case["links"]), (what, got["links"].tolist())


def test_model_reproduces_kats():
    cm = KATS["can_merge"]
    g, exp = model_of_gfa(cm["gfa"])
    assert [u + 1 for u in range(g["n"]) if exp["fixed"][u] & M.FIXED_START] == cm["fixed_starts"]
    assert [u + 1 for u in range(g["n"]) if exp["fixed"][u] & M.FIXED_END] == cm["fixed_ends"]
    assert [c["gfa"] for c in KATS["merge_linear_paths"]] == ["test_gfa_3.gfa", "test_gfa_4.gfa", "test_gfa_5.gfa", "test_gfa_14.gfa"]
    for case in KATS["merge_linear_paths"]:
        assert_kat(case, model_of_gfa(case["gfa"])[1], "model: " + case["gfa"])
    for case in KATS["merge_unitig_seqs"]:
        seqs = [s.encode() for s in case["sequences"]]
        assert b"".join(seqs[abs(x) - 1] if x > 0 else M.reverse_complement(seqs[abs(x) - 1]) for x in case["path"]) == case["expected"].encode()


def test_host_functions_stand_alone(tmp_path):
    """merge_host.cpp without the library (tests/c_client/merge_host_check.cpp), under the address and undefined-behaviour sanitizers: the
    fixed seeds, the three depth rules, the type rule, the totals, the refusal of arrays that do not fit together, the error texts"""
    import subprocess
    root = emu_lib.ROOT
    exe = tmp_path / "merge_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           str(root / "autocycler_amd" / "csrc"), str(root / "tests" / "c_client" / "merge_host_check.cpp"),
                           str(root / "autocycler_amd" / "csrc" / "merge_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "merge_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


# ---- through the library ----------------------------------------------------------------------------------------------------------------------
def run_raw(lib_path, n, links, lens, alive=None, path_ends=None, depths=None, fwd=None, rev=None, types=None, seqs=None, device=0):
    p = merge_plan_from_links(n, links, lens, alive, path_ends, depths, fwd, rev, types, seqs, device=device, lib_path=lib_path)
    assert isinstance(p, MergePlan)
    return p


def check_against_model(p, what="", **case):
    exp = M.model_expected(**case)
    M.assert_same(M.library_result(p), exp, what)
    return exp


def check_kats(lib_path, device=0):
    cm = KATS["can_merge"]
    for case in KATS["merge_linear_paths"]:
        name = case["gfa"]
        g = M.gfa_graph(name)
        kw = dict(n=g["n"], links=g["links"], lens=g["lens"], alive=g["alive"], path_ends=g["path_ends"], depths=g["depths"], fwd=g["fwd"], rev=g["rev"], seqs=g["seqs"])
        by_arrays = run_raw(lib_path, device=device, **kw)
        assert_kat(case, M.library_result(by_arrays), name)
        check_against_model(by_arrays, name, types=None, **kw)
        if name == cm["gfa"]:
            assert [u + 1 for u in range(g["n"]) if by_arrays.fixed[u] & MergePlan.FIXED_START] == cm["fixed_starts"]
            assert [u + 1 for u in range(g["n"]) if by_arrays.fixed[u] & MergePlan.FIXED_END] == cm["fixed_ends"]
        if g["alive"] is None:      # (the GFA loader takes segments numbered 1, 2, 3, ...: test_gfa_14, whose numbers have gaps, goes through the arrays alone)
            handle, _, _ = graph_from_gfa((U.GOLDEN / name).read_text(), lib_path=lib_path)
            by_handle = graph_merge_plan(handle, device=device)
            assert M.result_bytes(by_handle) == M.result_bytes(by_arrays), name
            assert M.result_bytes(graph_merge_plan(handle, use_paths=False, device=device)) == M.result_bytes(by_arrays), name      # (these GFAs have no paths)
            without = graph_merge_plan(handle, with_sequences=False, device=device)
            assert len(without.sequences) == 0 and without.chain_members() == by_arrays.chain_members() and without.chains["seq_off"].tolist() == by_arrays.chains["seq_off"].tolist()
    for case in KATS["merge_unitig_seqs"]:      # the path as links: one chain, its sequence merge_unitig_seqs'
        seqs = [s.encode() for s in case["sequences"]]
        path = case["path"]
        got = run_raw(lib_path, len(seqs), M.closed_set(list(zip(path[:-1], path[1:]))), [len(s) for s in seqs], seqs=seqs, device=device)
        assert got.chain_members() == [path] and got.chain_sequences() == [case["expected"].encode()], case
    return True


def test_kats(emu):
    assert check_kats(emu)


# ---- random sweep -----------------------------------------------------------------------------------------------------------------------------
COVERAGE = ("chains", "from_reverse_strand", "closing_a_loop", "cut_by_a_fixed_end", "depth_rule_1", "depth_rule_2", "depth_rule_3", "consentigs")


def check_sweep(lib_path, seed, cases, device=0):
    """returns what the sweep met, by the names of COVERAGE"""
    rng = random.Random(seed)
    met = dict.fromkeys(COVERAGE, 0)
    for i in range(cases):
        case = M.random_case(rng)
        got = run_raw(lib_path, case["n"], case["links"], case["lens"], case["alive"], case["path_ends"], case["depths"], case["fwd"], case["rev"], case["types"],
                      case["seqs"], device=device)
        exp = check_against_model(got, f"seed {seed} case {i}", **case)
        met["chains"] += len(exp["chains"])
        for chain, loop, rule, typ in zip(exp["chains"], exp["loops"], exp["depth_rules"], exp["types"]):
            met["from_reverse_strand"] += chain[0] < 0
            met["closing_a_loop"] += loop
            # cut by a fixed end: the last member has a single exclusive output that only the fixed sets keep out of the chain
            last = chain[-1]
            met["cut_by_a_fixed_end"] += bool(exp["fixed"][abs(last) - 1] & (M.FIXED_END if last > 0 else M.FIXED_START)) and not loop
            met[f"depth_rule_{rule}"] += 1
            met["consentigs"] += typ == M.CONSENTIG
    return met


def assert_sweep_coverage(results, least=20):
    total = {k: sum(r[k] for r in results) for k in COVERAGE}
    assert all(v >= least for v in total.values()), total


def test_random_sweep(emu):
    assert_sweep_coverage([check_sweep(emu, 9000 + seed, 150) for seed in range(4)])      # 600 graphs


# ---- named cases ------------------------------------------------------------------------------------------------------------------------------
RING = M.closed_set([(14, -4), (-4, -12), (-12, 16), (16, 14)])      # 14+ -> 4- -> 12- -> 16+ -> 14+


def named_cases():
    """(name, arguments, expected chains or None = whatever the model says)"""
    ones = lambda n: [1 + (u % 4) for u in range(n)]
    yield "ring with a path that fixes 4 and 14", dict(n=20, links=RING, lens=ones(20), path_ends=[(-14, 20)]), [[-14, -16, 12]]
    yield "ring without a path", dict(n=20, links=RING, lens=ones(20), path_ends=[]), [[4, -14, -16, 12]]
    yield "ring with the path (+12, +12)", dict(n=20, links=RING, lens=ones(20), path_ends=[(12, 12)]), [[4, -14, -16]]
    yield "Moebius ring", dict(n=2, links=M.closed_set([(1, 2), (2, -1), (-1, -2), (-2, 1)]), lens=[3, 4], path_ends=[]), []
    yield "hairpin at a chain end", dict(n=4, links=M.closed_set([(1, 2), (2, 3), (3, -3), (4, 1)]), lens=[5, 1, 2, 3], path_ends=[]), None
    yield "hairpin at a chain start", dict(n=3, links=M.closed_set([(-1, 1), (1, 2), (2, 3)]), lens=[5, 1, 2], path_ends=[]), None
    yield "last links back to first, alongside other inputs", dict(n=5, links=M.closed_set([(1, 2), (2, 3), (3, 1), (4, 1), (5, 1)]), lens=[2, 3, 4, 1, 1],
                                                                  path_ends=[]), None
    yield "last links back to first on the reverse strands", dict(n=5, links=M.closed_set([(-3, -2), (-2, -1), (-1, -3), (-1, 4), (-1, 5)]), lens=[2, 3, 4, 1, 1],
                                                                 path_ends=[]), None
    yield "dead unitig at the top: numbers still start behind n", dict(n=4, links=M.closed_set([(1, 2), (2, 4)]), lens=[1, 2, 3, 4], alive=[1, 1, 1, 0], path_ends=[]), [[1, 2]]


def check_named_cases(lib_path, device=0):
    for name, kw, chains in named_cases():
        n = kw["n"]
        rng = random.Random(n)
        kw = dict(kw, seqs=[bytes(rng.choice(b"ACGT") for _ in range(l)) for l in kw["lens"]], depths=[float(u % 3) + 0.5 for u in range(n)])
        got = run_raw(lib_path, device=device, **kw)
        exp = check_against_model(got, name, **kw)
        if chains is not None:
            assert got.chain_members() == chains == exp["chains"], (name, got.chain_members())
        else:
            assert len(exp["chains"]) >= 1, name
        if name.startswith("ring with a path that"):
            assert [u + 1 for u in range(n) if got.fixed[u] & 1] == [4] and [u + 1 for u in range(n) if got.fixed[u] & 2] == [4, 14, 20]
            assert got.chain_of[3] == MergePlan.NOT_MERGED
        if name.startswith("last links back"):
            assert exp["loops"] == [1] and got.chains["loop"].tolist() == [1]
        if name.startswith("dead unitig"):
            assert got.chains["number"].tolist() == [5]
    return True


def test_named_cases(emu):
    assert check_named_cases(emu)


# ---- boundary table ---------------------------------------------------------------------------------------------------------------------------
CHAIN_LENGTHS = (63, 64, 65, 255, 256, 257)
TILE_SIZES = (2047, 2048, 2049, 4095, 4096, 4097)      # one radix-sort tile (RS_TILE) and one scan tile (SCAN_TILE) of device_prims.hpp, each +- 1


def boundary_shapes(sizes):
    """(name, (arguments, expected)); pairs take an odd n"""
    for n in sizes:
        yield f"straight chain, n = {n}", M.shape_straight(n)
        yield f"permuted chain, n = {n}", M.shape_permuted(n, seed=n)
        yield f"ring, n = {n}", M.shape_ring(n, seed=n)
        yield f"pairs, n = {n | 1}", M.shape_pairs(n | 1)
        yield f"singletons, n = {n}", M.shape_singletons(n)


def sequence_shapes():
    """member lengths 1, 3, 4, 5, 31, 32, 33 on both strands (shape_lengths' pattern, the permuted chains above) — and here: one member of
    100 001 bases among 1-base members, on either strand, with chains that start at odd byte offsets"""
    for big_at, big_forward in ((0, True), (17, False), (39, True)):
        n = 41
        lens = [1] * n
        lens[big_at] = 100001
        strands = [(u % 3) != 1 for u in range(n)]
        strands[big_at] = big_forward
        yield f"one member of 100 001 bases at {big_at}", M.shape_chain(n, range(1, n + 1), strands, lens=lens)
    # several chains whose merged bytes begin at odd offsets: pairs with odd total lengths
    yield "pairs of odd lengths", M.shape_pairs(41)


def check_shape(lib_path, name, kw, exp, with_model, device=0):
    if with_model:
        M.assert_same(M.model_expected(kw["n"], kw["links"], kw["lens"], None, kw["path_ends"], kw["depths"], None, None, None, kw["seqs"]), exp, "model: " + name)
    got = run_raw(lib_path, kw["n"], kw["links"], kw["lens"], None, kw["path_ends"], kw["depths"], None, None, None, kw["seqs"], device=device)
    M.assert_same(M.library_result(got), exp, name)
    return got.summary


def check_boundary_table(lib_path, sizes, with_model, device=0):
    launches = {}
    for name, (kw, exp) in boundary_shapes(sizes):
        sm = check_shape(lib_path, name, kw, exp, with_model, device)
        launches[name] = sm["launches"]
        assert sm["read_backs"] <= 6, (name, sm)
    for n in sizes:      # independent of the length of the chains: one chain of n, one permuted chain of n, n / 2 chains of two — at equal n
        if n % 2:
            assert launches[f"straight chain, n = {n}"] == launches[f"permuted chain, n = {n}"] == launches[f"pairs, n = {n}"] > 0, (n, launches)
        else:
            assert launches[f"straight chain, n = {n}"] == launches[f"permuted chain, n = {n}"] > 0, (n, launches)
    for name, (kw, exp) in sequence_shapes():
        check_shape(lib_path, name, kw, exp, with_model, device)
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu, CHAIN_LENGTHS + TILE_SIZES, True)


# ---- scheduling independence ----------------------------------------------------------------------------------------------------------------
def scheduling_case(seed=78, n=3000):
    """rings, chains, hubs and loose links in one graph, with an alive mask, path ends, positions, anchors and sequences"""
    rng = random.Random(seed)
    order = list(range(1, n + 1))
    rng.shuffle(order)
    links, at = [], 0
    while at < n:
        size = min(n - at, rng.randint(1, 40))
        s = [u if rng.random() < 0.5 else -u for u in order[at:at + size]]
        links += list(zip(s[:-1], s[1:])) + ([(s[-1], s[0])] if rng.random() < 0.5 else [])
        at += size
    links += [(order[0], rng.choice((1, -1)) * rng.randint(1, n)) for _ in range(100)]
    links += [(rng.choice((1, -1)) * rng.randint(1, n), rng.choice((1, -1)) * rng.randint(1, n)) for _ in range(100)]
    alive = [int(rng.random() < 0.95) for _ in range(n)]
    living = [u for u in range(1, n + 1) if alive[u - 1]]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.choice((1, 2, 3, 7, 16, 40)))) for _ in range(n)]
    return dict(n=n, links=M.closed_set(links), lens=[len(s) for s in seqs], alive=alive,
                path_ends=[(rng.choice((1, -1)) * rng.choice(living), rng.choice((1, -1)) * rng.choice(living)) for _ in range(30)],
                depths=[rng.random() * 50 for _ in range(n)], fwd=[rng.randint(0, 3) for _ in range(n)], rev=[rng.randint(0, 3) for _ in range(n)],
                types=[rng.choice((M.OTHER, M.OTHER, M.ANCHOR, M.BRIDGE)) for _ in range(n)], seqs=seqs)


def check_scheduling(lib_path, device=0):
    case = scheduling_case()
    call = lambda links: run_raw(lib_path, case["n"], links, case["lens"], case["alive"], case["path_ends"], case["depths"], case["fwd"], case["rev"], case["types"],
                                 case["seqs"], device=device)
    first = call(case["links"])
    exp = check_against_model(first, "scheduling case", **case)
    assert len(exp["chains"]) > 20 and sum(exp["loops"]) >= 1 and any(c[0] < 0 for c in exp["chains"])
    want = M.result_bytes(first)
    shuffled = list(case["links"])
    random.Random(1).shuffle(shuffled)
    for variant in (case["links"][::-1], shuffled):
        assert M.result_bytes(call(variant)) == want
    return True


@pytest.mark.parametrize("order", [0, 1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))      # the emulation's launch order: ascending, descending, pseudo-random
    assert check_scheduling(emu)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def check_errors(lib_path, torch_device, device=0):
    import ctypes as C
    lib = _capi.load_library(lib_path)
    ok_links, lens = [(1, 2), (-2, -1)], [3, 4, 5]
    works = lambda: run_raw(lib_path, 3, ok_links, lens, device=device).chain_members() == [[1, 2]]      # a call after a failed one works
    for bad in ((1, 0), (0, -2), (1, 4), (-4, 2), (1, -2147483648)):
        with pytest.raises(AutocyclerError, match="names no unitig"):
            run_raw(lib_path, 3, ok_links + [bad] + ok_links, lens, device=device)
        assert works()
    with pytest.raises(AutocyclerError, match=r"link 2 \(1 -> 4\)"):
        run_raw(lib_path, 3, ok_links + [(1, 4), (0, 0)], lens, device=device)
    with pytest.raises(AutocyclerError, match="names no unitig"):
        run_raw(lib_path, 0, [(1, 1)], [], device=device)
    # a duplicated link among alive unitigs: the first repeated entry is quoted
    with pytest.raises(AutocyclerError, match=r"link 3 \(-2 -> -1\) is a duplicate"):
        run_raw(lib_path, 3, ok_links + [(2, 3), (-2, -1), (-3, -2), (1, 2)], lens, device=device)
    assert works()
    # ... among dead unitigs it is no error
    assert run_raw(lib_path, 3, ok_links + [(3, 3), (3, 3)], lens, alive=[1, 1, 0], device=device).chain_members() == [[1, 2]]
    # a link whose reverse complement is missing: the first such entry is quoted, with what is missing
    with pytest.raises(AutocyclerError, match=r"link 2 \(2 -> 3\) has no reverse complement \(-3 -> -2\)"):
        run_raw(lib_path, 3, ok_links + [(2, 3), (3, -1)], lens, device=device)
    assert works()
    # a path end that names a dead or nonexistent unitig
    with pytest.raises(AutocyclerError, match=r"last entry of sequence 1 \(-3\) names a unitig that is not alive"):
        run_raw(lib_path, 3, ok_links, lens, alive=[1, 1, 0], path_ends=[(1, 2), (2, -3)], device=device)
    for end in ((0, 1), (1, 4), (-4, 1)):
        with pytest.raises(AutocyclerError, match="names no unitig"):
            run_raw(lib_path, 3, ok_links, lens, path_ends=[end], device=device)
    assert works()
    links = (_capi.Link * 2)(_capi.Link(1, 2), _capi.Link(-2, -1))
    ln = (C.c_uint32 * 3)(3, 4, 5)
    seq, begin = (C.c_uint8 * 13)(*b"ACGTACGTACGTA"), (C.c_uint64 * 3)(0, 3, 7)
    h = C.c_void_p()
    raw = lambda links_, ln_, seq_, begin_, out: lib.ac_merge_plan_from_links(3, links_, 2, ln_, None, None, 0, None, None, None, None, seq_, begin_, device, out)
    assert raw(links, None, None, None, C.byref(h)) != 0 and b"unitig_len" in lib.ac_last_error() and not h.value
    assert raw(links, ln, seq, None, C.byref(h)) != 0 and b"both or neither" in lib.ac_last_error() and not h.value
    assert raw(links, ln, None, begin, C.byref(h)) != 0 and b"both or neither" in lib.ac_last_error() and not h.value
    assert raw(links, ln, None, None, None) != 0 and b"null pointer" in lib.ac_last_error()
    assert raw(None, ln, None, None, C.byref(h)) != 0 and b"without links" in lib.ac_last_error() and not h.value
    assert raw(links, ln, seq, begin, C.byref(h)) == 0 and h.value
    assert MergePlan(lib, h, 3).chain_sequences() == [b"ACGTACG"]
    g, _, _ = graph_from_gfa((U.GOLDEN / "test_gfa_4.gfa").read_text(), lib_path=lib_path)
    assert lib.ac_graph_merge_plan(g._h, 1, 1, device, None) != 0 and b"null pointer" in lib.ac_last_error()
    assert lib.ac_graph_merge_plan(None, 1, 1, device, C.byref(h)) != 0 and b"null pointer" in lib.ac_last_error()
    assert graph_merge_plan(g, device=device).summary["unitigs_after"] == 2
    from test_components_emu import handle_without_host_arrays
    with pytest.raises(AutocyclerError, match="kept no host arrays"):
        graph_merge_plan(handle_without_host_arrays(lib_path, torch_device), device=device)
    empty = run_raw(lib_path, 0, [], [], device=device)
    assert empty.chain_members() == [] and len(empty.links) == 0 and len(empty.fixed) == 0 and empty.summary["unitigs_after"] == 0
    nothing_alive = run_raw(lib_path, 3, ok_links, lens, alive=[0, 0, 0], device=device)
    assert nothing_alive.chain_members() == [] and len(nothing_alive.links) == 0 and nothing_alive.summary["unitigs_after"] == 0
    return True


def test_errors(emu):
    import torch
    assert check_errors(emu, torch.device("cpu"))


# ---- on a graph handle ------------------------------------------------------------------------------------------------------------------------
def check_graph(lib_path, seed, k, device=0):
    """a built graph and its reload: with its paths (the path ends fix unitig ends, the position counts are the histogram of the path
    entries) and as a graph without sequences"""
    seqs, fn, hd = seqgen.make_case(seed, k)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    n = g.unitig_count
    links = [(a if fa else -a, b if fb else -b) for a, fa, b, fb in g.links()]
    unitigs = [g.unitig(i) for i in range(n)]
    useq, depths = [u[0].encode() if isinstance(u[0], str) else bytes(u[0]) for u in unitigs], [float(u[1]) for u in unitigs]
    paths = [[int(e) for e in g.path(s)] for s in range(len(seqs))]
    fwd, rev = [0] * n, [0] * n
    for p in paths:
        for e in p:
            (fwd if e > 0 else rev)[abs(e) - 1] += 1
    kw = dict(n=n, links=links, lens=[len(s) for s in useq], depths=depths, seqs=useq)
    with_paths = graph_merge_plan(g, use_paths=True, device=device)
    check_against_model(with_paths, f"built graph with paths, seed {seed}, k {k}", path_ends=[(p[0], p[-1]) for p in paths if p], fwd=fwd, rev=rev, **kw)
    without = graph_merge_plan(g, use_paths=False, device=device)
    check_against_model(without, f"built graph without paths, seed {seed}, k {k}", path_ends=[], **kw)
    g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)
    assert M.result_bytes(graph_merge_plan(g2, use_paths=True, device=device)) == M.result_bytes(with_paths)
    return len(with_paths.chains), len(without.chains)


@pytest.mark.parametrize("seed,k", [(3, 11), (8, 51)])
def test_graph_built_and_reloaded(emu, seed, k):
    with_paths, without = check_graph(emu, seed, k)
    assert without >= with_paths
