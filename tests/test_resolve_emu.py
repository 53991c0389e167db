"""ac_path_distances / ac_resolve_bridge_paths / ac_resolve_bridges on the CPU emulation of the shipped kernel (kernels_resolve.inc under the
lockstep emulation of wave_rt.hpp) against the reference's own known answers (golden/resolve_kats.json) and the plain-Python model
(resolve_util.py).  Every comparison is equality: the arithmetic is integer.  The same checks run on the device in test_resolve_gpu.py."""
import random

import pytest

import emu_lib
import parity_util
import resolve_util as R
import seqgen
from autocycler_amd import AutocyclerError, graph_from_gfa, path_distances, resolve_bridge_paths
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


KATS = R.load_kats()
MODEL_KEYS = ("start", "end", "depth", "status", "best_path", "best_total", "distinct_paths", "conflicting", "culled", "cull_rank")


def dense(wdict):
    """{unitig: length} -> the list the library takes (weights[u - 1]; numbers the dict leaves out get 0 and are never named)"""
    return [wdict.get(u, 0) for u in range(1, max(wdict) + 1)]


def assert_equals_model(got, paths, w, n_unitigs, cw=None, dist=R.global_alignment_distance):
    anchors, bridges, sm = got
    exp_anchors, exp_bridges = R.resolve_expected(paths, w, n_unitigs, cw, dist)
    assert anchors == exp_anchors
    assert [{k: b[k] for k in MODEL_KEYS} for b in bridges] == exp_bridges
    return sm


# ---- the model reproduces the reference's known answers --------------------------------------------------------------------------------
def test_model_reproduces_kats():
    for c in KATS["global_alignment_distance"]:
        for a, b in ((c["a"], c["b"]), (c["b"], c["a"])):
            assert R.global_alignment_distance(a, b, c["weights"]) == c["expected"], c["test"]
            assert R.global_alignment_distance_numpy(a, b, c["weights"]) == c["expected"], c["test"]
    for c in KATS["get_anchor_to_anchor_paths"]:
        assert R.get_anchor_to_anchor_paths(c["sequence_paths"], set(c["anchors"])) == c["expected"]
    for c in KATS["group_paths_by_start_end"]:
        assert R.group_paths_by_start_end(c["paths"]) == {(g["start"], g["end"]): g["paths"] for g in c["expected"]}
    for c in KATS["bridge_unitig_nums"]:
        b = R.new_bridge(c["start"], c["end"], c["paths"], c["weights"])
        assert (-b["end"], -b["start"], b["depth"]) == (c["rev_start"], c["rev_end"], c["depth"])
    for c in KATS["determine_ambiguity"]:
        bridges = [R.new_bridge(s, e, ps, c["weights"]) for s, e, ps in c["bridges"]]
        R.determine_ambiguity(bridges)
        assert [bool(b["_c"]) for b in bridges] == c["expected"], c["test"]
    for c in KATS["best_path"]:
        assert R.new_bridge(c["start"], c["end"], c["paths"], c["weights"])["best_path"] == c["expected"], c["test"]
    for c in KATS["consensus_weight"]:
        assert R.consensus_weight(c["header"]) == c["expected"], c["header"]


def test_model_numpy_equals_plain():
    rng = random.Random(31)
    for _ in range(200):
        U = rng.randint(1, 12)
        w = [rng.randint(1, 5000) for _ in range(U)]
        a = R.random_path(rng, rng.randint(0, 30), U)
        b = R.edited_copy(rng, a, 0.3, U) if rng.random() < 0.6 else R.random_path(rng, rng.randint(0, 30), U)
        assert R.global_alignment_distance_numpy(a, b, w) == R.global_alignment_distance(a, b, w)


def test_host_functions_stand_alone(tmp_path):
    """resolve_host.cpp without the library, a CPU stub for the distances (tests/c_client/resolve_host_check.cpp; the same program is what a
    sanitizer build runs)"""
    import subprocess
    root = emu_lib.ROOT
    exe = tmp_path / "resolve_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-I", str(root / "autocycler_amd" / "csrc"), str(root / "tests" / "c_client" / "resolve_host_check.cpp"),
                           str(root / "autocycler_amd" / "csrc" / "resolve_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "resolve_host_check: OK" in out.stdout, out.stdout[-2000:]


# ---- the known answers through the library ---------------------------------------------------------------------------------------------
def check_kats(lib_path, device=0):
    kw = dict(device=device, lib_path=lib_path)
    assert len(KATS["global_alignment_distance"]) == 7
    for c in KATS["global_alignment_distance"]:
        d, st = path_distances([c["a"], c["b"]], [(0, 1), (1, 0)], dense(c["weights"]), **kw)
        assert d == [c["expected"]] * 2 and st == [0, 0], c["test"]
    # Bridge::new's KATs (test_best_path_*, test_bridge_unitig_nums): the bridge's paths as sequences, plus one sequence of consensus
    # weight 0 that holds the two end unitigs alone — it takes no part in the bridge, but leaves only those two as anchors
    for c in KATS["best_path"] + KATS["bridge_unitig_nums"]:
        w = dense(c["weights"])
        first, last = c["paths"][0][0], c["paths"][0][-1]
        seqs, cw = c["paths"] + [[first, last]], [1] * len(c["paths"]) + [0]
        got = resolve_bridge_paths(seqs, w, cw, **kw)
        anchors, bridges, _ = got
        assert anchors == sorted((abs(first), abs(last))) and len(bridges) == 1
        b = bridges[0]
        assert (b["start"], b["end"], b["depth"], b["status"]) == (first, last, len(c["paths"]), 0)      # (each of these paths is larger than its reverse)
        if "expected" in c:
            assert b["best_path"] == c["expected"], c["test"]
        else:
            assert (-b["end"], -b["start"], b["depth"]) == (-last, -first, c["depth"]) and (c["rev_start"], c["rev_end"]) == (-c["end"], -c["start"])
        assert_equals_model(got, seqs, c["weights"], len(w), cw)
    # test_get_anchor_to_anchor_paths / test_group_paths_by_start_end: the same device for the anchor set {1, 2, 6, 8}; the bridges are
    # the known groups, their paths the known anchor-to-anchor paths
    (c,), (grp,) = KATS["get_anchor_to_anchor_paths"], KATS["group_paths_by_start_end"]
    assert grp["paths"] == c["expected"]
    seqs, cw, w = c["sequence_paths"] + [c["anchors"]], [1, 1, 1, 0], [10] * 12
    got = resolve_bridge_paths(seqs, w, cw, **kw)
    assert got[0] == c["anchors"]
    from collections import Counter
    assert sorted((b["start"], b["end"], b["depth"], sorted((tuple(p), n) for p, n in b["distinct_paths"])) for b in got[1]) == \
        sorted((e["start"], e["end"], len(e["paths"]), sorted(Counter(tuple(p[1:-1]) for p in e["paths"]).items())) for e in grp["expected"])
    assert_equals_model(got, seqs, w, 12, cw)
    # (test_determine_ambiguity_* build Bridge objects whose start / end no set of sequences produces — (4, -5) would be kept as (5, -4),
    # resolve.rs:354 — so they are held through the model alone, which the sweeps hold the library's flags and cull order to)
    return True


def test_kats(emu):
    assert check_kats(emu)


def test_consensus_weight_from_headers(emu):
    # test_consensus_weight through the library: the headers travel in a GFA's HD:Z tags
    paths = [[1, 2, 3], [1, 4, 3]]
    lines = ["H\tVN:Z:1.0\tKM:i:3"] + [f"S\t{u}\tACGTA\tDP:f:1.00" for u in (1, 2, 3, 4)] + \
            ["L\t1\t+\t2\t+\t0M", "L\t2\t-\t1\t-\t0M", "L\t2\t+\t3\t+\t0M", "L\t3\t-\t2\t-\t0M",
             "L\t1\t+\t4\t+\t0M", "L\t4\t-\t1\t-\t0M", "L\t4\t+\t3\t+\t0M", "L\t3\t-\t4\t-\t0M"]
    for c in KATS["consensus_weight"]:
        p_lines = [f"P\t1\t1+,2+,3+\t*\tLN:i:15\tFN:Z:a.fasta\tHD:Z:{c['header']}", "P\t2\t1+,4+,3+\t*\tLN:i:15\tFN:Z:b.fasta\tHD:Z:c2"]
        g, _, hds = graph_from_gfa("\n".join(lines + p_lines) + "\n", lib_path=emu)
        assert hds[0] == c["header"]
        anchors, bridges, _ = g.resolve_bridges()
        exp = R.resolve_expected(paths, [5] * 4, 4, [c["expected"], 1])
        assert (anchors, [{k: b[k] for k in MODEL_KEYS} for b in bridges]) == exp
        assert bridges[0]["depth"] == c["expected"] + 1 and R.consensus_weight(c["header"]) == c["expected"]


# ---- random sweep ------------------------------------------------------------------------------------------------------------------------
def check_sweep(lib_path, seed, cases, device=0):
    rng = random.Random(seed)
    jobs = bridges_seen = culled = 0
    for _ in range(cases):
        paths, w, cw = R.random_case(rng)
        got = resolve_bridge_paths(paths, w, cw, device=device, lib_path=lib_path)
        sm = assert_equals_model(got, paths, w, len(w), cw)
        jobs += sm["jobs"]; bridges_seen += len(got[1]); culled += sum(b["culled"] for b in got[1])
        assert sm["jobs_not_launched"] == 0 and sm["jobs"] == sum(len(b["distinct_paths"]) * (len(b["distinct_paths"]) - 1) // 2 for b in got[1])
    return jobs, bridges_seen, culled


@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(emu, seed):
    jobs, bridges, culled = check_sweep(emu, 9000 + seed, 75)
    assert jobs > 50 and bridges > 150      # (or the sweep tests nothing)


def test_sweep_culls_somewhere(emu):
    assert sum(check_sweep(emu, 9100 + s, 40)[2] for s in range(3)) > 0


@pytest.mark.parametrize("order", [1, 2])
def test_scheduling_independence(emu, monkeypatch, order):
    monkeypatch.setenv("AC_EMU_ORDER", str(order))
    check_sweep(emu, 9200 + order, 25)


# ---- kernel boundaries -------------------------------------------------------------------------------------------------------------------
BOUNDARY_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300)


def boundary_paths(seed=77, n_unitigs=9):
    """one path per boundary length, each a noisy cut of one long path so that the alignments are not all-mismatch"""
    rng = random.Random(seed)
    w = [rng.randint(1, 5000) for _ in range(n_unitigs)]
    base = R.random_path(rng, 300, n_unitigs)
    return [(R.edited_copy(rng, base, 0.1, n_unitigs) + R.random_path(rng, n, n_unitigs))[:n] for n in BOUNDARY_LENGTHS], w


_expected_boundary = {}


def expected_boundary():
    if not _expected_boundary:
        paths, w = boundary_paths()
        assert [len(p) for p in paths] == list(BOUNDARY_LENGTHS)
        for i, a in enumerate(paths):
            for j, b in enumerate(paths):
                _expected_boundary[(i, j)] = R.global_alignment_distance_numpy(a, b, w)
                if len(a) * len(b) <= 65 * 65:
                    assert _expected_boundary[(i, j)] == R.global_alignment_distance(a, b, w)
    return _expected_boundary


def check_boundary_table(lib_path, device=0):
    paths, w = boundary_paths()
    exp = expected_boundary()
    pairs = sorted(exp)
    d, st = path_distances(paths, pairs, w, device=device, lib_path=lib_path)      # all (n, m) crossings, both orders, 81 jobs in one call
    assert st == [0] * len(pairs)
    assert d == [exp[p] for p in pairs]
    assert all(d[pairs.index((i, j))] == d[pairs.index((j, i))] for i, j in pairs)
    for n_jobs in (1, 3, 4, 5, 257):      # the workgroup's four slots: one, partly filled, full, one over, many groups
        some = [pairs[(7 * q) % len(pairs)] for q in range(n_jobs)]
        assert path_distances(paths, some, w, device=device, lib_path=lib_path)[0] == [exp[p] for p in some], n_jobs
    return True


def test_boundary_table(emu):
    assert check_boundary_table(emu)


def check_special_pairs(lib_path, device=0):
    rng = random.Random(5)
    w = [rng.randint(1, 5000) for _ in range(9)]
    for n in (1, 64, 65, 130):
        p = R.random_path(rng, n, 9)
        flipped = [-u for u in p]
        d, st = path_distances([p, list(p), flipped, []], [(0, 1), (0, 2), (2, 0), (0, 3), (3, 0), (3, 3)], w, device=device, lib_path=lib_path)
        total = sum(R.weight_of(w, u) for u in p)
        assert st == [0] * 6
        assert d[0] == 0                                                          # equal paths
        assert d[1] == d[2] == R.global_alignment_distance_numpy(p, flipped, w)  # they differ only in sign: no entry matches its twin
        assert 0 < d[1] <= total                                                  # (a mismatch of equal weights costs that weight once)
        assert d[3] == d[4] == total and d[5] == 0                                # all gaps, one side empty
    return True


def test_special_pairs(emu):
    assert check_special_pairs(emu)


# ---- batching, deduplication, limits -------------------------------------------------------------------------------------------------
def test_batches_equal_one_launch(emu, monkeypatch):
    rng = random.Random(8)
    w = [rng.randint(1, 5000) for _ in range(12)]
    inner = [R.random_path(rng, rng.randint(70, 100), 12) for _ in range(5)]
    paths = [[13] + p + [14] for p in inner] + [[13] + inner[0] + [14]]
    w += [100, 100]
    whole = resolve_bridge_paths(paths, w, lib_path=emu)
    assert whole[2]["launches"] == 1 and whole[2]["jobs"] == 10
    monkeypatch.setenv("AC_RESOLVE_BATCH_BYTES", str(2 * 101 * 4))      # two jobs' worth of scratch rows
    cut = resolve_bridge_paths(paths, w, lib_path=emu)
    assert cut[2]["launches"] >= 5 and cut[:2] == whole[:2] and cut[2]["cells"] == whole[2]["cells"]
    assert_equals_model(whole, paths, w, len(w))


def test_deduplication_equals_the_model_on_all_copies(emu):
    rng = random.Random(12)
    w = [rng.randint(1, 5000) for _ in range(10)] + [7, 9]
    base = R.random_path(rng, 6, 10) * 2      # (every unitig twice: none of them is an anchor, the 150 paths form one bridge)
    three = [base]
    while len(three) < 3:
        p = R.edited_copy(rng, base, 0.3, 10)
        if p not in three:
            three.append(p)
    paths = [[11] + three[i % 3] + [12] for i in range(150)]
    got = resolve_bridge_paths(paths, w, lib_path=emu)
    sm = assert_equals_model(got, paths, w, len(w))      # (the model aligns all 150 x 149 pairs)
    assert got[0] == [11, 12] and sm["jobs"] == 3 and len(got[1]) == 1 and got[1][0]["depth"] == 150 and [c for _, c in got[1][0]["distinct_paths"]] == [50, 50, 50]


def test_empty_bridges_launch_nothing(emu):
    paths = [[1, 2, 3], [1, 2, 3], [-3, -2, -1]]
    got = resolve_bridge_paths(paths, [4, 5, 6], lib_path=emu)
    sm = assert_equals_model(got, paths, [4, 5, 6], 3)
    assert got[0] == [1, 2, 3] and [b["best_path"] for b in got[1]] == [[], []] and (sm["jobs"], sm["launches"]) == (0, 0)


def test_overflowing_pairs_report_status_2(emu):
    big = [0x80000000, 0x7FFFFFFF, 1, 5, 5]      # w(1) + w(2) = 2^32 - 1: still fine; w(1) + w(2) + w(3) = 2^32
    d, st = path_distances([[1], [2], [2, 3], [3]], [(0, 1), (0, 2), (2, 0), (1, 3)], big, lib_path=emu)
    assert st == [0, 2, 2, 0] and d == [0x80000000, 0, 0, 0x7FFFFFFF]
    paths = [[4, 1, 5], [4, 2, 3, 5], [4, 3, 5]]
    got = resolve_bridge_paths(paths, big, lib_path=emu)
    sm = assert_equals_model(got, paths, big, 5)
    assert [b["status"] for b in got[1]] == [2] and got[1][0]["best_path"] is None
    assert (sm["jobs"], sm["launches"], sm["jobs_not_launched"]) == (0, 0, 1)      # nothing launched for that bridge
    # a total that reaches u32::MAX although no pair overflows
    w2 = [0x7FFFFFFF, 0x7FFFFFFF, 1, 1, 5, 5]
    paths = [[5, 1, 6], [5, 2, 6], [5, 3, 6], [5, 4, 6]]
    got = resolve_bridge_paths(paths, w2, lib_path=emu)
    assert_equals_model(got, paths, w2, 6)
    assert got[1][0]["status"] == 2 and got[2]["jobs"] == 6


def check_above_max_path(lib_path, device=0):
    n = _capi.max_resolve_path(lib_path) + 1
    assert n > 20000
    p = [1 + (i % 3) for i in range(n)]
    with pytest.raises(AutocyclerError, match="ac_resolve_max_path"):
        path_distances([p, [1, 2]], [(0, 1)], [1, 1, 1], device=device, lib_path=lib_path)
    with pytest.raises(AutocyclerError, match="ac_resolve_max_path"):
        resolve_bridge_paths([[4] + p + [5], [4, 1, 5]], [1, 1, 1, 1, 1], device=device, lib_path=lib_path)
    return True


def test_above_max_path_fails_cleanly(emu):
    assert check_above_max_path(emu)


def test_validation_errors(emu):
    for bad in ([1, 0, 3], [1, -4, 3], [-2147483648]):
        with pytest.raises(AutocyclerError, match="names no unitig"):
            path_distances([[1, 2], bad], [(0, 1)], [5, 5, 5], lib_path=emu)
        with pytest.raises(AutocyclerError, match="names no unitig"):
            resolve_bridge_paths([[1, 2], bad], [5, 5, 5], lib_path=emu)
    with pytest.raises(AutocyclerError, match="names a path that does not exist"):
        path_distances([[1, 2]], [(0, 1)], [5, 5, 5], lib_path=emu)
    assert path_distances([], [], [5], lib_path=emu) == ([], [])
    assert resolve_bridge_paths([[1, 2, 1]], [5, 5], lib_path=emu)[:2] == ([2], [])


# ---- on a graph handle ---------------------------------------------------------------------------------------------------------------
def variant_assemblies(seed, k, n=5, length=700):
    """n assemblies of one replicon: a common sequence with a different stretch replaced in some of them (a bubble between two shared
    stretches), one assembly reverse-complemented"""
    r = random.Random(seed)
    base = seqgen.rand_seq(r, length)
    seqs = []
    for i in range(n):
        s = base
        for at in (150, 420):
            if r.random() < 0.5:
                s = s[:at] + seqgen.rand_seq(r, 3 * k) + s[at + 3 * k:]
        seqs.append(seqgen.rc(s) if i == 2 else s)
    return seqs, [f"assembly_{i}.fasta" for i in range(n)], [f"contig_{i}" for i in range(n)]


def check_graph(lib_path, seed, k, device=0):
    seqs, fn, hd = variant_assemblies(seed, k)
    g, gfa, _ = parity_util.check_case(k, seqs, fn, hd, lib_path=lib_path, repair=False, device=device)
    paths = [list(g.path(s)) for s in range(g.n_seqs)]
    w = [len(g.unitig(i)[0]) for i in range(g.unitig_count)]
    got = g.resolve_bridges(device=device)
    sm = assert_equals_model(got, paths, w, len(w))
    assert got[0] and got[1] and sm["jobs"] > 0      # anchors, bridges, and a bridge with more than one path
    g2, _, _ = graph_from_gfa(gfa, lib_path=lib_path)      # what `autocycler resolve` itself starts from
    assert g2.resolve_bridges(device=device)[:2] == got[:2]
    # the same file with a consensus weight on one contig and a zero on another
    tagged = gfa.replace("HD:Z:contig_1", "HD:Z:contig_1 Autocycler_consensus_weight=3").replace("HD:Z:contig_3", "HD:Z:contig_3 autocycler_consensus_weight=0")
    assert tagged != gfa
    g3, _, _ = graph_from_gfa(tagged, lib_path=lib_path)
    assert_equals_model(g3.resolve_bridges(device=device), paths, w, len(w), [1, 3, 1, 0, 1])
    return True


@pytest.mark.parametrize("seed,k", [(3, 11), (8, 21)])
def test_graph_built_and_reloaded(emu, seed, k):
    assert check_graph(emu, seed, k)
