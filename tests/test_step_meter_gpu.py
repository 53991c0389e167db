"""The step meter on the device: the graph steps' launch and read-back counts against the ones recorded at the parent commit (the cases of
test_step_meter_emu.py; default environment, read-backs through the mailbox), and for every step that times itself — components, merge,
subsets, merged paths, trim, resolve, cluster, cluster QC — that its device seconds are positive and no more than the wall time around the
call."""
import random
import time

import pytest

import resolve_util as R
import step_meter_cases as K

pytestmark = pytest.mark.gpu

# (launches, read_backs) of summary[...] on an MI355X, recorded through step_meter_cases.collect at commit ac646a2: above the emulation's by
# the fused fill flushes and the mailbox's publishing kernel, which count as launches there
RECORDED = {
    "components: one unitig, no links": (8, 2),
    "components: ring of 3": (18, 2),
    "components: 65 unitigs, two components, some dead": (24, 2),
    "components: nothing": (0, 0),
    "merge: chain of 4": (43, 4),
    "merge: chain of 4 with sequences": (44, 4),
    "merge: handle with paths": (47, 4),
    "subsets: no link kept": (13, 2),
    "subsets: links kept": (19, 2),
    "subsets: no kept entry": (0, 0),
    "merged paths: chains": (9, 2),
    "merged paths: no chain": (8, 2),
    "merged paths: no entry": (0, 0),
}


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


@pytest.fixture(scope="module")
def rows():
    K.collect()      # (the first call of a process pays for the context, the arena and the code objects: not what the wall time below is about)
    t0 = time.perf_counter()
    got = K.collect()
    return got, time.perf_counter() - t0


def test_table_covers_the_cases():
    assert tuple(RECORDED) == K.CASES


@pytest.mark.parametrize("case", K.CASES)
def test_counts_are_the_recorded_ones(rows, case):
    got, _ = rows
    print(case, got[case])
    assert (got[case]["launches"], got[case]["read_backs"]) == RECORDED[case]


def test_graph_steps_time_themselves(rows):
    """every case that launches: seconds_device > 0; all of them together no more than the wall time around the calls"""
    got, wall = rows
    launching = [c for c in K.CASES if c not in K.NOTHING_LAUNCHED]
    print({c: got[c]["seconds_device"] for c in launching}, wall)
    assert all(got[c]["seconds_device"] > 0 for c in launching)
    assert all(got[c]["seconds_device"] == 0 for c in K.NOTHING_LAUNCHED)
    assert sum(got[c]["seconds_device"] for c in launching) <= wall
    plain, with_seq = got["merge: chain of 4"], got["merge: chain of 4 with sequences"]
    assert plain["seconds_copy"] == 0 and 0 < with_seq["seconds_copy"] <= with_seq["seconds_device"]


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t0


def test_each_graph_step_within_its_wall_time():
    from autocycler_amd import components_from_links, merge_plan_from_links, subsets_from_paths
    import merge_util as M
    links, lens = M.closed_set([(1, 2), (2, 3), (3, 4)]), [3, 4, 5, 6]
    comp, wall = timed(lambda: components_from_links(4, links, lens))
    assert 0 < comp.summary["seconds_device"] <= wall
    plan, wall = timed(lambda: merge_plan_from_links(4, links, lens, sequences=[b"ACG", b"TTGA", b"CCATG", b"GATTAC"]))
    assert 0 < plan.summary["seconds_copy"] < plan.summary["seconds_device"] <= wall      # (the components inside it count)
    sub, wall = timed(lambda: subsets_from_paths(4, links, lens, [[1, 2, 3], [-3, -2], [4]], [1, 2, 1], 2))
    assert 0 < sub.summary["seconds_device"] <= wall
    cluster_plan = sub.merge_plan(1, with_sequences=False)
    paths, wall = timed(lambda: sub.merged_paths(1, cluster_plan))
    assert 0 < paths.summary["seconds_device"] <= wall


def test_trim_times_its_batches():
    """two paths of 40 entries, one with a start-end overlap of 10"""
    from autocycler_amd import trim_path_slices
    core = list(range(1, 31))
    paths = [core + core[:10], list(range(31, 71))]
    (res, sm), wall = timed(lambda: trim_path_slices(paths, [5] * 70))
    print(sm, wall)
    assert res[0]["start_end"]["status"] == 1 and res[0]["start_end"]["end"] - res[0]["start_end"]["begin"] == 30 and res[1]["start_end"]["status"] != 1
    assert sm["launches"] >= 1 and 0 < sm["seconds_device"] <= wall


def test_resolve_times_its_batches(monkeypatch):
    """three paths between two anchors: their distances in one launch, then (AC_RESOLVE_BATCH_BYTES, as in test_resolve_emu.py) in several, which
    reuses the one interval; and two pairs of them through ac_path_distances, which has no summary"""
    from autocycler_amd import path_distances, resolve_bridge_paths
    rng = random.Random(8)
    w = [rng.randint(1, 5000) for _ in range(12)] + [100, 100]
    paths = [[13] + R.random_path(rng, rng.randint(70, 100), 12) + [14] for _ in range(3)]
    d, status = path_distances(paths, [(0, 1), (1, 2)], w)
    assert status == [0, 0] and d == [R.global_alignment_distance_numpy(paths[0], paths[1], w), R.global_alignment_distance_numpy(paths[1], paths[2], w)]
    whole, wall = timed(lambda: resolve_bridge_paths(paths, w))
    print(whole[2], wall)
    assert whole[2]["launches"] == 1 and whole[2]["jobs"] >= 2 and 0 < whole[2]["seconds_device"] <= wall
    monkeypatch.setenv("AC_RESOLVE_BATCH_BYTES", str(101 * 4))      # one job's worth of scratch rows
    cut, wall = timed(lambda: resolve_bridge_paths(paths, w))
    print(cut[2], wall)
    assert cut[2]["launches"] == cut[2]["jobs"] == whole[2]["jobs"] and cut[:2] == whole[:2]
    assert 0 < cut[2]["seconds_device"] <= wall


@pytest.mark.parametrize("n", [2, 3])
def test_cluster_times_its_loop(n):
    from autocycler_amd import cluster_tree
    asym = [[0.0 if a == b else 0.125 * (1 + abs(a - b)) for b in range(n)] for a in range(n)]
    t, wall = timed(lambda: cluster_tree(asym, list(range(1, n + 1)), normalise=False))
    print(t.summary, wall)
    assert t.summary["launches"] == 3 + 3 * (n - 1) and 0 < t.summary["seconds"] <= wall


def test_cluster_qc_times_its_evaluations():
    """the smallest refinement case of test_cluster_qc_gpu.py: two sequences, the cut at the root, one alternative — the start clustering and one
    round, an interval each"""
    import cluster_qc_util as Q
    from autocycler_amd import cluster_tree
    asym = [[0.0, 0.25], [0.25, 0.0]]
    t = cluster_tree(asym, [3, 8], normalise=False)
    inp = Q.Inputs([5, 6], [0, 1], [1, 1], [0, 0])
    got, wall = timed(lambda: t.generate(asym, *inp.args(), 0.5, 2, ()))
    print(got.summary, wall)
    assert [len(r["scores"]) for r in got.trace][0] == 1 and got.summary["evaluations"] == 2 and got.summary["readbacks"] == 2
    assert 0 < got.summary["seconds"] <= wall
