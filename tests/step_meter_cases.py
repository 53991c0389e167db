"""The graph steps' launch and read-back counts: the smallest inputs that reach every branch of components_device, merge_plan_device,
subsets_device and merged_paths_device, and one function that runs them all through the Python API and returns what their summaries say.
test_step_meter_emu.py holds the emulation to the table recorded at the parent commit, test_step_meter_gpu.py the device."""
import merge_util as M
import subset_util as S
from autocycler_amd import components_from_links, graph_from_gfa, graph_merge_plan, merge_plan_from_links, subsets_from_paths

# the order of the rows in the recorded tables
CASES = ("components: one unitig, no links", "components: ring of 3", "components: 65 unitigs, two components, some dead", "components: nothing",
         "merge: chain of 4", "merge: chain of 4 with sequences", "merge: handle with paths",
         "subsets: no link kept", "subsets: links kept", "subsets: no kept entry",
         "merged paths: chains", "merged paths: no chain", "merged paths: no entry")
NOTHING_LAUNCHED = ("components: nothing", "subsets: no kept entry", "merged paths: no entry")


def _row(summary):
    return dict(launches=summary["launches"], read_backs=summary["read_backs"], seconds_device=summary["seconds_device"], seconds_copy=summary.get("seconds_copy"))


def collect(lib_path=None, device=0):
    """{case: dict(launches, read_backs, seconds_device, seconds_copy or None)} in the order of CASES"""
    kw = dict(device=device, lib_path=lib_path)
    rows = {}
    # components
    rows[CASES[0]] = _row(components_from_links(1, [], [5], **kw).summary)
    ring = components_from_links(3, M.closed_set([(1, 2), (2, 3), (3, 1)]), [5, 6, 7], **kw)
    assert [int(r["circular_loop"]) for r in ring.records] == [1]
    rows[CASES[1]] = _row(ring.summary)
    links = M.closed_set([(u, u + 1) for u in range(1, 40)] + [(u, u + 1) for u in range(41, 65)])
    alive = [int(u not in (40, 65)) for u in range(1, 66)]      # the last unitig of either chain: two components still
    two = components_from_links(65, links, [1] * 65, alive=alive, **kw)
    assert [int(r["unitigs"]) for r in two.records] == [39, 24]
    rows[CASES[2]] = _row(two.summary)
    rows[CASES[3]] = _row(components_from_links(0, [], [], **kw).summary)
    # the merge plan
    chain, lens = M.closed_set([(1, 2), (2, 3), (3, 4)]), [3, 4, 5, 6]
    plain = merge_plan_from_links(4, chain, lens, **kw)
    with_seq = merge_plan_from_links(4, chain, lens, sequences=[b"ACG", b"TTGA", b"CCATG", b"GATTAC"], **kw)
    assert plain.chain_members() == with_seq.chain_members() == [[1, 2, 3, 4]] and with_seq.chain_sequences() == [b"ACGTTGACCATGGATTAC"]
    rows[CASES[4]], rows[CASES[5]] = _row(plain.summary), _row(with_seq.summary)
    n, hl, hlens, paths = 6, M.closed_set([(1, 2), (2, 3), (3, 4), (3, 5), (5, 6)]), [9, 8, 7, 3, 2, 1], [[1, 2, 3, 4], [1, 2, 3, 5, 6], [2, 3, 5, 6]]
    seqs = [bytes(b"ACGT"[(u + i) & 3] for i in range(l)) for u, l in enumerate(hlens)]
    g, _, _ = graph_from_gfa(S.hand_gfa_text(n, hl, seqs, paths), lib_path=lib_path)
    handle = graph_merge_plan(g, use_paths=True, device=device)
    assert handle.chain_members() == [[2, 3], [5, 6]]
    rows[CASES[6]] = _row(handle.summary)
    # subsets: 3 sequences in 2 clusters
    none_kept = subsets_from_paths(4, M.closed_set([(1, 4)]), lens, [[1], [2], [3]], [1, 1, 2], 2, **kw)
    assert none_kept.summary["links"] == 0
    rows[CASES[7]] = _row(none_kept.summary)
    slinks, spaths = [(1, 2), (-2, -1), (2, 3), (-3, -2)], [[1, 2, 3], [-3, -2], []]
    sub = subsets_from_paths(4, slinks, lens, spaths, [1, 2, 1], 2, **kw)
    assert sub.summary["links"] == 6
    rows[CASES[8]] = _row(sub.summary)
    rows[CASES[9]] = _row(subsets_from_paths(4, slinks, lens, spaths, [0, 0, 0], 2, **kw).summary)
    # merged paths
    plan = sub.merge_plan(1, with_sequences=False, device=device)
    assert plan.chain_members() == [[1, 2, 3]]
    rows[CASES[10]] = _row(sub.merged_paths(1, plan, device=device).summary)
    fork = subsets_from_paths(3, M.closed_set([(1, 2), (1, 3)]), [2, 3, 4], [[1, 2], [1, 3], []], [1, 1, 2], 2, **kw)
    fork_plan = fork.merge_plan(1, with_sequences=False, device=device)
    assert fork_plan.chain_members() == []
    rows[CASES[11]] = _row(fork.merged_paths(1, fork_plan, device=device).summary)
    empty_plan = fork.merge_plan(2, with_sequences=False, device=device)
    rows[CASES[12]] = _row(fork.merged_paths(2, empty_plan, device=device).summary)
    assert tuple(rows) == CASES
    return rows
