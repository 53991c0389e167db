"""ac_graph_subsets / ac_subsets_from_paths, the composed entries and ac_subsets_merged_paths on the device: the exports, the named cases, a
slice of the random sweep with its coverage, the boundary table, independence and the launch counts, composition, trim's slices, the errors
(each followed by a call that works), and one larger case where several sort tiles and more than 2^19 threads engage.  Every comparison
is equality; the checks are those of test_subset_emu.py."""
import numpy as np
import pytest

import merge_util as M
import subset_util as S
from test_subset_emu import (assert_sweep_coverage, check_boundary_table, check_composition, check_counts, check_errors, check_exports,
                             check_handle_reproduces_graph_merge_plan, check_independence, check_named_cases, check_sweep, check_trim)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_abi_is_13_and_exports_subsets():
    assert check_exports(None)


def test_named_cases():
    assert check_named_cases(None)


def test_handle_reproduces_graph_merge_plan():
    assert check_handle_reproduces_graph_merge_plan(None)


def test_sweep_slice():
    assert_sweep_coverage([check_sweep(None, 11000, 150)])      # 150 graphs, every coverage class at least 20 times


def test_boundary_table():
    assert check_boundary_table(None)


def test_independence():
    assert check_independence(None)


def test_counts_do_not_follow_the_clusters():
    assert check_counts(None)


def test_composition():
    assert check_composition(None)


def test_trim_slices():
    assert check_trim(None)


def test_errors():
    import torch
    assert check_errors(None, torch.device("cuda:0"))


def ring_case(n, n_paths, path_len, n_clusters, seed):
    links, entries, off = S.ring_with_chords(n, n_paths, path_len, seed)
    labels = (np.random.default_rng(seed + 1).permutation(n_paths) % n_clusters + 1).astype(np.uint16)
    return links, entries, off, labels


def test_ring_of_600001():
    """600 001 unitigs of one base on a ring with chords, 64 random walks of 20 000 entries, 8 clusters: 1.28 M keys (625 sort tiles, 313 scan
    tiles, above 2^19 threads), 2.4 M links.  The subsets are np.unique's; the merge plan and the re-threaded paths of one cluster are held
    to the length invariant here and to the model on a 2 000-unitig ring of the same shape."""
    from autocycler_amd import subsets_from_paths
    n, nc = 600001, 8
    links, entries, off, labels = ring_case(n, 64, 20000, nc, seed=21)
    lens = np.ones(n, dtype=np.uint32)
    sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc)
    S.assert_numpy_same(sub, S.expected_by_numpy(n, links, lens, entries, off, labels, nc), "ring of 600 001")
    assert sub.summary["read_backs"] == 2 and sub.summary["entries_kept"] == 64 * 20000
    plan = sub.merge_plan(3, with_sequences=False)
    assert plan.summary["chains"] > 1000
    got = sub.merged_paths(3, plan)
    assert got.seq_index.tolist() == sub.seqs(3).tolist() and got.summary["entries_before"] == 8 * 20000 > got.summary["entries_after"]
    chain_len = np.zeros(n + 1 + len(plan.chains), dtype=np.int64)
    chain_len[1:n + 1] = 1
    chain_len[plan.chains["number"]] = plan.chains["length"]
    new_len = np.add.reduceat(chain_len[np.abs(got.entries)], got.path_off[:-1].astype(np.int64))
    assert new_len.tolist() == [20000] * 8      # every sequence as long over the merged unitigs as before
    assert not np.isin(np.abs(got.entries), np.flatnonzero(plan.chain_of != M.NOT_MERGED) + 1).any()      # no merged member is left in a path


def test_ring_of_2000_against_the_model():
    from autocycler_amd import subsets_from_paths
    from test_subset_emu import check_clusters
    n, nc = 2000, 8
    links, entries, off, labels = ring_case(n, 64, 300, nc, seed=22)
    lens = [1] * n
    sub = subsets_from_paths(n, links, lens, (entries, off), labels, nc)
    paths = [entries[int(off[s]):int(off[s + 1])].tolist() for s in range(64)]
    met = check_clusters(sub, n, [tuple(l) for l in links.tolist()], lens, None, paths, labels.tolist(), nc, what="ring of 2000")
    assert met["chain"] and met["shorter_path"] and met["shared_unitig"] and met["link_dropped"]
