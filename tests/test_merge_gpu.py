"""ac_graph_merge_plan / ac_merge_plan_from_links on the device: the reference's known answers, a slice of the random sweep with its
coverage, the named cases, the boundary table with the permuted chain at a size where several scan and sort tiles and more than 2^19
threads engage, scheduling independence, the errors and graph handles.  Every comparison is equality; the checks are those of
test_merge_emu.py."""
import numpy as np
import pytest

import merge_util as M
from test_merge_emu import (CHAIN_LENGTHS, TILE_SIZES, assert_sweep_coverage, check_boundary_table, check_errors, check_graph, check_kats, check_named_cases,
                            check_scheduling, check_sweep)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"
    assert lib.ac_abi_version() == 13


def test_kats():
    assert check_kats(None)


def test_sweep_slice():
    assert_sweep_coverage([check_sweep(None, 9000, 150)])      # 150 graphs, every coverage class at least 20 times


def test_named_cases():
    assert check_named_cases(None)


def test_boundary_table():
    assert check_boundary_table(None, CHAIN_LENGTHS + TILE_SIZES, False)


def test_permuted_chain_of_600001():
    """every unitig 1 base, one chain of 600 001 members in a random order on random strands: above 2048 workgroups x 256 threads, 147 scan
    tiles, 586 sort tiles of the links; 21 rounds of pointer jumping whatever the order.  Expected by construction, in numpy."""
    from autocycler_amd import merge_plan_from_links
    n = 600001
    rng = np.random.default_rng(11)
    order = (rng.permutation(n) + 1).astype(np.int64)
    s = np.where(rng.random(n) < 0.5, order, -order)
    links = np.empty((2 * (n - 1), 2), dtype=np.int32)
    links[0::2, 0] = s[:-1]; links[0::2, 1] = s[1:]
    links[1::2, 0] = -s[1:]; links[1::2, 1] = -s[:-1]
    codes = rng.integers(0, 4, n)
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    got = merge_plan_from_links(n, links, np.ones(n, dtype=np.uint32), depth=np.full(n, 2.0), sequences=[bytes([b]) for b in seqs.tolist()])
    want = s if order[0] < order[-1] else -s[::-1]      # emitted from the end whose unitig has the lower number
    assert got.chain_dicts() == [dict(number=n + 1, members=n, length=n, member_off=0, seq_off=0, depth=2.0, type=0, loop=0)]
    assert np.array_equal(got.members, want.astype(np.int32))
    assert not got.chain_of.any() and not got.fixed.any() and len(got.links) == 0
    comp = np.frombuffer(b"TGCA", dtype=np.uint8)[codes]
    assert np.array_equal(got.sequences, np.where(want > 0, seqs[np.abs(want) - 1], comp[np.abs(want) - 1]))
    sm = got.summary
    assert (sm["chains"], sm["merged_unitigs"], sm["unitigs_after"], sm["links_after"], sm["bases_copied"]) == (1, n, 1, 0, n)
    # the same launches as n / 2 chains of two at this n: nothing grows with the length of a chain
    a = np.arange(1, n, 2, dtype=np.int32)
    pairs = np.empty((2 * len(a), 2), dtype=np.int32)
    pairs[0::2, 0] = a; pairs[0::2, 1] = a + 1
    pairs[1::2, 0] = -(a + 1); pairs[1::2, 1] = -a
    two = merge_plan_from_links(n, pairs, np.ones(n, dtype=np.uint32))
    assert two.summary["chains"] == n // 2 and two.summary["launches"] == sm["launches"] - 1      # (- 1: no sequences, no copy kernel)


def test_scheduling_independence():
    assert check_scheduling(None)


def test_errors():
    import torch
    assert check_errors(None, torch.device("cuda:0"))


@pytest.mark.parametrize("seed,k", [(3, 11), (8, 51)])
def test_graph_handle(seed, k):
    with_paths, without = check_graph(None, seed, k)
    assert without >= with_paths
