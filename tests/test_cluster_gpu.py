"""ac_cluster_tree_* on the device: the reference's known answers, the tie, exact-sum, refresh-branch, generic, asymmetric, graph-handle,
host-function and argument checks of test_cluster_emu.py (the same functions), and one larger matrix against the model's numpy form.
Every comparison of merges and nodes is bit for bit."""
import pytest

import cluster_util as U
from autocycler_amd import cluster_tree
from test_cluster_emu import (EXACT_SIZES, TIE_SIZES, check_argument_errors, check_asymmetric, check_exact_sums, check_generic, check_graph,
                              check_host_functions, check_kats, check_quarter_grid, check_refresh_branches, check_smallest, check_ties_small)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_kats():
    assert check_kats(None)


def test_smallest():
    assert check_smallest(None)


def test_ties_small():
    assert check_ties_small(None)


@pytest.mark.parametrize("n", TIE_SIZES)
def test_quarter_grid(n):
    assert check_quarter_grid(None, n)


@pytest.mark.parametrize("n", EXACT_SIZES)
def test_exact_sums(n):
    assert check_exact_sums(None, n)


def test_refresh_branches():
    assert check_refresh_branches(None)


@pytest.mark.parametrize("block", range(6))
def test_generic_small(block):
    for seed in range(10 * block, 10 * block + 10):
        assert check_generic(None, seed)


def test_generic_300():
    assert check_generic(None, "large")


def test_asymmetric():
    assert check_asymmetric(None)


def test_graph_built_and_reloaded():
    assert check_graph(None, 4, 21)


def test_host_functions():
    assert check_host_functions(None)


def test_argument_errors():
    assert check_argument_errors(None)


def test_generic_1025():
    # device only: 1024 merges, more rows than one pick pass of 256 threads takes at once, 257 workgroups of refresh
    import numpy as np
    n = 1025
    rng = np.random.default_rng(1025)
    m = np.triu(rng.random((n, n)), 1)
    m = m + m.T
    exp = U.upgma_recurrence_numpy(m)
    t = cluster_tree(m, range(1, n + 1), normalise=False)
    assert U.same_bits(t.merges, U.id_merges(list(range(1, n + 1)), exp))
    assert U.same_bits(t.nodes, U.build_nodes(list(range(1, n + 1)), exp, False))
    sm = t.summary
    assert sm["launches"] == 3 + 3 * (n - 1) and sm["rescans"] >= n - 2 and sm["compares"] > 0
