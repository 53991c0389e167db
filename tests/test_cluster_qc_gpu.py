"""ac_cluster_generate / ac_cluster_qc_nodes on the device: the checks of test_cluster_qc_emu.py (the same functions) with the shipped
library: the reference's known answers, the smallest shapes, nested accepted splits, the running best, reorder_clusters, the chain's order
dependence, tip ranges on and across the 64-bit words, 70 alternatives with and without pair batches, the random sweep, manual clusters,
the graph route, the argument errors and the schedule.  Every comparison with the model is bit for bit."""
import pytest

from test_cluster_qc_emu import (BOUNDARY_SIZES, check_argument_errors, check_chain, check_graph, check_kats, check_manual, check_many_alternatives,
                                 check_reorder, check_running_best, check_schedule, check_smallest, check_split_twice, check_sweep,
                                 check_word_boundaries)

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


def test_split_twice():
    assert check_split_twice(None)


def test_running_best():
    assert check_running_best(None)


def test_reorder():
    assert check_reorder(None)


def test_chain():
    assert check_chain(None)


@pytest.mark.parametrize("S", sorted(BOUNDARY_SIZES))
def test_word_boundaries(S):
    assert check_word_boundaries(None, S)


def test_many_alternatives():
    assert check_many_alternatives(None)


def test_many_alternatives_batched(monkeypatch):
    monkeypatch.setenv("AC_CLUSTER_QC_PAIR_BATCH", "8000")      # 24640 pair entries in the round: four launches
    sm = check_many_alternatives(None, default_batches=False)
    assert sm["pair_batches"] == 1 + 4 and sm["launches"] == 1 + 5 + 2 and sm["readbacks"] == 2


def test_schedule():
    assert check_schedule(None)


@pytest.mark.parametrize("block", range(6))
def test_sweep(block):
    for seed in range(10 * block, 10 * block + 10):
        assert check_sweep(None, seed)


def test_manual():
    assert check_manual(None)


def test_graph_built_and_reloaded():
    assert check_graph(None, 4, 21)


def test_argument_errors():
    assert check_argument_errors(None)
