"""ac_apply_bridges / ac_graph_resolve_apply, the composed entries and ac_resolve_graphs on the device: the exports, the named cases, the
culling case, the boundary table, two seeds' worth of the random sweep, the graph handle, the error list, two runs and the launch counts.
Every comparison is equality; the checks are those of test_apply_emu.py.  Nothing here is at workload size."""
import pytest

from test_apply_emu import (check_boundary_table, check_culling_case, check_errors, check_exports, check_graph, check_launches_do_not_follow_bridges, check_named_cases,
                            check_sweep, check_two_runs_identical)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_abi_is_13_and_exports_apply():
    assert check_exports(None)


def test_named_cases():
    assert check_named_cases(None)


def test_culling_makes_kept_differ_from_unique():
    assert check_culling_case(None)


def test_boundary_table():
    assert check_boundary_table(None)


@pytest.mark.parametrize("seeds", [(0, 1, 2, 3, 4, 5), (6, 7, 8, 9, 10, 11)])
def test_sweep_seeds(seeds):
    check_sweep(None, seeds)


def test_graph_built_and_reloaded():
    assert check_graph(None, 3, 11)


def test_errors():
    assert check_errors(None)


def test_two_runs_give_identical_products():
    assert check_two_runs_identical(None)


def test_launches_do_not_follow_the_bridges():
    assert check_launches_do_not_follow_bridges(None)
