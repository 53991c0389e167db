"""ac_clean_graph / ac_graph_clean, the composed entries, ac_clean_gfa, ac_clean and the `clean` command of the CLI on the device: the exports,
the reference's known answers, the named cases, the boundary table, two parameter sets of six seeds of the random sweep, the handle form, the
error list, two runs and the launch counts.  Every comparison is equality with the model of clean_util.py; the checks are those of
test_clean_emu.py.  Nothing here is at workload size."""
import pytest

from test_clean_emu import (ROOT, check_boundary_table, check_errors, check_exports, check_handle_form, check_kats, check_launch_counts, check_named_cases, check_sweep,
                            check_two_runs_identical)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_abi_is_13_and_exports_clean():
    assert check_exports(None)


def test_reference_known_answers():
    assert check_kats(None)


def test_named_cases():
    assert check_named_cases(None)


def test_boundary_table():
    assert check_boundary_table(None)


@pytest.mark.parametrize("seeds,kw", [((0, 1, 2, 3, 4, 5), {}), ((6, 7, 8, 9, 10, 11), dict(max_unitigs=16, link_factor=1.2))])
def test_sweep_seeds(seeds, kw):
    met = check_sweep(None, seeds, **kw)
    assert met["removed"] and met["duplicated"] and met["low"] and met["dead_end"] and met["rounds_above_one"], met


def test_handle_text_command_and_cli_give_the_same_bytes():
    assert check_handle_form(None, cli=ROOT / "autocycler_amd" / "autocycler-compress")


def test_errors():
    assert check_errors(None)


def test_two_runs_give_identical_products():
    assert check_two_runs_identical(None)


def test_launches_follow_the_rounds_alone():
    assert check_launch_counts(None)
