"""ac_trim_apply / ac_graph_trim_apply / ac_graph_trim, the Trimmed object, ac_trim_gfa, ac_trim_dir and the `trim` and `resolve` commands of
the CLI on the device: the exports, the known answers, the named cases, the chain cases of test_chain_gpu.py apart from the large one, the
renumbered text, the boundary table, the random sweep, the error list, the five forms, two runs and the launch counts.  Every comparison is
equality with the model of trim_apply_util.py or with the glue of chain_util.run_from; the checks are those of test_trim_apply_emu.py.
Nothing here is at workload size."""
import pytest

from test_trim_apply_emu import (CHAIN_CASES, ROOT, check_boundary_table, check_chain_case, check_errors, check_exports, check_forms, check_kats, check_launch_counts,
                                 check_named_cases, check_numbers_do_not_matter, check_sweep, check_two_runs_identical)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_abi_is_13_and_exports_trim_apply():
    assert check_exports(None)


def test_reference_known_answers():
    assert check_kats(None)


def test_named_cases():
    assert check_named_cases(None)


@pytest.mark.parametrize("name,seed", CHAIN_CASES)
def test_chain_agrees_with_the_glue(name, seed):
    assert check_chain_case(name, seed, None)


def test_segment_numbers_do_not_matter():
    assert check_numbers_do_not_matter(None)


def test_boundary_table():
    assert check_boundary_table(None)


def test_sweep_seeds():
    met = check_sweep(None, range(24))
    assert met["start_end"] and met["hairpin"] and met["nothing"] and met["excluded"] and met["unitig_died"], met


def test_errors():
    assert check_errors(None)


def test_forms_give_the_same_bytes():
    assert check_forms(None, cli=ROOT / "autocycler_amd" / "autocycler-compress")


def test_two_runs_give_identical_products():
    assert check_two_runs_identical(None)


def test_launches_follow_the_key_width_and_the_exclusion_alone():
    assert check_launch_counts(None)
