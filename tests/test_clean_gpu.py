"""ac_clean_graph / ac_graph_clean, the composed entries, ac_clean_gfa, ac_clean and the `clean` command of the CLI on the device: the exports,
the reference's known answers, the named cases, the boundary table, two parameter sets of six seeds of the random sweep, the handle form, the
error list, two runs and the launch counts.  Every comparison is equality with the model of clean_util.py; the checks are those of
test_clean_emu.py.  The boundary table's tile, key-width, multi-arm and dense rows run here as on the emulation; two cases fill the grid
(more than 2048 workgroups of 256 threads in the unitig and link launches; 200 003 unitigs of a random graph) and are held to
clean_model_fast without the texts, twice each: on the device the work list's order differs from run to run, the products may not."""
import pytest

from test_clean_emu import (ROOT, candidates_case, check_boundary_table, check_errors, check_exports, check_handle_form, check_kats, check_large, check_launch_counts,
                            check_named_cases, check_sweep, check_two_runs_identical, tile_case)

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
    assert check_boundary_table(None, only="one wavefront")


@pytest.mark.parametrize("only", [("tile: n =", "tile: n_out", "tile: one"), ("tile: nl", "tile: ne"), ("tile: candidates", "wide keys"), ("multi-arm", "dense")],
                         ids=["unitigs", "links", "candidates-and-wide-keys", "rounds"])
def test_boundary_table_beyond_a_wavefront(only):
    assert check_boundary_table(None, only=only)


def test_every_boundary_row_runs_on_the_device():
    """the groups above and the rows of one wavefront are the whole table"""
    from test_clean_emu import boundary_cases, rounds_per_batch
    rows = boundary_cases(rounds_per_batch(None))
    prefixes = ("tile: n =", "tile: n_out", "tile: one", "tile: nl", "tile: ne", "tile: candidates", "wide keys", "multi-arm", "dense")
    assert all(("expect" not in case) != name.startswith(prefixes) for name, case in rows.items())


_MID = []


def mid_size_case():
    """built once, read only: the two-run check compares the same case again"""
    if not _MID:
        _MID.append(tile_case(23, 200_003, n_remove=50, n_dup=100, low=0.01))
    return _MID[0]


def test_grid_filling_bubbles():
    """131 073 bubbles: 524 292 unitigs and 1 048 584 link entries, the smallest that exceeds 2048 workgroups x 256 threads = 524 288 in the unitig
    and in the link launches (at 150 001 bubbles the Python side, case and model, took 8 of the test's seconds); one round decides all"""
    case = candidates_case(131_073)
    assert case["n"] == 524_292 > 2048 * 256 and len(case["links"]) == 1_048_584
    _, sm = check_large(case, None, what="131 073 bubbles")
    assert sm["rounds"] == 1 and sm["low_depth"] == 131_073 and sm["kept_dead_end"] == 0


def test_mid_size_random_graph():
    """200 003 unitigs, 1 % low, 50 removals, 100 duplications"""
    exp, sm = check_large(mid_size_case(), None, what="200 003 unitigs")
    assert sm["duplicated"] == 100 and sm["removed"] == 50 and sm["low_depth"] >= 256 and sm["kept_dead_end"] >= 256 and sm["rounds"] >= 2


@pytest.mark.parametrize("seeds,kw", [((0, 1, 2, 3, 4, 5), {}), ((6, 7, 8, 9, 10, 11), dict(max_unitigs=16, link_factor=1.2))])
def test_sweep_seeds(seeds, kw):
    met = check_sweep(None, seeds, **kw)
    assert met["removed"] and met["duplicated"] and met["low"] and met["dead_end"] and met["rounds_above_one"], met


def test_handle_text_command_and_cli_give_the_same_bytes():
    assert check_handle_form(None, cli=ROOT / "autocycler_amd" / "autocycler-compress")


def test_errors():
    assert check_errors(None)


def test_two_runs_give_identical_products():
    assert check_two_runs_identical(None, more=[mid_size_case()])


def test_launches_follow_the_rounds_alone():
    assert check_launch_counts(None)
