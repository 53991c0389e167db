"""ac_combine_graphs / ac_combine_handles, ac_combine_gfas, ac_combine, the gfa2fasta entries and the `combine` and `gfa2fasta` commands of the CLI on the
device: the exports, the reference's known answers, the named cases, the boundary table, a sweep, the errors, the entry forms, two runs, the launch
counts and the finished chain.  Every comparison is equality with the model of combine_util.py, and every record and text is byte-equal to what
the CPU emulation gives for the same input; the checks are those of test_combine_emu.py.  Nothing here is at workload size."""
import random

import pytest

import combine_util as CU
import emu_lib
from autocycler_amd import combine_graphs
from test_combine_emu import (CHAIN_CASES, ROOT, chain_graph, check_boundary_table, check_chain, check_entry_forms, check_errors, check_exports, check_gfa2fasta, check_kats,
                              check_launch_counts, check_named_cases, check_sweep, check_two_runs_identical, link_count_graph, named_cases, random_texts, read_depth_cases,
                              SCAN_TILE)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()      # (host code: it needs nothing but the compiler)


def test_abi_is_13_and_exports_combine():
    assert check_exports(None)


def test_reference_known_answers():
    assert check_kats(None)


def test_named_cases():
    assert check_named_cases(None)


def test_boundary_table():
    assert check_boundary_table(None)


def test_sweep_seeds():
    met = check_sweep(None, range(40))
    assert all(met.values()), met


def test_errors():
    assert check_errors(None)


def test_arrays_handles_texts_directory_and_cli_give_the_same_bytes():
    assert check_entry_forms(None, cli=ROOT / "autocycler_amd" / "autocycler-compress")


def test_two_runs_give_identical_results():
    assert check_two_runs_identical(None)


def test_launches_do_not_follow_the_sizes():
    assert check_launch_counts(None)


def test_gfa2fasta():
    assert check_gfa2fasta(None)


def test_device_and_emulation_give_the_same_bytes(emu):
    rng = random.Random(3)
    inputs = [(texts, None) for texts in named_cases().values()] + list(read_depth_cases().values()) + [random_texts(rng) for _ in range(10)] + \
        [([chain_graph(SCAN_TILE + 1, first=3, step=2, closed=True), link_count_graph(5000)], None)]
    for texts, rd in inputs:
        forms = [CU.array_form(CU.from_gfa_text(t)) for t in texts]
        dev, ref = combine_graphs(forms, read_depths=rd), combine_graphs(forms, read_depths=rd, lib_path=emu)
        assert CU.combined_bytes(dev) == CU.combined_bytes(ref)
        assert (dev.gfa(), dev.fasta(), dev.yaml(), dev.depth_lines()) == (ref.gfa(), ref.fasta(), ref.yaml(), ref.depth_lines())
        assert dev.summary["read_backs"] == ref.summary["read_backs"]
        dev.close(); ref.close()


@pytest.mark.parametrize("name,seed", CHAIN_CASES)
def test_chain_ends_in_the_planted_consensus(name, seed):
    check_chain(name, seed, None)
