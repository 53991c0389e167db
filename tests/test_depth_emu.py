"""Read-based unitig depths (ac_depth_*, ReadDepth) on the CPU emulation of the kernels against the checker of depth_util.py; the cases
are depth_cases.py's, shared with test_depth_gpu.py.  Every comparison is equality."""
import pytest

import depth_cases as DC
import emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib.emu_path()


def test_checker_reproduces_reference_kats():
    assert DC.check_kats_checker() >= 35


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numpy_tally_equals_plain(seed):
    DC.check_numpy_tally(seed)


def test_kat_graphs(lib):
    DC.check_kat_graphs(lib)


def test_handle_form(lib):
    DC.check_handles(lib)


@pytest.mark.parametrize("k,seed", [(11, 101), (21, 102), (31, 103)])
def test_random_graph_read_edges(lib, k, seed):
    DC.check_random_graph(lib, k, seed)


def test_long_read_and_packed_short_reads(lib):
    DC.check_long_and_short_reads(lib)


def test_threshold_boundaries(lib):
    DC.check_threshold(lib)


def test_poly_a_key_zero(lib):
    DC.check_poly_a(lib)


def test_two_graphs_and_graph_shapes(lib):
    DC.check_two_graphs_and_shapes(lib)


def test_step_budget(lib):
    DC.check_step_budget(lib)


def test_batches(lib, monkeypatch):
    DC.check_batches(lib, monkeypatch)


def test_fastq(lib, tmp_path):
    DC.check_fastq(lib, tmp_path)


def test_errors(lib):
    DC.check_errors(lib)
