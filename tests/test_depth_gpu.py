"""Read-based unitig depths (ac_depth_*, ReadDepth) on the device against the checker of depth_util.py: the cases of test_depth_emu.py
(depth_cases.py) and one mid-size job against the numpy tally.  Every comparison is equality."""
import pytest

import depth_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_kat_graphs():
    DC.check_kat_graphs(None)


def test_handle_form():
    DC.check_handles(None)


@pytest.mark.parametrize("k,seed", [(11, 101), (21, 102), (31, 103)])
def test_random_graph_read_edges(k, seed):
    DC.check_random_graph(None, k, seed)


def test_long_read_and_packed_short_reads():
    DC.check_long_and_short_reads(None)


def test_threshold_boundaries():
    DC.check_threshold(None)


def test_poly_a_key_zero():
    DC.check_poly_a(None)


def test_two_graphs_and_graph_shapes():
    DC.check_two_graphs_and_shapes(None)


def test_step_budget():
    DC.check_step_budget(None)


def test_batches(monkeypatch):
    DC.check_batches(None, monkeypatch)


def test_fastq(tmp_path):
    DC.check_fastq(None, tmp_path)


def test_errors():
    DC.check_errors(None)


def test_midsize_job():
    DC.check_midsize(None)
