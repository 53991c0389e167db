"""ac_merge_finish / ac_subsets_finish on the device: the exports, the named cases, the known answers, a 150-case slice of the random sweep
with its coverage, the boundary table, independence, the round trip through a handle, the errors, and the shapes that are the smallest to
cross the tie-group paths, each against sorted() with the reference's comparator.  Every comparison is equality; the checks are those of
test_finish_emu.py."""
import pytest

from test_finish_emu import (assert_sweep_coverage, check_boundary_table, check_errors, check_exports, check_independence, check_kats, check_last_byte,
                             check_launch_counts, check_length_classes, check_named_cases, check_one_base_unitigs, check_ring, check_ring_against_the_model,
                             check_round_trip, check_shared_prefix, check_sweep)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


def test_abi_is_13_and_exports_finish():
    assert check_exports(None)


def test_named_cases():
    assert check_named_cases(None)


def test_known_answers():
    assert check_kats(None)


def test_sweep_slice():
    assert_sweep_coverage([check_sweep(None, 12000, 150)])      # 150 graphs, every coverage class at least 20 times


def test_boundary_table():
    assert check_boundary_table(None)


def test_same_bytes_run_after_run():
    assert check_independence(None, orders=(None, None))


def test_round_trip_through_a_handle():
    assert check_round_trip(None)


def test_errors():
    assert check_errors(None)


# ---- the shapes that are the smallest to cross the tie-group paths, each against sorted() ---------------------------------------------------------
def test_huge_full_ties_of_one_base_unitigs():
    """70 001 one-base unitigs over ACGT with three depth values: four groups of about 17 500 full sequence ties — stability at scale (35 radix tiles)"""
    assert check_one_base_unitigs(None, 70001)


def test_long_shared_prefix():
    """4 097 unitigs of 40 bases that share 32, the first difference at byte 32 + i % 8: one tie group of all of them"""
    assert check_shared_prefix(None, 4097)


def test_difference_in_the_last_byte():
    """130 unitigs of 100 001 bases, identical but for the last byte, two of them fully identical with different depths"""
    assert check_last_byte(None, 100001)


def test_length_classes():
    """lengths 1 ... 300 mixed"""
    assert check_length_classes(None, 300)


def test_launches_do_not_follow_group_size_or_prefix_length():
    assert check_launch_counts(None, 4097)


def test_ring_of_600001():
    """600 001 one-base unitigs on a ring with chords, 64 walks of 20 000 entries, 8 clusters, one finished with renumber = 1: several sort and
    scan tiles, more than 2^19 threads"""
    assert check_ring(None, 600001, 20000, 50000)


def test_ring_of_2000_against_the_model():
    assert check_ring_against_the_model(None)
