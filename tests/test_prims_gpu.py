"""tests/prim_cases.py on the MI355X: the device primitives and the wave layer through the ac_selftest_* hooks of the product library."""
import pytest

import prim_cases as P
from autocycler_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"
    return lib


@pytest.mark.parametrize("kind", list(_capi.SCAN_KINDS))
def test_scan_every_size(lib, kind):
    P.scan_every_size(None, kind, gpu=True)


@pytest.mark.parametrize("kind", list(_capi.SCAN_KINDS))
def test_scan_misaligned_pointers(lib, kind):
    P.scan_misaligned(None, kind)


@pytest.mark.parametrize("window", P.WINDOWS, ids=lambda w: f"{w[0]}-{w[1]}")
def test_radix_bit_window(lib, window):
    P.radix_window(None, window, gpu=True)


@pytest.mark.parametrize("n", P.sizes(True))
def test_radix_every_size(lib, n):
    P.radix_one_size(None, n, gpu=True)


def test_radix_trivial_passes(lib):
    P.radix_trivial_passes(None, gpu=True)


def test_radix_i32_values(lib):
    P.radix_i32_values(None, gpu=True)


def test_radix_prepared_scratch(lib):
    P.radix_prepared_scratch(None, gpu=True)


@pytest.mark.parametrize("op", ["min", "argmin"])
def test_segments(lib, op):
    P.segments(None, op, gpu=True)


@pytest.mark.parametrize("op", ["min", "argmin"])
def test_segments_count_mismatch(lib, op):
    P.segments_count_mismatch(None, op)


def test_sort_by_key_cmp(lib):
    P.sort_pairs_cmp(None, gpu=True)


def test_sort_keys_cmp(lib):
    P.sort_indices_cmp(None, gpu=True)


def test_scan_pool_epoch_wrap(lib):
    P.pool_epoch_wrap(None)


def test_scan_pool_invalidate(lib):
    P.pool_invalidate(None)


def test_scan_pool_growth(lib):
    P.pool_growth(None)


@pytest.mark.parametrize("program", range(len(P.PROGRAM_NAMES)), ids=lambda p: P.PROGRAM_NAMES[p].replace(" ", "_"))
def test_wave_program_equals_the_model(lib, program):
    P.wave_program(None, program)
