"""tests/prim_cases.py on the CPU emulation of the kernels: the device primitives and the wave layer through the ac_selftest_* hooks."""
import pytest

import emu_lib
import prim_cases as P
from autocycler_amd import _capi


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


@pytest.mark.parametrize("kind", list(_capi.SCAN_KINDS))
def test_scan_every_size(emu, kind):
    P.scan_every_size(emu, kind, gpu=False)


@pytest.mark.parametrize("kind", list(_capi.SCAN_KINDS))
def test_scan_misaligned_pointers(emu, kind):
    P.scan_misaligned(emu, kind)


@pytest.mark.parametrize("window", P.WINDOWS, ids=lambda w: f"{w[0]}-{w[1]}")
def test_radix_bit_window(emu, window):
    P.radix_window(emu, window, gpu=False)


@pytest.mark.parametrize("n", P.sizes(False))
def test_radix_every_size(emu, n):
    P.radix_one_size(emu, n, gpu=False)


def test_radix_trivial_passes(emu):
    P.radix_trivial_passes(emu, gpu=False)


def test_radix_i32_values(emu):
    P.radix_i32_values(emu, gpu=False)


def test_radix_prepared_scratch(emu):
    P.radix_prepared_scratch(emu, gpu=False)


@pytest.mark.parametrize("op", ["min", "argmin"])
def test_segments(emu, op):
    P.segments(emu, op, gpu=False)


@pytest.mark.parametrize("op", ["min", "argmin"])
def test_segments_count_mismatch(emu, op):
    P.segments_count_mismatch(emu, op)


def test_sort_by_key_cmp(emu):
    P.sort_pairs_cmp(emu, gpu=False)


def test_sort_keys_cmp(emu):
    P.sort_indices_cmp(emu, gpu=False)


def test_scan_pool_epoch_wrap(emu):
    P.pool_epoch_wrap(emu)


def test_scan_pool_invalidate(emu):
    P.pool_invalidate(emu)


@pytest.mark.parametrize("program", range(len(P.PROGRAM_NAMES)), ids=lambda p: P.PROGRAM_NAMES[p].replace(" ", "_"))
def test_wave_program_equals_the_model(emu, program):
    P.wave_program(emu, program)
