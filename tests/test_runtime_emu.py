"""tests/runtime_cases.py on the CPU emulation: the hooks of the device runtime (csrc/selftest_runtime.inc) and their models.  The arena and the
event ring's bookkeeping are the same code here as on the device; fills, read-backs and atomics are the emulation's plain forms."""
import subprocess
from pathlib import Path

import pytest

import emu_lib
import runtime_cases as R
from autocycler_amd import _capi

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def emu():
    return emu_lib.emu_path()


@pytest.mark.parametrize("kind", ["all", "from", "first", "side_stream"])
def test_fill_every_size(emu, kind):
    R.fill_every_size(emu, kind)


@pytest.mark.parametrize("count", R.REGION_COUNTS)
def test_fill_region_count(emu, count):
    R.fill_region_count(emu, count)


def test_fill_triggers(emu):
    for trigger in _capi.FILL_TRIGGERS:
        R.fill_trigger(emu, trigger)


def test_fill_drop_on_reset(emu):
    R.fill_drop_on_reset(emu)


def test_fill_order(emu):
    R.fill_order(emu)


def test_readbacks(emu):
    R.readback_all(emu)


def test_readback_bad_arguments(emu):
    R.readback_bad_arguments(emu)


@pytest.mark.parametrize("name", list(R.ARENA_PROGRAMS))
def test_arena_program(emu, name):
    R.arena_program(emu, R.ARENA_PROGRAMS[name], name)


@pytest.mark.parametrize("first", range(0, 200, 50))
def test_arena_random_programs(emu, first):
    R.arena_random(emu, range(first, first + 50))


def test_arena_bad_arguments(emu):
    R.arena_bad_arguments(emu)


@pytest.mark.parametrize("which", ["launch", "launch_full", "launch_wave_kernel"])
def test_launcher(emu, which):
    for n in R.LAUNCH_SIZES:
        R.launcher(emu, which, n)


def test_launcher_grid_limits(emu):
    R.launcher_grid_limits(emu)


@pytest.mark.parametrize("name", list(R.FINAL_OPS))
def test_atomic_final_value(emu, name):
    R.atomic_final_value(emu, name)


@pytest.mark.parametrize("name", ["add32", "add64"])
def test_atomic_add_returns_old_values(emu, name):
    R.atomic_add_returns(emu, name)


@pytest.mark.parametrize("name", ["cas32", "cas64"])
def test_atomic_cas_claims(emu, name):
    R.atomic_cas_claims(emu, name)


def test_atomic_load(emu):
    R.atomic_load(emu)


def test_wave_alloc32(emu):
    R.wave_alloc(emu)


def test_wave_add64(emu):
    R.wave_add(emu)


def test_atomics_bad_arguments(emu):
    R.atomics_bad_arguments(emu)


@pytest.mark.parametrize("mode", ["after_main", "main_event"])
def test_side_stream_order(emu, mode):
    R.side_order(emu, mode, 0)
    R.side_order(emu, mode, 1)


def test_event_ring_program(emu):
    R.ring_program(emu)


def test_runtime_host_check_under_sanitizers(tmp_path):
    """The arena of device_rt.hpp alone (-DAC_EMU), a fixed subset of the programs above replayed against expected numbers, under the address and
    undefined-behaviour sanitizers (tests/c_client/runtime_host_check.cpp; `make runtime_host_check` in csrc builds the same program)."""
    exe = tmp_path / "runtime_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-DAC_EMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "autocycler_amd" / "csrc"),
                           str(ROOT / "tests" / "c_client" / "runtime_host_check.cpp"), "-o", str(exe), "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime_host_check: OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
