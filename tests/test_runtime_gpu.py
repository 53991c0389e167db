"""tests/runtime_cases.py on the MI355X: the device runtime (csrc/device_rt.hpp) through the ac_selftest_* hooks of the product library — the
fused fill kernel, the mailbox and the other read-back paths, the launchers, the atomic wrappers, the side stream and its event ring."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

import parity_util
import runtime_cases as R
import seqgen
from autocycler_amd import _capi

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module", autouse=True)
def _need_lib():
    import autocycler_amd
    lib = autocycler_amd.load_library()       # raises HipLibraryMissing: the product has no fallback
    assert lib.ac_device_count() >= 1, "no HIP device visible"


# ---- 1. fused fills ----
@pytest.mark.parametrize("kind", list(_capi.FILL_KINDS))
def test_fill_every_size(kind):
    R.fill_every_size(None, kind)


@pytest.mark.parametrize("count", R.REGION_COUNTS)
def test_fill_region_count(count):
    R.fill_region_count(None, count)


@pytest.mark.parametrize("trigger", list(_capi.FILL_TRIGGERS))
def test_fill_trigger(trigger):
    R.fill_trigger(None, trigger)


def test_fill_drop_on_reset():
    R.fill_drop_on_reset(None)


def test_fill_order():
    R.fill_order(None)


# ---- 2. read-backs ----
@pytest.mark.parametrize("path", ["copy_d2h", "to_host"])
def test_d2h_every_size_and_misalignment(path):
    R.d2h_single(None, path)


def test_read_batch():
    R.batch(None)
    R.batch_run_twice(None)


def test_read_sequences():
    R.large_then_small(None)
    R.scalars(None)
    R.scalar_chain(None)
    R.side_stream_fetch(None)


def test_readback_bad_arguments():
    R.readback_bad_arguments(None)


def _read_backs_in_a_fresh_process(env):
    """use_mailbox() and the scratch switch are read once per process: the same case list in a child of its own (this process only waits)"""
    code = (f"import sys; sys.path.insert(0, {str(HERE.parent)!r}); sys.path.insert(0, {str(HERE)!r}); "
            "import runtime_cases as R; R.readback_all(None); R.fill_trigger(None, 'copy_d2h'); print('read-backs ok')")
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "read-backs ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_read_backs_without_the_mailbox():
    _read_backs_in_a_fresh_process({"AC_NO_MAILBOX": "1"})


def test_read_backs_without_the_mailbox_and_the_scratch_page():
    _read_backs_in_a_fresh_process({"AC_NO_MAILBOX": "1", "AC_NO_PINNED_SCRATCH": "1"})


# ---- 3. the arena ----
@pytest.mark.parametrize("name", list(R.ARENA_PROGRAMS))
def test_arena_program(name):
    R.arena_program(None, R.ARENA_PROGRAMS[name], name)


@pytest.mark.parametrize("first", range(0, 200, 50))
def test_arena_random_programs(first):
    R.arena_random(None, range(first, first + 50))


def test_arena_bad_arguments():
    R.arena_bad_arguments(None)


# ---- 4. the launchers ----
@pytest.mark.parametrize("which", ["launch", "launch_full", "launch_wave_kernel"])
def test_launcher(which):
    for n in R.LAUNCH_SIZES:
        R.launcher(None, which, n)


@pytest.mark.parametrize("which", ["launch", "launch_full", "launch_wave_kernel"])
def test_launcher_second_launch(which):
    """2^31 + 257 threads: the smallest grid above MAX_LAUNCH_BLOCKS workgroups (DESIGN.md 5c has the measured time)"""
    R.launcher(None, which, R.LAUNCH_BIG)


def test_launcher_grid_limits():
    R.launcher_grid_limits(None)


# ---- 5. atomics ----
@pytest.mark.parametrize("name", list(R.FINAL_OPS))
def test_atomic_final_value(name):
    R.atomic_final_value(None, name)


@pytest.mark.parametrize("name", ["add32", "add64"])
def test_atomic_add_returns_old_values(name):
    R.atomic_add_returns(None, name)


@pytest.mark.parametrize("name", ["cas32", "cas64"])
def test_atomic_cas_claims(name):
    R.atomic_cas_claims(None, name)


def test_atomic_load():
    R.atomic_load(None)


def test_wave_alloc32():
    R.wave_alloc(None)


def test_wave_add64():
    R.wave_add(None)


def test_atomics_bad_arguments():
    R.atomics_bad_arguments(None)


# ---- 6. the side stream and its event ring ----
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("mode", ["after_main", "main_event"])
def test_side_stream_order(mode, which):
    R.side_order(None, mode, which)


def test_event_ring_program():
    R.ring_program(None)


def _build_and_count(k, seqs, fn, hd):
    _capi.selftest_event_ring()      # clear
    parity_util.check_case(k, seqs, fn, hd)
    r = _capi.selftest_event_ring()
    print("events_taken", r["events_taken"], "recycled_waits", r["recycled_waits"])
    assert r["recycled_waits"] == 0, r
    assert 0 < r["events_taken"] < R.N_EV, r      # N_EV = 64: no handle of this build can have been recycled
    return r["events_taken"]


def test_event_ring_many_path_entries():
    from test_gpu_parity import _synth_case
    _build_and_count(51, *_synth_case(12, 300_000, 10_000, 5e-3, 2e-4, 777))


@pytest.mark.parametrize("knobs", [{"AC_LATE_COPIES": "2"}, {"AC_HOST_REMAP": "2"}, {"AC_REMAP_BLOCK": "128"}, {"AC_PATH_CHUNK": "64"}, {"AC_PATH_COPY": "1"},
                                   {"AC_LATE_COPIES": "2", "AC_HOST_REMAP": "2", "AC_REMAP_BLOCK": "128", "AC_SEQ_CODES": "2"}],
                         ids=lambda d: ",".join(f"{a}={b}" for a, b in d.items()))
def test_event_ring_under_the_chunk_knobs(monkeypatch, knobs):
    from test_gpu_parity import _synth_case
    for a, b in knobs.items():
        monkeypatch.setenv(a, b)
    for k, seed in ((11, 7), (51, 13)):
        _build_and_count(k, *seqgen.make_case(seed, k))
    _build_and_count(51, *_synth_case(6, 60_000, 3_000, 1e-3, 1e-4, 99))
