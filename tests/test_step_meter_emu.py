"""The graph steps meter themselves through the runtime's own counters (StepMeter, device_rt.hpp) in both builds.  Under the emulation the
launch and read-back counts used to come from a count kept by hand beside every launch; this file holds the counters to what that hand
count gave, case by case, and runs the meter's stand-alone check (tests/c_client/step_meter_check.cpp) under the sanitizers.  The same cases
run on the device in test_step_meter_gpu.py."""
import math
import subprocess

import pytest

import emu_lib
import step_meter_cases as K

# (launches, read_backs) of summary[...] under the emulation, recorded through step_meter_cases.collect at commit ac646a2 ("Add sequence
# subsets of a graph on the device, up to re-threaded paths"), the last one whose graph steps counted their launches by hand
RECORDED = {
    "components: one unitig, no links": (6, 2),
    "components: ring of 3": (15, 2),
    "components: 65 unitigs, two components, some dead": (21, 2),
    "components: nothing": (0, 0),
    "merge: chain of 4": (37, 4),
    "merge: chain of 4 with sequences": (38, 4),
    "merge: handle with paths": (41, 4),
    "subsets: no link kept": (11, 2),
    "subsets: links kept": (16, 2),
    "subsets: no kept entry": (0, 0),
    "merged paths: chains": (7, 2),
    "merged paths: no chain": (6, 2),
    "merged paths: no entry": (0, 0),
}


@pytest.fixture(scope="module")
def rows():
    return K.collect(lib_path=emu_lib.emu_path())


def test_table_covers_the_cases():
    assert tuple(RECORDED) == K.CASES and all(RECORDED[c] == (0, 0) for c in K.NOTHING_LAUNCHED)


@pytest.mark.parametrize("case", K.CASES)
def test_counts_are_the_recorded_ones(rows, case):
    assert (rows[case]["launches"], rows[case]["read_backs"]) == RECORDED[case]


def test_sequences_cost_the_copy_launch_alone(rows):
    plain, with_seq = rows["merge: chain of 4"], rows["merge: chain of 4 with sequences"]
    assert with_seq["launches"] == plain["launches"] + 1 and with_seq["read_backs"] == plain["read_backs"]


@pytest.mark.parametrize("case", [c for c in K.CASES if c not in K.NOTHING_LAUNCHED])
def test_seconds_are_finite(rows, case):
    assert math.isfinite(rows[case]["seconds_device"]) and rows[case]["seconds_device"] >= 0


def test_seconds_copy_is_the_second_interval(rows):
    plain, with_seq = rows["merge: chain of 4"], rows["merge: chain of 4 with sequences"]
    assert plain["seconds_copy"] == 0
    assert math.isfinite(with_seq["seconds_copy"]) and 0 <= with_seq["seconds_copy"] <= with_seq["seconds_device"]


def test_meter_stands_alone(tmp_path):
    """the meter without the library, under the address and undefined-behaviour sanitizers: a meter never begun, two intervals and their sum,
    ten laps on one interval, the counts of a launch, a launch_full, a scan and a three-pass sort, a meter destroyed with an interval open, an
    exception between begin and end (`make step_meter_check` in csrc builds the same program)"""
    root = emu_lib.ROOT
    exe = tmp_path / "step_meter_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-DAC_EMU", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           str(root / "autocycler_amd" / "csrc"), str(root / "tests" / "c_client" / "step_meter_check.cpp"), "-o", str(exe), "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "step_meter_check: OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
