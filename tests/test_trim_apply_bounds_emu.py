"""Sanitizer runs of trim's edit (CPU only, stand-alone programs with their own main):
  trim_apply_host.cpp alone in tests/c_client/trim_apply_host_check.cpp, and
  kernels_trim_apply.inc with the subset stages it feeds: the emulation linked into tests/c_client/trim_apply_bounds_check.cpp with the guarded
  arena of csrc/device_rt.hpp (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons rewound memory), from the per-level objects
  of `make kernel_bounds_check`,
both under the address and undefined-behaviour sanitizers.  The named cases and the boundary table of test_trim_apply_emu.py are replayed at
both levels: exit status 0, no sanitizer report, and every result equal to the model's.  `make trim_apply_bounds_check` in csrc builds the
same programs.  Nothing is loaded into Python and nothing is preloaded."""
import fcntl
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bounds_cases as B
import emu_lib
import trim_apply_util as TA
from test_trim_apply_emu import K, exclusion_case, line_case, metas_of, named_cases, run_model, scan_tile

LEVELS = [1, 2]
CHOOSE = {"auto": 0, "none": 1, None: 1, "start_end": 2, "hairpin": 3}
KIND = {None: 0, "start_end": 1, "hairpin": 2}


def test_host_functions_stand_alone(tmp_path):
    root = emu_lib.ROOT
    exe = tmp_path / "trim_apply_host_check"
    csrc = root / "autocycler_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(csrc),
                           str(root / "tests" / "c_client" / "trim_apply_host_check.cpp"), str(csrc / "trim_apply_host.cpp"), "-o", str(exe), "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "trim_apply_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"trim_apply_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "trim_apply_bounds_check.cpp"]
    B.GUARD_DIR.mkdir(parents=True, exist_ok=True)
    with open(B.GUARD_DIR / ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not exe.exists() or any(s.stat().st_mtime > exe.stat().st_mtime for s in srcs):
            subprocess.check_call(["make", "-j", "8", "-C", str(B.CSRC), str(Path("../../tests/_emu/guard") / exe.name)], stdout=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module", params=LEVELS, ids=lambda l: f"guard{l}")
def exe(request):
    return driver(request.param)


def seq_block(seqs):
    begin = np.zeros(max(len(seqs), 1), dtype=np.uint64)[:len(seqs)]
    if len(seqs) > 1:
        begin[1:] = np.cumsum([len(s) for s in seqs[:-1]], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), begin      # (an exact block: no byte behind the last unitig)


def results_bytes(results):
    rows = [[r[kind][f] for kind in ("start_end", "hairpin") for f in ("status", "begin", "end", "trimmed_length")] + [0, 0] for r in results]
    return np.asarray(rows, dtype=np.uint32).tobytes()


def add_call(calls, case, label):
    exp = run_model(case)
    ids, fns, hds = metas_of(len(case["paths"]))
    want_text, want_yaml = TA.model_gfa(exp, K, ids, fns, hds), TA.model_yaml(exp)
    sb, sg = seq_block(case["seqs"])
    off = np.zeros(len(case["paths"]) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in case["paths"]], dtype=np.uint64)

    def check(outs, label):
        assert len(outs) == 7
        rec = np.frombuffer(outs[0], dtype=np.dtype([("begin", "<u4"), ("end", "<u4"), ("length", "<u8"), ("trimmed", "<u4"), ("excluded", "<u4")], align=True))
        assert [tuple(r) for r in rec.tolist()] == exp["records"], (label, "records")
        assert np.frombuffer(outs[1], dtype="<u4").tolist() == exp["cluster"]["unitigs"], (label, "unitigs")
        assert np.frombuffer(outs[2], dtype="<u4").tolist() == [exp["cluster"]["fwd"][u - 1] for u in exp["cluster"]["unitigs"]], (label, "positions")
        assert [tuple(l) for l in np.frombuffer(outs[3], dtype="<i4").reshape(-1, 2).tolist()] == exp["cluster"]["links"], (label, "links")
        assert bytes(outs[4]) == want_text and bytes(outs[5]) == want_yaml, (label, "texts")
        counts = np.frombuffer(outs[6], dtype="<u8").tolist()
        assert counts[2:] == [exp["median"], exp["mad"], exp["min"], exp["max"], KIND[exp["kind"]]], (label, counts)
    calls.add("trim_apply", [case["n"], len(case["links"]), len(case["paths"]), CHOOSE[case["chosen"]], B.f64_bits(case["mad"]), 1],
              [B.arr(np.asarray(case["links"], dtype=np.int32).reshape(-1, 2), np.int32), B.arr(case["lens"], np.uint32), B.arr(case["alive"], np.uint8),
               B.arr([e for p in case["paths"] for e in p], np.int32), off.tobytes(), B.arr(case["seq_lengths"], np.uint32), results_bytes(case["results"]),
               sb.tobytes(), sg.tobytes()], check, label=label)


def named_calls():
    calls = B.Calls()
    for name, case, _ in named_cases():
        add_call(calls, case, name)
    return calls


def boundary_table():
    tile = scan_tile()
    cases = {f"slice of {n}": line_case(n) for n in (1, 63, 64, 65, tile - 1, tile, tile + 1)}
    cases.update({f"{n} sequences": line_case(5, n) for n in (1, 2, 64, 65)})
    for n in (3, 64, 65):
        cases[f"{n} sequences, excluded first"] = exclusion_case(n, [s == 0 for s in range(n)])
        cases[f"{n} sequences, excluded last"] = exclusion_case(n, [s == n - 1 for s in range(n)])
        cases[f"{n} sequences, excluded alternating"] = exclusion_case(n, [s % 2 == 1 for s in range(n)])
        if n % 2:
            cases[f"{n} sequences, excluded all but one"] = exclusion_case(n, [s != n // 2 for s in range(n)])
    return cases


def boundary_calls():
    calls = B.Calls()
    for name, case in boundary_table().items():
        add_call(calls, case, name)
    return calls


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", named_calls).run(exe, tmp_path) == len(named_cases())


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", boundary_calls).run(exe, tmp_path) == len(boundary_table())
