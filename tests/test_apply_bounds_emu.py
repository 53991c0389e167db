"""Sanitizer runs of the bridge edit (CPU only, stand-alone programs with their own main):
  apply_host.cpp alone (with gfa_writer.cpp for the text) in tests/c_client/apply_host_check.cpp, and
  kernels_apply.inc: the emulation linked into tests/c_client/apply_bounds_check.cpp with the guarded arena of csrc/device_rt.hpp
  (AC_ARENA_GUARD: exact sizes and red zones; level 2 also poisons rewound memory), from the per-level objects of `make kernel_bounds_check`,
both under the address and undefined-behaviour sanitizers.  The named cases and the boundary table of test_apply_emu.py are replayed at both
levels: exit status 0, no sanitizer report, and every result equal to the model's.  `make apply_bounds_check` in csrc builds the same programs."""
import ctypes as C
import fcntl
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import apply_util as A
import bounds_cases as B
import emu_lib
import finish_util as F
from autocycler_amd import _capi
from test_apply_emu import K, TILE_SIZES, bridge_length_case, hub_case, named_cases, ring_case

LEVELS = [1, 2]


def test_host_functions_stand_alone(tmp_path):
    root = emu_lib.ROOT
    exe = tmp_path / "apply_host_check"
    csrc = root / "autocycler_amd" / "csrc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(csrc),
                           str(root / "tests" / "c_client" / "apply_host_check.cpp"), str(csrc / "apply_host.cpp"), str(csrc / "gfa_writer.cpp"), "-o", str(exe),
                           "-pthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "apply_host_check: OK" in out.stdout, (out.stdout + out.stderr)[-2000:]


def driver(level):
    """builds (make, at most 8 jobs) and returns the driver of one guard level; rebuilt when a source is newer"""
    exe = B.GUARD_DIR / f"apply_bounds_check_l{level}"
    srcs = list(B.CSRC.glob("*.[ch]*")) + list(B.CSRC.glob("*.inc")) + [B.ROOT / "include" / "autocycler_hip.h", B.CSRC / "Makefile",
                                                                    B.ROOT / "tests" / "c_client" / "apply_bounds_check.cpp"]
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


def bridge_arrays(bridges):
    """the ac_bridge records and the two pools of a list of bridge dicts, as exact blocks"""
    recs = (_capi.Bridge * max(len(bridges), 1))()
    best, dist, doff, mult = [], [], [0], []
    for i, b in enumerate(bridges):
        r = recs[i]
        r.start, r.end, r.status, r.conflicting, r.culled = b["start"], b["end"], b["status"], b["conflicting"], b["culled"]
        r.best_off, r.best_len = len(best), len(b["best_path"])
        best.extend(b["best_path"])
        r.first_distinct, r.n_distinct = len(mult), len(b["distinct_paths"])
        for path, m in b["distinct_paths"]:
            dist.extend(path); doff.append(len(dist)); mult.append(m)
    return bytes(recs)[:len(bridges) * C.sizeof(_capi.Bridge)], best, dist, doff, mult


def add_call(calls, case, label, texts=True):
    exp, _ = A.apply_model(case["n"], case["links"], case["lens"], case["anchors"], case["bridges"], case["applied"], case["bridge_depth"], case["alive"], case["depths"],
                           case["seqs"])
    texts = texts and not any(math.isnan(d) and a for d, a in zip(exp["depth"], exp["alive"]))
    want_bridged = A.bridged_text(exp, K)
    want_merged = F.save_gfa(A.merged_model(exp)[0], K) if texts else b""
    sb, sg = seq_block(case["seqs"])
    recs, best, dist, doff, mult = bridge_arrays(case["bridges"])

    def check(outs, label):
        assert len(outs) == 11
        off = np.frombuffer(outs[7], dtype="<u8").tolist()
        got = dict(n_total=len(outs[1]), len=np.frombuffer(outs[0], dtype="<u4").tolist(), alive=list(outs[1]), type=list(outs[3]),
                   bridge_of=np.frombuffer(outs[4], dtype="<u4").tolist(), links=[tuple(l) for l in np.frombuffer(outs[5], dtype="<i4").reshape(-1, 2).tolist()],
                   bridge_seqs=[bytes(outs[6][off[i]:off[i + 1]]) for i in range(len(off) - 1)])
        for key in got:
            assert got[key] == exp[key], (label, key)
        assert bytes(outs[2]) == np.asarray(exp["depth"], dtype=np.float64).tobytes(), (label, "depth")
        assert bytes(outs[8]) == want_bridged and bytes(outs[9]) == want_merged, (label, "texts")
    calls.add("apply", [case["n"], len(case["links"]), len(case["anchors"]), len(case["bridges"]), len(best), len(mult), B.f64_bits(case["bridge_depth"]), int(texts)],
              [B.arr(np.asarray(case["links"], dtype=np.int32).reshape(-1, 2), np.int32), B.arr(case["lens"], np.uint32), B.arr(case["alive"], np.uint8),
               B.arr(case["depths"], np.float64), B.arr(case["anchors"], np.uint32), sb.tobytes(), sg.tobytes(), recs, B.arr(best, np.int32), B.arr(dist, np.int32),
               B.arr(doff, np.uint64), B.arr(mult, np.uint32), B.arr([int(bool(x)) for x in case["applied"]], np.uint8)], check, label=label)


def named_calls():
    calls = B.Calls()
    for name, case in named_cases().items():
        add_call(calls, case, name)
    return calls


def boundary_calls():
    calls = B.Calls()
    add_call(calls, bridge_length_case(), "bridge lengths")
    for n in TILE_SIZES:
        add_call(calls, ring_case(n), f"ring of {n}", texts=n <= 257)
    add_call(calls, hub_case(), "hub")
    return calls


_GROUPS = {}      # (one cached list per group: the expected values are computed once and serve both levels)


def _calls(name, make):
    if name not in _GROUPS:
        _GROUPS[name] = make()
    return _GROUPS[name]


def test_named_cases(exe, tmp_path):
    assert _calls("named", named_calls).run(exe, tmp_path) == len(named_cases())


def test_boundary_table(exe, tmp_path):
    assert _calls("boundary", boundary_calls).run(exe, tmp_path) == 2 + len(TILE_SIZES)
